"""Host stand-ins for the device work of train.py (tests/test_train_host.py), in the manner of
tests/sweep_stubs.py: sweep.load gives 4x4 photos with one judgement each, train.pack and train.fit
record what they were called with and touch no device."""
import numpy as np

CALLS = []


def load(photos, src_files=None, guidance_files=None, png_decoder="host", photo_pixels=True):
    images = [np.zeros((4, 4, 3), dtype=np.uint8) for _ in photos]
    judgements = [np.array([[0.25, 0.25, 0.75, 0.75, 1.0, 1.0]]) for _ in photos]
    return images, None, None, judgements, None


class FakePacked(object):
    def __init__(self, n):
        self.n, self.total, self.comps = n, 2 * n, np.zeros((n, 3), dtype=np.int32)


def pack(images, comparisons_px, order_seed=None, ratio=1.0, eval_dense=True, device=None):
    CALLS.append(("pack", len(images), order_seed, ratio, eval_dense))
    return FakePacked(len(images))


def fit(packed, weights=None, **options):
    CALLS.append(("fit", packed.n, options))
    entry = {"iteration": options["iterations"], "batch_loss": 0.5,
             "train": {"hinge": 0.5, "whdr": 0.25}}
    if options.get("held_out") is not None:
        entry["held_out"] = {"hinge": 0.75, "whdr": 0.5}
    options["log"](entry)
    return np.asarray(weights, dtype=np.float32) + np.float32(1.0), [entry]


def install(setattr_):
    from reflectance_filtering_amd import sweep, train
    del CALLS[:]
    setattr_(sweep, "load", load)
    setattr_(train, "pack", pack)
    setattr_(train, "fit", fit)
    return train
