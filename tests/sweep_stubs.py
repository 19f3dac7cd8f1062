"""Host stand-ins for the device work of sweep.py / score.py (tests/test_sweep_dataset.py): every
per-photo value is a function of the photo's file name alone, so whatever slices the photos are cut
into, the merged matrix has to be the one of a single call.

Run as a program it is one rank of a tool with the stand-ins installed:

    python tests/sweep_stubs.py {sweep|score} <the tool's arguments>

RF_STUB_FAIL_RANK=r makes the work of rank r raise, RF_STUB_DIE_RANK=r makes rank r end at once inside
its work, without a word to its peers; RF_STUB_THREADS_DIR=d makes every call of run() record
batch.IO_THREADS in d/threads_rank<r>.json.
"""
import json
import os
import sys
import zlib

import numpy as np

FAIL_MESSAGE = "judgement file of %s is missing"


def key(photo):
    """0..1023 from the file name (without its directory: the same in every tmp_path)."""
    return zlib.crc32(os.path.basename(photo).encode("utf-8")) % 1024


def judged(photo):
    return key(photo) % 5 != 3


def value(photo, pair, k=0):
    """The WHDR the stand-in gives photo `photo` under pair (sigma_color, sigma_spatial) after pass
    k + 1; 0 for a photo without judgements, as run() gives it."""
    if not judged(photo):
        return 0.0
    return ((key(photo) * 7 + int(pair[0] * 16) * 13 + int(pair[1] * 16) * 5) % 1009) / 1024.0 + k / 4096.0


def source_value(photo):
    return (key(photo) % 251) / 256.0 if judged(photo) else 0.0


def run(photos, filter_type, sigma_color, sigma_spatial, guidance="cnn", delta=0.1, src_files=None,
        guidance_files=None, iterations=1, png_decoder="host", src_coding="linear"):
    from reflectance_filtering_amd import batch, sweep
    rank = os.environ.get("RANK", "0")
    if os.environ.get("RF_STUB_THREADS_DIR"):
        with open(os.path.join(os.environ["RF_STUB_THREADS_DIR"], "threads_rank%s.json" % rank), "w") as fh:
            json.dump(batch.IO_THREADS, fh)
    if os.environ.get("RF_STUB_FAIL_RANK") == rank:
        raise IOError(FAIL_MESSAGE % photos[0])
    if os.environ.get("RF_STUB_DIE_RANK") == rank:
        os._exit(3)
    assert photos, "run() is not called for an empty slice"
    pairs = sweep.grid_pairs(sigma_color, sigma_spatial)
    per_image = np.array([[[value(f, pair, k) for f in photos] for pair in pairs]
                          for k in range(iterations)], dtype=np.float64)
    has = np.array([judged(f) for f in photos], dtype=bool)
    return pairs, (per_image if iterations > 1 else per_image[0]), has


def load(photos, src_files=None, guidance_files=None, png_decoder="host", photo_pixels=True):
    """sweep.load for score.py: 2x2 images, the source of a photo filled with its key % 251."""
    if os.environ.get("RF_STUB_FAIL_RANK") == os.environ.get("RANK", "0"):
        raise IOError(FAIL_MESSAGE % photos[0])
    images = [np.zeros((2, 2, 3), dtype=np.uint8) for _ in photos]
    sources = [np.full((2, 2, 3), key(f) % 251, dtype=np.uint8) for f in photos]
    judgements = [np.array([[0.25, 0.25, 0.75, 0.75, 1.0, 1.0]] if judged(f) else []).reshape(-1, 6)
                  for f in photos]
    return images, sources, None, judgements, [True] * len(photos)


def score_sources(sources, grey, comps, coding="linear", delta=0.1):
    return np.array([int(src[0, 0, 0]) / 256.0 if c.shape[0] else 0.0 for src, c in zip(sources, comps)],
                    dtype=np.float64)


def install(setattr_=setattr):
    """The stand-ins in place of sweep.run, sweep.load and score.score_sources (setattr_:
    monkeypatch.setattr in a test)."""
    from reflectance_filtering_amd import score, sweep
    setattr_(sweep, "run", run)
    setattr_(sweep, "load", load)
    setattr_(score, "score_sources", score_sources)
    return sweep, score


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    tools = dict(zip(("sweep", "score"), install()))
    sys.exit(tools[sys.argv[1]].main(sys.argv[2:]))
