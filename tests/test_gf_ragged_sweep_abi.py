"""CPU suite: the host logic that routes whdr.sweep('guided') over a mixed one-channel device list
through the ragged guided filter (ops.guided_filter_ragged_sweep_u8: a packed list at one radius for
several eps, one rf_gf_ragged_u8 call per eps) - packs, grouping of pairs by radius, pairs named twice,
eps chunks, and the lists and pairs that keep the shape groups.  Stubs only, no compute calls."""
import numpy as np

from reflectance_filtering_amd import filter_reflectance as fr
from reflectance_filtering_amd import whdr

SHAPES = [(341, 512), (512, 341), (341, 512), (384, 512), (512, 341)]


# ---- whdr.sweep('guided') over lists: the host side -----------------------------------------------

class _Img(object):
    """Stands for a device image: a shape, an id and a device."""
    device = "dev"
    is_cuda = True

    def __init__(self, shape, ident):
        self.shape, self.ident = shape, ident


class _Batch(list):
    """Stands for a stacked batch: the images and their common shape."""

    @property
    def shape(self):
        return (len(self),) + tuple(self[0].shape)


def _stub(monkeypatch, calls, batches, cap=1 << 40):
    def fake_pack(images, torch):
        return [im.ident for im in images]

    def fake_sweep_op(guides, srcs, radius, eps_list, grey_as_bgr=False, sizes=None, out=None):
        calls.append((list(guides), list(srcs), radius, list(eps_list), grey_as_bgr,
                      [tuple(s) for s in sizes], guides is srcs))
        return ("filtered", radius, tuple(eps_list), tuple(srcs))

    def fake_points(samples, point_offsets, comps, weights, comp_offsets, delta=0.1):
        # [k, n]: 1000 * radius + 10 * eps + image id
        _, radius, eps, ids = samples
        return np.array([[1000.0 * radius + 10 * e + i for i in ids] for e in eps])

    def fake_batch(filter_type, src, joint, comparisons_px, pairs, delta, grey_as_bgr):
        batches.append(([im.ident for im in src], pairs.tolist()))
        return np.array([[-1.0 - im.ident for im in src] for _ in range(pairs.shape[0])])

    from reflectance_filtering_amd import ops
    monkeypatch.setattr(ops, "guided_filter_ragged_sweep_u8", fake_sweep_op)
    monkeypatch.setattr(ops, "gf_workspace_cap", lambda device, torch: cap)
    monkeypatch.setattr(whdr, "whdr_points_u8", fake_points)
    monkeypatch.setattr(whdr, "_pack_list", fake_pack)
    monkeypatch.setattr(whdr, "_sweep_batch", fake_batch)
    monkeypatch.setattr(whdr, "_stack", lambda images: _Batch(images))
    monkeypatch.setattr(whdr._ffi, "require_gpu", lambda: None)


COMP = np.array([[0, 0, 1, 1, 1, 1.0]])
PAIRS = [(3, 45), (7, 52.5), (1, 45.9), (3, 52), (3, 45), (5, 45)]


def test_a_mixed_device_list_is_one_call_per_pack_and_radius(monkeypatch):
    calls, batches = [], []
    _stub(monkeypatch, calls, batches)
    imgs = [_Img((h, w, 1), i) for i, (h, w) in enumerate(SHAPES)]
    comps = [COMP] * 5
    out = whdr.sweep("guided", imgs, imgs, comps, PAIRS, grey_as_bgr=True)
    assert not batches
    # radius 45 with eps 3, 1, 5 (the pair named twice computed once), radius 52 with eps 7, 3
    assert [(c[2], c[3]) for c in calls] == [(45, [3.0, 1.0, 5.0]), (52, [7.0, 3.0])]
    for c in calls:
        assert c[0] == c[1] == [0, 1, 2, 3, 4] and c[4] is True and c[5] == SHAPES and c[6]
    want = [[1000.0 * int(ss) + 10 * sc + i for i in range(5)] for sc, ss in PAIRS]
    assert out.tolist() == want
    assert out[0].tolist() == out[4].tolist()
    # a colour guide: its own pack, the same calls
    del calls[:]
    guides = [_Img((h, w, 3), 100 + i) for i, (h, w) in enumerate(SHAPES)]
    whdr.sweep("guided", imgs, guides, comps, PAIRS)
    assert [(c[0], c[1], c[2], c[4], c[6]) for c in calls] == [
        ([100, 101, 102, 103, 104], [0, 1, 2, 3, 4], 45, False, False),
        ([100, 101, 102, 103, 104], [0, 1, 2, 3, 4], 52, False, False)]


def test_packs_and_eps_chunks(monkeypatch):
    calls, batches = [], []
    _stub(monkeypatch, calls, batches)
    imgs = [_Img((h, w, 1), i) for i, (h, w) in enumerate(SHAPES)]
    monkeypatch.setattr(fr, "GF_RAGGED_MAX_BYTES", 400000)       # two images per pack
    out = whdr.sweep("guided", imgs, imgs, [COMP] * 5, [(3, 45), (7, 45), (3, 52)], grey_as_bgr=True)
    assert [(c[1], c[2], c[3]) for c in calls] == [
        ([0, 1], 45, [3.0, 7.0]), ([0, 1], 52, [3.0]), ([2, 3], 45, [3.0, 7.0]), ([2, 3], 52, [3.0]),
        ([4], 45, [3.0, 7.0]), ([4], 52, [3.0])]
    assert out.tolist() == [[45030.0 + i for i in range(5)], [45070.0 + i for i in range(5)],
                            [52030.0 + i for i in range(5)]]
    # the filtered bytes in flight: two images of a pack are 349184 bytes, so 700000 hold two eps
    del calls[:]
    monkeypatch.setattr(whdr, "SWEEP_GUIDED_BYTES", 700000)
    whdr.sweep("guided", imgs[:2], imgs[:2], [COMP] * 2, [(3, 45), (7, 45), (5, 45)], grey_as_bgr=True)
    assert [(c[2], c[3]) for c in calls] == [(45, [3.0, 7.0]), (45, [5.0])]
    # the workspace cap of a pack: 7 MB hold two 341 x 512 images (3.2 MB each)
    del calls[:]
    monkeypatch.setattr(fr, "GF_RAGGED_MAX_BYTES", 1 << 30)
    monkeypatch.setattr(whdr, "SWEEP_GUIDED_BYTES", 1 << 30)
    _stub(monkeypatch, calls, batches, cap=7 << 20)
    whdr.sweep("guided", imgs, imgs, [COMP] * 5, [(e, 45) for e in (1, 3, 5, 7)], grey_as_bgr=True)
    assert [c[1] for c in calls] == [[0, 1], [2, 3], [4]]
    assert all(c[3] == [1.0, 3.0, 5.0, 7.0] for c in calls)


def test_every_other_list_and_pair_keeps_the_shape_groups(monkeypatch):
    calls, batches = [], []
    _stub(monkeypatch, calls, batches)
    comps = [COMP] * 5
    one = [_Img((h, w, 1), i) for i, (h, w) in enumerate(SHAPES)]
    three = [_Img((h, w, 3), i) for i, (h, w) in enumerate(SHAPES)]
    host = [type("HostImg", (_Img,), {"is_cuda": False})((h, w, 1), i) for i, (h, w) in enumerate(SHAPES)]
    same = [_Img((341, 512, 1), i) for i in range(4)]
    for src, joint in ((three, three), (host, host), (one, host)):
        del batches[:]
        out = whdr.sweep("guided", src, joint, comps, [(3, 45), (7, 52)])
        assert sorted(b[0] for b in batches) == [[0, 2], [1, 4], [3]] and not calls
        assert all(b[1] == [[3, 45], [7, 52]] for b in batches)
        assert out.tolist() == [[-1.0 - i for i in range(5)]] * 2
    del batches[:]
    whdr.sweep("guided", same, same, [COMP] * 4, [(3, 45)], grey_as_bgr=True)
    assert [b[0] for b in batches] == [[0, 1, 2, 3]] and not calls
    # radii outside 1..128 stay with the shape groups, pair by pair
    del batches[:]
    out = whdr.sweep("guided", one, one, comps, [(3, 129), (3, 45), (7, 0.5)], grey_as_bgr=True)
    assert [(c[2], c[3]) for c in calls] == [(45, [3.0])]
    assert sorted(b[0] for b in batches) == [[0, 2], [1, 4], [3]]
    assert all(b[1] == [[3, 129], [7, 0.5]] for b in batches)
    assert out[1].tolist() == [45030.0 + i for i in range(5)]
    assert out[0].tolist() == out[2].tolist() == [-1.0 - i for i in range(5)]
