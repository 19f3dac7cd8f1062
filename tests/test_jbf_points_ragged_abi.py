"""CPU suite: the ragged point-evaluated joint bilateral (rf_jbf_points_ragged_u8: images of
different sizes packed one after another, one launch) - refusals before any GPU work, the
workspace size, the per-image point check and the packing plan of whdr.sweep, and the guided
half's grouping of equal shapes wherever they stand in a list.  No compute calls."""
import ctypes

import numpy as np
import pytest

from reflectance_filtering_amd import _ffi, ops, whdr


def _dbl(values):
    a = np.ascontiguousarray(values, dtype=np.float64)
    return a, a.ctypes.data


def _ints(values):
    a = np.ascontiguousarray(values, dtype=np.int32)
    return a, a.ctypes.data


def _align256(b):
    return (b + 255) & ~255


def test_ragged_refusals_need_no_gpu(built):
    lib = _ffi.load_library()
    buf = ctypes.create_string_buffer(1 << 16)
    base = ctypes.addressof(buf)
    j, s, pts, off, out = base, base + 4096, base + 8192, base + 12288, base + 16384
    sc, p_sc = _dbl([20.0, 15.0])
    ss, p_ss = _dbl([22.0, 28.0])
    hs, p_h = _ints([8, 3, 5])
    wsz, p_w = _ints([8, 7, 2])                                # 64 + 21 + 10 = 95 pixels
    ws_need = lib.rf_jbf_points_ragged_workspace_bytes(3, 2, p_ss, -1, 1, _ffi.JBF_GREY_AS_BGR)
    assert ws_need > 0

    def call(joint=j, src=s, n=3, ph=p_h, pw=p_w, jcn=1, scn=1, points=pts, offsets=off, total=4,
             n_params=2, p_c=p_sc, p_s=p_ss, d=-1, border=4, flags=_ffi.JBF_GREY_AS_BGR, o=out,
             ws=base + 32768, ws_bytes=1 << 40):
        return lib.rf_jbf_points_ragged_u8(joint, src, n, ph, pw, jcn, scn, points, offsets, total,
                                           n_params, p_c, p_s, d, border, flags, o, ws, ws_bytes,
                                           None)

    assert call(joint=None) == _ffi.RF_E_BADARG
    assert b"NULL" in lib.rf_last_error() and b"rf_jbf_points_ragged_u8" in lib.rf_last_error()
    for kw in ({"src": None}, {"points": None}, {"offsets": None}, {"o": None}, {"ph": None},
               {"pw": None}):
        assert call(**kw) == _ffi.RF_E_BADARG, kw
    assert call(n=0, joint=None, ph=None, pw=None) == _ffi.RF_OK   # an empty list is valid
    assert call(n=-1) == _ffi.RF_E_BADARG
    assert call(total=-1) == _ffi.RF_E_BADARG
    for bad_h, bad_w in (([8, 0, 5], [8, 7, 2]), ([8, 3, 5], [8, 7, 0]), ([8, 3, -5], [8, 7, 2]),
                         ([8, 3, 5], [-8, 7, 2])):
        a, p_a = _ints(bad_h)
        b, p_b = _ints(bad_w)
        assert call(ph=p_a, pw=p_b) == _ffi.RF_E_BADARG, (bad_h, bad_w)
        assert b"size" in lib.rf_last_error()
    assert call(n_params=0) == _ffi.RF_E_BADARG
    assert call(n_params=-3) == _ffi.RF_E_BADARG
    assert call(p_c=None) == _ffi.RF_E_BADARG
    assert call(p_s=None) == _ffi.RF_E_BADARG
    assert call(jcn=2) == _ffi.RF_E_UNSUPPORTED
    assert call(scn=4) == _ffi.RF_E_UNSUPPORTED
    assert b"channels" in lib.rf_last_error()
    assert call(border=5) == _ffi.RF_E_UNSUPPORTED
    assert call(border=-1) == _ffi.RF_E_UNSUPPORTED
    assert call(flags=0x1000) == _ffi.RF_E_BADARG
    assert b"flag" in lib.rf_last_error()
    assert call(flags=8) == _ffi.RF_E_BADARG
    assert call(ws_bytes=ws_need - 1) == _ffi.RF_E_WORKSPACE
    # the tables alone are not enough: the image records need their block
    tables = lib.rf_jbf_points_workspace_bytes(2, p_ss, -1, 1, _ffi.JBF_GREY_AS_BGR)
    assert call(ws_bytes=tables) == _ffi.RF_E_WORKSPACE
    assert call(ws=None) == _ffi.RF_E_WORKSPACE
    big, p_big = _dbl([20.0, 3000.0])                          # radius 4500 > 4096, as rf_jbf_u8
    assert call(p_s=p_big) == _ffi.RF_E_UNSUPPORTED
    assert b"radius" in lib.rf_last_error()


def test_ragged_overlap_is_judged_on_the_summed_pixel_count(built):
    """95 pixels in images of 64, 21 and 10: `out` (2 sets x 4 points = 8 bytes) overlaps the joint
    from byte 87 on and is clear of it at byte 95 - beyond n*h*w of the last image (30), short of
    that of the first (192).  With three channels the images end at byte 285."""
    lib = _ffi.load_library()
    buf = ctypes.create_string_buffer(1 << 16)
    base = ctypes.addressof(buf)
    j, s, pts, off = base, base + 4096, base + 8192, base + 12288
    sc, p_sc = _dbl([20.0, 15.0])
    ss, p_ss = _dbl([22.0, 28.0])
    hs, p_h = _ints([8, 3, 5])
    wsz, p_w = _ints([8, 7, 2])

    def call(o, joint=j, src=s, jcn=1, scn=1):
        # a NULL workspace: a call that passes the overlap check is refused for it right after
        return lib.rf_jbf_points_ragged_u8(joint, src, 3, p_h, p_w, jcn, scn, pts, off, 4, 2, p_sc,
                                           p_ss, -1, 4, 0, o, None, 0, None)

    for o in (j, j + 30, j + 94, j - 7, s + 94, s + 64):
        assert call(o) == _ffi.RF_E_BADARG, o - base
        assert b"overlap" in lib.rf_last_error()
    for o in (j + 95, j - 8, s + 95, s - 8):
        assert call(o) == _ffi.RF_E_WORKSPACE, o - base
    assert call(j + 284, jcn=3) == _ffi.RF_E_BADARG
    assert call(j + 285, jcn=3) == _ffi.RF_E_WORKSPACE
    # out of a 3-channel src is 24 bytes
    assert call(s - 23, scn=3) == _ffi.RF_E_BADARG
    assert call(s - 24, scn=3) == _ffi.RF_E_WORKSPACE


def test_ragged_workspace_is_the_uniform_one_plus_the_image_records(built):
    lib = _ffi.load_library()
    ragged, uniform = lib.rf_jbf_points_ragged_workspace_bytes, lib.rf_jbf_points_workspace_bytes
    for ss in ([22.0], [22.0, 66.0, 22.0], [3.0] * 65):
        a, p = _dbl(ss)
        for jcn, flags in ((3, 0), (1, 0), (1, _ffi.JBF_GREY_AS_BGR)):
            for d in (-1, 5):
                base = uniform(len(ss), p, d, jcn, flags)
                assert base > 0
                for n in (0, 1, 16, 17, 1000, 100000):
                    assert ragged(n, len(ss), p, d, jcn, flags) == base + _align256(16 * n)
    a, p = _dbl([22.0])
    assert _align256(16 * 16) == 256 and _align256(16 * 17) == 512
    assert ragged(-1, 1, p, -1, 3, 0) == 0
    assert ragged(4, 0, p, -1, 3, 0) == 0
    assert ragged(4, 1, None, -1, 3, 0) == 0
    assert ragged(4, 1, p, -1, 2, 0) == 0
    big, p_big = _dbl([3000.0])
    assert ragged(4, 1, p_big, -1, 3, 0) == 0


def test_the_launch_plan_serves_the_ragged_entry_unchanged(built):
    """One plan query for both entries: it takes no image sizes at all."""
    lib = _ffi.load_library()
    assert not hasattr(_ffi, "jbf_points_ragged_plan")
    with pytest.raises(AttributeError):
        lib.rf_debug_jbf_points_ragged_plan
    assert _ffi.jbf_points_plan([3.0, 5.0], -1, 1, 0, 4096) == [(8, 1, 2, 2048), (4, 1, 2, 2048)]


# ---- the host side: point check per image, packing, grouping ----------------------------------

def test_points_are_checked_against_their_own_image():
    sizes = [(5, 9), (9, 5), (1, 1)]                           # (h, w)
    ok = np.array([[8, 4], [0, 0], [4, 8], [0, 0]])            # (x, y)
    pts, off = ops.check_points_ragged(ok, [0, 2, 3, 4], sizes)
    assert pts.dtype == np.int32 and off.dtype == np.int32
    assert pts.tolist() == ok.tolist() and off.tolist() == [0, 2, 3, 4]
    # (8, 4) is inside image 0 (9 wide) but outside image 1 (5 wide): the offsets decide
    with pytest.raises(IndexError) as err:
        ops.check_points_ragged(ok, [0, 0, 3, 4], sizes)
    assert "image 1" in str(err.value)
    # (4, 8) fits image 1 (9 high) and not image 0 (5 high)
    with pytest.raises(IndexError) as err:
        ops.check_points_ragged(ok, [0, 3, 3, 4], sizes)
    assert "image 0" in str(err.value)
    for bad in ([[9, 0]], [[0, 5]], [[-1, 0]], [[0, -1]]):
        with pytest.raises(IndexError):
            ops.check_points_ragged(bad, [0, 1, 1, 1], sizes)
    with pytest.raises(IndexError):
        ops.check_points_ragged([[1, 0]], [0, 0, 0, 1], sizes)  # the 1x1 image holds (0, 0) only
    for off in ([0, 2, 3], [1, 2, 3, 4], [0, 3, 2, 4], [0, 2, 3, 5]):
        with pytest.raises(ValueError):
            ops.check_points_ragged(ok, off, sizes)
    with pytest.raises(ValueError):
        ops.check_points_ragged(ok, [0, 2, 3, 4], [(5, 9), (0, 5), (1, 1)])
    # an image without points, and no points at all
    assert ops.check_points_ragged(ok[:2], [0, 2, 2, 2], sizes)[1].tolist() == [0, 2, 2, 2]
    assert ops.check_points_ragged(np.zeros((0, 2)), [0, 0, 0, 0], sizes)[0].shape == (0, 2)


def test_ragged_dedup_uses_each_images_size():
    sizes = [(5, 9), (9, 5)]
    c0 = np.array([[8, 4, 0, 0, 1, 1.0], [0, 0, 8, 4, 2, 0.5]])
    c1 = np.array([[4, 8, 1, 1, 0, 2.0]])
    pts, po, comps, wts, co = whdr.dedup_points_ragged([c0, c1], sizes)
    assert pts.tolist() == [[0, 0], [8, 4], [1, 1], [4, 8]]
    assert po.tolist() == [0, 2, 4] and co.tolist() == [0, 2, 3]
    assert comps.tolist() == [[1, 0, 1], [0, 1, 2], [1, 0, 0]]  # indices within the image's points
    assert wts.tolist() == [1.0, 0.5, 2.0]
    # equal sizes: exactly dedup_points
    a = whdr.dedup_points_ragged([c0, c0[:1]], [(5, 9), (5, 9)])
    b = whdr.dedup_points([c0, c0[:1]], 5, 9)
    assert all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(a, b))
    with pytest.raises(IndexError):
        whdr.dedup_points_ragged([c1, c0], sizes)               # each fits the other's image only


def test_sweep_rejects_a_point_of_the_neighbouring_images_size_before_device_work():
    """(x 8, y 4) lies inside the 5x9 image and outside the 9x5 one beside it."""
    wide, tall = np.zeros((5, 9, 1), np.uint8), np.zeros((9, 5, 1), np.uint8)
    comp = np.array([[8, 4, 0, 0, 1, 1.0]])
    none = np.zeros((0, 6))
    for ftype in ("bilateral", "guided"):
        with pytest.raises(IndexError):
            whdr.sweep(ftype, [wide, tall], [wide, tall], [comp, comp], [(20, 22)])
        with pytest.raises(IndexError):
            whdr.sweep(ftype, [tall, wide], [tall, wide], [comp, none], [(20, 22)])
    with pytest.raises(ValueError):                              # src and joint of different sizes
        whdr.sweep("bilateral", [wide], [tall], [none], [(20, 22)])


def test_packs_ignore_the_order_and_respect_both_budgets(monkeypatch):
    keys = [(1, 1), (1, 3), (1, 1), (3, 3), (1, 1), (1, 3)]
    px = [100, 200, 300, 400, 500, 600]
    points = [10, 20, 30, 40, 50, 60]
    scn = lambda k: k[0]
    assert whdr.plan_packs(keys, px, points, 6, scn) == [[0, 2, 4], [1, 5], [3]]
    assert whdr.plan_packs([], [], [], 6, scn) == []
    monkeypatch.setattr(whdr, "SWEEP_PACK_PIXELS", 800)
    # 100 + 300 fit, + 500 does not; 200 + 600 fit exactly
    assert whdr.plan_packs(keys, px, points, 6, scn) == [[0, 2], [4], [1, 5], [3]]
    monkeypatch.setattr(whdr, "SWEEP_PACK_PIXELS", 250)          # an image over the limit goes alone
    assert whdr.plan_packs(keys, px, points, 6, scn) == [[0], [2], [4], [1], [5], [3]]
    monkeypatch.setattr(whdr, "SWEEP_PACK_PIXELS", 1 << 30)
    monkeypatch.setattr(whdr, "SWEEP_PACK_OUT_BYTES", 6 * 40)    # 6 pairs x 40 points x 1 channel
    assert whdr.plan_packs(keys, px, points, 6, scn) == [[0, 2], [4], [1], [5], [3]]
    monkeypatch.setattr(whdr, "SWEEP_PACK_OUT_BYTES", 3 * 6 * 40)
    assert whdr.plan_packs(keys, px, points, 6, scn) == [[0, 2, 4], [1, 5], [3]]


def test_guided_sweep_groups_equal_shapes_wherever_they_stand(monkeypatch):
    """An interleaved list of three shapes is three guided batches, not seven runs; the results
    return to the caller's order."""
    shapes = [(5, 9), (9, 5), (5, 9), (6, 8), (9, 5), (5, 9), (6, 8)]
    imgs = [np.full((h, w, 1), i, np.uint8) for i, (h, w) in enumerate(shapes)]
    comps = [np.array([[0, 0, 1, 1, 1, 1.0]]) for _ in shapes]
    calls = []

    def fake_batch(filter_type, src, joint, comparisons_px, pairs, delta, grey_as_bgr):
        assert filter_type == "guided" and src.shape == joint.shape
        calls.append(tuple(src.shape))
        # column = the image's own fill value, so the scatter back by index shows
        ids = src[:, 0, 0, 0].astype(np.float64)
        return np.stack([ids + 100 * p for p in range(pairs.shape[0])])

    monkeypatch.setattr(whdr, "_sweep_batch", fake_batch)
    monkeypatch.setattr(whdr, "_stack", lambda images: np.stack([np.asarray(im) for im in images]))
    monkeypatch.setattr(whdr._ffi, "require_gpu", lambda: None)
    out = whdr.sweep("guided", imgs, imgs, comps, [(3, 5), (7, 9)], grey_as_bgr=True)
    assert sorted(calls) == [(2, 6, 8, 1), (2, 9, 5, 1), (3, 5, 9, 1)]
    assert out.tolist() == [[0, 1, 2, 3, 4, 5, 6], [100, 101, 102, 103, 104, 105, 106]]
