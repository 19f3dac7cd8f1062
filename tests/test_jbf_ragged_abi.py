"""CPU suite: the ragged full-image joint bilateral (rf_jbf_ragged_u8: images of different sizes
packed one after another, one launch per tile class) - refusals before any GPU work, the
workspace size, the launch plan against plans worked out by hand from the strip rules of
rf_jbf.hip (tile64_areas), and the host logic of filter_reflectance.apply_filter_list.
No compute calls."""
import ctypes

import numpy as np
import pytest

from reflectance_filtering_amd import _ffi
from reflectance_filtering_amd import filter_reflectance as fr


def _ints(values):
    a = np.ascontiguousarray(values, dtype=np.int32)
    return a, a.ctypes.data


def _align256(b):
    return (b + 255) & ~255


def _tiles64(sizes):
    return sum(-(-h // 64) * -(-w // 64) for h, w in sizes)


def test_ragged_refusals_need_no_gpu(built):
    lib = _ffi.load_library()
    buf = ctypes.create_string_buffer(1 << 16)
    base = (ctypes.addressof(buf) + 255) & ~255
    j, s, o, ws = base, base + 4096, base + 8192, base + 16384
    hs, p_h = _ints([8, 3, 5])
    wsz, p_w = _ints([8, 7, 2])                                # 64 + 21 + 10 = 95 pixels
    ws_need = lib.rf_jbf_ragged_workspace_bytes(3, p_h, p_w, 1, 1, -1, 22.0, _ffi.JBF_GREY_AS_BGR)
    assert ws_need == 256                                      # three 64x64 tiles of 32 bytes

    def call(joint=j, src=s, dst=o, n=3, ph=p_h, pw=p_w, jcn=1, scn=1, d=-1, sc=20.0, ss=22.0,
             border=4, flags=_ffi.JBF_GREY_AS_BGR, w=ws, ws_bytes=ws_need - 1):
        # the workspace is one byte short: a call that passes every other check is refused for it
        return lib.rf_jbf_ragged_u8(joint, src, dst, n, ph, pw, jcn, scn, d, sc, ss, border, flags,
                                    w, ws_bytes, None)

    assert call(joint=None) == _ffi.RF_E_BADARG
    assert b"NULL" in lib.rf_last_error() and b"rf_jbf_ragged_u8" in lib.rf_last_error()
    for kw in ({"src": None}, {"dst": None}, {"ph": None}, {"pw": None}):
        assert call(**kw) == _ffi.RF_E_BADARG, kw
        assert b"NULL" in lib.rf_last_error()
    # an empty list is valid whatever the pointers are
    assert call(n=0, joint=None, src=None, dst=None, ph=None, pw=None, w=None) == _ffi.RF_OK
    assert call(n=-1) == _ffi.RF_E_BADARG
    for bad_h, bad_w in (([8, 0, 5], [8, 7, 2]), ([8, 3, 5], [8, 7, 0]), ([8, 3, -5], [8, 7, 2]),
                         ([8, 3, 5], [-8, 7, 2])):
        a, p_a = _ints(bad_h)
        b, p_b = _ints(bad_w)
        assert call(ph=p_a, pw=p_b) == _ffi.RF_E_BADARG, (bad_h, bad_w)
        assert b"size" in lib.rf_last_error()
    assert call(jcn=2) == _ffi.RF_E_UNSUPPORTED
    assert call(scn=4) == _ffi.RF_E_UNSUPPORTED
    assert b"channels" in lib.rf_last_error()
    assert call(border=5) == _ffi.RF_E_UNSUPPORTED
    assert call(border=-1) == _ffi.RF_E_UNSUPPORTED
    assert b"border" in lib.rf_last_error()
    assert call(flags=0x1000) == _ffi.RF_E_BADARG
    assert b"flag" in lib.rf_last_error()
    assert call(flags=8) == _ffi.RF_E_BADARG
    assert call(ss=3000.0) == _ffi.RF_E_UNSUPPORTED           # radius 4500 > 4096, as rf_jbf_u8
    assert b"radius" in lib.rf_last_error()
    # the small workspace itself, a missing and a misaligned one
    assert call() == _ffi.RF_E_BADARG
    assert b"workspace" in lib.rf_last_error()
    assert call(ws_bytes=0) == _ffi.RF_E_BADARG
    assert call(w=None, ws_bytes=1 << 20) == _ffi.RF_E_BADARG
    assert call(w=ws + 8, ws_bytes=1 << 20) == _ffi.RF_E_BADARG
    assert b"workspace" in lib.rf_last_error()
    # ... also where the call would fall back to one launch per image (radius 54, the generic kernel)
    assert call(ss=36.0) == _ffi.RF_E_BADARG
    assert call(flags=_ffi.JBF_FORCE_GENERIC) == _ffi.RF_E_BADARG
    assert b"workspace" in lib.rf_last_error()


def test_ragged_overlap_is_judged_on_the_summed_pixel_count(built):
    """95 pixels in images of 64, 21 and 10: dst overlaps the joint up to byte 94 and is clear of it
    at byte 95 - beyond n*h*w of the last image (30), short of that of the first (192)."""
    lib = _ffi.load_library()
    buf = ctypes.create_string_buffer(1 << 16)
    base = ctypes.addressof(buf)
    j, s = base + 4096, base + 8192
    hs, p_h = _ints([8, 3, 5])
    wsz, p_w = _ints([8, 7, 2])

    def call(dst, jcn=1, scn=1):
        # a NULL workspace: a call that passes the overlap check is refused for it right after
        return lib.rf_jbf_ragged_u8(j, s, dst, 3, p_h, p_w, jcn, scn, -1, 20.0, 22.0, 4, 0, None, 0,
                                    None)

    for dst in (j, j + 30, j + 94, j - 94, s, s + 94, s - 94):
        assert call(dst) == _ffi.RF_E_BADARG, dst - base
        assert b"overlap" in lib.rf_last_error()
    for dst in (j + 95, j - 95, s + 95, s - 95):
        assert call(dst) == _ffi.RF_E_BADARG, dst - base
        assert b"workspace" in lib.rf_last_error()
    # a 3-channel joint ends at byte 285; a 3-channel dst is 285 bytes long
    assert call(j + 284, jcn=3) == _ffi.RF_E_BADARG and b"overlap" in lib.rf_last_error()
    assert call(j + 285, jcn=3) == _ffi.RF_E_BADARG and b"workspace" in lib.rf_last_error()
    assert call(s - 284, scn=3) == _ffi.RF_E_BADARG and b"overlap" in lib.rf_last_error()
    assert call(s - 285, scn=3) == _ffi.RF_E_BADARG and b"workspace" in lib.rf_last_error()


def test_workspace_is_32_bytes_per_64x64_tile(built):
    """No plan has more tiles than the 64x64 tiling (a strip is only taken where it saves
    workgroups), so that count sizes the workspace whatever sigma_color will be."""
    lib = _ffi.load_library()
    size = lib.rf_jbf_ragged_workspace_bytes
    sizes = [(64, 64), (65, 65), (81, 200), (112, 520)]
    assert _tiles64(sizes) == 1 + 4 + 2 * 4 + 2 * 9 == 31
    hs, p_h = _ints([h for h, _ in sizes])
    wsz, p_w = _ints([w for _, w in sizes])
    for jcn, scn, flags in ((1, 1, 0), (1, 1, _ffi.JBF_GREY_AS_BGR), (3, 3, 0), (3, 1, 0)):
        for d, ss in ((-1, 22.0), (-1, 28.0), (-1, 36.0), (9, 1.0), (-1, -5.0)):
            assert size(4, p_h, p_w, jcn, scn, d, ss, flags) == _align256(32 * 31) == 1024
            for n, tiles in ((1, 1), (2, 5), (3, 13)):
                assert size(n, p_h, p_w, jcn, scn, d, ss, flags) == _align256(32 * tiles)
    big_h, p_bh = _ints([341, 512, 384] * 30)
    big_w, p_bw = _ints([512, 341, 512] * 30)
    assert size(90, p_bh, p_bw, 1, 1, -1, 22.0, 0) == _align256(32 * 30 * (6 * 8 + 8 * 6 + 6 * 8))
    assert size(0, p_h, p_w, 1, 1, -1, 22.0, 0) == 0
    # arguments the call refuses
    assert size(-1, p_h, p_w, 1, 1, -1, 22.0, 0) == 0
    assert size(4, None, p_w, 1, 1, -1, 22.0, 0) == 0
    assert size(4, p_h, None, 1, 1, -1, 22.0, 0) == 0
    assert size(4, p_h, p_w, 2, 1, -1, 22.0, 0) == 0
    assert size(4, p_h, p_w, 1, 4, -1, 22.0, 0) == 0
    assert size(4, p_h, p_w, 1, 1, -1, 22.0, 8) == 0
    assert size(4, p_h, p_w, 1, 1, -1, 3000.0, 0) == 0
    zero, p_z = _ints([64, 0, 81, 112])
    assert size(4, zero.ctypes.data, p_w, 1, 1, -1, 22.0, 0) == 0


# ---- the launch plan ---------------------------------------------------------------------------
# Radius 33 (sigma_space 22), single-channel src: row pitch 144 and all four tile classes, as
# {tile rows, tile columns, pitch, tiles}.  By the rules of tile64_areas:
#   64x64    one 64x64 tile.
#   65x65    w % 64 = 1 <= 32 and one 128-row tile covers the 65 rows where 64-row tiles need two:
#            the last column goes to one 128x32 tile; the last row would take a 16x256 tile, no
#            fewer than the one more 64x64 tile - rejected by the cost rule: 2 + 1 tiles.
#   81x200   the last 8 columns go to one 128x32 tile; 192 columns remain; the last 17 rows take
#            two 32x128 tiles against three more 64x64: 1 x 3, 2 and 1.
#   112x520  the last 8 columns go to one 128x32 tile; 512 remain; of the last 48 rows 32 take four
#            32x128 tiles and 16 two 16x256 tiles, 6 against 8 more 64x64: 1 x 8, 4, 2 and 1.
GREY_PLANS = [
    ((64, 64), [(64, 64, 144, 1)]),
    ((65, 65), [(64, 64, 144, 2), (128, 32, 136, 1)]),
    ((81, 200), [(64, 64, 144, 3), (32, 128, 208, 2), (128, 32, 136, 1)]),
    ((112, 520), [(64, 64, 144, 8), (32, 128, 208, 4), (16, 256, 336, 2), (128, 32, 136, 1)]),
]


@pytest.mark.parametrize("jcn,flags", [(1, 0), (1, _ffi.JBF_GREY_AS_BGR), (3, 0)])
def test_plans_at_radius_33_with_a_grey_src(built, jcn, flags):
    for size, plan in GREY_PLANS:
        assert _ffi.jbf_ragged_plan([size], jcn, 1, -1, 20.0, 22.0, flags) == plan, size
    # all four in one call: the sums per class, one launch each
    together = _ffi.jbf_ragged_plan([s for s, _ in GREY_PLANS], jcn, 1, -1, 20.0, 22.0, flags)
    assert together == [(64, 64, 144, 1 + 2 + 3 + 8), (32, 128, 208, 2 + 4), (16, 256, 336, 2),
                        (128, 32, 136, 1 + 1 + 1)]
    # the order of the images does not change the classes or their sizes
    assert _ffi.jbf_ragged_plan([s for s, _ in GREY_PLANS][::-1], jcn, 1, -1, 20.0, 22.0,
                                flags) == together
    # sixteen IIW-like photos: 341x512 is 5 x 8 tiles and four 32x128 tiles for its last 21 rows,
    # 512x341 is 8 x 5 and four 128x32 tiles for its last 21 columns, 384x512 is 6 x 8
    iiw = [(341, 512), (512, 341), (384, 512), (341, 512)] * 4
    plan = _ffi.jbf_ragged_plan(iiw, jcn, 1, -1, 20.0, 22.0, flags)
    assert plan == [(64, 64, 144, 8 * 40 + 4 * 40 + 4 * 48), (32, 128, 208, 8 * 4),
                    (128, 32, 136, 4 * 4)]


def test_a_colour_src_has_no_16_row_and_no_right_strip(built):
    plan = lambda size: _ffi.jbf_ragged_plan([size], 3, 3, -1, 20.0, 22.0)
    assert plan((64, 64)) == [(64, 64, 144, 1)]
    # the last row: one 32x128 tile against two more 64x64
    assert plan((65, 65)) == [(64, 64, 144, 2), (32, 128, 208, 1)]
    # 17 rows left: two 32x128 tiles against four more 64x64; the 8 columns stay with the 64x64 tiles
    assert plan((81, 200)) == [(64, 64, 144, 4), (32, 128, 208, 2)]
    # 48 rows left need both strips: 64x64 tiles alone
    assert plan((112, 520)) == [(64, 64, 144, 2 * 9)]
    assert _ffi.jbf_ragged_plan([(81, 200), (112, 520), (65, 65)], 1, 3, -1, 20.0, 22.0,
                                _ffi.JBF_GREY_AS_BGR) == [(64, 64, 144, 4 + 18 + 2),
                                                          (32, 128, 208, 2 + 1)]


def test_radius_42_runs_64x64_tiles_at_pitch_176(built):
    sizes = [(81, 200), (64, 64), (130, 70)]
    for jcn, scn, flags in ((1, 1, 0), (1, 1, _ffi.JBF_GREY_AS_BGR), (3, 3, 0), (3, 1, 0)):
        assert _ffi.jbf_ragged_plan(sizes, jcn, scn, -1, 15.0, 28.0, flags) == [
            (64, 64, 176, 2 * 4 + 1 + 3 * 2)]
    # d decides the radius when positive: d = 85 is radius 42 whatever sigma_space is
    assert _ffi.jbf_ragged_plan(sizes, 1, 1, 85, 15.0, 3.0) == [(64, 64, 176, 15)]
    assert _ffi.jbf_ragged_plan(sizes, 1, 1, 105, 15.0, 3.0) == [(64, 64, 176, 15)]   # radius 52


def test_the_routes_that_fall_back_to_one_launch_per_image(built):
    sizes = [(70, 90), (1, 1), (64, 64)]
    assert _ffi.jbf_ragged_plan(sizes, 1, 1, -1, 20.0, 36.0) is None          # radius 54: slabs
    assert _ffi.jbf_ragged_plan(sizes, 1, 1, 107, 20.0, 3.0) is None          # radius 53
    assert _ffi.jbf_ragged_plan(sizes, 3, 3, -1, 20.0, 400.0) is None         # generic kernel
    assert _ffi.jbf_ragged_plan(sizes, 1, 1, -1, 20.0, 22.0, _ffi.JBF_FORCE_GENERIC) is None
    assert _ffi.jbf_ragged_plan(sizes, 1, 1, -1, 20.0, 22.0) is not None
    with _ffi.debug_options(jbf_tune=7):
        assert _ffi.jbf_ragged_plan(sizes, 1, 1, -1, 20.0, 22.0) is None
    with _ffi.debug_options(jbf_tile64_only=1):
        assert _ffi.jbf_ragged_plan([(112, 520)], 1, 1, -1, 20.0, 22.0) == [(64, 64, 144, 18)]


def test_the_plan_query_refuses_what_the_entry_refuses(built):
    lib = _ffi.load_library()
    for kw in ({"joint_cn": 2}, {"src_cn": 4}, {"sigma_space": 3000.0}, {"flags": 8}):
        args = dict(sizes=[(8, 8)], joint_cn=1, src_cn=1, d=-1, sigma_color=20.0, sigma_space=22.0)
        args.update(kw)
        with pytest.raises(ValueError):
            _ffi.jbf_ragged_plan(**args)
    with pytest.raises(ValueError):
        _ffi.jbf_ragged_plan([(8, 8), (0, 3)], 1, 1, -1, 20.0, 22.0)
    # -1 is the fall-back too; a refusal's message left behind does not turn one into the other
    assert lib.rf_last_error()
    assert _ffi.jbf_ragged_plan([(8, 8)], 1, 1, -1, 20.0, 36.0) is None
    assert lib.rf_debug_jbf_ragged_plan(0, None, None, 1, 1, -1, 20.0, 36.0, 0, None, 0) \
        == _ffi.RF_E_BADARG
    hs, p_h = _ints([81])
    assert lib.rf_debug_jbf_ragged_plan(1, None, p_h, 1, 1, -1, 20.0, 22.0, 0, None, 0) \
        == _ffi.RF_E_BADARG and lib.rf_last_error()
    # the count alone: out may be NULL when cap is 0; a short cap keeps the first launches
    ws, p_w = _ints([200])
    assert lib.rf_debug_jbf_ragged_plan(1, p_h, p_w, 1, 1, -1, 20.0, 22.0, 0, None, 0) == 3
    out = np.full(8, -7, dtype=np.int32)
    assert lib.rf_debug_jbf_ragged_plan(1, p_h, p_w, 1, 1, -1, 20.0, 22.0, 0, out.ctypes.data,
                                        1) == 3
    assert out.tolist() == [64, 64, 144, 3, -7, -7, -7, -7]
    assert lib.rf_debug_jbf_ragged_plan(1, p_h, p_w, 1, 1, -1, 20.0, 22.0, 0, None, 2) \
        == _ffi.RF_E_BADARG


# ---- filter_reflectance.apply_filter_list: the host side -------------------------------------------

class _Img(object):
    """Stands for a device image: a shape and an id."""

    def __init__(self, shape, ident):
        self.shape, self.ident = shape, ident


@pytest.mark.parametrize("shapes", [
    [(5, 9), (9, 5), (5, 9), (6, 8), (9, 5), (5, 9), (6, 8)],
    # photo sizes: a group is cut by bytes (1 GiB), which these are far from - 341 x 512 x 1 x 3
    # is half a megabyte per image
    [(341, 512), (512, 341), (341, 512), (384, 512), (512, 341), (341, 512), (384, 512)],
])
def test_guided_lists_are_grouped_by_shape_and_return_in_the_callers_order(monkeypatch, shapes):
    imgs = [_Img((h, w, 1), i) for i, (h, w) in enumerate(shapes)]
    guides = [_Img((h, w, 3), 100 + i) for i, (h, w) in enumerate(shapes)]
    calls = []

    def fake_batch(filter_type, images, joints, sigma_color, sigma_spatial, iterations=1,
                   grey_as_bgr=False):
        assert filter_type == "guided" and (sigma_color, sigma_spatial, iterations) == (3, 45, 3)
        assert [j.ident for j in joints] == [100 + im.ident for im in images]
        assert len(set(im.shape for im in images)) == 1
        calls.append([im.ident for im in images])
        return ["filtered %d" % im.ident for im in images]

    monkeypatch.setattr(fr, "apply_filter_batch", fake_batch)
    monkeypatch.setattr(fr, "_stack", lambda images: list(images))
    monkeypatch.setattr(fr._ffi, "require_gpu", lambda: None)
    out = fr.apply_filter_list("guided", imgs, guides, 3, 45, iterations=3)
    assert sorted(calls) == [[0, 2, 5], [1, 4], [3, 6]]          # three batches, not seven runs
    assert out == ["filtered %d" % i for i in range(7)]


def test_a_self_guided_bilateral_list_is_packed_once(monkeypatch):
    """images is joints: one pack serves as joint and src of the first pass, and stays the joint of
    the later ones; a generator given as both is read once."""
    packs, calls = [], []

    class FakeTorch(object):
        @staticmethod
        def empty_like(t):
            return "buffer"

    def fake_pack(images, name, torch):
        packs.append(name)
        return "pack of %s" % name, [im.shape[:2] for im in images]

    def fake_ragged(joint, src, d, sc, ss, grey_as_bgr=False, sizes=None, out=None):
        calls.append((joint, src))
        return "pass %d" % len(calls), ["view"] * len(sizes)

    monkeypatch.setattr(fr._ffi, "require_gpu", lambda: FakeTorch)
    monkeypatch.setattr(fr.ops, "pack_images", fake_pack)
    monkeypatch.setattr(fr.ops, "joint_bilateral_ragged_u8", fake_ragged)
    imgs = [_Img((5, 9, 1), 0), _Img((9, 5, 1), 1)]
    assert fr.apply_filter_list("bilateral", imgs, imgs, 20, 22, iterations=2) == ["view"] * 2
    assert packs == ["images"]
    assert calls == [("pack of images", "pack of images"), ("pack of images", "pass 1")]
    del packs[:], calls[:]
    gen = (im for im in imgs)
    assert len(fr.apply_filter_list("bilateral", gen, gen, 20, 22)) == 2
    assert packs == ["images"] and calls == [("pack of images", "pack of images")]
    del packs[:], calls[:]
    fr.apply_filter_list("bilateral", imgs, list(imgs), 20, 22)
    assert packs == ["images", "joints"] and calls == [("pack of joints", "pack of images")]


def test_list_arguments_are_checked_before_any_device_work(monkeypatch):
    def no_device():
        raise AssertionError("device work before the arguments were checked")

    monkeypatch.setattr(fr._ffi, "require_gpu", no_device)
    a, b = _Img((5, 9, 1), 0), _Img((9, 5, 1), 1)
    for ftype in ("bilateral", "guided"):
        with pytest.raises(ValueError):
            fr.apply_filter_list(ftype, [a, b], [a, b], 20, 22, iterations=0)
        with pytest.raises(ValueError):
            fr.apply_filter_list(ftype, [a, b], [a, b], 20, 22, iterations=-1)
        with pytest.raises(ValueError):
            fr.apply_filter_list(ftype, [a, b], [b, a], 20, 22)       # sizes differ image by image
        with pytest.raises(ValueError):
            fr.apply_filter_list(ftype, [a, b], [a], 20, 22)          # lengths differ
        with pytest.raises(ValueError):
            fr.apply_filter_list(ftype, [a, b], [a, b], 0, 22)        # the reference's parameter rule
        assert fr.apply_filter_list(ftype, [], [], 20, 22) == []
    with pytest.raises(ValueError):
        fr.apply_filter_list("median", [a], [a], 20, 22)
