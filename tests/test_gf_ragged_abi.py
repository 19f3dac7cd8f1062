"""CPU suite: the ragged guided filter (rf_gf_ragged_u8: images of different sizes packed one after
another; a one-channel src at radius 1..128 runs stage 1, the row walk and the column walk once per
pass over all images) - refusals before any GPU work, the workspace size and the launch plan against
figures worked out by hand from kSB = 16, kBRows = 64 and the strip rule of rf_gf.hip, and the host
logic of filter_reflectance.apply_filter_list("guided").  No compute calls."""
import ctypes

import numpy as np
import pytest

from reflectance_filtering_amd import _ffi
from reflectance_filtering_amd import filter_reflectance as fr

GREY = _ffi.GF_GREY_AS_BGR


def _ints(values):
    a = np.ascontiguousarray(values, dtype=np.int32)
    return a, a.ctypes.data


def _align256(b):
    return (b + 255) & ~255


def _cdiv(a, b):
    return -(-a // b)


def test_exports_are_declared(built):
    assert "rf_gf_ragged_workspace_bytes" in _ffi.EXPORTS and "rf_gf_ragged_u8" in _ffi.EXPORTS
    assert "rf_debug_gf_ragged_plan" in _ffi.DEBUG_EXPORTS
    lib = _ffi.load_library()
    for name in ("rf_gf_ragged_workspace_bytes", "rf_gf_ragged_u8", "rf_debug_gf_ragged_plan"):
        getattr(lib, name)


def test_ragged_refusals_need_no_gpu(built):
    lib = _ffi.load_library()
    buf = ctypes.create_string_buffer(1 << 16)
    base = (ctypes.addressof(buf) + 255) & ~255
    g, s, o, ws = base, base + 4096, base + 8192, base + 16384
    hs, p_h = _ints([8, 3, 5])
    wsz, p_w = _ints([8, 7, 2])                                # 64 + 21 + 10 = 95 pixels
    ws_need = lib.rf_gf_ragged_workspace_bytes(3, p_h, p_w, 1, 1, 9, GREY)
    assert ws_need > 0

    def call(guide=g, src=s, dst=o, n=3, ph=p_h, pw=p_w, gcn=1, scn=1, radius=9, eps=3.0, it=1,
             flags=GREY, w=ws, ws_bytes=ws_need - 1):
        # the workspace is one byte short: a call that passes every other check is refused for it
        return lib.rf_gf_ragged_u8(guide, src, dst, n, ph, pw, gcn, scn, radius, eps, it, flags, w,
                                   ws_bytes, None)

    assert call(guide=None) == _ffi.RF_E_BADARG
    assert b"NULL" in lib.rf_last_error() and b"rf_gf_ragged_u8" in lib.rf_last_error()
    for kw in ({"src": None}, {"dst": None}, {"ph": None}, {"pw": None}):
        assert call(**kw) == _ffi.RF_E_BADARG, kw
        assert b"NULL" in lib.rf_last_error()
    # an empty list is valid whatever the pointers are
    assert call(n=0, guide=None, src=None, dst=None, ph=None, pw=None, w=None) == _ffi.RF_OK
    assert call(n=-1) == _ffi.RF_E_BADARG
    for bad_h, bad_w in (([8, 0, 5], [8, 7, 2]), ([8, 3, 5], [8, 7, 0]), ([8, 3, -5], [8, 7, 2]),
                         ([8, 3, 5], [-8, 7, 2])):
        a, p_a = _ints(bad_h)
        b, p_b = _ints(bad_w)
        assert call(ph=p_a, pw=p_b) == _ffi.RF_E_BADARG, (bad_h, bad_w)
        assert b"size" in lib.rf_last_error()
    assert call(it=0) == _ffi.RF_E_BADARG
    # the guide's channels and the flag, as rf_gf_ex_u8
    assert call(gcn=1, flags=0) == _ffi.RF_E_UNSUPPORTED
    assert b"guide" in lib.rf_last_error()
    assert call(gcn=3, flags=GREY) == _ffi.RF_E_BADARG
    assert b"RF_GF_GREY_AS_BGR" in lib.rf_last_error()
    assert call(scn=2) == _ffi.RF_E_UNSUPPORTED
    assert b"src channels" in lib.rf_last_error()
    assert call(radius=-1) == _ffi.RF_E_UNSUPPORTED
    assert call(radius=4097) == _ffi.RF_E_UNSUPPORTED
    assert b"radius" in lib.rf_last_error()
    assert call(flags=GREY | 2) == _ffi.RF_E_BADARG
    assert b"flag" in lib.rf_last_error() and b"rf_gf_ragged_u8" in lib.rf_last_error()
    assert call(flags=0x1000) == _ffi.RF_E_BADARG
    # the debug options rf_gf_ex_u8 refuses with a grey guide
    for opt in ("gf_guide_cache", "gf_exact"):
        with _ffi.debug_options(**{opt: 1}):
            assert call() == _ffi.RF_E_UNSUPPORTED, opt
            assert b"debug option" in lib.rf_last_error()
    # the small workspace itself, a missing and a misaligned one
    assert call() == _ffi.RF_E_BADARG
    assert b"workspace" in lib.rf_last_error() and b"rf_gf_ragged_u8" in lib.rf_last_error()
    assert call(ws_bytes=0) == _ffi.RF_E_BADARG
    assert call(w=None, ws_bytes=1 << 20) == _ffi.RF_E_BADARG
    assert call(w=ws + 8, ws_bytes=1 << 20) == _ffi.RF_E_BADARG
    assert b"workspace" in lib.rf_last_error()
    # ... also where the call would fall back to one rf_gf_ex_u8 call per image
    for kw in ({"radius": 0}, {"radius": 129}):
        need = lib.rf_gf_ragged_workspace_bytes(3, p_h, p_w, 1, 1, kw["radius"], GREY)
        assert need > 0
        assert call(ws_bytes=need - 1, **kw) == _ffi.RF_E_BADARG, kw
        assert b"workspace" in lib.rf_last_error()


def test_ragged_overlap_is_judged_on_the_summed_pixel_count(built):
    """95 pixels in images of 64, 21 and 10: dst overlaps the guide up to byte 94 and is clear of it at
    byte 95 - beyond n*h*w of the last image (30), short of that of the first (192).  dst may BE src
    but not overlap it partially; the guide may be the src."""
    lib = _ffi.load_library()
    buf = ctypes.create_string_buffer(1 << 16)
    base = ctypes.addressof(buf)
    g, s = base + 4096, base + 8192
    hs, p_h = _ints([8, 3, 5])
    wsz, p_w = _ints([8, 7, 2])

    def call(dst, gcn=1, scn=1, guide=g, src=s):
        # a NULL workspace: a call that passes the overlap check is refused for it right after
        return lib.rf_gf_ragged_u8(guide, src, dst, 3, p_h, p_w, gcn, scn, 9, 3.0, 1,
                                   GREY if gcn == 1 else 0, None, 0, None)

    for dst in (g, g + 30, g + 94, g - 94, s + 1, s + 94, s - 94):
        assert call(dst) == _ffi.RF_E_BADARG, dst - base
        assert b"overlap" in lib.rf_last_error()
    for dst in (g + 95, g - 95, s + 95, s - 95, s):
        assert call(dst) == _ffi.RF_E_BADARG, dst - base
        assert b"workspace" in lib.rf_last_error()
    # a 3-channel guide ends at byte 285; a 3-channel dst is 285 bytes long
    assert call(g + 284, gcn=3) == _ffi.RF_E_BADARG and b"overlap" in lib.rf_last_error()
    assert call(g + 285, gcn=3) == _ffi.RF_E_BADARG and b"workspace" in lib.rf_last_error()
    assert call(s - 284, scn=3) == _ffi.RF_E_BADARG and b"overlap" in lib.rf_last_error()
    assert call(s - 285, scn=3) == _ffi.RF_E_BADARG and b"workspace" in lib.rf_last_error()
    # self-guided: guide == src passes the overlap rules; dst == guide does not
    assert call(g + 200, guide=s, src=s) == _ffi.RF_E_BADARG and b"workspace" in lib.rf_last_error()
    assert call(s, guide=s, src=s) == _ffi.RF_E_BADARG and b"overlap" in lib.rf_last_error()


# ---- workspace and plan, by hand -----------------------------------------------------------------
# Stage-1 strips are 256 threads x 3 columns = 768 columns including the halo.  Radius 52: left halo
# 64 and 640 output columns (a whole wave either side); radius 128: halo 128, (768 - 128 - 128) = 512
# output columns.  Row walk: one workgroup per 64 rows (kBRows).  Column walk: one workgroup per 16
# columns (kSB), dealt to 8 XCDs in equal runs, i.e. 8 x ceil(blocks / 8) workgroups.
LIST52 = [(100, 700), (64, 64), (130, 17)]        # strips at radius 52: 2, 1, 1
LIST128 = [(100, 600), (64, 64), (130, 17)]       # strips at radius 128: 2, 1, 1


def _by_hand(sizes, out_w, s1_items):
    rs = sum(_cdiv(h, 64) for h, _ in sizes)
    blocks = sum(_cdiv(w, 16) for _, w in sizes)
    cw = 8 * _cdiv(blocks, 8)
    table = _align256(48 * len(sizes) + 16 * (s1_items + rs + cw))
    states = sum(8 * 4 * _cdiv(w, 16) * h for h, w in sizes)
    ab = 16 * sum(h * w for h, w in sizes)
    return rs, cw, table + states + ab


@pytest.mark.parametrize("sizes,radius,out_w,hl", [(LIST52, 52, 640, 64), (LIST128, 128, 512, 128)])
@pytest.mark.parametrize("gcn,flags", [(1, GREY), (3, 0)])
def test_workspace_and_grids_of_a_three_image_list(built, sizes, radius, out_w, hl, gcn, flags):
    lib = _ffi.load_library()
    hs, p_h = _ints([h for h, _ in sizes])
    wsz, p_w = _ints([w for _, w in sizes])
    strips = [_cdiv(w, out_w) for _, w in sizes]
    assert strips == [2, 1, 1]
    # rows per segment = the whole image ("gf_seg_rows" beyond every height): one item per strip
    with _ffi.debug_options(gf_seg_rows=1 << 20):
        rs, cw, need = _by_hand(sizes, out_w, sum(strips))
        assert (rs, cw) == (2 + 1 + 3, 8 * _cdiv(_cdiv(sizes[0][1], 16) + 4 + 2, 8))
        assert lib.rf_gf_ragged_workspace_bytes(3, p_h, p_w, gcn, 1, radius, flags) == need
        plan = _ffi.gf_ragged_plan(sizes, gcn, 1, radius, flags)
        assert plan == {"launches": 3, "stage1": 4, "rowstate": rs, "colwalk": cw, "hl": hl,
                        "out_w": out_w}
    # the library's segment rule: whole segments of every strip, the rest of the figures unchanged
    plan = _ffi.gf_ragged_plan(sizes, gcn, 1, radius, flags)
    assert plan["launches"] == 3 and (plan["rowstate"], plan["colwalk"]) == (rs, cw)
    assert (plan["hl"], plan["out_w"]) == (hl, out_w)
    assert plan["stage1"] >= 4 and plan["stage1"] <= 2 * 100 + 64 + 130
    assert lib.rf_gf_ragged_workspace_bytes(3, p_h, p_w, gcn, 1, radius, flags) \
        == _by_hand(sizes, out_w, plan["stage1"])[2]
    # one segment row: as many items as strips x rows
    with _ffi.debug_options(gf_seg_rows=1):
        assert _ffi.gf_ragged_plan(sizes, gcn, 1, radius, flags)["stage1"] == 2 * 100 + 64 + 130


def test_three_launches_per_pass_whatever_n_is(built):
    iiw = [(341, 512), (512, 341), (384, 512), (341, 512)]
    for n in (1, 2, 4, 64):
        sizes = (iiw * 16)[:n]
        plan = _ffi.gf_ragged_plan(sizes, 1, 1, 52, GREY)
        assert plan["launches"] == 3
        assert plan["rowstate"] == sum(_cdiv(h, 64) for h, _ in sizes)
        assert plan["colwalk"] == 8 * _cdiv(sum(_cdiv(w, 16) for _, w in sizes), 8)
    # a narrow halo where it saves the list a strip: radius 9 takes 16 + 736 columns for a 700-column
    # image (one strip instead of two), the whole-wave halo of 640 where every image fits either way
    assert _ffi.gf_ragged_plan([(9, 700), (64, 64)], 3, 1, 9)["out_w"] == 736
    assert _ffi.gf_ragged_plan([(9, 600), (64, 64)], 3, 1, 9)["out_w"] == 640


def test_the_fallback_route_and_its_workspace(built):
    lib = _ffi.load_library()
    sizes = [(70, 90), (130, 200), (64, 64)]
    hs, p_h = _ints([h for h, _ in sizes])
    wsz, p_w = _ints([w for _, w in sizes])
    assert _ffi.gf_ragged_plan(sizes, 3, 1, 52) is not None
    for gcn, scn, radius, flags in ((3, 3, 52, 0), (1, 3, 52, GREY), (3, 1, 0, 0), (3, 1, 129, 0),
                                    (1, 1, 129, GREY), (3, 3, 129, 0)):
        assert _ffi.gf_ragged_plan(sizes, gcn, scn, radius, flags) is None, (gcn, scn, radius)
        largest = max(lib.rf_gf_workspace_bytes(1, h, w, gcn, scn, radius) for h, w in sizes)
        assert largest == lib.rf_gf_workspace_bytes(1, 130, 200, gcn, scn, radius)
        assert lib.rf_gf_ragged_workspace_bytes(3, p_h, p_w, gcn, scn, radius, flags) == largest
    for opt in ("gf_two_kernel", "gf_chained"):
        with _ffi.debug_options(**{opt: 1}):
            assert _ffi.gf_ragged_plan(sizes, 3, 1, 52) is None, opt
    with _ffi.debug_options(gf_exact=1, gf_guide_cache=1):
        assert _ffi.gf_ragged_plan(sizes, 3, 1, 52) is None
    assert _ffi.gf_ragged_plan([], 3, 1, 52) is None           # an empty list launches nothing


def test_size_and_plan_queries_refuse_what_the_entry_refuses(built):
    lib = _ffi.load_library()
    size = lib.rf_gf_ragged_workspace_bytes
    hs, p_h = _ints([8, 3])
    wsz, p_w = _ints([8, 7])
    assert size(2, p_h, p_w, 3, 1, 9, 0) > 0
    assert size(0, p_h, p_w, 3, 1, 9, 0) == 0
    assert size(-1, p_h, p_w, 3, 1, 9, 0) == 0
    assert size(2, None, p_w, 3, 1, 9, 0) == 0
    assert size(2, p_h, None, 3, 1, 9, 0) == 0
    assert size(2, p_h, p_w, 1, 1, 9, 0) == 0
    assert size(2, p_h, p_w, 3, 1, 9, GREY) == 0
    assert size(2, p_h, p_w, 3, 2, 9, 0) == 0
    assert size(2, p_h, p_w, 3, 1, -1, 0) == 0
    assert size(2, p_h, p_w, 3, 1, 4097, 0) == 0
    assert size(2, p_h, p_w, 3, 1, 9, 4) == 0
    zero, p_z = _ints([8, 0])
    assert size(2, p_z, p_w, 3, 1, 9, 0) == 0
    for kw in ({"guide_cn": 1}, {"src_cn": 2}, {"radius": 4097}, {"radius": -1}, {"flags": 4},
               {"sizes": [(8, 8), (0, 3)]}):
        args = dict(sizes=[(8, 8)], guide_cn=3, src_cn=1, radius=9, flags=0)
        args.update(kw)
        with pytest.raises(ValueError):
            _ffi.gf_ragged_plan(**args)
    # out may be NULL when cap is 0; a short cap keeps the first ints; a bad cap is refused
    assert lib.rf_debug_gf_ragged_plan(2, p_h, p_w, 3, 1, 9, 0, None, 0) == 1
    out = np.full(6, -7, dtype=np.int32)
    assert lib.rf_debug_gf_ragged_plan(2, p_h, p_w, 3, 1, 9, 0, out.ctypes.data, 2) == 1
    assert out[0] == 3 and out[1] >= 2 and out[2:].tolist() == [-7] * 4
    assert lib.rf_debug_gf_ragged_plan(2, p_h, p_w, 3, 1, 9, 0, None, 2) == _ffi.RF_E_BADARG


# ---- filter_reflectance.apply_filter_list("guided"): the host side ----------------------------------

class _Img(object):
    """Stands for a device image: a shape, an id and a device."""
    device = "dev"
    is_cuda = True

    def __init__(self, shape, ident):
        self.shape, self.ident = shape, ident


def _stub(monkeypatch, ragged, batches, cap=1 << 40):
    def fake_ragged(guides, srcs, radius, eps, iterations=1, grey_as_bgr=False, sizes=None, out=None):
        ragged.append(([g.ident for g in guides], [s.ident for s in srcs], radius, eps, iterations,
                       grey_as_bgr, guides is srcs))
        return "packed", ["ragged %d" % s.ident for s in srcs]

    def fake_batch(filter_type, images, joints, sigma_color, sigma_spatial, iterations=1,
                   grey_as_bgr=False):
        assert len(set(im.shape for im in images)) == 1
        batches.append([im.ident for im in images])
        return ["batch %d" % im.ident for im in images]

    monkeypatch.setattr(fr.ops, "guided_filter_ragged_u8", fake_ragged)
    monkeypatch.setattr(fr.ops, "gf_workspace_cap", lambda device, torch: cap)
    monkeypatch.setattr(fr, "apply_filter_batch", fake_batch)
    monkeypatch.setattr(fr, "_stack", lambda images: list(images))
    monkeypatch.setattr(fr._ffi, "require_gpu", lambda: None)


SHAPES = [(341, 512), (512, 341), (341, 512), (384, 512), (512, 341)]


def test_a_mixed_one_channel_list_goes_ragged_in_one_call(monkeypatch):
    ragged, batches = [], []
    _stub(monkeypatch, ragged, batches)
    imgs = [_Img((h, w, 1), i) for i, (h, w) in enumerate(SHAPES)]
    guides = [_Img((h, w, 3), 100 + i) for i, (h, w) in enumerate(SHAPES)]
    out = fr.apply_filter_list("guided", imgs, guides, 3, 45.9, iterations=3)
    assert out == ["ragged %d" % i for i in range(5)] and not batches
    assert ragged == [([100, 101, 102, 103, 104], [0, 1, 2, 3, 4], 45, 3, 3, False, False)]
    # self-guided (GF(CNN, CNN)): one list serves as guide and src
    del ragged[:]
    out = fr.apply_filter_list("guided", imgs, imgs, 7, 52, grey_as_bgr=True)
    assert ragged == [([0, 1, 2, 3, 4], [0, 1, 2, 3, 4], 52, 7, 1, True, True)] and not batches
    for radius in (1, 128):
        del ragged[:]
        fr.apply_filter_list("guided", imgs, guides, 3, radius)
        assert len(ragged) == 1 and ragged[0][2] == radius and not batches


def test_every_other_guided_list_keeps_the_shape_groups(monkeypatch):
    ragged, batches = [], []
    _stub(monkeypatch, ragged, batches)
    guides = [_Img((h, w, 3), 100 + i) for i, (h, w) in enumerate(SHAPES)]
    one = [_Img((h, w, 1), i) for i, (h, w) in enumerate(SHAPES)]
    three = [_Img((h, w, 3), i) for i, (h, w) in enumerate(SHAPES)]
    # a three-channel src
    assert fr.apply_filter_list("guided", three, guides, 3, 45) == ["batch %d" % i for i in range(5)]
    assert sorted(batches) == [[0, 2], [1, 4], [3]] and not ragged
    # radius 129 and radius 0 (int(0.5))
    for sigma in (129, 129.9, 0.5):
        del batches[:]
        fr.apply_filter_list("guided", one, guides, 3, sigma)
        assert sorted(batches) == [[0, 2], [1, 4], [3]] and not ragged, sigma
    # images that are not device tensors (nothing to pack): the stacked batches take them as before
    del batches[:]
    host_img = type("HostImg", (_Img,), {"is_cuda": False})
    fr.apply_filter_list("guided", [host_img((h, w, 1), i) for i, (h, w) in enumerate(SHAPES)], guides, 3, 45)
    assert sorted(batches) == [[0, 2], [1, 4], [3]] and not ragged
    # one shape
    del batches[:]
    same = [_Img((341, 512, 1), i) for i in range(4)]
    fr.apply_filter_list("guided", same, [_Img((341, 512, 3), 100 + i) for i in range(4)], 3, 45)
    assert batches == [[0, 1, 2, 3]] and not ragged


def test_a_long_list_is_split_into_packs(monkeypatch):
    ragged, batches = [], []
    _stub(monkeypatch, ragged, batches)
    imgs = [_Img((h, w, 1), i) for i, (h, w) in enumerate(SHAPES)]
    # the byte cap: 341 x 512 = 512 x 341 = 174592, 384 x 512 = 196608 bytes; 400000 holds two images
    monkeypatch.setattr(fr, "GF_RAGGED_MAX_BYTES", 400000)
    out = fr.apply_filter_list("guided", imgs, imgs, 7, 52, grey_as_bgr=True)
    assert [r[1] for r in ragged] == [[0, 1], [2, 3], [4]]
    assert all(r[0] == r[1] for r in ragged)
    assert out == ["ragged %d" % i for i in range(5)]
    assert fr.guided_ragged_packs(SHAPES, 2 * 174592, 1 << 40) == [[0, 1], [2], [3], [4]]
    assert fr.guided_ragged_packs(SHAPES, 1, 1 << 40) == [[0], [1], [2], [3], [4]]
    assert fr.guided_ragged_packs(SHAPES, 1 << 30, 1 << 40) == [[0, 1, 2, 3, 4]]
    # the workspace cap: an image of 341 x 512 needs 16 B/px of alpha/beta + 32 B x 32 blocks x 341 rows
    # of states + records = 3.2 MB; 7 MB hold two of them
    assert fr.guided_ragged_packs(SHAPES, 1 << 30, 7 << 20) == [[0, 1], [2, 3], [4]]
    # ... and the bound is one: the library asks for no more than the bound of a pack
    lib = _ffi.load_library()
    for radius in (1, 52, 128):
        hs, p_h = _ints([h for h, _ in SHAPES])
        wsz, p_w = _ints([w for _, w in SHAPES])
        need = lib.rf_gf_ragged_workspace_bytes(5, p_h, p_w, 1, 1, radius, GREY)
        bound = 256 + sum(48 + 16 * (_cdiv(w, 512) * h + _cdiv(h, 64) + _cdiv(w, 16) + 8)
                          + 32 * _cdiv(w, 16) * h + 16 * h * w for h, w in SHAPES)
        assert 0 < need <= bound
        assert fr.guided_ragged_packs(SHAPES, 1 << 30, bound) == [[0, 1, 2, 3, 4]]
        assert len(fr.guided_ragged_packs(SHAPES, 1 << 30, bound - 1)) == 2
