"""CPU suite: the slab launch of the ragged joint bilateral (rf_jbf_ragged_u8 at radius 53..468:
every image's 64x64 tiles in one launch of jbf_slab_kernel) as rf_debug_jbf_ragged_slab_plan
reports it - plans worked out by hand from the arithmetic of slab_fits (rf_jbf.hip), the routes
that do not take the launch, and the refusals.  No compute calls.

The arithmetic.  r4 = the radius rounded up to 4; the pitch is the narrowest of
    208 (r4 <= 68), 240 (84), 272 (100), 304 (116), 336 (132), 400 (164), 496 (212), 624 (276),
    816 (372), 1008 (468).
The LDS holds 163,840 bytes: 16 for the flag word, the colour LUT's nz entries before its zero tail
`rep` times as 4-byte floats at the end, rows of `pitch` texels of 4 bytes (grey src, grey tile) or 6
bytes (colour tile) between them:
    rows(rep, bytes) = (163,840 - 16 - 4 nz rep) // (pitch bytes)
A band of crows = 64 output rows needs rows - 63 >= 24 rows for a slab, a band of 32 needs
rows - 31 >= 24, a band of 16 needs rows - 15 >= 8; the first that holds is taken and
slab = min(rows - crows + 1, 2 radius + 1).  16 LUT replicas unless 8 give a taller band; the
6-byte rows are fitted beside the replicas chosen for the 4-byte ones (crows_c = 0: no band fits).

nz: the LUT entry exp(-i^2 / (2 sigma_color^2)) is 0 in float32 from i > sigma_color sqrt(2 ln 2^150)
= 14.42 sigma_color on.  A 3-channel joint (or GREY_AS_BGR) has 768 entries: sigma_color 20 -> the
first zero is entry 289, nz = 289; sigma_color 100 -> 1442 > 767, no zero, nz = 768.  A 1-channel
joint has 256 entries: sigma_color 20 -> nz = 256.
    free(nz 289, 16 replicas) = 163,824 - 18,496 = 145,328      free(289, 8) = 154,576
    free(nz 768, 16 replicas) = 163,824 - 49,152 = 114,672      free(768, 8) = 139,248
    free(nz 256, 16 replicas) = 163,824 - 16,384 = 147,440
"""
import numpy as np
import pytest

from reflectance_filtering_amd import _ffi


def _ints(values):
    a = np.ascontiguousarray(values, dtype=np.int32)
    return a, a.ctypes.data


def _nz(sigma_color, cn):
    lut = np.exp(np.arange(256 * cn, dtype=np.float64) ** 2 * (-0.5 / sigma_color ** 2)).astype(np.float32)
    zeros = np.flatnonzero(lut == 0)
    return int(zeros[0]) if zeros.size else 256 * cn


def test_the_lut_lengths_the_derivations_start_from():
    assert (_nz(20.0, 3), _nz(100.0, 3), _nz(20.0, 1)) == (289, 768, 256)
    assert 163824 - 4 * 289 * 16 == 145328 and 163824 - 4 * 289 * 8 == 154576
    assert 163824 - 4 * 768 * 16 == 114672 and 163824 - 4 * 768 * 8 == 139248
    assert 163824 - 4 * 256 * 16 == 147440


ONE = [(64, 64)]     # one tile: the shape does not depend on the sizes

# (d, sigma_space, radius), grey src, 3-channel joint, sigma_color 20 (nz 289):
# {pitch, replicas, crows_g, slab_g, 0, 0, tiles}
#   radius 54   r4 56 -> 208; 145,328 // 832 = 174 rows; 174 - 63 = 111 >= 24: band 64,
#               slab min(111, 109) = 109 - the whole disk in one slab.  8 replicas: no taller band.
#   radius 70   (sigma 47: 70.5 rounds to even) r4 72 -> 240; 145,328 // 960 = 151; slab 88 of 141
#   radius 99   r4 100 -> 272; 145,328 // 1088 = 133; slab 70
#   radius 132  r4 132 -> 336; 145,328 // 1344 = 108; slab 45
#   radius 150  r4 152 -> 400; 145,328 // 1600 = 90; slab 27
#   radius 373  r4 376 -> 1008; 145,328 // 4032 = 36: 36 - 63 and 36 - 31 = 5 are no slab; band 16,
#               slab 21.  8 replicas: 154,576 // 4032 = 38, 38 - 31 = 7: band 16 as well -> 16 stay
#   radius 468  r4 468 -> 1008, the same rows: the last radius of the route
GREY = [
    ((-1, 36.0, 54), (208, 16, 64, 109, 0, 0, 1)),
    ((-1, 47.0, 70), (240, 16, 64, 88, 0, 0, 1)),
    ((-1, 66.0, 99), (272, 16, 64, 70, 0, 0, 1)),
    ((-1, 88.0, 132), (336, 16, 64, 45, 0, 0, 1)),
    ((-1, 100.0, 150), (400, 16, 64, 27, 0, 0, 1)),
    ((747, 3.0, 373), (1008, 16, 16, 21, 0, 0, 1)),
    ((937, 3.0, 468), (1008, 16, 16, 21, 0, 0, 1)),
]


@pytest.mark.parametrize("case,want", GREY, ids=["r%d" % c[0][2] for c in GREY])
def test_hand_computed_plans_of_a_grey_src(built, case, want):
    d, ss, radius = case
    assert radius == (d // 2 if d > 0 else int(np.rint(1.5 * ss)))
    assert _ffi.jbf_ragged_slab_plan(ONE, 3, 1, d, 20.0, ss) == want
    # GREY_AS_BGR: the tables of three channels
    assert _ffi.jbf_ragged_slab_plan(ONE, 1, 1, d, 20.0, ss, _ffi.JBF_GREY_AS_BGR) == want


def test_a_single_channel_joint_has_the_256_entry_table(built):
    # nz 256: 147,440 // 832 = 177 rows at radius 54: the slab is the whole disk all the same;
    # radius 99: 147,440 // 1088 = 135, slab 72 where the 3-channel table leaves 70
    assert _ffi.jbf_ragged_slab_plan(ONE, 1, 1, -1, 20.0, 36.0) == (208, 16, 64, 109, 0, 0, 1)
    assert _ffi.jbf_ragged_slab_plan(ONE, 1, 1, -1, 20.0, 66.0) == (272, 16, 64, 72, 0, 0, 1)


def test_eight_lut_replicas_where_they_give_a_taller_band(built):
    # radius 150 (pitch 400) with the full 768-entry table of sigma_color 100: 16 replicas leave
    # 114,672 // 1600 = 71 rows, 71 - 63 = 8 < 24: band 32 (slab 40); 8 replicas leave
    # 139,248 // 1600 = 87, 87 - 63 = 24: band 64, slab 24 -> 8 replicas
    assert _ffi.jbf_ragged_slab_plan(ONE, 3, 1, -1, 100.0, 100.0) == (400, 8, 64, 24, 0, 0, 1)
    # a colour src beside the same 8 replicas: 139,248 // 2400 = 58: 58 - 31 = 27 -> band 32, slab 27
    assert _ffi.jbf_ragged_slab_plan(ONE, 3, 3, -1, 100.0, 100.0) == (400, 8, 64, 24, 32, 27, 1)


def test_hand_computed_plans_of_a_colour_src(built):
    """6-byte texels beside the replicas of the 4-byte plan (16, nz 289: 145,328 bytes)."""
    plan = lambda d, ss, sc=20.0: _ffi.jbf_ragged_slab_plan(ONE, 3, 3, d, sc, ss)
    # radius 54: 145,328 // 1248 = 116; 116 - 63 = 53: the colour plane fits in bands of 64
    assert plan(-1, 36.0) == (208, 16, 64, 109, 64, 53, 1)
    # radius 70: 145,328 // 1440 = 100 -> slab 37; radius 99: 145,328 // 1632 = 89 -> slab 26
    assert plan(-1, 47.0) == (240, 16, 64, 88, 64, 37, 1)
    assert plan(-1, 66.0) == (272, 16, 64, 70, 64, 26, 1)
    # radius 132: 145,328 // 2016 = 72; 72 - 63 = 9 < 24: bands of 32, slab 41
    assert plan(-1, 88.0) == (336, 16, 64, 45, 32, 41, 1)
    # radius 150: 145,328 // 2400 = 60: bands of 32, slab 29
    assert plan(-1, 100.0) == (400, 16, 64, 27, 32, 29, 1)
    # radius 373 at pitch 1008: 145,328 // 6048 = 24; 24 - 15 = 9 >= 8: bands of 16, slab 9
    assert plan(747, 3.0) == (1008, 16, 16, 21, 16, 9, 1)
    # ... and with the 768-entry table of sigma_color 100: 4-byte rows 114,672 // 4032 = 28 -> band 16,
    # slab 13 (8 replicas: 139,248 // 4032 = 34, 34 - 31 = 3: band 16 too, so 16 stay);
    # 6-byte rows 114,672 // 6048 = 18, 18 - 15 = 3 < 8: the colour plane does NOT fit - crows_c = 0,
    # one grey pass per channel
    assert plan(747, 3.0, 100.0) == (1008, 16, 16, 13, 0, 0, 1)
    # a grey src never has a colour plane
    assert _ffi.jbf_ragged_slab_plan(ONE, 3, 1, 747, 100.0, 3.0) == (1008, 16, 16, 13, 0, 0, 1)


def test_tiles_are_the_64x64_tiles_of_every_image(built):
    sizes = [(1, 1), (3, 200), (64, 64), (65, 65), (40, 130), (130, 40), (341, 512), (512, 341)]
    tiles = 1 + 4 + 1 + 4 + 3 + 3 + 6 * 8 + 8 * 6
    assert tiles == sum(-(-h // 64) * -(-w // 64) for h, w in sizes) == 112
    for jcn, scn, flags in ((1, 1, _ffi.JBF_GREY_AS_BGR), (3, 3, 0), (3, 1, 0)):
        plan = _ffi.jbf_ragged_slab_plan(sizes, jcn, scn, -1, 20.0, 36.0, flags)
        assert plan[:4] == (208, 16, 64, 109) and plan[6] == tiles
        assert _ffi.jbf_ragged_slab_plan(sizes[::-1], jcn, scn, -1, 20.0, 36.0, flags) == plan
    # the workspace the entry asks for holds exactly these records
    hs, p_h = _ints([h for h, _ in sizes])
    ws, p_w = _ints([w for _, w in sizes])
    assert _ffi.load_library().rf_jbf_ragged_workspace_bytes(8, p_h, p_w, 1, 1, -1, 36.0, 0) \
        == (32 * tiles + 255) & ~255


def test_a_positive_d_decides_the_radius(built):
    sizes = [(70, 90), (1, 1), (64, 64)]
    # d = 107 is radius 53 whatever sigma_space is: r4 56, the rows of radius 54, the disk's 107 rows
    assert _ffi.jbf_ragged_slab_plan(sizes, 1, 1, 107, 20.0, 3.0, _ffi.JBF_GREY_AS_BGR) \
        == (208, 16, 64, 107, 0, 0, 4 + 1 + 1)
    assert _ffi.jbf_ragged_slab_plan(sizes, 1, 1, 109, 20.0, 300.0, _ffi.JBF_GREY_AS_BGR) \
        == (208, 16, 64, 109, 0, 0, 6)


def test_the_routes_that_do_not_take_the_slab_launch(built):
    sizes = [(70, 90), (1, 1), (64, 64)]
    slab = lambda *a, **kw: _ffi.jbf_ragged_slab_plan(sizes, *a, **kw)
    assert slab(1, 1, -1, 20.0, 22.0) is None                         # radius 33: the tile classes
    assert slab(1, 1, -1, 15.0, 28.0) is None                         # radius 42
    assert slab(3, 3, 105, 20.0, 3.0) is None                         # radius 52
    assert slab(1, 1, 3, 20.0, 3.0) is None                           # radius 1
    assert slab(3, 3, 939, 20.0, 3.0) is None                         # radius 469: the generic kernel
    assert slab(3, 3, -1, 20.0, 400.0) is None                        # radius 600
    assert slab(1, 1, -1, 20.0, 36.0) is not None
    assert slab(1, 1, -1, 20.0, 36.0, _ffi.JBF_FORCE_GENERIC) is None
    for tune in (1, 7):
        with _ffi.debug_options(jbf_tune=tune):
            assert slab(1, 1, -1, 20.0, 36.0) is None
    assert slab(1, 1, -1, 20.0, 36.0) is not None
    # the query of the tile classes keeps its answers at these radii
    assert _ffi.jbf_ragged_plan(sizes, 1, 1, -1, 20.0, 36.0) is None
    assert _ffi.jbf_ragged_plan(sizes, 1, 1, 107, 20.0, 3.0) is None
    assert _ffi.jbf_ragged_plan(sizes, 3, 3, -1, 20.0, 66.0) is None
    assert _ffi.jbf_ragged_plan(sizes, 1, 1, -1, 20.0, 22.0) is not None


def test_the_slab_query_refuses_what_the_tile_query_refuses(built):
    lib = _ffi.load_library()
    for kw in ({"joint_cn": 2}, {"src_cn": 4}, {"sigma_space": 3000.0}, {"flags": 8},
               {"flags": 0x1000}, {"sizes": [(8, 8), (0, 3)]}, {"sizes": [(8, 8), (3, -1)]}):
        args = dict(sizes=[(8, 8)], joint_cn=1, src_cn=1, d=-1, sigma_color=20.0, sigma_space=36.0)
        args.update(kw)
        with pytest.raises(ValueError):
            _ffi.jbf_ragged_slab_plan(**args)
        with pytest.raises(ValueError):
            _ffi.jbf_ragged_plan(**args)
    # -1 is "not this launch" too; a refusal's message left behind does not turn one into the other
    assert lib.rf_last_error()
    assert _ffi.jbf_ragged_slab_plan([(8, 8)], 1, 1, -1, 20.0, 22.0) is None
    hs, p_h = _ints([81])
    ws, p_w = _ints([200])
    both = (lib.rf_debug_jbf_ragged_slab_plan, lib.rf_debug_jbf_ragged_plan)
    # the same codes from both queries: NULL size arrays (also for n = 0), a bad n, channels, radius
    for fn in both:
        assert fn(0, None, None, 1, 1, -1, 20.0, 36.0, 0, None, 0) == _ffi.RF_E_BADARG
        assert fn(1, None, p_w, 1, 1, -1, 20.0, 36.0, 0, None, 0) == _ffi.RF_E_BADARG
        assert fn(1, p_h, None, 1, 1, -1, 20.0, 36.0, 0, None, 0) == _ffi.RF_E_BADARG
        assert lib.rf_last_error()
        assert fn(-1, p_h, p_w, 1, 1, -1, 20.0, 36.0, 0, None, 0) == _ffi.RF_E_BADARG
        assert fn(1, p_h, p_w, 2, 1, -1, 20.0, 36.0, 0, None, 0) == _ffi.RF_E_UNSUPPORTED
        assert fn(1, p_h, p_w, 1, 1, -1, 20.0, 3000.0, 0, None, 0) == _ffi.RF_E_UNSUPPORTED
        # cap: negative, or positive without an out
        assert fn(1, p_h, p_w, 1, 1, -1, 20.0, 36.0, 0, None, -1) == _ffi.RF_E_BADARG
        assert fn(1, p_h, p_w, 1, 1, -1, 20.0, 36.0, 0, None, 2) == _ffi.RF_E_BADARG
        assert b"cap" in lib.rf_last_error()
    # the answer alone: out may be NULL when cap is 0, and is not written then
    assert lib.rf_debug_jbf_ragged_slab_plan(1, p_h, p_w, 1, 1, -1, 20.0, 36.0, 0, None, 0) == 1
    out = np.full(9, -7, dtype=np.int32)
    assert lib.rf_debug_jbf_ragged_slab_plan(1, p_h, p_w, 1, 1, -1, 20.0, 36.0, 0, out.ctypes.data, 0) == 1
    assert out.tolist() == [-7] * 9
    # one record of seven ints, whatever room cap promises beyond it
    assert lib.rf_debug_jbf_ragged_slab_plan(1, p_h, p_w, 1, 1, -1, 20.0, 36.0, 0, out.ctypes.data, 3) == 1
    assert out.tolist() == [208, 16, 64, 109, 0, 0, 2 * 4, -7, -7]
    # an empty list takes the route of its radius with no tile
    assert lib.rf_debug_jbf_ragged_slab_plan(0, p_h, p_w, 1, 1, -1, 20.0, 36.0, 0, out.ctypes.data, 1) == 1
    assert out.tolist()[:7] == [208, 16, 64, 109, 0, 0, 0]
    assert lib.rf_debug_jbf_ragged_slab_plan(0, p_h, p_w, 1, 1, -1, 20.0, 22.0, 0, out.ctypes.data, 1) == -1
