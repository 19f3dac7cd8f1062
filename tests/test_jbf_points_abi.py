"""CPU suite: the point-evaluated joint bilateral (rf_jbf_points_u8), the sampled-byte WHDR
(rf_whdr_points_u8) and the WHDR sweep's host side - refusals before any GPU work, the launch
plan (rf_debug_jbf_points_plan: chunks and points per wave), the point deduplication, and the
command line's grid parsing.  No compute calls."""
import ctypes

import numpy as np
import pytest

from reflectance_filtering_amd import _ffi, whdr
from reflectance_filtering_amd import sweep as sweep_cli


def _dbl(values):
    a = np.ascontiguousarray(values, dtype=np.float64)
    return a, a.ctypes.data


def test_jbf_points_refusals_need_no_gpu(built):
    lib = _ffi.load_library()
    buf = ctypes.create_string_buffer(1 << 16)
    base = ctypes.addressof(buf)
    j, s, pts, off, out = base, base + 4096, base + 8192, base + 12288, base + 16384
    sc, p_sc = _dbl([20.0, 15.0])
    ss, p_ss = _dbl([22.0, 28.0])
    ws_need = lib.rf_jbf_points_workspace_bytes(2, p_ss, -1, 1, _ffi.JBF_GREY_AS_BGR)
    assert ws_need > 0

    def call(joint=j, src=s, n=1, h=8, w=8, jcn=1, scn=1, points=pts, offsets=off, total=4,
             n_params=2, p_c=p_sc, p_s=p_ss, d=-1, border=4, flags=_ffi.JBF_GREY_AS_BGR, o=out,
             ws=base + 32768, ws_bytes=1 << 40):
        return lib.rf_jbf_points_u8(joint, src, n, h, w, jcn, scn, points, offsets, total,
                                    n_params, p_c, p_s, d, border, flags, o, ws, ws_bytes, None)

    assert call(joint=None) == _ffi.RF_E_BADARG
    assert b"NULL" in lib.rf_last_error()
    for kw in ({"src": None}, {"points": None}, {"offsets": None}, {"o": None}):
        assert call(**kw) == _ffi.RF_E_BADARG, kw
    assert call(n=0, joint=None) == _ffi.RF_OK              # an empty batch is valid
    assert call(h=0) == _ffi.RF_E_BADARG
    assert call(total=-1) == _ffi.RF_E_BADARG
    assert call(n_params=0) == _ffi.RF_E_BADARG
    assert call(n_params=-3) == _ffi.RF_E_BADARG
    assert call(p_c=None) == _ffi.RF_E_BADARG
    assert call(p_s=None) == _ffi.RF_E_BADARG
    assert call(jcn=2) == _ffi.RF_E_UNSUPPORTED
    assert call(scn=4) == _ffi.RF_E_UNSUPPORTED
    assert b"channels" in lib.rf_last_error()
    assert call(border=5) == _ffi.RF_E_UNSUPPORTED
    assert call(flags=0x1000) == _ffi.RF_E_BADARG
    assert b"flag" in lib.rf_last_error()
    assert call(flags=8) == _ffi.RF_E_BADARG
    assert call(o=j + 16) == _ffi.RF_E_BADARG               # out overlaps the joint image
    assert b"overlap" in lib.rf_last_error()
    assert call(ws_bytes=ws_need - 1) == _ffi.RF_E_WORKSPACE
    assert call(ws=None) == _ffi.RF_E_WORKSPACE
    big, p_big = _dbl([20.0, 3000.0])                        # radius 4500 > 4096, as rf_jbf_u8
    assert call(p_s=p_big) == _ffi.RF_E_UNSUPPORTED
    assert b"radius" in lib.rf_last_error()


def test_jbf_points_workspace_bytes(built):
    lib = _ffi.load_library()
    ss, p_ss = _dbl([22.0, 66.0, 22.0])
    small, p_small = _dbl([22.0])
    assert lib.rf_jbf_points_workspace_bytes(0, p_ss, -1, 3, 0) == 0
    assert lib.rf_jbf_points_workspace_bytes(3, None, -1, 3, 0) == 0
    assert lib.rf_jbf_points_workspace_bytes(3, p_ss, -1, 2, 0) == 0
    one = lib.rf_jbf_points_workspace_bytes(1, p_small, -1, 1, 0)
    grey = lib.rf_jbf_points_workspace_bytes(1, p_small, -1, 1, _ffi.JBF_GREY_AS_BGR)
    three = lib.rf_jbf_points_workspace_bytes(3, p_ss, -1, 1, 0)
    assert 0 < one < grey < lib.rf_jbf_points_workspace_bytes(1, p_small, -1, 3, 0) + 1
    assert three > one
    # d > 0 fixes the radius whatever sigma_space is
    assert lib.rf_jbf_points_workspace_bytes(1, p_small, 3, 1, 0) < one


# ---- the launch plan (rf_debug_jbf_points_plan) --------------------------------------------------
# ppw = max(1, min(64 // nsets, total_points * nchunks // 4096)); every expected value below is
# worked out by hand from that rule, none by a restatement of it in code.

def _plan(ss, total, d=-1, jcn=3, flags=0):
    return _ffi.jbf_points_plan(ss, d, jcn, flags, total)


def test_points_plan_groups_sets_by_sigma_space(built):
    # sigma_space <= 0 counts as 1, so -3, 0 and 1 are one group; radius = max(1, lrint(1.5 ss))
    plan = _plan([22.0, 0.0, 4.0, 22.0, -3.0, 1.0, 4.0, 22.0], 10)
    assert plan == [(33, 3, 1, 10), (6, 2, 1, 10), (2, 3, 1, 10)]
    # groups are by sigma_space, not by radius: 3.9 and 4.1 both round to radius 6 and stay apart,
    # in the caller's order (the sort by radius is stable)
    assert _plan([4.1, 3.9, 4.1], 10) == [(6, 2, 1, 10), (6, 1, 1, 10)]
    # d > 0 fixes the radius (d // 2) of every group; the groups remain
    assert _plan([22.0, 4.0, 22.0], 10, d=9) == [(4, 2, 1, 10), (4, 1, 1, 10)]
    assert _plan([0.2], 7) == [(1, 1, 1, 7)]                  # radius floor 1
    # the channel count and the flags of the tables do not enter the plan
    ss = [5.0] * 3 + [2.0] * 70
    for jcn, flags in ((1, 0), (1, _ffi.JBF_GREY_AS_BGR), (3, _ffi.JBF_GREY_AS_BGR),
                       (3, _ffi.JBF_TRUE_DIVISION | _ffi.JBF_FORCE_GENERIC)):
        assert _plan(ss, 5000, jcn=jcn, flags=flags) == _plan(ss, 5000)


def test_points_plan_chunks_hold_at_most_64_sets_by_decreasing_radius(built):
    # 65 sets of one sigma: chunks of 64 and 1; 200 of another: 64, 64, 64, 8
    ss = [2.0] * 30 + [6.0] * 65 + [2.0] * 170 + [4.0] * 64
    plan = _plan(ss, 100)
    assert [(r, n) for r, n, _, _ in plan] == [(9, 64), (9, 1), (6, 64), (3, 64), (3, 64), (3, 64),
                                               (3, 8)]
    assert all(ppw == 1 and waves == 100 for _, _, ppw, waves in plan)   # 100 * 7 < 8192
    assert sum(n for _, n, _, _ in plan) == len(ss)


def test_points_plan_points_per_wave_follow_the_rule(built):
    # one chunk: total * 1 // 4096 is 1 at 8191, 2 at 8192
    assert _plan([3.0], 8191) == [(4, 1, 1, 8191)]
    assert _plan([3.0], 8192) == [(4, 1, 2, 4096)]
    assert _plan([3.0], 4095) == [(4, 1, 1, 4095)]             # 0 -> the floor of 1
    assert _plan([3.0], 0) == [(4, 1, 1, 0)]
    # two chunks: 4095 * 2 = 8190 -> 1; 4096 * 2 = 8192 -> 2
    assert _plan([3.0, 5.0], 4095) == [(8, 1, 1, 4095), (4, 1, 1, 4095)]
    assert _plan([3.0, 5.0], 4096) == [(8, 1, 2, 2048), (4, 1, 2, 2048)]
    # 65 sets = chunks of 64 and 1: 64 // 64 = 1 for the first whatever the cap; the second
    # takes the cap 100000 * 2 // 4096 = 48, in ceil(100000 / 48) = 2084 waves
    assert _plan([3.0] * 65, 100000) == [(4, 64, 1, 100000), (4, 1, 48, 2084)]
    # nsets 1, 3, 5, 33, 64 in five chunks, cap 60000 * 5 // 4096 = 73: 64 // nsets decides;
    # waves = ceil(60000 / ppw): 938 (64), 2858 (21), 5000 (12)
    ss = [1.0] * 1 + [2.0] * 3 + [3.0] * 5 + [4.0] * 33 + [5.0] * 64
    assert _plan(ss, 60000) == [(8, 64, 1, 60000), (6, 33, 1, 60000), (4, 5, 12, 5000),
                                (3, 3, 21, 2858), (2, 1, 64, 938)]
    # the same grid, cap 9000 * 5 // 4096 = 10: limits the chunks of 1, 3 and 5 sets alike
    assert _plan(ss, 9000) == [(8, 64, 1, 9000), (6, 33, 1, 9000), (4, 5, 10, 900),
                               (3, 3, 10, 900), (2, 1, 10, 900)]
    # a last wave that is partly filled still counts: ceil(8193 / 2) = 4097
    assert _plan([3.0], 8193) == [(4, 1, 2, 4097)]


def test_points_plan_agrees_with_the_workspace_size(built):
    """The workspace starts with one chunk record per planned chunk: with the tables unchanged
    (same groups, same number of sets), 64 sets in one chunk or in two differ by the records
    alone, and the chunk count the plan reports is the one the layout was sized for."""
    lib = _ffi.load_library()

    def bytes_of(ss, jcn=3, flags=0):
        a, p = _dbl(ss)
        return lib.rf_jbf_points_workspace_bytes(len(ss), p, -1, jcn, flags)

    def layout(ss, jcn, flags):
        """Restated layout: 256-aligned [chunk records][8-byte taps][float tables]."""
        plan = _plan(ss, 0, jcn=jcn, flags=flags)
        align = lambda b: (b + 255) & ~255
        record = 4 * (6 + 64)
        taps = 0
        groups = {}
        for v in ss:
            groups.setdefault(1.0 if v <= 0 else v, 0)
        for v in groups:
            r = max(1, int(np.rint(v * 1.5)))
            taps += sum(1 for i in range(-r, r + 1) for j in range(-r, r + 1)
                        if not np.sqrt(float(i * i + j * j)) > r)
        nlut = 256 * (3 if (flags & _ffi.JBF_GREY_AS_BGR and jcn == 1) else jcn)
        return align(record * len(plan)) + align(8 * taps) + align(4 * nlut * len(ss))

    for ss in ([22.0], [3.0] * 64, [3.0] * 65, [2.0] * 30 + [6.0] * 65 + [2.0] * 170,
               [1.0, 0.0, -1.0, 5.0]):
        for jcn, flags in ((3, 0), (1, 0), (1, _ffi.JBF_GREY_AS_BGR)):
            assert bytes_of(ss, jcn, flags) == layout(ss, jcn, flags), (len(ss), jcn, flags)
    # one more chunk record (a multiple of 256 once aligned) is the whole difference
    assert len(_plan([3.0] * 64 + [3.0], 0)) == len(_plan([3.0] * 64, 0)) + 1


def test_points_plan_refuses_what_the_entry_refuses(built):
    lib = _ffi.load_library()
    ss, p_ss = _dbl([22.0, 28.0])
    out = (ctypes.c_int * 8)()

    def call(n_params=2, p=p_ss, d=-1, jcn=1, flags=0, total=100, o=out, room=2):
        return lib.rf_debug_jbf_points_plan(n_params, p, d, jcn, flags, total, o, room)

    assert call() == 2
    assert list(out) == [42, 1, 1, 100, 33, 1, 1, 100]
    assert call(o=None, room=0) == 2                          # the count alone
    out[4] = -7
    assert call(room=1) == 2 and out[4] == -7                 # writes no more than max_chunks
    assert call(n_params=0) == _ffi.RF_E_BADARG
    assert call(p=None) == _ffi.RF_E_BADARG
    assert call(total=-1) == _ffi.RF_E_BADARG
    assert call(o=None) == _ffi.RF_E_BADARG
    assert call(room=-1) == _ffi.RF_E_BADARG
    assert call(jcn=2) == _ffi.RF_E_UNSUPPORTED
    assert call(flags=8) == _ffi.RF_E_BADARG
    assert b"flag" in lib.rf_last_error()
    big, p_big = _dbl([20.0, 3000.0])                          # radius 4500 > 4096
    assert call(p=p_big) == _ffi.RF_E_UNSUPPORTED
    assert b"radius" in lib.rf_last_error()
    # 2^31 - 1 points in two chunks of 64 sets: more waves than one launch addresses
    many, p_many = _dbl([3.0] * 128)
    assert call(n_params=128, p=p_many, total=2 ** 31 - 1, o=None, room=0) == _ffi.RF_E_UNSUPPORTED
    with pytest.raises(ValueError):
        _ffi.jbf_points_plan([22.0], -1, 2, 0, 10)


def test_gpu_point_cases_run_at_many_points_per_wave(built):
    """The coverage claim of tests/test_gpu_points_fuzz.py, checked without a GPU on the inputs
    those tests build: cases a, b and d have chunks with ppw > 1, case a the nine hand-computed
    values, and the first 16 fuzz cases alone meet every mapping class three times."""
    from tests import test_gpu_points_fuzz as pf
    pairs = pf.case_a_pairs()
    pts, off = pf.case_a_points(4, 100, 130)
    assert len(pairs) == 146 and pts.shape == (52000, 2) and off.tolist() == [0, 13000, 26000, 39000, 52000]
    assert len(np.unique(pts[:13000], axis=0)) == 13000        # every pixel once
    assert not np.array_equal(pts[:13000], pts[13000:26000])   # each image in an order of its own
    plan = _plan([ss for _, ss in pairs], 52000)
    assert [c[:3] for c in plan] == pf.A_PLAN_52000
    assert [c[2] for c in plan] == [1, 4, 1, 4, 9, 12, 21, 32, 64]
    for shape in pf.B_SHAPES:
        for pool, ppw in zip(pf.B_POOLS, (2, 4)):
            pts, off = pf.case_b_points(shape, pool)
            per_image = np.diff(off)
            assert per_image[list(pf.B_EMPTY)].tolist() == [0, 0]
            assert np.all(np.abs(np.delete(per_image, pf.B_EMPTY) - pool) < 0.05 * pool)
            plan = _plan([ss for _, ss in pf.B_PAIRS], int(off[-1]), jcn=1, flags=_ffi.JBF_GREY_AS_BGR)
            assert [c[:3] for c in plan] == [(99, 1, ppw), (33, 2, ppw)], (shape, pool, plan)
    total = whdr.dedup_points(pf.case_d_comparisons(), *pf.D_SHAPE)[0].shape[0]
    plan = _plan([ss for _, ss in pf.D_PAIRS["bilateral"]], total, jcn=1, flags=_ffi.JBF_GREY_AS_BGR)
    assert min(c[2] for c in plan) > 1, (total, plan)
    rng = np.random.default_rng(65536)
    seen = dict.fromkeys(pf.C_CLASSES, 0)
    slabs = 0
    for index in range(16):
        case = pf.draw_fuzz_case(rng, index)
        assert case["total"] == case["off"][-1] == case["pts"].shape[0] >= 1
        assert case["pts"][:, 0].max() < case["w"] and case["pts"][:, 1].max() < case["h"]
        for name in case["classes"]:
            seen[name] += 1
        slabs += case["slab"]
    assert min(seen.values()) >= 3, seen


def test_whdr_points_refusals_need_no_gpu(built):
    lib = _ffi.load_library()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)

    def call(samples=p, n_sets=2, stride=10, c=1, n=1, po=p, comps=p, wts=p, co=p, delta=0.1,
             out=p + 2048):
        return lib.rf_whdr_points_u8(samples, n_sets, stride, c, n, po, comps, wts, co, delta,
                                     out, None)

    assert call(n=0, samples=None) == _ffi.RF_OK
    for kw in ({"samples": None}, {"po": None}, {"comps": None}, {"wts": None}, {"co": None},
               {"out": None}):
        assert call(**kw) == _ffi.RF_E_BADARG, kw
    assert call(n_sets=0) == _ffi.RF_E_BADARG
    assert call(stride=0) == _ffi.RF_E_BADARG
    assert call(n=-1) == _ffi.RF_E_BADARG
    assert call(c=2) == _ffi.RF_E_UNSUPPORTED
    assert call(delta=-0.5) == _ffi.RF_E_BADARG
    assert call(delta=float("nan")) == _ffi.RF_E_BADARG


def _brute_dedup(comparisons_px):
    """Restatement: per image, the sorted set of distinct (x, y) tuples, and each comparison's
    two points looked up in it by a linear search."""
    pts, po, comps, wts, co = [], [0], [], [], [0]
    for comp in comparisons_px:
        comp = np.asarray(comp, dtype=np.float64).reshape(-1, 6)
        xy = [(int(r[0]), int(r[1])) for r in comp] + [(int(r[2]), int(r[3])) for r in comp]
        uniq = sorted(set(xy))
        for row in comp:
            a = uniq.index((int(row[0]), int(row[1])))
            b = uniq.index((int(row[2]), int(row[3])))
            comps.append((a, b, int(row[4])))
            wts.append(row[5])
        pts.extend(uniq)
        po.append(len(pts))
        co.append(len(comps))
    return pts, po, comps, wts, co


def test_dedup_points_matches_a_restatement():
    rng = np.random.default_rng(3)
    h, w = 37, 53
    comparisons = []
    for n_comp in (0, 1, 17, 300, 5):
        pool = np.stack([rng.integers(0, w, 12), rng.integers(0, h, 12)], axis=1)  # shared points
        a = pool[rng.integers(0, 12, n_comp)]
        b = pool[rng.integers(0, 12, n_comp)]
        rows = np.concatenate([a, b, rng.integers(0, 3, (n_comp, 1)),
                               rng.random((n_comp, 1))], axis=1).astype(np.float64)
        rows[:, :4] += rng.random((n_comp, 4)) * 0.9          # fractions truncate like whdr_batch
        comparisons.append(rows)
    pts, po, comps, wts, co = whdr.dedup_points(comparisons, h, w)
    b_pts, b_po, b_comps, b_wts, b_co = _brute_dedup(comparisons)
    assert pts.dtype == np.int32 and comps.dtype == np.int32 and wts.dtype == np.float64
    assert [tuple(p) for p in pts.tolist()] == b_pts
    assert po.tolist() == b_po and co.tolist() == b_co
    assert [tuple(c) for c in comps.tolist()] == b_comps
    assert np.array_equal(wts, np.array(b_wts))
    assert po[-1] < 2 * co[-1]                                  # shared points stored once
    # every comparison still names its own two pixels
    for i in range(len(comparisons)):
        for k in range(co[i], co[i + 1]):
            row = comparisons[i][k - co[i]]
            assert tuple(pts[po[i] + comps[k, 0]]) == (int(row[0]), int(row[1]))
            assert tuple(pts[po[i] + comps[k, 1]]) == (int(row[2]), int(row[3]))


def test_dedup_points_rejects_points_outside_the_image():
    with pytest.raises(IndexError):
        whdr.dedup_points([np.array([[10, 0, 0, 0, 1, 1.0]])], 5, 10)
    with pytest.raises(IndexError):
        whdr.dedup_points([np.array([[0, 0, 0, 5, 1, 1.0]])], 5, 10)
    with pytest.raises(IndexError):
        whdr.dedup_points([np.array([[0, -1, 0, 0, 1, 1.0]])], 5, 10)


def test_sweep_rejects_points_outside_the_image_before_device_work():
    img = np.zeros((6, 9, 1), np.uint8)
    ok = np.array([[1, 1, 2, 2, 0, 1.0]])
    bad = np.array([[1, 1, 9, 2, 0, 1.0]])                      # x == width
    for ftype in ("bilateral", "guided"):
        with pytest.raises(IndexError):
            whdr.sweep(ftype, [img, img], [img, img], [ok, bad], [(20, 22)])
    with pytest.raises(ValueError):
        whdr.sweep("bilateral", [img], [img], [ok], [])
    with pytest.raises(ValueError):
        whdr.sweep("bilateral", [img], [img], [ok], [(0, 22)])  # sigmas must be positive
    with pytest.raises(ValueError):
        whdr.sweep("median", [img], [img], [ok], [(20, 22)])


def test_cli_grid_and_options():
    assert sweep_cli.parse_grid("10,15,20,25") == [10.0, 15.0, 20.0, 25.0]
    assert sweep_cli.parse_grid("7.5") == [7.5]
    for bad in ("", "10,-1", "0", "a,b"):
        with pytest.raises(ValueError):
            sweep_cli.parse_grid(bad)
    pairs = sweep_cli.grid_pairs([10, 15], [16, 22, 28])
    assert pairs.tolist() == [[10, 16], [10, 22], [10, 28], [15, 16], [15, 22], [15, 28]]
    args = sweep_cli.build_parser().parse_args(
        ["--inputs", "a/*.png", "b.png", "--filter_type", "guided", "--sigma_color", "3,7",
         "--sigma_spatial", "45,52", "--guidance", "image", "--delta", "0.2", "--out", "o.json",
         "--per_image", "o.npz"])
    assert args.inputs == ["a/*.png", "b.png"] and args.filter_type == "guided"
    assert args.sigma_color == [3.0, 7.0] and args.sigma_spatial == [45.0, 52.0]
    assert args.guidance == "image" and args.delta == 0.2
    assert args.out == "o.json" and args.per_image == "o.npz"
    args = sweep_cli.build_parser().parse_args(
        ["--inputs", "x.png", "--sigma_color", "20", "--sigma_spatial", "22"])
    assert (args.filter_type, args.guidance, args.delta, args.per_image) == \
        ("bilateral", "cnn", 0.1, None)
    for bad in (["--filter_type", "median"], ["--guidance", "flat"], ["--sigma_color", "0"]):
        with pytest.raises(SystemExit):
            sweep_cli.build_parser().parse_args(
                ["--inputs", "x.png", "--sigma_color", "20", "--sigma_spatial", "22"] + bad)
    assert sweep_cli.judgements_for("dir/123.png") == "dir/123.json"


def test_cli_summary_picks_the_lowest_mean_over_judged_images():
    pairs = np.array([[10, 16], [20, 22], [30, 28]], dtype=np.float64)
    per_image = np.array([[0.3, 0.1, 0.0], [0.2, 0.1, 0.0], [0.25, 0.0, 0.0]])
    mean, best = sweep_cli.summarise(pairs, per_image, [True, True, False])
    assert np.allclose(mean, [0.2, 0.15, 0.125]) and best == 2
