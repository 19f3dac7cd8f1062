"""GPU suite: the joint bilateral evaluated at listed pixels (rf_jbf_points_u8) gives, byte for
byte, what rf_jbf_u8 writes there, and the WHDR sweep built on it (whdr.sweep and the
`python -m reflectance_filtering_amd.sweep` command line) equals the host-computed pipeline
filter -> float32 bytes / 255 -> whdr_batch, bit for bit."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B101, BREP, BCONST = 4, 1, 0


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _scene(h, w, seed):
    from tests import synth
    return synth.scene_u8(h, w, seed)


def _grey(h, w, seed):
    from tests import synth
    return np.ascontiguousarray(synth.reflectance_like_u8(h, w, seed)[:, :, :1])


def _edge_points(h, w, rng, extra):
    """Every corner, points on every edge and next to it, and `extra` random ones."""
    pts = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w // 2, 0), (w // 2, h - 1),
           (0, h // 2), (w - 1, h // 2), (1, 1), (w - 2, h - 2)]
    pts += [(int(x), int(y)) for x, y in zip(rng.integers(0, w, extra), rng.integers(0, h, extra))]
    return np.array(pts, dtype=np.int32)


def _run(torch, joints, srcs, pts_per_image, pairs, border=B101, flags=0, grey=False, d=-1):
    """(points result [P,total,C] host, per-pair full rf_jbf_u8 outputs sampled at the points)."""
    import reflectance_filtering_amd as rf
    jt = torch.from_numpy(np.ascontiguousarray(joints)).cuda()
    st = torch.from_numpy(np.ascontiguousarray(srcs)).cuda()
    pts = np.concatenate(pts_per_image, axis=0)
    off = np.cumsum([0] + [p.shape[0] for p in pts_per_image]).astype(np.int32)
    got = rf.ops.joint_bilateral_points_u8(jt, st, pts, off, pairs, d=d, border=border,
                                           flags=flags, grey_as_bgr=grey).cpu().numpy()
    img_of = np.repeat(np.arange(len(pts_per_image)), np.diff(off))
    want = []
    for sc, ss in pairs:
        full = rf.ops.joint_bilateral_u8(jt, st, d, sc, ss, border=border, flags=flags,
                                         grey_as_bgr=grey).cpu().numpy()
        want.append(full[img_of, pts[:, 1], pts[:, 0]])
    return got, np.stack(want)


@pytest.mark.parametrize("jcn,grey", [(1, True), (3, False)])
@pytest.mark.parametrize("scn", [1, 3])
@pytest.mark.parametrize("border", [B101, BREP, BCONST])
@pytest.mark.parametrize("true_div", [False, True])
def test_points_equal_the_full_filter(jcn, grey, scn, border, true_div):
    torch = _torch()
    import reflectance_filtering_amd as rf
    rng = np.random.default_rng(11 + jcn + 3 * scn + border)
    h, w = 41, 57
    joints = np.stack([_grey(h, w, 1) if jcn == 1 else _scene(h, w, 1),
                       _grey(h, w, 2) if jcn == 1 else _scene(h, w, 2)])
    srcs = np.stack([_grey(h, w, 3) if scn == 1 else _scene(h, w, 3),
                     _grey(h, w, 4) if scn == 1 else _scene(h, w, 4)])
    pts = [_edge_points(h, w, rng, 20), _edge_points(h, w, rng, 7)]
    pairs = [(20, 22), (15, 28), (3, 5), (60, 4), (0, -1)]     # sigma <= 0 -> 1, as rf_jbf_u8
    flags = rf._ffi.JBF_TRUE_DIVISION if true_div else 0
    got, want = _run(torch, joints, srcs, pts, pairs, border=border, flags=flags, grey=grey)
    assert got.shape == (len(pairs), sum(p.shape[0] for p in pts), scn)
    assert np.array_equal(got, want)


def test_force_generic_is_accepted_and_changes_nothing():
    torch = _torch()
    import reflectance_filtering_amd as rf
    h, w = 30, 44
    pts = [_edge_points(h, w, np.random.default_rng(5), 12)]
    j, s = _grey(h, w, 6)[None], _grey(h, w, 6)[None]
    a, want = _run(torch, j, s, pts, [(20, 22)], grey=True)
    b, _ = _run(torch, j, s, pts, [(20, 22)], grey=True, flags=rf._ffi.JBF_FORCE_GENERIC)
    assert np.array_equal(a, want) and np.array_equal(b, want)


def test_grids_that_mix_radii_and_one_beyond_the_tiled_kernels():
    torch = _torch()
    rng = np.random.default_rng(21)
    h, w = 70, 90
    pts = [_edge_points(h, w, rng, 25)]
    # radii 1, 33, 54, 132 and 471 (> 468: rf_jbf_u8's untiled kernel), in one call, unsorted
    pairs = [(20, 88), (20, 0.5), (25, 314), (20, 22), (10, 36), (30, 22)]
    got, want = _run(torch, _scene(h, w, 8)[None], _grey(h, w, 9)[None], pts, pairs)
    assert np.array_equal(got, want)
    got, want = _run(torch, _grey(h, w, 8)[None], _scene(h, w, 9)[None], pts, pairs[:3], grey=True,
                     border=BCONST)
    assert np.array_equal(got, want)
    # d > 0 fixes the radius for every set
    got, want = _run(torch, _scene(h, w, 8)[None], _scene(h, w, 9)[None], pts, pairs[:4], d=9)
    assert np.array_equal(got, want)


def test_more_than_64_sets_leave_the_table_cache_alone():
    torch = _torch()
    import reflectance_filtering_amd as rf
    h, w = 48, 64
    j = torch.from_numpy(_grey(h, w, 12)[None]).cuda()
    before = [rf.ops.joint_bilateral_u8(j, j, -1, sc, 22, grey_as_bgr=True).cpu().numpy()
              for sc in (20, 21)]
    pairs = [(float(sc), ss) for ss in (22, 7) for sc in range(1, 41)]   # 80 sets, two chunks + 16
    rng = np.random.default_rng(13)
    pts = [_edge_points(h, w, rng, 30)]
    got, want = _run(torch, _grey(h, w, 12)[None], _grey(h, w, 12)[None], pts, pairs, grey=True)
    assert got.shape[0] == 80 and np.array_equal(got, want)
    after = [rf.ops.joint_bilateral_u8(j, j, -1, sc, 22, grey_as_bgr=True).cpu().numpy()
             for sc in (20, 21)]
    for a, b in zip(before, after):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("jcn,scn,border", [(3, 1, B101), (3, 3, BREP), (1, 1, BCONST)])
def test_points_equal_the_oracle(jcn, scn, border):
    torch = _torch()
    import reflectance_filtering_amd as rf
    from oracle import c_oracle
    h, w = 36, 50
    joint = _scene(h, w, 30) if jcn == 3 else _grey(h, w, 30)
    src = _scene(h, w, 31) if scn == 3 else _grey(h, w, 31)
    pts = _edge_points(h, w, np.random.default_rng(32), 15)
    pairs = [(20, 22), (7, 40)]
    got = rf.ops.joint_bilateral_points_u8(torch.from_numpy(joint[None]).cuda(),
                                           torch.from_numpy(src[None]).cuda(), pts,
                                           [0, pts.shape[0]], pairs, border=border).cpu().numpy()
    for p, (sc, ss) in enumerate(pairs):
        ref = c_oracle.joint_bilateral_filter(joint, src, -1, sc, ss, border)
        ref = ref.reshape(h, w, -1)
        assert np.array_equal(got[p], ref[pts[:, 1], pts[:, 0]])


# ---- WHDR sweep --------------------------------------------------------------------------------

def _comparisons(h, w, rng, m, n_points=24):
    """IIW-like judgements in pixel coordinates: points shared between comparisons, all three
    verdicts, fractional coordinates (truncated like to_pixels output would be)."""
    if m == 0:
        return np.zeros((0, 6))
    pool = np.stack([rng.integers(0, w, n_points), rng.integers(0, h, n_points)], axis=1)
    a, b = pool[rng.integers(0, n_points, m)], pool[rng.integers(0, n_points, m)]
    return np.concatenate([a, b, rng.integers(0, 3, (m, 1)), rng.random((m, 1)) + 0.05],
                          axis=1).astype(np.float64)


def _host_pipeline(torch, filtered_nhwc, comps, delta):
    """whdr_batch on the filtered bytes as planar float32 / 255, the division done by numpy."""
    from reflectance_filtering_amd import whdr
    planar = np.ascontiguousarray(np.transpose(filtered_nhwc, (0, 3, 1, 2)))
    refl = torch.from_numpy(planar.astype(np.float32) / np.float32(255)).cuda()
    return whdr.whdr_batch(refl, comps, delta)


def _filter_full(torch, ftype, joint, src, sc, ss, grey):
    import reflectance_filtering_amd as rf
    if ftype == "bilateral":
        return rf.ops.joint_bilateral_u8(joint, src, -1, sc, ss, grey_as_bgr=grey).cpu().numpy()
    return rf.ops.guided_filter_u8(joint, src, int(ss), sc, grey_as_bgr=grey).cpu().numpy()


def _tie_delta(torch, ftype, joint, src, comps, sc, ss, grey):
    """A delta whose float32(1 + delta) is exactly the ratio of a judged pair's lightnesses under
    (sc, ss), and the delta one float32 ulp below it."""
    f = _filter_full(torch, ftype, joint, src, sc, ss, grey)
    for i, comp in enumerate(comps):
        for row in comp:
            x1, y1, x2, y2 = (int(v) for v in row[:4])
            l1 = np.float32(f[i, y1, x1].astype(np.float32) / np.float32(255)).mean(dtype=np.float32)
            l2 = np.float32(f[i, y2, x2].astype(np.float32) / np.float32(255)).mean(dtype=np.float32)
            lo, hi = sorted((max(l1, np.float32(np.finfo(np.float32).eps)),
                             max(l2, np.float32(np.finfo(np.float32).eps))))
            r = np.float32(hi / lo)
            if 1.02 < r < 1.5:
                below = np.nextafter(r, np.float32(0))
                return [float(r) - 1.0, float(below) - 1.0]
    return []


@pytest.mark.parametrize("ftype", ["bilateral", "guided"])
@pytest.mark.parametrize("scn", [1, 3])
def test_sweep_equals_the_host_pipeline(ftype, scn):
    torch = _torch()
    from reflectance_filtering_amd import whdr
    rng = np.random.default_rng(40 + scn)
    h, w, n = 44, 60, 4
    joint = np.stack([_grey(h, w, 50 + i) for i in range(n)])
    src = joint if scn == 1 else np.stack([_scene(h, w, 60 + i) for i in range(n)])
    comps = [_comparisons(h, w, rng, m) for m in (90, 0, 40, 12)]
    comps[3][:, 5] = 0.0                                      # zero total weight -> 0
    comps[2][:5, 4] = 0                                       # 'E' judgements
    jt, st = torch.from_numpy(joint).cuda(), torch.from_numpy(np.ascontiguousarray(src)).cuda()
    pairs = [(20, 22), (3, 45), (7, 52), (15, 28)] if ftype == "guided" else \
        [(20, 22), (15, 28), (25, 66), (10, 4)]
    deltas = [0.1] + _tie_delta(torch, ftype, jt, st, comps, pairs[0][0], pairs[0][1], True)
    assert len(deltas) == 3, "no judged pair with a usable ratio"
    for delta in deltas:
        got = whdr.sweep(ftype, st, jt, comps, pairs, delta=delta, grey_as_bgr=True)
        assert got.shape == (len(pairs), n) and got.dtype == np.float64
        for p, (sc, ss) in enumerate(pairs):
            want = _host_pipeline(torch, _filter_full(torch, ftype, jt, st, sc, ss, True), comps,
                                  delta)
            assert np.array_equal(got[p], want), (delta, p, got[p], want)
        assert np.all(got[:, 1] == 0) and np.all(got[:, 3] == 0)
        assert np.any(got[:, 0] > 0)


def test_sweep_with_a_colour_joint():
    torch = _torch()
    from reflectance_filtering_amd import whdr
    rng = np.random.default_rng(70)
    h, w = 40, 52
    photo = np.stack([_scene(h, w, 71), _scene(h, w, 72)])
    r1 = np.stack([_grey(h, w, 73), _grey(h, w, 74)])
    comps = [_comparisons(h, w, rng, 50), _comparisons(h, w, rng, 30)]
    jt, st = torch.from_numpy(photo).cuda(), torch.from_numpy(r1).cuda()
    for ftype, pairs in (("bilateral", [(20, 22), (10, 16)]), ("guided", [(3, 45), (7, 5)])):
        got = whdr.sweep(ftype, st, jt, comps, pairs)
        for p, (sc, ss) in enumerate(pairs):
            want = _host_pipeline(torch, _filter_full(torch, ftype, jt, st, sc, ss, False), comps,
                                  0.1)
            assert np.array_equal(got[p], want)


@pytest.mark.parametrize("ftype", ["bilateral", "guided"])
def test_sweep_of_mixed_sizes_equals_per_image_calls(ftype):
    _torch()
    from reflectance_filtering_amd import whdr
    rng = np.random.default_rng(80)
    sizes = [(30, 40), (36, 28), (30, 40), (36, 28), (30, 40)]
    imgs = [_grey(h, w, 81 + i) for i, (h, w) in enumerate(sizes)]
    comps = [_comparisons(h, w, rng, 25 + 5 * i) for i, (h, w) in enumerate(sizes)]
    pairs = [(20, 22), (7, 12)]
    got = whdr.sweep(ftype, imgs, imgs, comps, pairs, grey_as_bgr=True)
    for i in range(len(imgs)):
        one = whdr.sweep(ftype, [imgs[i]], [imgs[i]], [comps[i]], pairs, grey_as_bgr=True)
        assert np.array_equal(got[:, i], one[:, 0])


def _write_iiw_json(path, comps_px, h, w):
    """IIW-style judgement file whose normalised points map back to comps_px under to_pixels."""
    points, comparisons = [], []
    for k, row in enumerate(comps_px):
        ids = []
        for x, y in ((row[0], row[1]), (row[2], row[3])):
            ids.append(len(points))
            points.append({"id": len(points), "x": (x + 0.5) / w, "y": (y + 0.5) / h})
        comparisons.append({"point1": ids[0], "point2": ids[1],
                            "darker": {0: "E", 1: "1", 2: "2"}[int(row[4])],
                            "darker_score": float(row[5])})
    with open(path, "w") as fh:
        json.dump({"intrinsic_points": points, "intrinsic_comparisons": comparisons}, fh)


@pytest.mark.parametrize("ftype", ["bilateral", "guided"])
def test_cli_end_to_end(tmp_path, ftype):
    torch = _torch()
    import reflectance_filtering_amd as rf
    from reflectance_filtering_amd import image_utils as iu
    from reflectance_filtering_amd import sweep as sweep_cli
    from reflectance_filtering_amd import whdr
    rng = np.random.default_rng(90)
    sizes = [(40, 56), (32, 48), (40, 56)]
    photos, comps = [], []
    for i, (h, w) in enumerate(sizes):
        img = _scene(h, w, 91 + i)
        path = str(tmp_path / ("%03d.png" % i))
        iu.imwrite(path, img)
        c = _comparisons(h, w, rng, 30)
        c[:, :4] = np.floor(c[:, :4])
        _write_iiw_json(str(tmp_path / ("%03d.json" % i)), c, h, w)
        photos.append(iu.imread(path))
        comps.append(whdr.to_pixels(whdr.load_judgements(str(tmp_path / ("%03d.json" % i))), h, w))
        assert np.array_equal(comps[-1][:, :4], c[:, :4])
    out_json, out_npz = str(tmp_path / "s.json"), str(tmp_path / "s.npz")
    sc_list, ss_list = ([3, 7], [45, 52]) if ftype == "guided" else ([15, 20], [22, 28])
    assert sweep_cli.main(["--inputs", str(tmp_path / "*.png"), "--filter_type", ftype,
                           "--sigma_color", ",".join(map(str, sc_list)),
                           "--sigma_spatial", ",".join(map(str, ss_list)),
                           "--out", out_json, "--per_image", out_npz]) == 0
    with open(out_json) as fh:
        res = json.load(fh)
    npz = np.load(out_npz)
    pairs = [(c, s) for c in sc_list for s in ss_list]
    assert res["pairs"] == [list(map(float, p)) for p in pairs] and res["images"] == 3
    # the API's numbers: decompose_and_filter_batch (BF/GF(CNN, CNN)) -> bytes / 255 -> whdr_batch
    want = np.zeros((len(pairs), 3))
    for i, img in enumerate(photos):
        for p, (sc, ss) in enumerate(pairs):
            _, filt = rf.decompose_and_filter_batch(torch.from_numpy(img[None]).cuda(), sc, ss,
                                                    filter_type=ftype)
            want[p, i] = _host_pipeline(torch, filt.cpu().numpy()[..., None], [comps[i]], 0.1)[0]
    assert np.array_equal(npz["whdr"], want)
    assert res["mean_whdr"] == want.mean(axis=1).tolist()
    best = int(np.argmin(want.mean(axis=1)))
    assert (res["best"]["sigma_color"], res["best"]["sigma_spatial"]) == tuple(map(float, pairs[best]))
