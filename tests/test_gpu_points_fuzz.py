"""GPU suite: the point-evaluated joint bilateral (rf_jbf_points_u8) at MANY POINTS PER WAVE and the
WHDR sweep built on it, against the ORACLE and against host arithmetic - never against another
kernel alone.

A wave of jbf_points_kernel takes ppw = max(1, min(64 / nsets, total_points * nchunks / 4096))
points of one chunk.  tests/test_gpu_jbf_points.py stays below 8192 point-chunks, so there every
active lane has `sub == 0`; the cases here run lanes of one wave on different points and images,
idle tail lanes, partly filled last waves and `sub > 0` output indices.  Which mapping a call runs
at is never restated: every case asserts it from rf_debug_jbf_points_plan, the plan the entry
launches from (tests/test_jbf_points_abi.py checks the same claims without a GPU).

  a  whole images as shuffled point lists, 146 sets in 9 chunks, every value of 64 / nsets at once
  b  an IIW-shaped batch (341x512 and 512x341 maps, ~300 judgement points each), radii 33 and 99
  c  seeded fuzz over shapes, borders, d, flags, grids and point lists, every mapping class seen
  d  whdr.sweep and whdr_points_u8 against oracle filter -> float32 bytes / 255 -> host whdr

The fuzz is bounded by `RF_FUZZ_SECONDS` / `RF_FUZZ_SEED` like tests/test_gpu_fuzz.py.
"""
import time

import numpy as np
import pytest

from tests.test_gpu_fuzz import SECONDS, SEED, _image, env  # noqa: F401  (env is a fixture)

pytestmark = pytest.mark.gpu

BCONST, BREP, BREFLECT, BWRAP, B101 = 0, 1, 2, 3, 4
GREY_AS_BGR = 4          # RF_JBF_GREY_AS_BGR
TRUE_DIVISION = 1        # RF_JBF_TRUE_DIVISION == co.FLAG_TRUE_DIVISION
FORCE_GENERIC = 2


# ---- shared helpers ------------------------------------------------------------------------------

def _plan(pairs, d, jcn, flags, total):
    """[(radius, nsets, ppw, waves)] per chunk in launch order, from the library (host only)."""
    from reflectance_filtering_amd import _ffi
    return _ffi.jbf_points_plan([ss for _, ss in pairs], d, jcn, flags, total)


def _offsets(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def _points_call(rf, torch, joints, srcs, pts, off, pairs, d, border, flags, grey):
    out = rf.ops.joint_bilateral_points_u8(
        torch.from_numpy(np.ascontiguousarray(joints)).cuda(),
        torch.from_numpy(np.ascontiguousarray(srcs)).cuda(), pts, off, pairs, d=d, border=border,
        flags=flags, grey_as_bgr=grey)
    return out.cpu().numpy()


def _oracle_full(co, joint, src, sc, ss, d, border, flags, grey):
    """The oracle on one whole image [h,w,scn]; a grey_as_bgr joint is repeated to 3 channels."""
    j = np.repeat(joint, 3, axis=2) if grey else joint
    return co.joint_bilateral_filter(j, src, d, sc, ss, border=border,
                                     flags=flags & co.FLAG_TRUE_DIVISION).reshape(src.shape)


def _oracle_at_points(co, joints, srcs, pts, off, sc, ss, d, border, flags, grey):
    """The oracle's bytes at the listed points [total, scn]; images without points are skipped."""
    total = int(off[-1])
    want = np.zeros((total, srcs.shape[-1]), np.uint8)
    for i in range(joints.shape[0]):
        k0, k1 = int(off[i]), int(off[i + 1])
        if k1 == k0:
            continue
        full = _oracle_full(co, joints[i], srcs[i], sc, ss, d, border, flags, grey)
        want[k0:k1] = full[pts[k0:k1, 1], pts[k0:k1, 0]]
    return want


def _mismatch(got, want, pts, off, what):
    """Assert message: where the first differing byte lies."""
    bad = np.flatnonzero((got != want).any(axis=-1))
    k = int(bad[0])
    img = int(np.searchsorted(off, k, side="right") - 1)
    return "%s: %d of %d points differ, first k=%d (image %d, x=%d y=%d) got %s want %s" % (
        what, bad.size, got.shape[0], k, img, pts[k, 0], pts[k, 1], got[k].tolist(),
        want[k].tolist())


# ---- a. whole images as point lists ----------------------------------------------------------------

A_GROUP_SETS = (1, 2, 3, 5, 7, 16, 33, 79)
A_SIGMA_SPACE = np.linspace(1.0, 6.0, 8)         # radii 2, 3, 4, 5, 6, 7, 8, 9
# 79 sets are chunks of 64 and 15; chunks launch by decreasing radius.  With 52,000 points the cap
# 52000 * 9 / 4096 = 114 limits nothing, so ppw = 64 / nsets:
A_PLAN_52000 = [(9, 64, 1), (9, 15, 4), (8, 33, 1), (7, 16, 4), (6, 7, 9), (5, 5, 12), (4, 3, 21),
                (3, 2, 32), (2, 1, 64)]


def case_a_pairs(seed=0):
    """146 (sigma_color, sigma_space) pairs: 8 sigma_space groups of A_GROUP_SETS sets, every set
    with a sigma_color of its own, in an order that scatters the groups over the caller's list."""
    rng = np.random.default_rng(100 + seed)
    pairs = [(float(np.round(rng.uniform(2.0, 70.0), 2)), float(ss))
             for ss, count in zip(A_SIGMA_SPACE, A_GROUP_SETS) for _ in range(count)]
    return [pairs[i] for i in rng.permutation(len(pairs))]


def case_a_points(n, h, w, seed=0):
    """Every pixel of every image, per image in a shuffled order: (points [n*h*w, 2], offsets)."""
    rng = np.random.default_rng(200 + seed)
    yy, xx = np.mgrid[0:h, 0:w]
    every = np.stack([xx.ravel(), yy.ravel()], axis=1)
    pts = np.concatenate([every[rng.permutation(h * w)] for _ in range(n)])
    return pts.astype(np.int32), _offsets([h * w] * n)


def _run_case_a(env, n, h, w, jcn, scn, grey, border, flags, want_plan):
    rf, co, torch = env
    rng = np.random.default_rng(300 + 7 * jcn + scn + border)
    joints = np.stack([_image(rng, h, w, jcn, i % 3) for i in range(n)])
    srcs = np.stack([_image(rng, h, w, scn, (i + 1) % 3) for i in range(n)])
    pairs = case_a_pairs()
    pts, off = case_a_points(n, h, w)
    total = pts.shape[0]
    plan = _plan(pairs, -1, jcn, flags | (GREY_AS_BGR if grey else 0), total)
    if want_plan is not None:
        assert [c[:3] for c in plan] == want_plan, plan
    assert sum(c[1] for c in plan) == 146 and len(plan) == 9
    assert max(c[2] for c in plan) > 1, plan
    got = _points_call(rf, torch, joints, srcs, pts, off, pairs, -1, border, flags, grey)
    assert got.shape == (146, total, scn)
    t0 = time.time()
    for p, (sc, ss) in enumerate(pairs):
        want = _oracle_at_points(co, joints, srcs, pts, off, sc, ss, -1, border, flags, grey)
        assert np.array_equal(got[p], want), _mismatch(
            got[p], want, pts, off, "set %d (sc %g ss %g) n %d %dx%d jcn %d scn %d grey %s border %d "
            "flags %d plan %s" % (p, sc, ss, n, h, w, jcn, scn, grey, border, flags, plan))
    return plan, time.time() - t0


@pytest.mark.parametrize("jcn,scn,grey,border,flags", [
    (3, 3, False, B101, 0),
    (1, 1, True, BREFLECT, TRUE_DIVISION),
    (1, 3, False, BWRAP, 0),
    (3, 3, False, BREP, TRUE_DIVISION),
    (1, 1, True, BCONST, 0),
])
def test_whole_images_as_point_lists_match_the_oracle(env, jcn, scn, grey, border, flags):
    """4 images of 100x130, every pixel a point (52,000 points, shuffled per image), 146 sets in 9
    chunks: one call runs ppw 1, 4, 9, 12, 21, 32 and 64 - full waves, idle tail lanes (64 % nsets
    of 3, 5, 7, 15) and partly filled last waves - and every byte of every set must equal the
    oracle on the whole image.  The plan is asserted from the library, so a change of the
    points-per-wave rule fails here instead of emptying the test.  The oracle's share (584
    whole-image filters) measured 0.5 s per parametrisation on 16 CPUs, 2.7 s on 8."""
    plan, oracle_s = _run_case_a(env, 4, 100, 130, jcn, scn, grey, border, flags, A_PLAN_52000)
    print("points case a: plan %s, oracle %.1f s" % (plan, oracle_s))


@pytest.mark.parametrize("jcn,scn,grey,border,flags", [
    (3, 3, False, BWRAP, 0),
    (1, 1, True, BREFLECT, TRUE_DIVISION),
    (1, 3, False, B101, 0),
])
def test_images_smaller_than_the_disk_match_the_oracle(env, jcn, scn, grey, border, flags):
    """The same grid on 40 images of 7x9: smaller than a radius-9 disk, so every point folds at
    the border, wrap and reflect several times.  2,520 points in 9 chunks: the cap 2520 * 9 / 4096
    = 5 gives ppw 1, 4, 1, 4, 5, 5, 5, 5, 5."""
    want = [(9, 64, 1), (9, 15, 4), (8, 33, 1), (7, 16, 4), (6, 7, 5), (5, 5, 5), (4, 3, 5),
            (3, 2, 5), (2, 1, 5)]
    _run_case_a(env, 40, 7, 9, jcn, scn, grey, border, flags, want)


# ---- b. IIW-shaped batch ---------------------------------------------------------------------------

B_SHAPES = ((341, 512), (512, 341))
B_IMAGES = 16                                     # per shape; images 8 and 15 have no points
B_EMPTY = (8, 15)
B_PAIRS = [(20.0, 22.0), (15.0, 22.0), (20.0, 66.0)]   # radii 33, 33, 99: 2 groups, 2 chunks
B_POOLS = (310, 640)                              # judged points per image: IIW-like, and denser


def case_b_points(shape, pool, seed=0):
    """dedup_points of IIW-like judgements on B_IMAGES images of `shape`: `pool` judged points per
    image shared by 2 * pool comparisons, no judgements at all for the images B_EMPTY."""
    from reflectance_filtering_amd import whdr
    from tests.test_gpu_jbf_points import _comparisons
    h, w = shape
    rng = np.random.default_rng(400 + seed + h)
    comps = [_comparisons(h, w, rng, 0 if i in B_EMPTY else 2 * pool, n_points=pool)
             for i in range(B_IMAGES)]
    pts, off = whdr.dedup_points(comps, h, w)[:2]
    return pts, off.astype(np.int64)


@pytest.mark.parametrize("shape", B_SHAPES)
def test_iiw_shaped_batch_matches_the_oracle(env, shape):
    """16 grey maps of 341x512 (and of 512x341) filtered as BF(CNN, CNN) at ~300 distinct judgement
    points each (14 x ~300 x 2 chunks / 4096: ppw 2) and at ~630 each (ppw 4): the cap-limited class
    1 < ppw < 64 / nsets, asserted from the plan.  Images 8 and 15 have no points.  The radius-33
    sets are held to the oracle on every image that has points; the radius-99 set to the oracle on
    the first, the middle and the last such image and to rf_jbf_u8 on all of them, so no image is
    left unchecked.  Oracle share (28 radius-33 and 3 radius-99 whole-image filters per shape),
    measured on 16 CPUs: 6.2 s and 5.7 s for the two shapes, 12 s in all; on 8 CPUs about 40 s per
    shape.  The test prints the figure of its own run."""
    rf, co, torch = env
    from tests import synth
    h, w = shape
    joints = np.stack([np.ascontiguousarray(synth.reflectance_like_u8(h, w, 500 + i + h)[:, :, :1])
                       for i in range(B_IMAGES)])
    with_points = [i for i in range(B_IMAGES) if i not in B_EMPTY]
    r99_oracle = (with_points[0], with_points[len(with_points) // 2], with_points[-1])
    t0 = time.time()
    full = {}                                     # (pair, image) -> oracle on the whole image
    for p, (sc, ss) in enumerate(B_PAIRS):
        for i in (with_points if ss == 22.0 else r99_oracle):
            full[p, i] = _oracle_full(co, joints[i], joints[i], sc, ss, -1, B101, 0, True)
    oracle_s = time.time() - t0
    jt = torch.from_numpy(joints).cuda()
    full_r99 = rf.ops.joint_bilateral_u8(jt, jt, -1, B_PAIRS[2][0], B_PAIRS[2][1],
                                         grey_as_bgr=True).cpu().numpy()
    for i in r99_oracle:                          # the full filter itself, where both exist
        assert np.array_equal(full_r99[i], full[2, i]), (shape, i)
    for pool, want_ppw in zip(B_POOLS, (2, 4)):
        pts, off = case_b_points(shape, pool)
        total = int(off[-1])
        assert all(off[i + 1] == off[i] for i in B_EMPTY)
        plan = _plan(B_PAIRS, -1, 1, GREY_AS_BGR, total)
        assert [c[:3] for c in plan] == [(99, 1, want_ppw), (33, 2, want_ppw)], (plan, total)
        assert all(1 < ppw < 64 // nsets for _, nsets, ppw, _ in plan)
        got = _points_call(rf, torch, joints, joints, pts, off, B_PAIRS, -1, B101, 0, True)
        assert got.shape == (3, total, 1)
        checked = np.zeros((3, B_IMAGES), bool)
        for p in range(3):
            for i in with_points:
                sl = slice(int(off[i]), int(off[i + 1]))
                x, y = pts[sl, 0], pts[sl, 1]
                what = "%s pool %d pair %s image %d plan %s" % (shape, pool, B_PAIRS[p], i, plan)
                if (p, i) in full:
                    want = full[p, i][y, x]
                    assert np.array_equal(got[p, sl], want), _mismatch(
                        got[p, sl], want, pts[sl], np.array([0]), "oracle, " + what)
                    checked[p, i] = True
                if p == 2:
                    want = full_r99[i][y, x]
                    assert np.array_equal(got[p, sl], want), _mismatch(
                        got[p, sl], want, pts[sl], np.array([0]), "rf_jbf_u8, " + what)
                    checked[p, i] = True
        assert checked[:, with_points].all()
    print("points case b %s: oracle %.1f s" % (shape, oracle_s))


# ---- c. seeded fuzz --------------------------------------------------------------------------------

C_SIGMA_COLOR = [20, 15, 4, 60, 0.5, 0, -1]
C_MODES = ("one", "capped", "full_odd", "full64")
# nsets with 64 % nsets != 0 and 64 // nsets >= 3
C_ODD_SETS = (3, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15, 17, 18, 19, 20, 21)
C_CLASSES = ("ppw==1", "1<ppw<64/nsets", "ppw==64/nsets,64%nsets!=0", "ppw==64", "partial_last_wave",
             "wave_in_two_images")


def plan_classes(plan, off):
    """The mapping classes a call with this plan and these point offsets runs."""
    total = int(off[-1])
    inner = [int(b) for b in off[1:-1] if 0 < b < total]
    seen = set()
    for _, nsets, ppw, _ in plan:
        if ppw == 1:
            seen.add(C_CLASSES[0])
            continue
        if ppw < 64 // nsets:
            seen.add(C_CLASSES[1])
        elif 64 % nsets:
            seen.add(C_CLASSES[2])
        if ppw == 64:
            seen.add(C_CLASSES[3])
        if total % ppw:
            seen.add(C_CLASSES[4])
        if any(b % ppw for b in inner):           # points b - 1 and b share a wave
            seen.add(C_CLASSES[5])
    return seen


def draw_fuzz_case(rng, index):
    """One random case (host data only): shapes, channels, border, d, flags, grid, point list.  The
    first 16 cases cycle through C_MODES, which steer the grid and the number of points towards
    one mapping class each; later ones draw the mode."""
    from reflectance_filtering_amd import _ffi
    mode = C_MODES[index % 4] if index < 16 else str(rng.choice(C_MODES))
    slab = mode in ("one", "capped") and rng.random() < (1.0 / 3.0)      # about every sixth case
    u = rng.random()
    if u < 0.08:
        h, w = 1, 1
    elif u < 0.2:
        h, w = (1, int(rng.integers(2, 56))) if rng.random() < 0.5 else (int(rng.integers(2, 40)), 1)
    else:
        h, w = int(rng.integers(1, 40)), int(rng.integers(1, 56))
    if slab:
        h, w = min(h, 30), min(w, 40)
    jcn, scn = int(rng.choice([1, 3])), int(rng.choice([1, 3]))
    grey = jcn == 1 and rng.random() < 0.5
    border = int(rng.integers(0, 5))
    flags = (TRUE_DIVISION if rng.random() < 0.4 else 0) | (FORCE_GENERIC if rng.random() < 0.15 else 0)
    n = int(rng.integers(1, 6)) if mode == "one" else int(rng.integers(2, 6))
    # the grid: 1-6 sigma_space values with 1-70 sets each
    dkind = int(rng.integers(0, 3))               # -1, odd, even
    counts = [int(rng.integers(1, 71)) if rng.random() < 0.5 else int(rng.choice([1, 2, 3, 5, 8, 33, 64, 65]))
              for _ in range(int(rng.integers(1, 7)))]
    if slab and dkind:                            # d > 0 gives every group the slab radius
        counts = [int(rng.integers(1, 4)) for _ in range(int(rng.integers(1, 3)))]
    if mode == "capped":
        counts[0] = int(rng.choice([1, 2, 3, 4, 5, 8]))
    elif mode == "full_odd":
        counts[0] = int(rng.choice(C_ODD_SETS))
    elif mode == "full64":
        counts[0] = 1
    radii = [int(rng.integers(1, 13)) for _ in counts]
    if slab:
        radii[-1], counts[-1] = int(rng.integers(54, 141)), int(rng.integers(1, 4))
    if dkind == 0:
        d = -1
        sigma_space = [(r + float(rng.uniform(-0.3, 0.3))) / 1.5 for r in radii]
        if rng.random() < 0.2:                    # sigma_space <= 0 counts as 1 (radius 2)
            sigma_space[0] = float(rng.choice([0.0, -1.0]))
    else:
        r = radii[-1] if slab else int(rng.integers(1, 13))
        d = 2 * r + 1 if dkind == 1 else 2 * max(r, 1)
        sigma_space = list(rng.permutation(np.arange(1, 41))[:len(counts)] * 0.5)
    pairs = [(float(rng.choice(C_SIGMA_COLOR)), float(ss)) for ss, c in zip(sigma_space, counts)
             for _ in range(c)]
    pairs = [pairs[i] for i in rng.permutation(len(pairs))]
    eff = flags | (GREY_AS_BGR if grey else 0)
    plan0 = _ffi.jbf_points_plan([ss for _, ss in pairs], d, jcn, eff, 0)
    nchunks = len(plan0)
    # the number of points: cap = total * nchunks // 4096 is what the mode asks for
    if mode == "one":
        total = int(rng.integers(1, min(600, (8191 // nchunks)) + 1))
    else:
        if mode == "capped":
            cap = int(rng.integers(2, 6))         # below 64 // counts[0] >= 8
        elif mode == "full_odd":
            cap = 64 // counts[0] + int(rng.integers(0, 3))
        else:
            cap = 64 + int(rng.integers(0, 4))
        lo = -(-cap * 4096 // nchunks)
        total = lo + int(rng.integers(0, max(1, 4096 // nchunks)))
        assert total * nchunks // 4096 == cap
    # the list: random shares, images without points at any position, corners, edges, duplicates
    share = rng.random(n) * (rng.random(n) > 0.25)
    if mode != "one":
        share[rng.permutation(n)[:2]] += 0.3      # at least two images have points
    if not share.any():
        share[int(rng.integers(0, n))] = 1.0
    per_image = rng.multinomial(total, share / share.sum())
    off = _offsets(per_image)
    pts = np.stack([rng.integers(0, w, total), rng.integers(0, h, total)], axis=1)
    special = np.array([(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w // 2, 0), (w // 2, h - 1),
                        (0, h // 2), (w - 1, h // 2)])
    for i in range(n):
        k0, k1 = int(off[i]), int(off[i + 1])
        m = min(k1 - k0, 8)
        where = k0 + rng.permutation(k1 - k0)[:m]
        pts[where] = special[rng.permutation(8)[:m]]
        if k1 - k0 >= 4:                          # duplicates of earlier points of the image
            dup = k0 + rng.integers(1, k1 - k0, (k1 - k0) // 8 + 1)
            pts[dup] = pts[k0 + rng.integers(0, dup - k0)]
    kinds = [int(rng.integers(0, 4)) for _ in range(2 * n)]
    plan = _ffi.jbf_points_plan([ss for _, ss in pairs], d, jcn, eff, total)
    return dict(mode=mode, slab=slab, h=h, w=w, jcn=jcn, scn=scn, grey=grey, border=border,
                flags=flags, n=n, d=d, pairs=pairs, total=total, pts=pts.astype(np.int32), off=off,
                kinds=kinds, plan=plan, classes=plan_classes(plan, off))


def test_point_lists_random_cases_match_the_oracle(env):
    """rf_jbf_points_u8 on random shapes down to 1x1 and 1xN, both channel counts, all five
    borders, d = -1 / odd / even, sigma_color from [20, 15, 4, 60, 0.5, 0, -1], grids of 1-6
    sigma_space values with 1-70 sets each (radii 1-12, a slab radius 54-140 in about every sixth
    case), random RF_JBF_TRUE_DIVISION / FORCE_GENERIC / GREY_AS_BGR, point lists with duplicates,
    corners, edges and images without points: every byte against the oracle on the whole image,
    and every mapping class of the plan (C_CLASSES) at least three times."""
    rf, co, torch = env
    rng = np.random.default_rng(65536 + SEED)
    t_end = time.time() + SECONDS
    cases = 0
    seen = dict.fromkeys(C_CLASSES, 0)
    while time.time() < t_end or cases < 16:
        c = draw_fuzz_case(rng, cases)
        h, w, n = c["h"], c["w"], c["n"]
        img_rng = np.random.default_rng([65536 + SEED, cases])
        joints = np.stack([_image(img_rng, h, w, c["jcn"], k) for k in c["kinds"][:n]])
        srcs = np.stack([_image(img_rng, h, w, c["scn"], k % 3) for k in c["kinds"][n:]])
        pts, off, pairs = c["pts"], c["off"], c["pairs"]
        got = _points_call(rf, torch, joints, srcs, pts, off, pairs, c["d"], c["border"],
                           c["flags"], c["grey"])
        assert got.shape == (len(pairs), c["total"], c["scn"])
        cache = {}
        for p, pair in enumerate(pairs):
            if pair not in cache:
                cache[pair] = _oracle_at_points(co, joints, srcs, pts, off, pair[0], pair[1], c["d"],
                                                c["border"], c["flags"], c["grey"])
            want = cache[pair]
            assert np.array_equal(got[p], want), _mismatch(
                got[p], want, pts, off, "case %d mode %s set %d %s %dx%d n %d jcn %d scn %d grey %s "
                "border %d flags %d d %d offsets %s plan %s" % (
                    cases, c["mode"], p, pair, h, w, n, c["jcn"], c["scn"], c["grey"], c["border"],
                    c["flags"], c["d"], off.tolist(), c["plan"]))
        for name in c["classes"]:
            seen[name] += 1
        cases += 1
    print("point-list fuzz: %d cases (%s)" % (cases, ", ".join("%s %d" % kv for kv in seen.items())))
    assert min(seen.values()) >= 3, seen


# ---- d. the sweep against values no kernel computed -----------------------------------------------

D_SHAPE = (48, 64)
D_COUNTS = (700, 0, 130, 65, 600, 12, 1, 650, 560, 0, 800, 90)    # comparisons per image
D_ZERO_WEIGHT = 5                                                  # this image's weights are all 0
D_PAIRS = {"bilateral": [(20, 22), (15, 28), (25, 4), (10, 4), (7, 12), (30, 9)],
           "guided": [(20, 22), (3, 45), (7, 52), (15, 5)]}


def case_d_comparisons(seed=0):
    from tests.test_gpu_jbf_points import _comparisons
    h, w = D_SHAPE
    rng = np.random.default_rng(600 + seed)
    comps = [_comparisons(h, w, rng, m, n_points=max(2, int(0.9 * m))) for m in D_COUNTS]
    comps[D_ZERO_WEIGHT][:, 5] = 0.0
    comps[2][:9, 4] = 0                                            # 'E' judgements
    return comps


def _host_whdr(W, filtered_hwc, comp, delta):
    """Host arithmetic only: bytes -> planar float32 / 255 -> whdr.whdr (pinned to the reference's
    own whdr by tests/golden/whdr.npz)."""
    planar = np.ascontiguousarray(np.transpose(filtered_hwc, (2, 0, 1)))
    return float(W.whdr(planar.astype(np.float32) / np.float32(255), comp, delta))


def _oracle_filter(co, ftype, joint, src, sc, ss):
    joint3 = np.repeat(joint, 3, axis=2)
    if ftype == "bilateral":
        return co.joint_bilateral_filter(joint3, src, -1, sc, ss).reshape(src.shape)
    return co.guided_filter(joint3, src, int(ss), sc).reshape(src.shape)


def _tie_deltas(filtered, comps):
    """tests/test_gpu_jbf_points.py's _tie_delta on the oracle's bytes: a delta whose
    float32(1 + delta) is exactly the ratio of a judged pair's lightnesses, and the delta one
    float32 ulp below it."""
    tiny = np.float32(np.finfo(np.float32).eps)
    for i, comp in enumerate(comps):
        for row in comp:
            x1, y1, x2, y2 = (int(v) for v in row[:4])
            l1 = np.float32(filtered[i][y1, x1].astype(np.float32) / np.float32(255)).mean(dtype=np.float32)
            l2 = np.float32(filtered[i][y2, x2].astype(np.float32) / np.float32(255)).mean(dtype=np.float32)
            lo, hi = sorted((max(l1, tiny), max(l2, tiny)))
            r = np.float32(hi / lo)
            if 1.02 < r < 1.5:
                return [float(r) - 1.0, float(np.nextafter(r, np.float32(0))) - 1.0]
    return []


@pytest.mark.parametrize("ftype", ["bilateral", "guided"])
@pytest.mark.parametrize("scn", [1, 3])
def test_sweep_equals_oracle_filter_then_host_whdr(env, ftype, scn):
    """whdr.sweep and whdr_points_u8 against oracle filter -> float32 bytes / 255 -> host whdr, as
    float64 bit for bit: 12 grey maps of 48x64 as BF / GF(CNN, CNN), 1 and 3 src channels, 0 to
    800 comparisons per image, one image with all-zero weights, delta 0.1 and the exact-tie deltas
    of a judged pair recomputed from the oracle's bytes.  The bilateral half runs at ppw > 1
    (asserted from the plan)."""
    rf, co, torch = env
    from reflectance_filtering_amd import whdr as W
    from tests import synth
    h, w = D_SHAPE
    n = len(D_COUNTS)
    joint = np.stack([np.ascontiguousarray(synth.reflectance_like_u8(h, w, 700 + i)[:, :, :1])
                      for i in range(n)])
    src = joint if scn == 1 else np.stack([synth.scene_u8(h, w, 720 + i) for i in range(n)])
    comps = case_d_comparisons()
    pairs = D_PAIRS[ftype]
    pts, point_offsets, dcomps, weights, comp_offsets = W.dedup_points(comps, h, w)
    if ftype == "bilateral":
        plan = _plan(pairs, -1, 1, GREY_AS_BGR, pts.shape[0])
        assert max(c[2] for c in plan) > 1, (plan, pts.shape[0])
    filtered = [[_oracle_filter(co, ftype, joint[i], src[i], sc, ss) for i in range(n)]
                for sc, ss in pairs]
    deltas = [0.1] + _tie_deltas(filtered[0], comps)
    assert len(deltas) == 3, "no judged pair with a usable ratio"
    jt, st = torch.from_numpy(joint).cuda(), torch.from_numpy(np.ascontiguousarray(src)).cuda()
    # the oracle's bytes at the deduplicated points, as the samples of whdr_points_u8
    img_of = np.repeat(np.arange(n), np.diff(point_offsets))
    samples = np.stack([np.stack(f)[img_of, pts[:, 1], pts[:, 0]] for f in filtered])
    for delta in deltas:
        want = np.array([[_host_whdr(W, filtered[p][i], comps[i], delta) for i in range(n)]
                         for p in range(len(pairs))], dtype=np.float64)
        assert np.all(want[:, [1, 9, D_ZERO_WEIGHT]] == 0) and np.any(want > 0)
        got = W.sweep(ftype, st, jt, comps, pairs, delta=delta, grey_as_bgr=True)
        assert got.dtype == np.float64 and got.shape == want.shape
        assert np.array_equal(got, want), (ftype, scn, delta, np.argwhere(got != want).tolist(),
                                           got[got != want], want[got != want])
        direct = W.whdr_points_u8(torch.from_numpy(np.ascontiguousarray(samples)).cuda(),
                                  point_offsets, dcomps, weights, comp_offsets, delta)
        assert np.array_equal(direct, want), (ftype, scn, delta, np.argwhere(direct != want).tolist())
