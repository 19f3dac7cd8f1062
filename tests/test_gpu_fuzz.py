"""GPU suite: seeded random cases against the ORACLE (not against another kernel), sized so that
the C oracle answers in milliseconds - every radius of the fused guided filter (1..96) and beyond,
every border type, channel combination and flag of the joint bilateral, chained passes, batches
that mix grey and colour images, the CNN with the shipped and with random weights, the grey-guide
guided filter with the debug switches that apply to it, both float filters (every kernel form of
rf_jbf_f32), the colourised outputs with infinite and NaN shading.  Bounded by
time: `RF_FUZZ_SECONDS` (default 40) per filter test; `RF_FUZZ_SEED` (default 0) offsets the seeds
for longer runs on other cases.
"""
import os
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SECONDS = float(os.environ.get("RF_FUZZ_SECONDS", "40"))
SEED = int(os.environ.get("RF_FUZZ_SEED", "0"))


@pytest.fixture(scope="module")
def env(built):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device visible")
    import reflectance_filtering_amd as rf
    from oracle import c_oracle as co
    torch.cuda.set_device(0)
    return rf, co, torch


def _image(rng, h, w, c, kind):
    """uint8 [h,w,c]: smooth field, posterised field, white noise or a constant."""
    if kind == 0:
        yy, xx = np.mgrid[0:h, 0:w]
        base = sum(np.sin(xx * rng.uniform(0.02, 0.4) + yy * rng.uniform(0.02, 0.4) + rng.uniform(0, 6))
                   for _ in range(3))
        img = 128 + 40 * base[..., None] + rng.normal(0, 6, (h, w, c))
    elif kind == 1:
        img = rng.integers(0, 5, (h // 7 + 1, w // 9 + 1, c)).repeat(7, 0).repeat(9, 1)[:h, :w] * 60 + 7
    elif kind == 2:
        img = rng.integers(0, 256, (h, w, c))
    else:
        img = np.full((h, w, c), int(rng.integers(0, 256)))
    return np.clip(np.round(img), 0, 255).astype(np.uint8)


def test_guided_filter_random_cases_match_the_oracle(env):
    rf, co, torch = env
    rng = np.random.default_rng(2024 + SEED)
    t_end = time.time() + SECONDS
    cases = exact_cases = 0
    while time.time() < t_end or cases < 12:
        h, w = int(rng.integers(1, 150)), int(rng.integers(1, 220))
        radius = int(rng.integers(1, 101)) if rng.random() < 0.8 else int(rng.choice([45, 52, 104, 120, 128, 129]))
        # (round 6) a sixth of the cases through the exact-row stage 2: its radii, a width that is a
        # multiple of 16 - white-noise guides and tiny eps make rows fail the test, constants pass it
        exact = rng.random() < 1.0 / 6.0
        if exact:
            radius, w = int(rng.choice([45, 52])), 16 * int(rng.integers(1, 14))
        eps = float(rng.choice([3.0, 7.0, 0.5, 1e-3, 200.0]))
        iters = int(rng.choice([1, 1, 2, 3]))
        n = int(rng.integers(1, 4))
        scn = int(rng.choice([1, 3]))
        guides = [_image(rng, h, w, 3, int(rng.integers(0, 4))) for _ in range(n)]
        srcs = []
        for _ in range(n):
            s = _image(rng, h, w, scn, int(rng.integers(0, 3)))
            if scn == 3 and rng.random() < 0.4:          # a grey image among colour ones
                s = np.repeat(s[:, :, :1], 3, axis=2)
            srcs.append(s)
        with rf._ffi.debug_options(gf_exact=int(exact)):
            got = rf.ops.guided_filter_u8(torch.from_numpy(np.stack(guides)).cuda(),
                                          torch.from_numpy(np.stack(srcs)).cuda(), radius, eps,
                                          iterations=iters).cpu().numpy()
        exact_cases += int(exact)
        for i in range(n):
            cur = srcs[i]
            for _ in range(iters):
                cur = co.guided_filter(guides[i], cur, radius, eps).reshape(srcs[i].shape)
            assert np.array_equal(got[i], cur), (cases, h, w, radius, eps, iters, scn, i)
        cases += 1
    print("guided-filter fuzz: %d cases (%d through the exact-row stage 2)" % (cases, exact_cases))


def test_joint_bilateral_random_cases_match_the_oracle(env):
    """rf_jbf_u8 on batches of 1-3 distinct images with random RF_JBF_TRUE_DIVISION (at tile64,
    strip and slab radii alike), RF_JBF_FORCE_GENERIC, RF_JBF_GREY_AS_BGR on a 1-channel joint
    (against the oracle on the repeated joint) and, sometimes, one tensor as joint and src
    (OpenCV's bilateralFilter route)."""
    rf, co, torch = env
    rng = np.random.default_rng(4048 + SEED)
    t_end = time.time() + SECONDS
    cases = 0
    seen = {"true_div_tile": 0, "true_div_slab": 0, "generic": 0, "grey_as_bgr": 0, "same": 0}
    while time.time() < t_end or cases < 16:
        h, w = int(rng.integers(1, 110)), int(rng.integers(1, 150))
        jcn, scn = int(rng.choice([1, 3])), int(rng.choice([1, 3]))
        # radius 33 42 8 18 51 2 38 46 | 54 60 64 70 76 99 130 140 (tap-row slabs)
        ss = float(rng.choice([22.0, 28.0, 5.0, 12.3, 34.0, 1.0, 25.0, 31.0, 36.0, 40.0, 42.9, 47.0, 50.5,
                               66.0, 86.7, 93.3]))
        sc = float(rng.choice([20.0, 15.0, 4.0, 60.0, 0.5]))
        d = int(rng.choice([-1, -1, 5, 9, 31]))
        border = int(rng.choice([0, 1, 2, 3, 4]))
        n = int(rng.integers(1, 4))
        flags = (rf._ffi.JBF_TRUE_DIVISION if rng.random() < 0.4 else 0) | \
                (rf._ffi.JBF_FORCE_GENERIC if rng.random() < 0.15 else 0)
        grey = jcn == 1 and rng.random() < 0.5
        same = jcn == scn and rng.random() < 0.2
        joints = np.stack([_image(rng, h, w, jcn, int(rng.integers(0, 4))) for _ in range(n)])
        srcs = joints if same else np.stack([_image(rng, h, w, scn, int(rng.integers(0, 3)))
                                             for _ in range(n)])
        jd = torch.from_numpy(joints).cuda()
        sd = jd if same else torch.from_numpy(srcs).cuda()
        got = rf.ops.joint_bilateral_u8(jd, sd, d, sc, ss, border=border, flags=flags,
                                        grey_as_bgr=grey).cpu().numpy()
        for i in range(n):
            joint = np.repeat(joints[i], 3, axis=2) if grey else joints[i]
            want = co.joint_bilateral_filter(joint, srcs[i], d, sc, ss, border=border,
                                             flags=flags & co.FLAG_TRUE_DIVISION).reshape(srcs[i].shape)
            assert np.array_equal(got[i], want), (cases, h, w, jcn, scn, sc, ss, d, border, n, flags,
                                                  grey, same, i)
        radius = co.jbf_radius(d, ss)
        if flags & rf._ffi.JBF_TRUE_DIVISION:
            seen["true_div_tile" if radius <= 52 else "true_div_slab"] += 1
        seen["generic"] += bool(flags & rf._ffi.JBF_FORCE_GENERIC)
        seen["grey_as_bgr"] += grey
        seen["same"] += same
        cases += 1
    print("joint-bilateral fuzz: %d cases (%s)" % (cases, ", ".join("%s %d" % kv for kv in seen.items())))


def test_cnn_random_cases_match_the_oracle(env):
    """Random image sizes (odd pixel counts: the kernel pairs pixel i with pixel i + half), image
    statistics and - every other case - random weights of the magnitude of the shipped ones:
    float output within 2e-7 of the oracle (the contract of test_cnn_matches_oracle_and_golden),
    bytes within one count on < 1e-4 of the pixels."""
    rf, co, torch = env
    rng = np.random.default_rng(777 + SEED)
    shipped = rf.weights.load_weights()
    t_end = time.time() + SECONDS / 4
    cases = 0
    worst = 0.0
    while time.time() < t_end or cases < 6:
        h, w = int(rng.integers(1, 90)), int(rng.integers(1, 130))
        n = int(rng.integers(1, 4))
        imgs = np.stack([_image(rng, h, w, 3, int(rng.integers(0, 4))) for _ in range(n)])
        if cases % 2:
            wts = (shipped * rng.uniform(0.5, 1.5, shipped.shape)
                   + rng.normal(0, 0.02, shipped.shape)).astype(np.float32)
        else:
            wts = shipped
        r, r8 = rf.ops.cnn_reflectance_u8(torch.from_numpy(imgs).cuda(), weights=wts)
        r, r8 = r.cpu().numpy(), r8.cpu().numpy()
        for i in range(n):
            want_r, want_r8 = co.cnn_reflectance(imgs[i], wts)
            err = float(np.abs(r[i] - want_r).max())
            worst = max(worst, err)
            assert err <= 2e-7, (cases, h, w, i, err)
            d8 = np.abs(r8[i].astype(int) - want_r8.astype(int))
            assert d8.max() <= 1 and np.mean(d8 != 0) < 1e-4 + 1.0 / d8.size, (cases, h, w, i)
        cases += 1
    print("CNN fuzz: %d cases, largest |r - oracle| %.3g" % (cases, worst))


# switches of include/reflectance_filtering_debug.h that apply to the grey-guide guided filter
# (identical bytes by contract); a value of None draws the option's value
_GF_SWITCHES = (("gf_two_kernel", 1), ("gf_one_stream", 1), ("gf_force_two_streams", 1),
                ("gf_no_compact", 1), ("gf_s1_legacy_strips", 1), ("gf_seg_rows", None),
                ("gf_s1_cap", None))


def test_grey_guide_guided_filter_random_cases_match_the_oracle(env):
    """rf_gf_ex_u8 + RF_GF_GREY_AS_BGR: shapes down to 1x1 and 1xN, radius 0..150 (0, 128, 129 and
    >128 always among them), tiny to large eps, chained passes, grey and colour srcs mixed, one
    debug switch per case (checked against the default kernels too), in place and through a
    one-image workspace (the call splits into chunks) - against the oracle on the guide repeated
    to three channels."""
    rf, co, torch = env
    lib = rf._ffi.load_library()
    rng = np.random.default_rng(6072 + SEED)
    forced = [0, 128, 129, int(rng.integers(130, 151))]
    t_end = time.time() + SECONDS
    cases = 0
    seen = {"r0": 0, "r128": 0, "r129": 0, "r>129": 0, "switch": 0, "in_place": 0, "chunked": 0,
            "1xN": 0}
    while time.time() < t_end or cases < 16:
        u = rng.random()
        if u < 0.08:
            h, w = 1, 1
        elif u < 0.2:
            h, w = (1, int(rng.integers(2, 220))) if rng.random() < 0.5 else (int(rng.integers(2, 150)), 1)
        else:
            h, w = int(rng.integers(1, 150)), int(rng.integers(1, 220))
        if cases < len(forced):
            radius = forced[cases]
        elif rng.random() < 0.7:
            radius = int(rng.integers(0, 151))
        else:
            radius = int(rng.choice([0, 1, 45, 52, 128, 129, 150]))
        eps = float(rng.choice([0.5, 1e-3, 3.0, 7.0, 200.0]))
        iters = int(rng.integers(1, 4))
        n = int(rng.integers(1, 4))
        scn = int(rng.choice([1, 3]))
        guides = np.stack([_image(rng, h, w, 1, int(rng.integers(0, 4))) for _ in range(n)])
        srcs = []
        for _ in range(n):
            s = _image(rng, h, w, scn, int(rng.integers(0, 4)))
            if scn == 3 and rng.random() < 0.4:          # a grey image among colour ones
                s = np.repeat(s[:, :, :1], 3, axis=2)
            srcs.append(s)
        srcs = np.stack(srcs)
        opts = {}
        if rng.random() < 0.6:
            name, value = _GF_SWITCHES[int(rng.integers(0, len(_GF_SWITCHES)))]
            if value is None:
                value = int(rng.integers(1, 65)) if name == "gf_seg_rows" else int(rng.integers(1, 4))
            opts[name] = value
        mode = int(rng.choice([0, 0, 1, 2]))            # 1: in place, 2: one-image workspace
        g1 = torch.from_numpy(guides).cuda()
        s = torch.from_numpy(srcs).cuda()
        ws = None
        if mode == 2:
            ws = torch.empty(lib.rf_gf_workspace_bytes(1, h, w, 1, scn, radius), dtype=torch.uint8,
                             device=s.device)
        with rf._ffi.debug_options(**opts):
            if mode == 1:
                got = s.clone()
                rf.ops.guided_filter_u8(g1, got, radius, eps, iterations=iters, out=got,
                                        grey_as_bgr=True)
            else:
                got = rf.ops.guided_filter_u8(g1, s, radius, eps, iterations=iters, workspace=ws,
                                              grey_as_bgr=True)
        if opts:
            plain = rf.ops.guided_filter_u8(g1, s, radius, eps, iterations=iters, grey_as_bgr=True)
            assert torch.equal(got, plain), (cases, h, w, radius, eps, iters, n, scn, opts, mode)
        got = got.cpu().numpy()
        for i in range(n):
            guide3 = np.repeat(guides[i], 3, axis=2)
            cur = srcs[i]
            for _ in range(iters):
                cur = co.guided_filter(guide3, cur, radius, eps).reshape(srcs[i].shape)
            assert np.array_equal(got[i], cur), (cases, h, w, radius, eps, iters, n, scn, opts, mode, i)
        seen["r0"] += radius == 0
        seen["r128"] += radius == 128
        seen["r129"] += radius == 129
        seen["r>129"] += radius > 129
        seen["switch"] += bool(opts)
        seen["in_place"] += mode == 1
        seen["chunked"] += mode == 2 and n > 1
        seen["1xN"] += min(h, w) == 1
        cases += 1
    assert seen["r0"] and seen["r128"] and seen["r129"] and seen["r>129"]
    print("grey-guide guided-filter fuzz: %d cases (%s)"
          % (cases, ", ".join("%s %d" % kv for kv in seen.items())))


def _float_image(rng, h, w, c, kind):
    """float32 [h,w,c] in one of the value ranges the float filters are fuzzed on:
    0 [0,1], 1 [-1,2], 2 [0,1] x 1e-3, 3 integer-valued x 1e3, 4 two values (every channel of a
    pixel the same one: the colour distance of two different pixels is the whole table)."""
    base = _image(rng, h, w, c, int(rng.integers(0, 3))).astype(np.float32) / np.float32(255)
    if kind == 0:
        return base
    if kind == 1:
        return base * np.float32(3) - np.float32(1)
    if kind == 2:
        return base * np.float32(1e-3)
    if kind == 3:
        return np.round(base * 255).astype(np.float32) * np.float32(1e3)
    a, b = np.float32(rng.uniform(-2, 2)), np.float32(rng.uniform(-2, 2))
    pick = rng.random((h, w, 1)) < 0.5
    return np.ascontiguousarray(np.repeat(np.where(pick, a, b), c, axis=2).astype(np.float32))


_F32_SPAN = {0: 1.0, 1: 3.0, 2: 1e-3, 3: 255e3, 4: 4.0}
_FLT_EPSILON = float(np.finfo(np.float32).eps)


def _jbf_f32_form(joints, d, sigma_color, sigma_space):
    """Which kernel rf_jbf_f32 picks (its host code, restated): "untiled" when the full table and
    the weight rows do not fit 64 KiB of LDS, else "pair" when the pair form of the table does
    (the table of the batch that reaches zero last decides), else "quad".  The full table leaves
    room for the weight rows up to radius 40 at jcn = 3 and up to radius 72 at jcn = 1."""
    jcn = joints.shape[-1]
    sigma_color = sigma_color if sigma_color > 0 else 1.0
    sigma_space = sigma_space if sigma_space > 0 else 1.0
    radius = max(1, int(np.rint(sigma_space * 1.5)) if d <= 0 else d // 2)
    r4 = (radius + 3) & ~3
    sw = (radius + 1) * 2 * (r4 + 8)
    bins = 4096 * jcn
    if ((bins + 2 + 3) & ~3) + sw > 16384:
        return "untiled"
    coeff = -0.5 / (sigma_color * sigma_color)
    zmax = 0
    for j in joints:
        span = np.float32(float(j.max()) - float(j.min())) * np.float32(jcn)
        scale_index = np.float32(np.float32(bins) / span)
        val = np.arange(bins + 2, dtype=np.float64) / np.float64(scale_index)
        lut = np.exp(val * val * coeff).astype(np.float32)
        zero = np.flatnonzero(lut == 0)
        zmax = max(zmax, int(zero[0]) if zero.size else bins + 2)
    npair = zmax + 1
    if npair <= bins + 3 and ((2 * npair + 3) & ~3) + sw <= 16384:
        return "pair"
    return "quad"


def test_float_joint_bilateral_random_cases_match_the_oracle(env):
    """rf_jbf_f32 on random shapes, channel pairs, borders 1-4, d = -1 / odd / even, radii up to 80,
    value ranges [0,1], [-1,2], x1e-3, integer-valued x1e3 and two-valued joints, sigma_color small
    and large against the range (tables that end early and tables that never reach zero): every
    form of the kernel (restated choice: _jbf_f32_form) at least three times, each against the
    oracle and against the one-thread-per-pixel kernel.  A joint whose range is below FLT_EPSILON
    is refused by both."""
    rf, co, torch = env
    rng = np.random.default_rng(8192 + SEED)
    t_end = time.time() + SECONDS / 2
    cases = 0
    forms = {"pair": 0, "quad": 0, "untiled": 0}
    refused = 0
    while time.time() < t_end or cases < 18:
        want_form = ("untiled", "quad", "pair")[cases % 3] if cases < 18 else None
        h, w = int(rng.integers(1, 70)), int(rng.integers(1, 100))
        jcn, scn = int(rng.choice([1, 3])), int(rng.choice([1, 3]))
        n = int(rng.integers(1, 3))
        kind = int(rng.integers(0, 5))
        border = int(rng.integers(1, 5))
        sc_rel = float(rng.choice([0.003, 0.03, 0.1, 0.5, 3.0, 50.0]))
        if want_form == "untiled":
            jcn = 3
            radius = int(rng.integers(41, 81))
        elif want_form == "quad":
            jcn, sc_rel = 3, 50.0
            radius = int(rng.integers(1, 41))
        elif want_form == "pair":
            sc_rel = 0.003
            radius = int(rng.integers(1, 41))
        else:
            radius = int(rng.integers(1, 81))
        u = rng.random()
        if u < 0.5:
            d, ss = -1, radius / 1.5
        elif u < 0.75:
            d, ss = 2 * radius + 1, float(rng.uniform(0.5, 40))
        else:
            d, ss = 2 * radius, float(rng.uniform(0.5, 40))
        sc = sc_rel * _F32_SPAN[kind]
        joints = np.stack([_float_image(rng, h, w, jcn, kind) for _ in range(n)])
        srcs = np.stack([_float_image(rng, h, w, scn, int(rng.integers(0, 4))) for _ in range(n)])
        flat = [abs(float(j.max()) - float(j.min())) < _FLT_EPSILON for j in joints]
        jd, sd = torch.from_numpy(joints).cuda(), torch.from_numpy(srcs).cuda()
        if any(flat):
            with pytest.raises(ValueError, match="constant joint"):
                rf.ops.joint_bilateral_f32(jd, sd, d, sc, ss, border=border)
            for i in np.flatnonzero(flat):
                with pytest.raises(NotImplementedError):
                    co.joint_bilateral_filter_f32(joints[i], srcs[i], d, sc, ss, border=border)
            refused += 1
            continue
        form = _jbf_f32_form(joints, d, sc, ss)
        got = rf.ops.joint_bilateral_f32(jd, sd, d, sc, ss, border=border).cpu().numpy()
        for i in range(n):
            want = co.joint_bilateral_filter_f32(joints[i], srcs[i], d, sc, ss, border=border)
            assert np.array_equal(got[i], want.reshape(got[i].shape)), \
                (cases, form, h, w, jcn, scn, n, kind, border, d, sc, ss, i)
        if form != "untiled":
            with rf._ffi.debug_options(jbf_f32_untiled=1):
                ref = rf.ops.joint_bilateral_f32(jd, sd, d, sc, ss, border=border).cpu().numpy()
            assert np.array_equal(got, ref), (cases, form, h, w, jcn, scn, n, kind, border, d, sc, ss)
        forms[form] += 1
        cases += 1
    assert min(forms.values()) >= 3, forms
    print("float joint-bilateral fuzz: %d cases (%s), %d refused constant joints"
          % (cases, ", ".join("%s %d" % kv for kv in forms.items()), refused))


@pytest.mark.parametrize("jcn", [1, 3])
def test_float_joint_bilateral_refuses_a_range_below_flt_epsilon(env, jcn):
    """The constant-joint rule is `max - min < FLT_EPSILON` (in double, on the float values): just
    below it both the oracle and ops refuse; at it and just above it both filter, identically."""
    rf, co, torch = env
    h, w = 9, 11
    src = np.ascontiguousarray(_float_image(np.random.default_rng(jcn), h, w, 3, 0))
    pick = np.indices((h, w)).sum(axis=0)[:, :, None] % 3 == 0
    eps32 = np.float32(_FLT_EPSILON)
    for top, ok in ((np.nextafter(eps32, np.float32(0)), False), (eps32, True),
                    (np.nextafter(eps32, np.float32(1)), True)):
        joint = np.ascontiguousarray(np.repeat(np.where(pick, top, np.float32(0)), jcn, axis=2)
                                     .astype(np.float32))
        jd, sd = torch.from_numpy(joint[None]).cuda(), torch.from_numpy(src[None]).cuda()
        if not ok:
            with pytest.raises(NotImplementedError):
                co.joint_bilateral_filter_f32(joint, src, -1, 1e-7, 2.0)
            with pytest.raises(ValueError, match="constant joint"):
                rf.ops.joint_bilateral_f32(jd, sd, -1, 1e-7, 2.0)
            continue
        want = co.joint_bilateral_filter_f32(joint, src, -1, 1e-7, 2.0)
        got = rf.ops.joint_bilateral_f32(jd, sd, -1, 1e-7, 2.0).cpu().numpy()[0]
        assert np.array_equal(got, want), float(top)


_GF_F32_EPS = (0.0, 1e-4, 9.99e-3, 1e-2, 1e-2 * (1 + 2.0 ** -23), 3.0)


def test_float_guided_filter_random_cases_match_the_oracle(env):
    """rf_gf_f32: radius 0 and radii beyond the image, eps on both sides of the eps < 1e-2 branch,
    1-3 chained passes, batches of 1-3, grey and colour srcs, the float value ranges, in place
    (out = src) and through a one-image workspace (the C entry point splits the batch into
    chunks) - against the chained oracle, NaN where the oracle has NaN."""
    rf, co, torch = env
    lib = rf._ffi.load_library()
    rng = np.random.default_rng(16384 + SEED)
    t_end = time.time() + SECONDS / 2
    cases = 0
    seen = {"r0": 0, "r>image": 0, "eps<1e-2": 0, "eps>=1e-2": 0, "in_place": 0, "chunked": 0}
    while time.time() < t_end or cases < 16:
        h, w = int(rng.integers(1, 80)), int(rng.integers(1, 120))
        u = rng.random()
        radius = 0 if u < 0.2 else (int(rng.integers(max(h, w), max(h, w) + 40)) if u < 0.4
                                    else int(rng.integers(1, 60)))
        eps = float(rng.choice(_GF_F32_EPS))
        iters = int(rng.integers(1, 4))
        n = int(rng.integers(1, 4))
        scn = int(rng.choice([1, 3]))
        kind = int(rng.integers(0, 5))
        guides = np.stack([_float_image(rng, h, w, 3, kind) for _ in range(n)])
        srcs = np.stack([_float_image(rng, h, w, scn, int(rng.integers(0, 4))) for _ in range(n)])
        gd, sd = torch.from_numpy(guides).cuda(), torch.from_numpy(srcs).cuda()
        mode = int(rng.choice([0, 0, 1, 2]))            # 1: in place, 2: one-image workspace
        if mode == 0:
            got = rf.ops.guided_filter_f32(gd, sd, radius, eps, iterations=iters)
        elif mode == 1:
            got = sd.clone()
            rf.ops.guided_filter_f32(gd, got, radius, eps, iterations=iters, out=got)
        else:
            got = torch.empty_like(sd)
            ws = torch.empty(lib.rf_gf_f32_workspace_bytes(1, h, w, 3, scn, radius),
                             dtype=torch.uint8, device=sd.device)
            rc = lib.rf_gf_f32(gd.data_ptr(), sd.data_ptr(), got.data_ptr(), n, h, w, 3, scn, radius,
                               eps, iters, ws.data_ptr(), ws.numel(), rf._ffi.current_stream_ptr(torch))
            rf._ffi.check(rc, "rf_gf_f32")
        got = got.cpu().numpy()
        for i in range(n):
            cur = srcs[i]
            for _ in range(iters):
                cur = co.guided_filter_f32(guides[i], cur, radius, eps).reshape(srcs[i].shape)
            assert np.array_equal(got[i], cur, equal_nan=True), \
                (cases, h, w, radius, eps, iters, n, scn, kind, mode, i)
        seen["r0"] += radius == 0
        seen["r>image"] += radius >= max(h, w)
        seen["eps<1e-2" if eps < 1e-2 else "eps>=1e-2"] += 1
        seen["in_place"] += mode == 1
        seen["chunked"] += mode == 2 and n > 1
        cases += 1
    print("float guided-filter fuzz: %d cases (%s)" % (cases, ", ".join("%s %d" % kv for kv in seen.items())))


# pixel counts around the percentile rank rule's boundaries (tests/test_colorize.py)
_COLORIZE_PX = (333, 334, 667, 999, 1000, 1001, 1002, 2001)
_BYTE_256 = 1.0874   # rgb_to_srgb(x) * 255 reaches 256 near x = 1.08748: numpy's cast overflows above


def _colorize_shape(rng):
    if rng.random() < 0.5:
        npx = int(rng.choice(_COLORIZE_PX))
        divs = [k for k in range(1, npx + 1) if npx % k == 0]
        h = int(rng.choice(divs))
        return h, npx // h
    return int(rng.integers(1, 60)), int(rng.integers(1, 80))


def _colorize_floats(img, r):
    """The float64 shading and reflectance of oracle/colorize_numpy.py (for case bookkeeping)."""
    with np.errstate(all="ignore"):
        sh = img.astype(np.float64).sum(axis=2) / 3.0 / r.astype(np.float64)
        refl = img.astype(np.float64) / np.maximum(sh, 1e-3)[:, :, None]
    return sh, refl


def test_colorize_random_cases_match_the_oracle(env):
    """rf_colorize_srgb_u8 on batches mixing: r from the CNN, 10**U(-4,0), with denormals, with
    exact 1.0; r == 0 on non-black pixels below 0.1 % of them (the percentile stays finite) and
    above (the percentile is inf, inf/inf writes byte 0); r == 0 on black pixels (0/0: a NaN
    result, written without normalisation - its values above 1 count the sRGB steps past x = 1).
    Bytes equal to oracle/colorize_numpy.py."""
    from oracle import colorize_numpy as oc
    from reflectance_filtering_amd import image_utils as iu
    rf, co, torch = env
    rng = np.random.default_rng(32768 + SEED)
    t_end = time.time() + SECONDS / 4
    cases = 0
    seen = {"nan": 0, "inf_percentile": 0, "finite_with_inf": 0, "above_1": 0, "boundary_px": 0}
    while time.time() < t_end or cases < 16:
        h, w = _colorize_shape(rng)
        n = int(rng.integers(1, 4))
        imgs, rs = [], []
        for i in range(n):
            mode = (cases * 3 + i) % 6 if cases < 6 else int(rng.integers(0, 6))
            img = _image(rng, h, w, 3, int(rng.integers(0, 3)))
            if mode == 0:                                # the CNN's own r
                r = rf.ops.cnn_reflectance_u8(torch.from_numpy(img[None]).cuda(),
                                              want_u8=False)[0].cpu().numpy()[0]
            elif mode == 1:
                r = (10.0 ** rng.uniform(-4, 0, (h, w))).astype(np.float32)
            elif mode == 2:                              # denormals and exact 1.0 among them
                r = (10.0 ** rng.uniform(-3, 0, (h, w))).astype(np.float32)
                u = rng.random((h, w))
                r[u < 0.05] = np.float32(1.0)
                r[u > 0.97] = (rng.integers(1, 1 << 23, (h, w)).astype(np.uint32)
                               .view(np.float32))[u > 0.97]
            elif mode in (3, 4):                         # r == 0 on non-black pixels
                r = rng.uniform(0.05, 1.0, (h, w)).astype(np.float32)
                lit = np.flatnonzero(img.reshape(-1, 3).max(axis=1) > 0)
                room = h * w - 1 - iu.percentile_rank(h * w)   # infs the percentile stays finite with
                count = int(rng.integers(1, room + 1)) if mode == 3 and room else room + int(rng.integers(1, 4))
                r.reshape(-1)[rng.choice(lit, min(count, lit.size), replace=False)] = 0
            else:                                        # a NaN result: 0/0 on black pixels
                img = rng.integers(0, 2, (h, w, 3)).astype(np.uint8)
                img.reshape(-1, 3)[rng.integers(0, h * w)] = 0
                mean = img.astype(np.float64).sum(axis=2) / 3.0
                r = (mean / rng.uniform(0.93, 1.08, (h, w))).astype(np.float32)
                sh, refl = _colorize_floats(img, r)
                assert not (sh >= _BYTE_256).any() and not (refl >= _BYTE_256).any()
            imgs.append(img)
            rs.append(r)
        imgs, rs = np.stack(imgs), np.stack(rs)
        refl, shad = rf.ops.colorize_srgb_u8(torch.from_numpy(imgs).cuda(), torch.from_numpy(rs).cuda())
        refl, shad = refl.cpu().numpy(), shad.cpu().numpy()
        for i in range(n):
            want_refl, want_shad = oc.colorize_srgb_u8(imgs[i], rs[i])
            assert np.array_equal(refl[i], want_refl), (cases, h, w, n, i)
            assert np.array_equal(shad[i], want_shad), (cases, h, w, n, i)
            sh, rl = _colorize_floats(imgs[i], rs[i])
            if np.isnan(sh).any():
                seen["nan"] += 1
                seen["above_1"] += bool((sh > 1).any() or (rl > 1).any())
            elif np.isinf(sh).any():
                pct = np.sort(sh, axis=None)[iu.percentile_rank(h * w)]
                seen["inf_percentile" if np.isinf(pct) else "finite_with_inf"] += 1
        seen["boundary_px"] += h * w in _COLORIZE_PX
        cases += 1
    assert seen["nan"] and seen["inf_percentile"] and seen["finite_with_inf"]
    print("colorize fuzz: %d cases (%s)" % (cases, ", ".join("%s %d" % kv for kv in seen.items())))


@pytest.mark.parametrize("h,w,seed", [(20, 25, 0), (37, 27, 1), (1, 1, 2)])
def test_colorize_nan_result_is_written_unnormalised(env, h, w, seed):
    """A black pixel with r == 0 makes the shading 0/0 = NaN and that pixel's reflectance NaN.
    np.max of either result is then NaN, `NaN > 1` is false, and numpy writes it without
    normalisation: NaN as byte 0, values above 1 (here the shading 1/r of bytes 1) as bytes above
    246.  (Before, the device normalised both results: the NaN's bit pattern lies above 1.0's.)"""
    from oracle import colorize_numpy as oc
    rf, co, torch = env
    rng = np.random.default_rng(seed)
    img = np.ones((h, w, 3), np.uint8)
    r = rng.uniform(0.95, 0.999, (h, w)).astype(np.float32)
    img[h // 2, w // 2] = 0
    r[h // 2, w // 2] = 0
    refl, shad = rf.ops.colorize_srgb_u8(torch.from_numpy(img[None]).cuda(),
                                         torch.from_numpy(r[None]).cuda())
    want_refl, want_shad = oc.colorize_srgb_u8(img, r)
    assert want_shad[h // 2, w // 2] == 0 and (want_refl[h // 2, w // 2] == 0).all()
    if h * w > 1:
        assert want_shad.max() > 246
    assert np.array_equal(shad.cpu().numpy()[0], want_shad)
    assert np.array_equal(refl.cpu().numpy()[0], want_refl)
