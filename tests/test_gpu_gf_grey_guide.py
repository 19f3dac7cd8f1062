"""GPU: the guided filter with a grey guide (rf_gf_ex_u8 + RF_GF_GREY_AS_BGR,
ops.guided_filter_u8(grey_as_bgr=True)) - a 1-channel guide read as three equal channels.  Every
comparison is bitwise: against the oracle on the guide replicated to 3 channels, and against
rf_gf_u8 on that replicated guide."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(built):
    import torch
    import reflectance_filtering_amd as rf
    from oracle import c_oracle as co
    if not torch.cuda.is_available():
        pytest.skip("no HIP device visible (run with -m 'not gpu' on CPU-only machines)")
    rf._ffi.load_library()
    return rf, co, torch


def _grey_guide(h, w, seed):
    """Grey guide with flat regions (Voronoi cells) and texture (a smooth field plus noise)."""
    from tests import synth
    flat = synth.flat_guide_u8(h, w, seed, cells=9)[:, :, 0].astype(np.int32)
    tex = synth.reflectance_like_u8(h, w, seed + 1)[:, :, 0].astype(np.int32)
    rng = np.random.default_rng(seed)
    out = flat.copy()
    half = w // 2
    out[:, half:] = tex[:, half:] + rng.integers(-6, 7, (h, w - half))
    return np.clip(out, 0, 255).astype(np.uint8)


def _src(h, w, scn, seed):
    from tests import synth
    return (synth.scene_u8(h, w, seed) if scn == 3
            else synth.reflectance_like_u8(h, w, seed)[:, :, :1].copy())


def _dev(torch, *imgs):
    return [torch.from_numpy(np.ascontiguousarray(a if a.ndim == 4 else a[None])).cuda()
            for a in imgs]


def _rep3(t):
    return t.repeat(1, 1, 1, 3).contiguous()


# ------------------------------------------------------------------------- against the oracle
@pytest.mark.parametrize("radius", [0, 1, 9, 45, 52, 128, 129, 150])
@pytest.mark.parametrize("scn", [1, 3])
def test_grey_guide_matches_oracle_on_replicated_guide(env, radius, scn):
    rf, co, torch = env
    h, w = 61, 93                       # neither a multiple of 4 nor of 16
    guide = _grey_guide(h, w, seed=radius + 3)
    src = _src(h, w, scn, seed=radius + 11)
    g1, s = _dev(torch, guide[:, :, None], src)
    for eps in (3.0, 7.0, 0.0, 1e-7, 5e-3):
        got = rf.ops.guided_filter_u8(g1, s, radius, eps, grey_as_bgr=True)
        want = co.guided_filter(np.repeat(guide[:, :, None], 3, axis=2), src, radius, eps)
        assert np.array_equal(got[0].cpu().numpy(), want.reshape(h, w, scn)), (radius, eps)


@pytest.mark.parametrize("h,w", [(1, 1), (2, 3), (5, 7), (17, 1), (1, 33), (13, 250), (130, 47)])
def test_grey_guide_tiny_and_odd_sizes_match_oracle(env, h, w):
    rf, co, torch = env
    guide = _grey_guide(h, w, seed=h * 31 + w)
    for scn in (1, 3):
        src = _src(h, w, scn, seed=h + w)
        g1, s = _dev(torch, guide[:, :, None], src)
        for radius, eps in ((1, 3.0), (9, 1e-7), (52, 7.0)):
            got = rf.ops.guided_filter_u8(g1, s, radius, eps, grey_as_bgr=True)
            want = co.guided_filter(np.repeat(guide[:, :, None], 3, axis=2), src, radius, eps)
            assert np.array_equal(got[0].cpu().numpy(), want.reshape(h, w, scn)), (h, w, scn, radius)


# ------------------------------------------------------------------ against the colour guide
def _both(rf, g1, s, radius, eps, iterations=1):
    a = rf.ops.guided_filter_u8(g1, s, radius, eps, iterations=iterations, grey_as_bgr=True)
    b = rf.ops.guided_filter_u8(_rep3(g1), s, radius, eps, iterations=iterations)
    return a, b


def _tiled(h, w, seed, make):
    """A full-size image from a 270 x 480 one, tiled, plus noise (cheap to make at 4K)."""
    rng = np.random.default_rng(seed)
    small = make(270, 480).astype(np.int32)
    big = np.tile(small, (h // 270 + 1, w // 480 + 1) + (1,) * (small.ndim - 2))[:h, :w]
    return np.clip(big + rng.integers(-2, 3, big.shape), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("h,w", [(1080, 1920), (2160, 3840)])
def test_grey_guide_equals_replicated_guide_full_size(env, h, w):
    rf, co, torch = env
    guide = _tiled(h, w, 5, lambda a, b: _grey_guide(a, b, seed=5))
    src = _tiled(h, w, 6, lambda a, b: _src(a, b, 1, seed=6))
    g1, s = _dev(torch, guide[:, :, None], src)
    for radius, eps, its in ((52, 7.0, 1), (45, 3.0, 3)):
        a, b = _both(rf, g1, s, radius, eps, its)
        assert torch.equal(a, b), (h, w, radius, its)


def test_grey_guide_batches_two_halves_and_mixed_sources(env):
    """A batch of 12 forks its second half onto the side stream; grey and colour sources mixed in
    one 3-channel batch (the grey-source probe still decides per image)."""
    rf, co, torch = env
    h, w = 270, 333
    guides = np.stack([_grey_guide(h, w, seed=k)[:, :, None] for k in range(12)])
    srcs = []
    for k in range(12):
        s3 = _src(h, w, 3, seed=40 + k)
        if k % 3 == 0:                  # grey 3-channel source
            s3 = np.repeat(s3[:, :, :1], 3, axis=2)
        srcs.append(s3)
    g1, s = _dev(torch, guides, np.stack(srcs))
    for radius, eps, its in ((52, 7.0, 1), (9, 1e-7, 3), (0, 3.0, 1), (129, 3.0, 1)):
        a, b = _both(rf, g1, s, radius, eps, its)
        assert torch.equal(a, b), (radius, its)
    # grey 1-channel sources, the same batch size
    s1 = s[..., :1].contiguous()
    for radius, eps, its in ((52, 7.0, 1), (45, 3.0, 3)):
        a, b = _both(rf, g1, s1, radius, eps, its)
        assert torch.equal(a, b), (radius, its)
    # one stream and forced two streams say the same
    want = rf.ops.guided_filter_u8(g1[:4], s[:4], 45, 3.0, iterations=2, grey_as_bgr=True)
    for opt in ({"gf_one_stream": 1}, {"gf_force_two_streams": 1}, {"gf_two_kernel": 1},
                {"gf_no_compact": 1}, {"gf_s1_legacy_strips": 1}):
        with rf._ffi.debug_options(**opt):
            got = rf.ops.guided_filter_u8(g1[:4], s[:4], 45, 3.0, iterations=2, grey_as_bgr=True)
        assert torch.equal(got, want), opt


def test_grey_guide_in_place_and_one_image_workspace(env):
    rf, co, torch = env
    h, w = 200, 301
    n = 4
    g1, s = _dev(torch, np.stack([_grey_guide(h, w, seed=k)[:, :, None] for k in range(n)]),
                 np.stack([_src(h, w, 3, seed=k + 9) for k in range(n)]))
    for radius, its in ((52, 1), (9, 3), (128, 2), (150, 1)):
        want = rf.ops.guided_filter_u8(_rep3(g1), s, radius, 7.0, iterations=its)
        lib = rf._ffi.load_library()
        one = lib.rf_gf_workspace_bytes(1, h, w, 1, 3, radius)
        ws = torch.empty(one, dtype=torch.uint8, device=s.device)
        got = rf.ops.guided_filter_u8(g1, s, radius, 7.0, iterations=its, workspace=ws,
                                      grey_as_bgr=True)
        assert torch.equal(got, want), ("one-image workspace", radius, its)
        inplace = s.clone()
        rf.ops.guided_filter_u8(g1, inplace, radius, 7.0, iterations=its, out=inplace,
                                grey_as_bgr=True)
        assert torch.equal(inplace, want), ("in place", radius, its)


def test_grey_guide_captured_and_replayed(env):
    rf, co, torch = env
    h, w = 150, 190
    n = 8                               # forks the side stream inside the captured call
    g1, s = _dev(torch, np.stack([_grey_guide(h, w, seed=k)[:, :, None] for k in range(n)]),
                 np.stack([_src(h, w, 1, seed=k + 3) for k in range(n)]))
    out = torch.empty_like(s)
    ws = rf.ops.gf_workspace(n, h, w, 1, 52, s.device, torch)
    cap = rf.ops.CapturedCall(lambda: rf.ops.guided_filter_u8(g1, s, 52, 7.0, iterations=3, out=out,
                                                               workspace=ws, grey_as_bgr=True))
    for seed in (1, 2):
        s.copy_(torch.from_numpy(np.stack([_src(h, w, 1, seed=seed * 100 + k) for k in range(n)])))
        out.zero_()
        got = cap.replay()
        torch.cuda.synchronize()
        want = rf.ops.guided_filter_u8(_rep3(g1), s, 52, 7.0, iterations=3)
        assert torch.equal(got, want), seed


# ------------------------------------------------------------------------------ end to end
def test_decompose_and_filter_batch_guided(env):
    """GF(CNN, CNN) on the device == oracle CNN -> r_u8 -> oracle GF with r_u8 as its own
    3-channel guide (what the two CLIs do through `<base>-r.png`)."""
    from tests import synth
    rf, co, torch = env
    scenes = np.stack([synth.scene_u8(97, 141, seed=s) for s in (1, 2, 3)])
    r8, filt = rf.decompose_and_filter_batch(torch.from_numpy(scenes).cuda(), filter_type="guided",
                                             sigma_color=7, sigma_spatial=52)
    wts = rf.weights.load_weights()
    for i in range(3):
        _, want_r8 = co.cnn_reflectance(scenes[i], wts)
        assert np.array_equal(r8[i].cpu().numpy(), want_r8)
        r3 = np.repeat(want_r8[:, :, None], 3, 2)
        assert np.array_equal(filt[i].cpu().numpy(), co.guided_filter(r3, r3.copy(), 52, 7.0)[:, :, 0])
    # the default stays the bilateral
    _, bf = rf.decompose_and_filter_batch(torch.from_numpy(scenes[:1]).cuda())
    r3 = np.repeat(r8[0].cpu().numpy()[:, :, None], 3, 2)
    assert np.array_equal(bf[0].cpu().numpy(),
                          co.joint_bilateral_filter(r3, r3.copy(), -1, 20, 22)[:, :, 0])


def test_batch_filter_files_guided_grey_guidance(env, tmp_path):
    """batch.filter_files('guided') with grey guidance (the prediction as its own guidance, and a
    grey guidance file for a colour input) writes the bytes of apply_filter file by file."""
    from tests import synth
    rf, co, torch = env
    from reflectance_filtering_amd import batch
    iu = rf.image_utils
    preds, photos, out_dir, single = (tmp_path / d for d in ("preds", "photos", "out", "single"))
    for d in (preds, photos, out_dir, single):
        d.mkdir()
    sizes = [(60, 81), (60, 81), (45, 70)]
    for i, (h, w) in enumerate(sizes):
        iu.imwrite(str(preds / ("im%d-r.png" % i)), synth.reflectance_like_u8(h, w, seed=i))
        iu.imwrite(str(photos / ("im%d.png" % i)), synth.scene_u8(h, w, seed=i + 7))
    rfiles = batch.expand_inputs([str(preds / "*.png")])
    pfiles = batch.expand_inputs([str(photos / "*.png")])
    for files, pattern in ((rfiles, None), (pfiles, str(preds / "{stem}-r.png"))):
        for f in files:
            assert iu.imread(batch.guidance_for(f, pattern)).shape[2] == 3
        written = batch.filter_files("guided", files, pattern, 7.0, 52.0, str(out_dir))
        assert len(written) == len(files)
        for f, name in zip(files, written):
            img = iu.imread(f)
            gui = iu.imread(batch.guidance_for(f, pattern))
            want = rf.apply_filter("guided", img, gui, 7.0, 52.0)
            assert np.array_equal(iu.imread(name), want), name
            ref = co.guided_filter(gui, img, 52, 7.0)
            assert np.array_equal(want, ref), name
