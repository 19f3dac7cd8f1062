"""GPU suite: the ragged guided filter for several eps at one radius (ops.guided_filter_ragged_sweep_u8:
one packed list, one rf_gf_ragged_u8 call per eps) and the sweeps routed through it (whdr.sweep('guided')
over a mixed device list, sweep.run('guided')).  Every eps slice is held, byte for byte, to the ORACLE on
each image alone and to ops.guided_filter_ragged_u8 at that eps; no tolerance anywhere.

  a  the list at radii 1, 9, 45, 52, 128, both guide kinds, four eps on either side of the eps < 1e-2
     rule in one call; the ragged route asserted from the plan; src intact; guard bytes around dst
  b  1, 2, 8 and 9 eps
  c  the fallback routes (a colour src, radius 129) against per-eps calls
  d  whdr.sweep('guided') on an interleaved device list against oracle filter -> host whdr
  e  sweep.run('guided') on photos of three sizes against the per-photo path
"""
import numpy as np
import pytest

from tests.test_gpu_fuzz import env  # noqa: F401  (env is a fixture)
from tests.test_gpu_gf_ragged import _dev, _images, _oracle
from tests.test_gpu_points_fuzz import _host_whdr

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 4096, 0xA5
# smaller than every radius; one row-walk block and a strip; several row segments; 700 columns: two strips
# at radius 45 and above (at radius 1 and 9 the list's strip rule picks one 736-column strip); a tail block
# in the column walk (130 = 8 x 16 + 2): 29,197 pixels
SHAPES = [(1, 1), (3, 200), (70, 130), (130, 70), (9, 700), (64, 64)]
EPS = (3.0, 7.0, 1e-7, 5e-3)
EPS9 = (3.0, 7.0, 1e-7, 5e-3, 1.0, 5.0, 0.02, 9e-3, 100.0)

_cache = {}


def _inputs(gcn):
    """The list's guides and srcs (host), made once per guide kind."""
    if ("in", gcn) not in _cache:
        rng = np.random.default_rng(4100 + gcn)
        _cache["in", gcn] = (_images(rng, SHAPES, gcn), _images(rng, SHAPES, 1, 1))
    return _cache["in", gcn]


def _want(co, gcn, radius, eps):
    """The oracle on each image alone, packed: [total pixels, 1].  Computed once per case."""
    key = ("want", gcn, radius, eps)
    if key not in _cache:
        guides, srcs = _inputs(gcn)
        _cache[key] = np.concatenate([_oracle(co, g, s, radius, eps).reshape(-1, 1)
                                      for g, s in zip(guides, srcs)])
    return _cache[key]


def _sweep(rf, torch, guides, srcs, radius, eps_list):
    """One sweep call into a dst with GUARD sentinel bytes on either side: host [n_eps, total, C]; the
    packed srcs are checked to be intact afterwards."""
    grey = guides[0].shape[2] == 1
    g_p, sizes = rf.ops.pack_images(_dev(torch, guides), "guides", torch)
    s_p, _ = rf.ops.pack_images(_dev(torch, srcs), "srcs", torch)
    before = s_p.cpu().numpy().copy()
    total, scn = s_p.shape
    buf = torch.full((len(eps_list) * total * scn + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    out = buf[GUARD:GUARD + len(eps_list) * total * scn].view(len(eps_list), total, scn)
    got = rf.ops.guided_filter_ragged_sweep_u8(g_p, s_p, radius, eps_list, grey_as_bgr=grey, sizes=sizes,
                                               out=out)
    assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (len(eps_list), total, scn)
    host = buf.cpu().numpy()
    assert np.all(host[:GUARD] == SENTINEL), "bytes before dst were written"
    assert np.all(host[-GUARD:] == SENTINEL), "bytes after dst were written"
    assert np.array_equal(s_p.cpu().numpy(), before), "src was written"
    return got.cpu().numpy(), (g_p, s_p, sizes)


# ---- a. every radius class, both guide kinds, both sides of the small-eps rule -----------------------

@pytest.mark.parametrize("gcn", [1, 3])
@pytest.mark.parametrize("radius", [1, 9, 45, 52, 128])
def test_every_eps_slice_matches_the_oracle_and_the_single_eps_entry(env, radius, gcn):
    rf, co, torch = env
    flags = rf._ffi.GF_GREY_AS_BGR if gcn == 1 else 0
    plan = rf._ffi.gf_ragged_plan(SHAPES, gcn, 1, radius, flags)
    assert plan is not None and plan["launches"] == 3
    if radius >= 45:
        assert plan["out_w"] < 700                              # the 700-column image: two strips
    guides, srcs = _inputs(gcn)
    got, (g_p, s_p, sizes) = _sweep(rf, torch, guides, srcs, radius, EPS)
    for e, eps in enumerate(EPS):
        assert np.array_equal(got[e], _want(co, gcn, radius, eps)), (radius, gcn, eps)
        single, _ = rf.ops.guided_filter_ragged_u8(g_p, s_p, radius, eps, grey_as_bgr=gcn == 1, sizes=sizes)
        assert np.array_equal(got[e], single.cpu().numpy()), (radius, gcn, eps)


# ---- b. eps counts ------------------------------------------------------------------------------------

@pytest.mark.parametrize("gcn", [1, 3])
@pytest.mark.parametrize("n_eps", [1, 2, 8, 9])
def test_eps_counts(env, n_eps, gcn):
    rf, co, torch = env
    guides, srcs = _inputs(gcn)
    got, _ = _sweep(rf, torch, guides, srcs, 45, EPS9[:n_eps])
    for e, eps in enumerate(EPS9[:n_eps]):
        assert np.array_equal(got[e], _want(co, gcn, 45, eps)), (n_eps, gcn, eps)


def test_empty_eps_and_empty_list(env):
    rf, co, torch = env
    guides, srcs = _inputs(1)
    got, _ = _sweep(rf, torch, guides, srcs, 45, ())
    assert got.shape == (0, sum(h * w for h, w in SHAPES), 1)
    empty = torch.empty((0, 1), dtype=torch.uint8, device="cuda")
    out = rf.ops.guided_filter_ragged_sweep_u8(empty, empty, 45, EPS, grey_as_bgr=True,
                                               sizes=np.zeros((0, 2), np.int64))
    assert tuple(out.shape) == (4, 0, 1)
    with pytest.raises(ValueError):                             # in place: refused
        s_p, sizes = rf.ops.pack_images(_dev(torch, srcs), "srcs", torch)
        rf.ops.guided_filter_ragged_sweep_u8(s_p, s_p, 45, (3.0,), grey_as_bgr=True, sizes=sizes,
                                             out=s_p.view(1, -1, 1))


# ---- c. the fallback routes ---------------------------------------------------------------------------

@pytest.mark.parametrize("gcn,scn,radius", [(3, 3, 45), (1, 3, 9), (3, 1, 129), (1, 1, 129)])
def test_fallback_routes_equal_per_eps_calls(env, gcn, scn, radius):
    rf, co, torch = env
    flags = rf._ffi.GF_GREY_AS_BGR if gcn == 1 else 0
    shapes = [(1, 1), (33, 70), (70, 33), (9, 300)]
    assert rf._ffi.gf_ragged_plan(shapes, gcn, scn, radius, flags) is None
    rng = np.random.default_rng(4300 + radius + scn)
    guides, srcs = _images(rng, shapes, gcn), _images(rng, shapes, scn, 2)
    eps_list = (3.0, 1e-7, 7.0)
    got, (g_p, s_p, sizes) = _sweep(rf, torch, guides, srcs, radius, eps_list)
    for e, eps in enumerate(eps_list):
        single, _ = rf.ops.guided_filter_ragged_u8(g_p, s_p, radius, eps, grey_as_bgr=gcn == 1, sizes=sizes)
        assert np.array_equal(got[e], single.cpu().numpy()), (gcn, scn, radius, eps)
    want = np.concatenate([_oracle(co, g, s, radius, 3.0).reshape(-1, scn) for g, s in zip(guides, srcs)])
    assert np.array_equal(got[0], want)


# ---- d. whdr.sweep('guided') over an interleaved device list ------------------------------------------

@pytest.mark.parametrize("gcn", [1, 3])
def test_whdr_sweep_on_a_device_list_equals_oracle_filter_and_host_whdr(env, gcn, monkeypatch):
    rf, co, torch = env
    from reflectance_filtering_amd import whdr as W
    from tests.test_gpu_jbf_points import _comparisons
    rng = np.random.default_rng(4400 + gcn)
    shapes = [(43, 64), (64, 43), (43, 64), (48, 64), (64, 43), (1, 1)]
    guides, srcs = _images(rng, shapes, gcn), _images(rng, shapes, 1, 1)
    comps = [_comparisons(h, w, rng, 0 if i == 3 else 40) for i, (h, w) in enumerate(shapes)]
    # two radii, a pair named twice, one pair outside the ragged radii (the shape groups take it)
    pairs = [(3, 9), (7, 9.8), (1e-7, 9), (3, 45), (3, 9), (5e-3, 45), (3, 129)]
    calls = []
    real = rf.ops.guided_filter_ragged_sweep_u8
    monkeypatch.setattr(rf.ops, "guided_filter_ragged_sweep_u8",
                        lambda g, s, radius, eps, **kw: (calls.append((radius, list(eps))),
                                                         real(g, s, radius, eps, **kw))[1])
    got = W.sweep("guided", _dev(torch, srcs), _dev(torch, guides), comps, pairs, grey_as_bgr=gcn == 1)
    assert calls == [(9, [3.0, 7.0, 1e-7]), (45, [3.0, 5e-3])]
    assert got.shape == (len(pairs), len(shapes))
    for p, (sc, ss) in enumerate(pairs):
        for i in range(len(shapes)):
            f = _oracle(co, guides[i], srcs[i], int(ss), sc)
            assert got[p, i] == _host_whdr(W, f, comps[i], 0.1), (p, i)
    assert np.all(got[:, 3] == 0) and np.any(got > 0)


# ---- e. sweep.run('guided') on photos of three sizes --------------------------------------------------

@pytest.mark.parametrize("guidance", ["cnn", "image"])
def test_sweep_run_guided_on_mixed_sizes_equals_the_per_photo_path(env, tmp_path, guidance, monkeypatch):
    """The per-image WHDR matrix of sweep.run (one packed CNN call, one ragged guided call per pair)
    equals the per-photo path: the CNN on each photo alone, the oracle filter on its bytes, host whdr."""
    rf, co, torch = env
    from reflectance_filtering_amd import image_utils as iu
    from reflectance_filtering_amd import sweep as sweep_cli
    from reflectance_filtering_amd import whdr as W
    from tests import synth
    from tests.test_gpu_jbf_points import _comparisons, _write_iiw_json
    rng = np.random.default_rng(4500)
    shapes = [(43, 64), (64, 43), (48, 64), (64, 43), (43, 64)]
    files = []
    for i, (h, w) in enumerate(shapes):
        path = str(tmp_path / ("%03d.png" % i))
        iu.imwrite(path, synth.scene_u8(h, w, 4510 + i))
        _write_iiw_json(sweep_cli.judgements_for(path), _comparisons(h, w, rng, 0 if i == 2 else 45), h, w)
        files.append(path)
    cnn_calls, gf_calls = [], []
    real_cnn, real_gf = rf.ops.cnn_reflectance_u8, rf.ops.guided_filter_ragged_sweep_u8
    monkeypatch.setattr(rf.ops, "cnn_reflectance_u8",
                        lambda bgr, **kw: (cnn_calls.append(tuple(bgr.shape)), real_cnn(bgr, **kw))[1])
    monkeypatch.setattr(rf.ops, "guided_filter_ragged_sweep_u8",
                        lambda g, s, radius, eps, **kw: (gf_calls.append((radius, list(eps))),
                                                         real_gf(g, s, radius, eps, **kw))[1])
    sigma_color, sigma_spatial = [3.0, 5e-3], [9.0, 20.7]
    pairs, per_image, has = sweep_cli.run(files, "guided", sigma_color, sigma_spatial, guidance)
    assert cnn_calls == [(1, 1, sum(h * w for h, w in shapes), 3)]
    assert gf_calls == [(9, [3.0, 5e-3]), (20, [3.0, 5e-3])]
    monkeypatch.undo()
    assert pairs.tolist() == [[3, 9], [3, 20.7], [5e-3, 9], [5e-3, 20.7]]
    assert has.tolist() == [True, True, False, True, True]
    for i, path in enumerate(files):
        photo = iu.imread(path)
        h, w = photo.shape[:2]
        comp = W.to_pixels(W.load_judgements(sweep_cli.judgements_for(path)), h, w)
        _, r8 = rf.ops.cnn_reflectance_u8(torch.from_numpy(photo[None]).cuda(), want_float=False)
        r1 = r8[0].cpu().numpy()[:, :, None]
        joint = r1 if guidance == "cnn" else photo
        for p, (sc, ss) in enumerate(pairs):
            f = _oracle(co, joint, r1, int(ss), sc)
            assert per_image[p, i] == _host_whdr(W, f, comp, 0.1), (guidance, i, p)
    assert np.all(per_image[:, 2] == 0) and np.any(per_image > 0)
