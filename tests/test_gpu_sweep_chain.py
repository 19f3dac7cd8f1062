"""GPU suite: chained WHDR sweeps (whdr.sweep(iterations=K)) and the sweep tool's stored sources,
guidance files, device decoder and K-pass options (reflectance_filtering_amd.sweep.run / main).

The oracle is the per-photo path: filter_reflectance.apply_filter applied k times on the host arrays
of one photo, then whdr.whdr on the bytes as float32 / 255, planar - one channel for a grey source
(three equal channels in its file), three for a colour one.  Every comparison is exact equality of
float64 values; there is no tolerance anywhere.

Photos of 5x7, 9x4, 3x2 (smaller than the radii used: borders reflected more than once) and 12x12;
the 9x4 photo has no judgements, the others 40 each over at most 24 points, so points repeat.
"""
import json
import os

import numpy as np
import pytest

from tests.test_gpu_fuzz import env  # noqa: F401  (env is a fixture)
from tests.test_gpu_gf_ragged import _images
from tests.test_gpu_jbf_points import _comparisons, _write_iiw_json

pytestmark = pytest.mark.gpu

SHAPES = [(5, 7), (9, 4), (3, 2), (12, 12)]
NO_JUDGEMENTS = 1
GRID = {"guided": ([3.0, 5e-3], [2.9, 4.0]),        # holds (eps 3.0, radius 2) and (eps 5e-3, radius 4)
        "bilateral": ([20.0, 7.0], [1.4, 2.7])}     # holds (20, 1.4) and (7, 2.7)
SOURCE_KINDS = {"grey": (True, True, True, True), "colour": (False, False, False, False),
                "mixed": (True, False, False, True)}


def _files(tmp_path, seed=5100):
    """Photos with judgement files beside them, stored sources under grey/, colour/ and mixed/, and a
    colour guidance image per photo under flat/.  Returns the photo names."""
    from reflectance_filtering_amd import image_utils as iu
    from reflectance_filtering_amd import sweep as sweep_cli
    rng = np.random.default_rng(seed)
    photos = _images(rng, SHAPES, 3)
    flats = _images(rng, SHAPES, 3, 1)
    colour = _images(rng, SHAPES, 3, 2)
    grey = [np.repeat(g, 3, axis=2) for g in _images(rng, SHAPES, 1)]
    for d in ("grey", "colour", "mixed", "flat"):
        (tmp_path / d).mkdir()
    names = []
    for i, (h, w) in enumerate(SHAPES):
        name = str(tmp_path / ("%03d.png" % i))
        iu.imwrite(name, photos[i])
        iu.imwrite(str(tmp_path / "flat" / ("%03d.png" % i)), flats[i])
        iu.imwrite(str(tmp_path / "grey" / ("%03d.png" % i)), grey[i])
        iu.imwrite(str(tmp_path / "colour" / ("%03d.png" % i)), colour[i])
        iu.imwrite(str(tmp_path / "mixed" / ("%03d.png" % i)),
                   grey[i] if SOURCE_KINDS["mixed"][i] else colour[i])
        _write_iiw_json(sweep_cli.judgements_for(name),
                        _comparisons(h, w, rng, 0 if i == NO_JUDGEMENTS else 40), h, w)
        names.append(name)
    return names


def _chain_oracle(ftype, src, joint, comp, pairs, iterations, delta=0.1):
    """The per-photo path: float64 [K, P].  src [H,W,1] or [H,W,3], joint [H,W,3]; the joint is a
    buffer of its own and stays fixed, the uint8 result of one pass is the image of the next."""
    from reflectance_filtering_amd import filter_reflectance as fr
    from reflectance_filtering_amd import whdr as W
    out = np.zeros((iterations, len(pairs)), dtype=np.float64)
    for p, (sc, ss) in enumerate(pairs):
        cur = np.ascontiguousarray(src)
        for k in range(iterations):
            cur = fr.apply_filter(ftype, cur, joint.copy(), sc, ss).reshape(src.shape)
            planar = np.ascontiguousarray(np.transpose(cur, (2, 0, 1)))
            out[k, p] = W.whdr(planar.astype(np.float32) / np.float32(255), comp, delta)
    return out


def _comps_of(name, h, w):
    from reflectance_filtering_amd import sweep as sweep_cli
    from reflectance_filtering_amd import whdr as W
    return W.to_pixels(W.load_judgements(sweep_cli.judgements_for(name)), h, w)


def _cnn_r1(rf, torch, photo):
    _, r8 = rf.ops.cnn_reflectance_u8(torch.from_numpy(photo[None]).cuda(), want_float=False)
    return r8[0].cpu().numpy()[:, :, None]


def _check_columns(per_image, want_of, names, iterations):
    """per_image [K,P,N] against want_of(i) -> [K,P], photo by photo."""
    assert per_image.shape[0] == iterations and per_image.shape[2] == len(names)
    assert per_image.dtype == np.float64
    for i in range(len(names)):
        want = want_of(i)
        for k in range(iterations):
            for p in range(want.shape[1]):
                print("photo %d pass %d pair %d: got %.17g want %.17g"
                      % (i, k + 1, p, per_image[k, p, i], want[k, p]))
                assert per_image[k, p, i] == want[k, p], (i, k, p)
    assert np.all(per_image[:, :, NO_JUDGEMENTS] == 0) and np.any(per_image > 0)


# ---- the CNN's prediction, chained --------------------------------------------------------------------

@pytest.mark.parametrize("guided_by", ["cnn", "files"])
@pytest.mark.parametrize("ftype", ["guided", "bilateral"])
def test_a_three_pass_chain_of_the_prediction_equals_the_per_photo_path(env, tmp_path, ftype, guided_by):
    rf, co, torch = env
    from reflectance_filtering_amd import image_utils as iu
    from reflectance_filtering_amd import sweep as sweep_cli
    names = _files(tmp_path)
    sigma_color, sigma_spatial = GRID[ftype]
    flat = str(tmp_path / "flat" / "{name}")
    kwargs = {"guidance_files": flat} if guided_by == "files" else {}
    pairs, per_image, has = sweep_cli.run(names, ftype, sigma_color, sigma_spatial, "cnn", iterations=3,
                                          **kwargs)
    assert pairs.tolist() == [[c, s] for c in sigma_color for s in sigma_spatial]
    assert has.tolist() == [i != NO_JUDGEMENTS for i in range(len(SHAPES))]

    def want_of(i):
        photo = iu.imread(names[i])
        r1 = _cnn_r1(rf, torch, photo)
        joint = iu.imread(sweep_cli.file_for(names[i], flat)) if guided_by == "files" \
            else np.repeat(r1, 3, axis=2)
        return _chain_oracle(ftype, r1, joint, _comps_of(names[i], *photo.shape[:2]), pairs, 3)

    _check_columns(per_image, want_of, names, 3)


# ---- stored sources -------------------------------------------------------------------------------------

@pytest.mark.parametrize("guided_by", ["cnn", "files"])
@pytest.mark.parametrize("kind", ["grey", "colour", "mixed"])
@pytest.mark.parametrize("ftype", ["guided", "bilateral"])
def test_stored_sources_equal_the_per_photo_path_and_the_tool_writes_them(env, tmp_path, ftype, kind,
                                                                         guided_by, monkeypatch):
    rf, co, torch = env
    from reflectance_filtering_amd import image_utils as iu
    from reflectance_filtering_amd import sweep as sweep_cli
    names = _files(tmp_path)
    sigma_color, sigma_spatial = GRID[ftype]
    src_pattern = str(tmp_path / kind / "{name}")
    flat = str(tmp_path / "flat" / "{name}")
    kwargs = {"guidance_files": flat} if guided_by == "files" else {}
    cnn_calls = []
    real = rf.ops.cnn_reflectance_u8
    monkeypatch.setattr(rf.ops, "cnn_reflectance_u8",
                        lambda *a, **kw: (cnn_calls.append(1), real(*a, **kw))[1])
    pairs, per_image, has = sweep_cli.run(names, ftype, sigma_color, sigma_spatial, "cnn", iterations=2,
                                          src_files=src_pattern, **kwargs)
    _, single, _ = sweep_cli.run(names, ftype, sigma_color, sigma_spatial, "cnn",
                                 src_files=src_pattern, **kwargs)
    assert not cnn_calls, "the network was called for stored sources"

    def want_of(i):
        stored = iu.imread(sweep_cli.file_for(names[i], src_pattern))
        grey = SOURCE_KINDS[kind][i]
        src = stored[:, :, :1] if grey else stored
        joint = iu.imread(sweep_cli.file_for(names[i], flat)) if guided_by == "files" else stored
        return _chain_oracle(ftype, src, joint, _comps_of(names[i], *stored.shape[:2]), pairs, 2)

    _check_columns(per_image, want_of, names, 2)
    # one pass: [P, N], the chain's first slice
    assert single.shape == per_image.shape[1:] and np.array_equal(single, per_image[0])
    # the command line writes the same numbers
    out, npz = str(tmp_path / "sweep.json"), str(tmp_path / "sweep.npz")
    argv = ["--inputs", str(tmp_path / "*.png"), "--filter_type", ftype,
            "--sigma_color", ",".join(repr(v) for v in sigma_color),
            "--sigma_spatial", ",".join(repr(v) for v in sigma_spatial),
            "--src_files", src_pattern, "--iterations", "2", "--out", out, "--per_image", npz]
    if guided_by == "files":
        argv += ["--guidance_files", flat]
    assert sweep_cli.main(argv) == 0
    assert not cnn_calls
    with open(out) as fh:
        result = json.load(fh)
    assert result["iterations"] == 2 and result["src_files"] == src_pattern
    assert result.get("guidance_files") == (flat if guided_by == "files" else None)
    assert result["images"] == 4 and result["images_with_judgements"] == 3
    assert [p["pass"] for p in result["passes"]] == [1, 2]
    for k, entry in enumerate(result["passes"]):
        mean = per_image[k][:, has].mean(axis=1)
        assert entry["mean_whdr"] == mean.tolist()
        best = int(np.argmin(mean))
        assert entry["best"] == {"sigma_color": pairs[best, 0], "sigma_spatial": pairs[best, 1],
                                 "mean_whdr": mean[best]}
    assert result["mean_whdr"] == result["passes"][-1]["mean_whdr"]
    assert result["best"] == result["passes"][-1]["best"]
    with np.load(npz) as saved:
        assert saved["whdr"].shape == (2, len(pairs), 4) and np.array_equal(saved["whdr"], per_image)
        assert np.array_equal(saved["pairs"], pairs) and saved["has_judgements"].tolist() == has.tolist()
    # without the new options the keys stay what they were
    assert sweep_cli.main(argv[:8] + ["--out", out]) == 0
    with open(out) as fh:
        assert sorted(json.load(fh)) == sorted(
            ["filter_type", "guidance", "delta", "sigma_color", "sigma_spatial", "pairs", "mean_whdr",
             "best", "images", "images_with_judgements"])


# ---- the device decoder -----------------------------------------------------------------------------------

@pytest.mark.parametrize("ftype", ["guided", "bilateral"])
def test_the_device_decoder_gives_the_host_decoders_numbers(env, tmp_path, ftype):
    rf, co, torch = env
    from reflectance_filtering_amd import image_utils as iu
    from reflectance_filtering_amd import sweep as sweep_cli
    from tests import png_synth as ps
    from tests.test_gpu_png_decode import _interlaced, _save
    names = _files(tmp_path)
    # photo 0 interlaced (the parser declines it: imread), guidance file 3 with 16-bit samples, grey
    # source 0 a 16-bit grey file
    photo = iu.imread(names[0])
    _save(names[0], _interlaced(np.ascontiguousarray(photo[:, :, ::-1])))
    assert iu.png_parse(open(names[0], "rb").read()) is None
    assert np.array_equal(iu.imread(names[0]), photo)
    rng = np.random.default_rng(5200)
    h, w = SHAPES[3]
    flat3 = iu.imread(str(tmp_path / "flat" / "003.png"))
    wide = np.stack([flat3[:, :, ::-1], rng.integers(0, 256, flat3.shape).astype(np.uint8)], axis=3)
    _save(str(tmp_path / "flat" / "003.png"),
          ps.write_png(wide.reshape(h, -1), w, 16, 2, ps.filters_for("random", h, rng)))
    assert np.array_equal(iu.imread(str(tmp_path / "flat" / "003.png")), flat3)
    h, w = SHAPES[0]
    grey0 = iu.imread(str(tmp_path / "mixed" / "000.png"))
    wide = np.stack([grey0[:, :, 0], rng.integers(0, 256, (h, w)).astype(np.uint8)], axis=2)
    _save(str(tmp_path / "mixed" / "000.png"),
          ps.write_png(wide.reshape(h, -1), w, 16, 0, ps.filters_for("random", h, rng)))
    assert np.array_equal(iu.imread(str(tmp_path / "mixed" / "000.png")), grey0)
    sigma_color, sigma_spatial = GRID[ftype]
    flat = str(tmp_path / "flat" / "{name}")
    for kwargs in ({"guidance_files": flat},                                      # the CNN's prediction
                   {"guidance": "image"},
                   {"src_files": str(tmp_path / "mixed" / "{name}"), "guidance_files": flat},
                   {"src_files": str(tmp_path / "mixed" / "{name}"), "guidance": "image"},
                   {"src_files": str(tmp_path / "mixed" / "{name}")}):
        got = {dec: sweep_cli.run(names, ftype, sigma_color, sigma_spatial, iterations=2,
                                  png_decoder=dec, **kwargs) for dec in ("host", "device")}
        assert got["host"][1].shape == (2, 4, 4) and np.any(got["host"][1] > 0)
        assert np.array_equal(got["device"][1], got["host"][1]), sorted(kwargs)
        assert got["device"][2].tolist() == got["host"][2].tolist()


# ---- whdr.sweep: batches, and the defaults ------------------------------------------------------------------

@pytest.mark.parametrize("scn", [1, 3])
@pytest.mark.parametrize("ftype", ["guided", "bilateral"])
def test_a_chain_on_a_uniform_batch_and_an_equal_shape_list(env, ftype, scn):
    rf, co, torch = env
    from reflectance_filtering_amd import whdr as W
    rng = np.random.default_rng(5300 + scn)
    shapes = [(5, 7)] * 3
    srcs, joints = _images(rng, shapes, scn, 1), _images(rng, shapes, 3)
    comps = [_comparisons(5, 7, rng, 0 if i == 1 else 40) for i in range(3)]
    pairs = [(c, s) for c in GRID[ftype][0] for s in GRID[ftype][1]]
    want = np.stack([_chain_oracle(ftype, srcs[i], joints[i], comps[i], pairs, 3) for i in range(3)],
                    axis=2)
    batch = W.sweep(ftype, torch.from_numpy(np.stack(srcs)).cuda(), torch.from_numpy(np.stack(joints)).cuda(),
                    comps, pairs, iterations=3)
    assert batch.shape == (3, 4, 3) and np.array_equal(batch, want) and np.any(batch > 0)
    as_list = W.sweep(ftype, [torch.from_numpy(s).cuda() for s in srcs],
                      [torch.from_numpy(j).cuda() for j in joints], comps, pairs, iterations=3)
    assert np.array_equal(as_list, want)
    host_list = W.sweep(ftype, srcs, joints, comps, pairs, iterations=3)
    assert np.array_equal(host_list, want)


@pytest.mark.parametrize("guidance", ["cnn", "image"])
@pytest.mark.parametrize("ftype", ["guided", "bilateral"])
def test_one_pass_without_new_options_is_whdr_sweep_as_before(env, tmp_path, ftype, guidance):
    rf, co, torch = env
    from reflectance_filtering_amd import image_utils as iu
    from reflectance_filtering_amd import sweep as sweep_cli
    from reflectance_filtering_amd import whdr as W
    names = _files(tmp_path)
    sigma_color, sigma_spatial = GRID[ftype]
    pairs, per_image, has = sweep_cli.run(names, ftype, sigma_color, sigma_spatial, guidance)
    again = sweep_cli.run(names, ftype, sigma_color, sigma_spatial, guidance, 0.1, None, None, 1, "host")[1]
    photos = [iu.imread(f) for f in names]
    r1 = [torch.from_numpy(_cnn_r1(rf, torch, p)).cuda() for p in photos]
    joints = r1 if guidance == "cnn" else [torch.from_numpy(p).cuda() for p in photos]
    comps = [_comps_of(f, *p.shape[:2]) for f, p in zip(names, photos)]
    want = W.sweep(ftype, r1, joints, comps, pairs, grey_as_bgr=guidance == "cnn")
    assert per_image.shape == (4, 4) and per_image.dtype == np.float64
    assert np.array_equal(per_image, want) and np.array_equal(again, want) and np.any(want > 0)
    assert os.path.exists(names[0])
