"""The rRel* training modes, everything that needs no device: the float32 restatement against the reference's
own layers (tests/golden/recover.npz), the ordered float64 loss against the reference's float32 mean,
pack_dense() on the host, the distinct-pixel refusal, the command line, and the contract cases built on the host."""
import json
import math

import numpy as np
import pytest

from tests import recover_cases as RC
from tests import recover_numpy as restate
from tests.test_augment_host import on_the_host, same_bits, small_set

EPS32 = float(np.finfo(np.float32).eps)
PLAN = (256, 1024)          # pixels per pass, most workgroups (tests/test_recover_abi.py holds the library to it)


def plan_for(npixels):
    rows = min((npixels + PLAN[0] - 1) // PLAN[0], PLAN[1])
    return PLAN[0], rows, rows


def test_fixture_is_what_the_maker_describes(golden_dir):
    cases = RC.fixture_cases(golden_dir)
    assert [(c["mode"], c["penalty"]) for c in cases] == [
        (m, p) for m in ("rRelMean", "rRelMax", "rRelY", "rRelNorm") for p in (1, 2)]
    for c in cases:
        assert c["x"].shape == (3 * 24 * 40, 3) and c["e"].shape == (2880,) and c["scale"] == np.float32(0.1)
        assert c["e"].min() == 0 and (c["x"] == 0).all(axis=1).any() and (c["x"] < 0).any()
        assert (c["shading"].mean(axis=1) > 1).any() and (c["refl"].mean(axis=1) < 0).any()
        assert (c["refl"].mean(axis=1) > 1).any() or c["mode"] == "rRelNorm"


def test_float32_restatement_equals_the_reference_bit_for_bit(golden_dir):
    for c in RC.fixture_cases(golden_dir):
        rec = restate.recover32(c["x"], c["e"], c["norm"])
        assert same_bits(rec["refl"], c["refl"]), c["mode"]
        for k in range(3):
            assert same_bits(rec["s"], c["shading"][:, k]), c["mode"]
        _, _, grad = restate.boundary_backward32(c["x"], c["e"], c["norm"], c["penalty"], c["scale"], c["scale"])
        assert same_bits(grad, c["diff"]), (c["mode"], c["penalty"])
        # the lightness the hinge entry is given: the floored channel mean of the reference's reflectance
        mean = c["refl"].mean(axis=1, dtype=np.float32)
        assert same_bits(rec["lightness"], np.maximum(restate.EPS, mean)), c["mode"]


def test_ordered_float64_loss_is_within_pairwise_float32_summation_of_the_reference(golden_dir):
    """np.mean of float32 is pairwise summation, relative error at most log2(count) epsilons, and one division:
    (log2(count) + 2) float32 epsilons bound the distance of the reference's mean from an exact one.  The ordered
    float64 sum IS exact at this scale, so its distance equals the one the maker recorded."""
    for c in RC.fixture_cases(golden_dir):
        count = c["e"].size
        bound = (math.log2(count) + 2) * EPS32
        loss_r, loss_s, _ = restate.boundary_backward32(c["x"], c["e"], c["norm"], c["penalty"], 0.1, 0.1)
        for k, losses in enumerate((loss_r, loss_s)):
            mine = restate.ordered_mean(losses, count, plan_for(count))
            ref = float(c["losses"][k])
            dist = abs(mine - ref) / ref
            print("%s penalty %d loss %d: ordered %.9g reference %.9g distance %.3g eps (recorded %.3g eps, bound "
                  "%.3g eps)" % (c["mode"], c["penalty"], k, mine, ref, dist / EPS32,
                                 c["mean_distance"][k] / EPS32, bound / EPS32))
            assert dist <= bound and c["mean_distance"][k] <= bound
            assert abs(dist - c["mean_distance"][k]) <= 1e-3 * EPS32


def test_ordered_mean_dense_and_sparse_agree():
    rng = np.random.RandomState(5)
    npixels = 256 * 9 + 17
    plan = (256, 4, 4)                      # workgroups take a second and a third pass
    losses = np.zeros(npixels, dtype=np.float32)
    live = np.sort(rng.choice(npixels, 300, replace=False))
    losses[live] = rng.uniform(0, 5, 300).astype(np.float32)
    dense = restate.ordered_mean(losses, npixels, plan)
    assert dense == restate.ordered_mean(losses[live], npixels, plan, index=live)
    assert abs(dense - losses.astype(np.float64).sum() / npixels) <= 1e-12 * dense


def test_float64_restatement_follows_the_float32_one(golden_dir):
    c = RC.fixture_cases(golden_dir)[0]
    keep = np.ones(c["e"].size, dtype=bool)
    keep[[3 * 40 + 5, 960 + 7 * 40 + 11, 1920 + 20 * 40 + 33]] = False      # the planted pixels: huge terms
    x, e = c["x"][keep], c["e"][keep]
    for norm in range(4):
        for penalty in (1, 2):
            b_r, b_s, light = restate.dense_loss(restate.NumpyOps, x.astype(np.float64), e.astype(np.float64),
                                                 norm, penalty)
            loss_r, loss_s, _ = restate.boundary_backward32(x, e, norm, penalty, 0.1, 0.1)
            assert abs(b_r - loss_r.astype(np.float64).mean()) <= 1e-5 * max(b_r, 1e-3)
            assert abs(b_s - loss_s.astype(np.float64).mean()) <= 1e-5 * b_s
            assert np.allclose(light, restate.recover32(x, e, norm)["lightness"], rtol=1e-5, atol=0)


# ---- pack_dense ------------------------------------------------------------------------------------------------------

def mixed_set(seed):
    rng = np.random.RandomState(seed)
    sizes = [(9, 7), (24, 40), (33, 65), (5, 6)]
    images = [rng.randint(0, 256, s + (3,)).astype(np.uint8) for s in sizes]
    images[2] = (images[2].astype(np.float32) / np.float32(255))          # a linear float image among them
    comps = []
    for (h, w), m in zip(sizes, (12, 60, 0, 9)):
        rows = np.zeros((m, 6))
        rows[:, 0], rows[:, 2] = rng.randint(0, w, m), rng.randint(0, w, m)
        rows[:, 1], rows[:, 3] = rng.randint(0, h, m), rng.randint(0, h, m)
        rows[:, 4], rows[:, 5] = rng.randint(0, 3, m), rng.randint(1, 30, m) / 8.0
        if m:
            rows[0, :4] = (0, 0, w - 1, h - 1)          # the first and the last pixel of the image
        comps.append(rows)
    return images, comps, sizes


def test_pack_dense_on_the_host(monkeypatch):
    from reflectance_filtering_amd import image_utils as iu
    train, cpu = on_the_host(monkeypatch)
    images, comps, sizes = mixed_set(41)
    for seed in (None, 3):
        plain = train.pack(images, comps, seed, device=cpu)
        packed = train.pack_dense(images, comps, seed, device=cpu)
        for name in ("points", "point_offsets", "comps", "weights", "comp_offsets", "inc_offsets", "inc", "order"):
            assert same_bits(getattr(packed, name), getattr(plain, name)), name
        assert same_bits(packed.x.numpy(), plain.x.numpy())
        order = packed.order
        areas = [sizes[i][0] * sizes[i][1] for i in order]
        assert packed.pixel_offsets.dtype == np.int64 and packed.point_pixel.dtype == np.int64
        assert packed.pixel_offsets.tolist() == np.concatenate([[0], np.cumsum(areas)]).tolist()
        assert packed.pixels == sum(areas) and tuple(packed.x_dense.shape) == (sum(areas), 3)
        dense = packed.x_dense.numpy()
        assert dense.dtype == np.float32
        assert same_bits(dense[packed.point_pixel], packed.x.numpy())       # the points ARE dense pixels
        assert same_bits(packed.d_point_pixel.numpy(), packed.point_pixel)
        lut = iu.srgb_byte_lut()
        for i, src in enumerate(order):
            q0, q1 = packed.pixel_offsets[i], packed.pixel_offsets[i + 1]
            image = images[src]
            want = lut[image] if image.dtype == np.uint8 else image
            assert same_bits(dense[q0:q1], np.ascontiguousarray(want.reshape(-1, 3)))
            p0, p1 = packed.point_offsets[i], packed.point_offsets[i + 1]
            if p1 > p0:                                                     # first and last pixel are points
                assert packed.point_pixel[p0:p1].min() == q0 and packed.point_pixel[p0:p1].max() == q1 - 1
                assert ((packed.point_pixel[p0:p1] >= q0) & (packed.point_pixel[p0:p1] < q1)).all()
        assert "12 bytes per pixel" in train.pack_dense.__doc__ and "2 MB per IIW photo" in train.pack_dense.__doc__


def test_repeated_pixels_are_refused():
    from reflectance_filtering_amd import train
    assert train.check_distinct_pixels([5, 1, 9]).tolist() == [5, 1, 9]
    with pytest.raises(ValueError, match="pairwise distinct"):
        train.check_distinct_pixels([5, 1, 5])


def test_modes_and_dense_refusals(monkeypatch):
    train, cpu = on_the_host(monkeypatch)
    assert train.rs_norm("rDirectly") is None
    assert [train.rs_norm(m) for m in train.RS_MODES[1:]] == [0, 1, 2, 3]
    assert train.RS_MODES[1:] == ("rRelMean", "rRelMax", "rRelY", "rRelNorm")
    for bad in ("rAbs", "sRelMean", "RS", ""):
        with pytest.raises(ValueError, match="rs_mode"):
            train.rs_norm(bad)
    images, comps = small_set(42, [4, 3])
    plain = train.pack(images, comps, device=cpu)
    with pytest.raises(ValueError, match="pack_dense"):        # a points-only pack cannot train densely
        train.loss_and_grad(np.zeros(4513, np.float32), plain, 0, 2, rs_mode="rRelMean")
    with pytest.raises(ValueError, match="pack_dense"):
        train.fit(plain, np.zeros(4513, np.float32), iterations=1, rs_mode="rRelMax")


# ---- command line ----------------------------------------------------------------------------------------------------

def test_cli_options(capsys):
    from reflectance_filtering_amd import train
    _, args = train.parse_args(["--inputs", "a.png"])
    assert (args.RS_est_mode, args.loss_scale_whdr, args.loss_scale_boundaries01, args.boundary_penalty) == (
        "rDirectly", 1.0, 0.1, "L1")
    _, args = train.parse_args(["--inputs", "a.png", "--RS_est_mode", "rRelMean", "--loss_scale_whdr", "10",
                                "--loss_scale_boundaries01", "0.5", "--boundary_penalty", "L2"])
    assert (args.RS_est_mode, args.loss_scale_whdr, args.loss_scale_boundaries01, args.boundary_penalty) == (
        "rRelMean", 10.0, 0.5, "L2")
    for bad in (["--RS_est_mode", "rAbs"], ["--RS_est_mode", "RS"], ["--boundary_penalty", "L3"],
                ["--loss_scale_whdr", "-1"], ["--loss_scale_boundaries01", "nan"]):
        with pytest.raises(SystemExit) as stop:
            train.parse_args(["--inputs", "a.png"] + bad)
        assert stop.value.code == 2
    capsys.readouterr()
    text = train.build_parser().format_help()
    assert "reference's default: 10" in text and "reference's default: 0.1" in text and "rRelMax" in text


def run_main(tmp_path, monkeypatch, extra):
    from tests import train_stubs
    from tests.test_train_host import photos_in
    train = train_stubs.install(monkeypatch.setattr)
    seen = []

    def pack_dense(images, comparisons_px, order_seed=None, ratio=1.0, eval_dense=True, device=None,
                   hinge_comparisons_px=None):
        seen.append(len(images))
        packed = train_stubs.FakePacked(len(images))
        packed.pixels = 16 * len(images)
        return packed

    monkeypatch.setattr(train, "pack_dense", pack_dense)
    photos = photos_in(tmp_path, 3)
    log = str(tmp_path / "t.json")
    rc = train.main(["--inputs"] + photos + ["--iterations", "2", "--out", str(tmp_path / "w.caffemodel"),
                                              "--log", log] + extra)
    assert rc == 0
    (_, _, options), = [c for c in train_stubs.CALLS if c[0] == "fit"]
    with open(log) as fh:
        return seen, options, json.load(fh), [c for c in train_stubs.CALLS if c[0] == "pack"]


RDIRECTLY_KEYS = ["base_lr", "batch_size", "comparisons", "comparisons_type", "delta", "eval_dense", "full_batch",
                  "history", "images", "init", "iterations", "margin", "max_evaluated", "momentum", "out", "points",
                  "ratio", "seed", "solver"]
RDIRECTLY_OPTIONS = ["base_lr", "batch_size", "delta", "full_batch", "held_out", "iterations", "log", "margin",
                     "max_evaluated", "momentum", "report_every", "seed", "solver"]


def test_rdirectly_run_keeps_its_keys(tmp_path, monkeypatch, capsys):
    for extra in ([], ["--RS_est_mode", "rDirectly", "--loss_scale_whdr", "10", "--boundary_penalty", "L2"]):
        seen, options, result, packs = run_main(tmp_path, monkeypatch, extra)
        assert seen == [] and len(packs) == 1                  # the points-only pack, as before
        assert sorted(result) == RDIRECTLY_KEYS
        assert sorted(options) == RDIRECTLY_OPTIONS
    capsys.readouterr()


def test_rrel_run_packs_densely_and_records_the_mode(tmp_path, monkeypatch, capsys):
    seen, options, result, packs = run_main(tmp_path, monkeypatch, [
        "--RS_est_mode", "rRelMax", "--loss_scale_whdr", "10", "--loss_scale_boundaries01", "0.2"])
    assert seen == [3] and packs == []
    assert (options["rs_mode"], options["loss_scale_whdr"], options["loss_scale_boundaries"],
            options["boundary_penalty"]) == ("rRelMax", 10.0, 0.2, "L1")
    assert sorted(set(options) - set(RDIRECTLY_OPTIONS)) == ["boundary_penalty", "loss_scale_boundaries",
                                                             "loss_scale_whdr", "rs_mode"]
    assert sorted(set(result) - set(RDIRECTLY_KEYS)) == ["RS_est_mode", "boundary_penalty",
                                                         "loss_scale_boundaries01", "loss_scale_whdr", "pixels"]
    assert (result["RS_est_mode"], result["loss_scale_whdr"], result["loss_scale_boundaries01"],
            result["boundary_penalty"], result["pixels"]) == ("rRelMax", 10.0, 0.2, "L1", 48)
    capsys.readouterr()


# ---- the contract cases, on the host ---------------------------------------------------------------------------------

def test_contract_cases_and_their_decoys(built):
    import reflectance_filtering_amd as rf
    from reflectance_filtering_amd import _ffi_recover
    assert sorted(RC.CASES) == ["boundary-P777", "forward-list", "scatter-list"]
    assert set(e for entries, _, _ in RC.CASES.values() for e in entries) == set(
        n for n in _ffi_recover.EXPORTS if n.endswith("_f32"))
    for name in sorted(RC.CASES):
        entries, build, _ = RC.CASES[name]
        case = build((rf, None, None))
        assert case.entries == entries
        true = dict((b.name, b.data) for b in case.bufs if b.decoy is not None)
        decoys = dict((b.name, b.decoy) for b in case.bufs if b.decoy is not None)
        case.check(case.oracle_on(true))
        with pytest.raises(AssertionError):                 # the decoys' result fails the case's own check
            case.check(case.oracle_on(decoys))
        for b in case.bufs:
            if b.data is not None and b.decoy is None:
                assert b.name == "points" and b.data.dtype == np.int64
                assert b.data.min() == 0 and b.data.max() == 999 and np.unique(b.data).size == b.data.size
