"""Training ops library, everything that needs no device: the hinge fixture against the float64
restatement, the C ABI of librf_train_hip.so and its refusals, the host logic of train.py, the
caffemodel writer and the command line."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests import train_stubs, whdr_hinge_numpy as restate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32_EPS = float(np.finfo(np.float32).eps)
H, W = 24, 40


def fixture_cases(golden_dir):
    """Per case of tests/golden/whdr_hinge.npz: its parameters, the point arrays of the SELECTED
    comparisons, r at the points, and the layer's losses and gradient at the points."""
    from reflectance_filtering_amd import train, whdr
    data = np.load(os.path.join(golden_dir, "whdr_hinge.npz"))
    cases = []
    for c in range(int(data["n_cases"])):
        delta, margin, ratio, eval_dense = data["case%d_params" % c]
        rows = np.split(data["case%d_comparisons" % c], np.cumsum(data["case%d_counts" % c])[:-1])
        chosen = [train.select_comparisons(r, ratio, bool(eval_dense)) for r in rows]
        points, po, cp, wt, co = whdr.dedup_points(chosen, H, W)
        image = np.repeat(np.arange(len(rows)), np.diff(po))
        refl, diff = data["case%d_refl" % c], data["case%d_diff" % c]
        cases.append(dict(delta=delta, margin=margin, ratio=ratio, eval_dense=eval_dense,
                          arrays=(po, cp, wt, co), points=points,
                          r=refl[image, 0, points[:, 1], points[:, 0]],
                          grad=diff[image, 0, points[:, 1], points[:, 0]].astype(np.float64),
                          losses=data["case%d_losses" % c], loss=float(data["case%d_loss" % c]),
                          distance=data["case%d_distance" % c], chosen=chosen))
    return cases


def distance(grad, losses, ref_grad, ref_losses, po):
    """The fixture's measure: max |gradient difference| over max |gradient| per image (the largest),
    and the relative loss difference."""
    n = len(po) - 1
    dg = max(np.abs(grad[po[i]:po[i + 1]] - ref_grad[po[i]:po[i + 1]]).max()
             / np.abs(ref_grad[po[i]:po[i + 1]]).max() for i in range(n))
    dl = np.abs(np.asarray(losses) - ref_losses).max() / np.abs(ref_losses).max()
    return dg, dl


def test_restatement_stays_within_16_eps_of_the_reference_layer(golden_dir):
    cases = fixture_cases(golden_dir)
    assert [(c["delta"], c["margin"]) for c in cases] == [(0.1, 0.0), (0.12, 0.08), (0.1, 0.3), (0.1, 0.0)]
    assert (cases[3]["ratio"], cases[3]["eval_dense"]) == (0.5, 0)
    assert [len(r) for r in cases[0]["chosen"]] == [5, 300, 1181]
    assert [len(r) for r in cases[3]["chosen"]] == [3, 150, 1]
    for case in cases:
        po, cp, wt, co = case["arrays"]
        # the conditions the fixture was drawn under
        y = restate.ratios(case["r"], po, cp, co)
        same = cp[:, 0] == cp[:, 1]
        assert same.any()
        for lim in restate.borders(case["delta"], case["margin"]):
            assert (np.abs(y[~same] - lim) > 1e-3 * lim).all()
        assert (case["r"] == 0).sum() >= (2 if case["ratio"] == 1 else 0)
        losses, grad = restate.hinge_points(case["r"], po, cp, wt, co, case["delta"], case["margin"])
        dg, dl = distance(grad, losses, case["grad"], case["losses"], po)
        print("delta %g margin %g: gradient %.3g loss %.3g (recorded %s)"
              % (case["delta"], case["margin"], dg, dl, case["distance"]))
        assert dg <= 16 * F32_EPS and dl <= 16 * F32_EPS
        assert abs(losses.mean() - case["loss"]) <= 16 * F32_EPS * abs(case["loss"])
        assert case["distance"].max() <= 16 * F32_EPS
        assert dg <= 1.01 * case["distance"][0] + 1e-12


def test_restatement_empty_and_weightless_images():
    # whdr_hinge_loss_layer.py:155-160 by reading: no comparisons or a zero weight sum -> loss 0,
    # gradient 0, and the image still counts in the mean over the batch
    po, co = np.array([0, 2, 2, 4]), np.array([0, 1, 1, 2])
    cp = np.array([[0, 1, 1], [0, 1, 2]])
    r = np.array([0.5, 0.4, 0.3, 0.6])
    losses, grad = restate.hinge_points(r, po, cp, np.array([1.0, 0.0]), co, 0.1, 0.0)
    assert losses[1] == 0 and losses[2] == 0 and losses[0] > 0
    assert grad[2] == 0 and grad[3] == 0 and grad[0] != 0
    alone, grad1 = restate.hinge_points(r[:2], po[:2], cp[:1], np.array([1.0]), co[:2], 0.1, 0.0)
    assert alone[0] == losses[0] and np.allclose(grad1 / 3, grad[:2], rtol=1e-15)


# ---- ABI ---------------------------------------------------------------------------------------------

def header_functions():
    with open(os.path.join(ROOT, "include", "reflectance_filtering_train.h")) as fh:
        text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    return set(re.findall(r"\b(rf_train_\w+)\s*\(", text))


def test_header_exports_and_symbols(built):
    from reflectance_filtering_amd import _ffi, _ffi_train
    assert header_functions() == set(_ffi_train.EXPORTS)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _ffi_train.LIB_PATH]).decode()
    syms = {line.split()[-1] for line in out.splitlines()
            if len(line.split()) == 3 and line.split()[1] == "T" and line.split()[-1].startswith("rf_")}
    assert syms == set(_ffi_train.EXPORTS)
    assert not set(_ffi_train.EXPORTS) & (set(_ffi.EXPORTS) | set(_ffi.DEBUG_EXPORTS))
    # no symbol of the train library in the main one
    main = subprocess.check_output(["nm", "-D", "--defined-only", _ffi.LIB_PATH]).decode()
    assert "rf_train_" not in main and "rft" not in main
    with open(_ffi_train.LIB_PATH, "rb") as fh:
        blob = fh.read()
    archs = set(re.findall(rb"amdgcn-amd-amdhsa--(gfx[0-9a-f]+)", blob))
    assert archs == {b"gfx950"}


def test_version_and_refusals(built):
    from reflectance_filtering_amd import _ffi_train
    lib = _ffi_train.load_library()
    assert lib.rf_train_version() == 100
    err = (lambda: lib.rf_train_last_error().decode())
    p = ctypes.c_void_p(0x1000)          # invented: every refusal comes before any device work
    hinge = lib.rf_train_whdr_hinge_points_f32
    ok = [p, p, p, p, p, p, p, 3, 0.1, 0.0, p, p, None]
    assert hinge(*([None] * 7 + [0, 0.1, 0.0, None, None, None])) == 0
    for i in (0, 1, 2, 3, 4, 5, 6, 10, 11):
        args = list(ok)
        args[i] = None
        assert hinge(*args) == -1 and "NULL pointer" in err()
    for i, value, word in ((7, -1, "bad size"), (8, -0.1, "delta"), (8, float("nan"), "delta"),
                           (8, float("inf"), "delta"), (9, -1.0, "margin"),
                           (9, float("inf"), "margin"), (9, float("nan"), "margin")):
        args = list(ok)
        args[i] = value
        assert hinge(*args) == -1 and word in err()
    args = list(ok)
    args[7] = 1 << 24
    assert hinge(*args) == -2 and err().endswith("too many images for one launch")

    back = lib.rf_train_cnn_points_backward_f32
    need = lib.rf_train_cnn_points_workspace_bytes(100)
    ok = [p, p, p, 100, p, p, need, None]
    assert back(None, None, None, 0, None, None, 0, None) == 0
    for i in (0, 1, 2, 4):
        args = list(ok)
        args[i] = None
        assert back(*args) == -1 and "NULL pointer" in err()
    args = list(ok)
    args[3] = -5
    assert back(*args) == -1 and "bad size" in err()
    for ws, size in ((None, need), (p, need - 1), (ctypes.c_void_p(0x1004), need)):
        args = list(ok)
        args[5], args[6] = ws, size
        assert back(*args) == -1 and "16-byte aligned" in err()
    args = list(ok)
    args[3] = 1 << 31
    assert back(*args) == -2 and err().endswith("too many points for one launch")
    assert lib.rf_train_cnn_points_workspace_bytes(1 << 31) == 0
    assert lib.rf_train_cnn_points_workspace_bytes(-1) == 0
    out = (ctypes.c_int * 3)()
    assert lib.rf_train_cnn_points_plan(1 << 31, out) == -2
    assert lib.rf_train_cnn_points_plan(-1, out) == -1
    assert lib.rf_train_cnn_points_plan(5, None) == -1


def test_plan_and_workspace_are_monotone(built):
    from reflectance_filtering_amd import _ffi_train
    last = (0, 0, 0)
    per = _ffi_train.cnn_points_plan(1)[0]
    for npoints in [1, 2, per - 1, per, per + 1, 10 * per, 1000 * per, 10 ** 6, 10 ** 8, 2 ** 31 - 1]:
        pts, wgs, rows = _ffi_train.cnn_points_plan(npoints)
        size = _ffi_train.cnn_points_workspace_bytes(npoints)
        assert pts == per and 1 <= wgs <= (npoints + per - 1) // per and rows >= wgs
        assert size >= rows * 4513 * 4 and size % 16 == 0
        assert (wgs, rows, size) >= last[:0] and wgs >= last[0] and rows >= last[1] and size >= last[2]
        last = (wgs, rows, size)
    assert _ffi_train.cnn_points_workspace_bytes(0) == 0


# ---- host logic ----------------------------------------------------------------------------------------

def random_arrays(seed, counts, npts=7):
    rng = np.random.RandomState(seed)
    po = np.concatenate([[0], np.cumsum([npts + i for i in range(len(counts))])])
    co = np.concatenate([[0], np.cumsum(counts)])
    cp = np.concatenate([np.stack([rng.randint(0, npts + i, m), rng.randint(0, npts + i, m),
                                   rng.randint(0, 3, m)], axis=1) for i, m in enumerate(counts)])
    return po, cp, co


def test_point_incidence_against_a_loop():
    from reflectance_filtering_amd import train
    po, cp, co = random_arrays(3, [40, 0, 1, 25])
    cp[5, 1] = cp[5, 0]                     # coinciding ends: listed twice
    inc_off, inc = train.point_incidence(po, cp, co)
    assert inc_off.dtype == np.int32 and inc.dtype == np.int32
    assert inc_off.shape == (po[-1] + 1,) and inc.shape == (2 * len(cp),)
    for i in range(len(co) - 1):
        for p in range(po[i], po[i + 1]):
            want = []
            for k in range(co[i], co[i + 1]):
                for side in (0, 1):
                    if po[i] + cp[k, side] == p:
                        want.append(2 * (k - co[i]) + side)
            assert list(inc[inc_off[p]:inc_off[p + 1]]) == want
    with pytest.raises(IndexError):
        bad = cp.copy()
        bad[0, 0] = 99
        train.point_incidence(po, bad, co)


def test_select_comparisons():
    from reflectance_filtering_amd import train
    rows = np.arange(301 * 6, dtype=np.float64).reshape(301, 6)
    assert train.select_comparisons(rows).shape[0] == 301
    assert train.select_comparisons(rows, eval_dense=False).shape[0] == 1
    assert train.select_comparisons(rows[:300], eval_dense=False).shape[0] == 300
    assert np.array_equal(train.select_comparisons(rows[:5], 0.5), rows[:3])
    assert train.select_comparisons(rows, 0.5, eval_dense=False).shape[0] == 1
    assert train.select_comparisons(rows[:0], 0.5).shape == (0, 6)
    for ratio in (0.0, 1.5, -1.0):
        with pytest.raises(ValueError):
            train.select_comparisons(rows, ratio)


def test_a_run_of_images_is_the_run_packed_alone():
    from reflectance_filtering_amd import train
    po, cp, co = random_arrays(5, [12, 3, 0, 9, 20])
    inc_off, inc = train.point_incidence(po, cp, co)
    for i0, n in ((1, 3), (0, 5), (2, 1), (4, 1)):
        sub_po, sub_co = po[i0:i0 + n + 1] - po[i0], co[i0:i0 + n + 1] - co[i0]
        sub_off, sub_inc = train.point_incidence(sub_po, cp[co[i0]:co[i0 + n]], sub_co)
        lo, hi = po[i0], po[i0 + n]
        assert np.array_equal(inc_off[lo:hi + 1] - inc_off[lo], sub_off)
        assert np.array_equal(inc[inc_off[lo]:inc_off[hi]], sub_inc)
    assert train.batch_runs(25, 10) == [(0, 10), (10, 10), (20, 5)]
    assert train.batch_runs(25, 10, full_batch=True) == [(0, 25)]


def test_write_caffemodel_round_trip(tmp_path):
    from reflectance_filtering_amd import weights as wmod
    shipped = wmod.load_weights()
    rng = np.random.RandomState(11)
    odd = rng.standard_normal(wmod.N_PARAMS).astype(np.float32)
    odd[:4] = [np.float32(-0.0), np.float32(1e-42), np.float32(3.4e38), np.float32(-1e-30)]
    for k, flat in enumerate((shipped, odd)):
        path = str(tmp_path / ("w%d.caffemodel" % k))
        wmod.write_caffemodel(path, flat)
        layers = wmod.read_caffemodel(path)
        assert list(layers) == list(wmod.CONV_LAYERS)
        assert tuple(layers["conv0"][0].shape) == (32, 3, 1, 1)
        assert tuple(layers["fuse_skip_layers"][0].shape) == (1, 160, 1, 1)
        back = wmod.load_weights(path)
        assert np.array_equal(back.view(np.uint32), flat.view(np.uint32))
    with pytest.raises(ValueError):
        wmod.write_caffemodel(str(tmp_path / "bad"), shipped[:-1])
    with pytest.raises(ValueError):
        wmod.write_caffemodel(str(tmp_path / "bad"), shipped.astype(np.float64))


# ---- command line ------------------------------------------------------------------------------------

def photos_in(tmp_path, count):
    names = []
    for i in range(count):
        path = tmp_path / ("%03d.png" % i)
        path.write_bytes(b"")
        names.append(str(path))
    return names


def test_cli_parsing_and_refusals(capsys):
    from reflectance_filtering_amd import train
    _, args = train.parse_args(["--inputs", "a.png"])
    assert (args.split, args.split_scheme, args.report_split) == ("all", "train_val_test", None)
    assert (args.delta, args.margin, args.ratio, args.eval_dense) == (0.1, 0.0, 1.0, 1)
    assert (args.solver, args.batch_size, args.init) == ("sgd", 10, None)
    for bad in (["--delta", "-1"], ["--margin", "nan"], ["--ratio", "0"], ["--ratio", "1.5"],
                ["--solver", "lbfgs"], ["--iterations", "0"], ["--batch_size", "0"],
                ["--base_lr", "0"], ["--eval_dense", "2"], ["--report_split", "val"],
                ["--split", "train", "--report_split", "train"],
                ["--split", "val", "--split_scheme", "train_test"],
                ["--split", "train", "--report_split", "val", "--split_scheme", "train_test"]):
        with pytest.raises(SystemExit) as stop:
            train.parse_args(["--inputs", "a.png"] + bad)
        assert stop.value.code == 2
    capsys.readouterr()


def test_cli_runs_with_stubs(tmp_path, monkeypatch, capsys):
    from reflectance_filtering_amd import weights as wmod
    train = train_stubs.install(monkeypatch.setattr)
    photos = photos_in(tmp_path, 20)
    out, log = str(tmp_path / "w.caffemodel"), str(tmp_path / "t.json")
    rc = train.main(["--inputs"] + photos + ["--split", "train", "--report_split", "val", "--ratio",
                                              "0.5", "--eval_dense", "0", "--solver", "adam",
                                              "--iterations", "7", "--batch_size", "4", "--seed", "9",
                                              "--margin", "0.05", "--out", out, "--log", log])
    assert rc == 0
    packs = [c for c in train_stubs.CALLS if c[0] == "pack"]
    assert packs == [("pack", 14, 9, 0.5, False), ("pack", 2, None, 0.5, False)]
    (_, n, options), = [c for c in train_stubs.CALLS if c[0] == "fit"]
    assert n == 14 and options["solver"] == "adam" and options["iterations"] == 7
    assert options["batch_size"] == 4 and options["margin"] == 0.05 and options["held_out"].n == 2
    assert np.array_equal(wmod.load_weights(out), wmod.load_weights() + np.float32(1.0))
    with open(log) as fh:
        result = json.load(fh)
    assert result["split"]["name"] == "train" and result["report_split"] == "val"
    assert result["history"][0]["held_out"]["whdr"] == 0.5 and result["images"] == 14
    assert "val hinge 0.750000 whdr 0.5000" in capsys.readouterr().out
    with pytest.raises(SystemExit):
        train.main(["--inputs", str(tmp_path / "none*.png")])


# ---- the cases of the contract module (tests/train_cases.py, tests/test_gpu_train_contract.py) ------------

def _train_env():
    import torch

    import reflectance_filtering_amd as rf
    return rf, None, torch


def test_contract_cases_build_and_the_oracle_on_their_decoys_fails_their_check(built):
    """Building a case needs the plan and the workspace query only.  Per case: the entries it names, the
    buffer roles, a decoy that differs for every value input and none for the index-like ones, the case's
    check passing on the oracle's own result (as float32 where the device writes float32) and FAILING on the
    oracle's result for the decoys - otherwise a replay on decoys would prove nothing."""
    from tests import abi_cases as C
    from tests import train_cases as T
    env = _train_env()
    assert {"inc_offsets", "inc"} <= set(C.INDEX_LIKE)
    assert sorted(T.CASES) == ["backward-P32833", "backward-P65", "hinge-fixture", "hinge-run",
                               "hinge-wide-margin"]
    per, most, _ = env[0]._ffi_train.cnn_points_plan(2 ** 31 - 1)
    assert T.plan_p32833(env[0]) == (most + 1) * per + 1 == 32833
    for name in sorted(T.CASES):
        entries, build, opts = T.CASES[name]
        case = build(env)               # (the backward builder asserts the redraw cap of 2 % at its size)
        assert case.entries == entries and not case.sync and not opts, name
        values = []
        for b in case.bufs:
            if b.data is None:
                assert b.role in ("out", "ws"), (name, b.name)
            elif b.name in C.INDEX_LIKE:
                assert b.decoy is None and b.data.dtype == np.int32, (name, b.name)
            else:
                assert b.decoy is not None and not np.array_equal(b.decoy, b.data), (name, b.name)
                assert np.isfinite(b.decoy.astype(np.float64)).all(), (name, b.name)
                assert np.array_equal(np.sort(b.decoy, axis=None), np.sort(b.data, axis=None)) \
                    or np.array_equal(b.decoy, b.data * b.data.dtype.type(0.5)), (name, b.name)
                values.append(b.name)
        assert values == (["r", "weights"] if name.startswith("hinge") else ["x", "weights", "grad_r"]), name
        true = dict((b.name, b.data) for b in case.bufs if b.data is not None)
        decoys = dict((b.name, b.decoy if b.decoy is not None else b.data) for b in case.bufs
                      if b.data is not None)
        as_written = {"loss_out": np.float64, "grad_r": np.float32, "grad_w": np.float32}
        right = dict((k, v.astype(as_written[k])) for k, v in case.oracle_on(true).items())
        case.check(right)
        wrong = dict((k, v.astype(as_written[k])) for k, v in case.oracle_on(decoys).items())
        with pytest.raises(AssertionError):
            case.check(wrong)
        if name.startswith("hinge"):        # ... and the weights' decoy alone: no uniform scale, which cancels
            only_w = dict(true, weights=decoys["weights"])
            with pytest.raises(AssertionError):
                case.check(dict((k, v.astype(as_written[k])) for k, v in case.oracle_on(only_w).items()))
            scaled = dict(true, weights=true["weights"] * 0.5)
            case.check(dict((k, v.astype(as_written[k])) for k, v in case.oracle_on(scaled).items()))
    fix = T._fixture(1)
    assert (fix["delta"], fix["margin"]) == (0.12, 0.08) and T._fixture(2)["margin"] > T._fixture(2)["delta"]
    po, cp, wt, co = fix["arrays"]
    assert np.diff(co).tolist() == [5, 300, 1181] and np.diff(po).max() > 256


def test_hinge_run_case_reports_a_write_outside_the_run(built):
    """The callable `outputs` of hinge-run: grad_r in front of the run holds one fill byte throughout."""
    from tests import abi_cases as C
    from tests import train_cases as T
    case = T.CASES["hinge-run"][1](_train_env())
    sizes = dict((b.name, b.nbytes) for b in case.bufs)
    for fill in (0xA5, 0x00, 0xFF):
        raw = {"loss_out": np.full(sizes["loss_out"], fill, np.uint8),
               "grad_r": np.full(sizes["grad_r"], fill, np.uint8)}
        outs = C.typed_outputs(case, raw)
        assert outs["loss_out"].shape == (2,) and 4 * outs["grad_r"].size < sizes["grad_r"]
        raw["grad_r"][5] ^= 0x10
        with pytest.raises(AssertionError, match="outside the points"):
            C.typed_outputs(case, raw)


def test_every_train_entry_that_takes_a_stream_is_capturable_and_a_case_reaches_it():
    """The class list of tests/test_gpu_train_contract.py against include/reflectance_filtering_train.h, in
    the style of tests/test_capture_cases.py: the library has no refusing class."""
    from tests import test_gpu_train_contract as tc
    from tests import train_cases as T
    from tests.test_stream_cases import _entries_with_a_stream
    with open(os.path.join(ROOT, "include", "reflectance_filtering_train.h")) as fh:
        text = fh.read()
    names = _entries_with_a_stream(text)
    assert names == ["rf_train_cnn_points_backward_f32", "rf_train_whdr_hinge_points_f32"]
    assert sorted(tc.CAPTURABLE) == names and len(set(tc.CAPTURABLE)) == len(tc.CAPTURABLE)
    assert tc.REFUSING == () and tc.SYNCHRONISING == ()
    reached = set(e for entries, _, _ in T.CASES.values() for e in entries)
    assert reached == set(names)
    for test in (tc.test_buffer_contract, tc.test_entry_on_a_busy_side_stream,
                 tc.test_case_is_captured_and_replays_also_after_rf_shutdown):
        marks = [m for m in test.pytestmark if m.name == "parametrize"]
        assert len(marks) == 1 and list(marks[0].args[1]) == sorted(T.CASES), test.__name__
    preamble = text[:text.index("#ifndef")]
    for words in ("synchronises nothing", "ordered like any kernel launch", "safe to capture into a graph",
                  "does not concern", "tests/test_gpu_train_contract.py"):
        assert words in re.sub(r"\s*\n\s*\*\s*", " ", preamble), words
    assert "does not depend on what the workspace held" in re.sub(r"\s*\n\s*\*\s*", " ", text)


def test_contract_cases_sit_at_the_residues_the_documents_name(built):
    """float32 and int32 buffers at 4 and 12, float64 buffers at 8 and 24, the workspace at 16, in every layout but
    L0 (tests/test_gpu_buffer_contract._residues): the sentence of the header preamble, of DESIGN.md and of
    tests/test_gpu_train_contract.py."""
    from tests import train_cases as T
    from tests.test_gpu_buffer_contract import PAIRS, _residues
    env = _train_env()
    for name in sorted(T.CASES):
        case = T.CASES[name][1](env)
        assert set(_residues(case.bufs, "L0")) == {0}
        for layout in sorted(set(l for l, _ in PAIRS) - {"L0"}):
            by_elem = {}
            for b, res in zip(case.bufs, _residues(case.bufs, layout)):
                assert res % b.elem == 0, (name, b.name)
                by_elem.setdefault("ws" if b.role == "ws" else b.elem, set()).add(res)
            assert by_elem.pop(4) == {4, 12}, (name, layout)
            if name.startswith("hinge"):
                assert by_elem.pop(8) == {8, 24}, (name, layout)
            else:
                assert by_elem.pop("ws") == {16}, (name, layout)
            assert not by_elem, (name, layout, by_elem)
