"""The cases of the two device entries of librf_train_hip.so (include/reflectance_filtering_train.h) in the
format of tests/abi_cases.py (Case / Buf), run by tests/test_gpu_train_contract.py under the buffer, stream
and capture contracts; tests/test_train_host.py builds them on the host.

    hinge-fixture      case 1 of tests/golden/whdr_hinge.npz: delta 0.12, margin 0.08, three images with 5 /
                       300 / 1,181 comparisons (more than 256 comparisons and more than 256 points in one image)
    hinge-run          the same arrays with point_offsets + 1, comp_offsets + 1 and n = 2; the oracle is the run
                       packed alone, and grad_r in front of the run keeps whatever its buffer held
    hinge-wide-margin  case 2 of the fixture (margin > delta)
    backward-P65       65 points: two passes, the second of one point
    backward-P32833    (most workgroups + 1) passes and one point, from rf_train_cnn_points_plan: 514 passes over
                       512 workgroups, so two workgroups take a second pass and the last pass holds one point

Oracles and tolerances are those of tests/test_gpu_train.py: tests/whdr_hinge_numpy.hinge_points at 4 x the
distance the fixture records for the hinge entry; torch CPU float64 autograd per parameter block at 4 x the
distance of float32 autograd for the backward entry.

Residues (tests/test_gpu_buffer_contract._residues gives elem x 1 and elem x 3 in turn): loss_out is fixed at 8,
so that the hinge entry's two float64 buffers sit at 8 (loss_out) and 24 (weights); float32 and int32 buffers
take 4 and 12, the workspace 16.  tests/test_train_host.py pins this.

Decoys: r, x and the backward entry's grad_r are the same floats in another order; the CNN weights are the
true ones x 0.5; the hinge entry's float64 comparison weights are permuted within each image (a uniform scale
cancels in sum(w l) / sum(w) and in the gradient, so it would be no decoy).  Every Case carries `oracle_on`
(inputs by name -> the outputs the oracle gives for them), by which the host test sees the decoys' result fail
the case's own check.
"""
import os

import numpy as np

from tests import whdr_hinge_numpy as restate
from tests.abi_cases import Buf, Case, _i32, _once
from tests.test_gpu_train import BLOCKS, NP, autograd, backward_case

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HINGE, BACKWARD = "rf_train_whdr_hinge_points_f32", "rf_train_cnn_points_backward_f32"


def _fixture(index):
    from tests.test_train_host import fixture_cases
    if "fixture" not in _cache:
        _cache["fixture"] = fixture_cases(GOLDEN)
    return _cache["fixture"][index]


_cache = {}


def _within_images(values, offsets):
    """values reversed inside every run [offsets[i], offsets[i + 1])."""
    out = values.copy()
    for a, b in zip(offsets[:-1], offsets[1:]):
        out[a:b] = values[a:b][::-1]
    return out


def hinge(env, index, first=0, count=None):
    """Fixture case `index`; first / count: the run of images the call selects (all of them by default)."""
    from reflectance_filtering_amd import train
    from tests.test_train_host import distance
    fix = _fixture(index)
    po, cp, wt, co = fix["arrays"]
    delta, margin, recorded = float(fix["delta"]), float(fix["margin"]), fix["distance"]
    n = len(co) - 1
    count = n - first if count is None else count
    assert 0 <= first and count >= 1 and first + count <= n
    r = np.ascontiguousarray(fix["r"], dtype=np.float32)
    wt = np.ascontiguousarray(wt, dtype=np.float64)
    inc_off, inc = train.point_incidence(po, cp, co)
    total = int(po[-1])
    lo, hi = int(po[first]), int(po[first + count])
    k0, k1 = int(co[first]), int(co[first + count])
    sub_po, sub_co = po[first:first + count + 1] - lo, co[first:first + count + 1] - k0

    def oracle_on(data):
        """The run packed alone, in float64."""
        losses, grad = restate.hinge_points(np.asarray(data["r"], np.float64)[lo:hi], sub_po, cp[k0:k1],
                                            data["weights"][k0:k1], sub_co, delta, margin)
        return {"loss_out": losses, "grad_r": grad}
    oracle = _once(lambda: oracle_on({"r": r, "weights": wt}))

    def call(lib, p, stream):
        return lib.rf_train_whdr_hinge_points_f32(p["r"], p["point_offsets"] + 4 * first, p["comps"], p["weights"],
                                                  p["comp_offsets"] + 4 * first, p["inc_offsets"], p["inc"], count,
                                                  delta, margin, p["loss_out"], p["grad_r"], stream)

    def outputs(raw):
        """loss_out and the run's part of grad_r; the rest of grad_r holds what it held before the call: one
        byte value throughout (the fill of the arena, or the 0xA5 a runner wipes an output with)."""
        grad = raw["grad_r"][:4 * total]
        outside = np.concatenate([grad[:4 * lo], grad[4 * hi:]])
        if outside.size:
            assert outside[0] in (0xA5, 0x00, 0xFF) and (outside == outside[0]).all(), \
                "grad_r was written outside the points [%d, %d) of the run: %d bytes differ from 0x%02X" % (
                    lo, hi, int(np.count_nonzero(outside != outside[0])), outside[0])
        return {"loss_out": raw["loss_out"][:8 * count].view(np.float64).copy(),
                "grad_r": grad[4 * lo:4 * hi].view(np.float32).copy()}

    def check(outs):
        want = oracle()
        got_l, got_g = np.asarray(outs["loss_out"], np.float64), np.asarray(outs["grad_r"], np.float64)
        assert got_l.shape == want["loss_out"].shape and got_g.shape == want["grad_r"].shape
        assert np.isfinite(got_l).all() and np.isfinite(got_g).all()
        dg, dl = distance(got_g, got_l, want["grad_r"], want["loss_out"], sub_po)
        assert dg <= 4 * recorded[0] and dl <= 4 * recorded[1], (dg, dl, recorded)

    bufs = [Buf("r", "in", data=r, decoy=r[::-1]), Buf("point_offsets", "in", data=_i32(po)),
            Buf("comps", "in", data=_i32(cp)), Buf("weights", "in", data=wt, decoy=_within_images(wt, co)),
            Buf("comp_offsets", "in", data=_i32(co)), Buf("inc_offsets", "in", data=inc_off),
            Buf("inc", "in", data=inc), Buf("loss_out", "out", nbytes=8 * count, elem=8, fixed=8),
            Buf("grad_r", "out", nbytes=4 * total, elem=4)]
    case = Case(bufs, call, outputs, check, entries=(HINGE,))
    case.oracle_on = oracle_on
    return case


def plan_p32833(rf):
    """(most workgroups + 1) passes and one point more."""
    per = rf._ffi_train.cnn_points_plan(1)[0]
    most = rf._ffi_train.cnn_points_plan(2 ** 31 - 1)[1]
    return (most + 1) * per + 1


def backward(env, npoints):
    rf, co, torch = env
    need = rf._ffi_train.cnn_points_workspace_bytes(npoints)
    assert need > 0
    x, w, grad_r = backward_case(npoints, 100 + npoints % 97)      # (asserts its redraw cap of 2 %)

    def oracle_on(data):
        return {"grad_w": autograd(data["x"], data["weights"], data["grad_r"], np.float64)}
    oracle = _once(lambda: (autograd(x, w, grad_r, np.float64), autograd(x, w, grad_r, np.float32)))

    def call(lib, p, stream):
        return lib.rf_train_cnn_points_backward_f32(p["x"], p["weights"], p["grad_r"], npoints, p["grad_w"], p["ws"],
                                                    need, stream)

    def check(outs):
        want, f32 = oracle()
        got = np.asarray(outs["grad_w"], np.float64)
        assert got.shape == (NP,) and np.isfinite(got).all()
        misses = []
        for name, a, b in BLOCKS:
            scale = np.abs(want[a:b]).max()
            d32 = np.abs(f32[a:b] - want[a:b]).max() / scale if scale else 0.0
            dev = np.abs(got[a:b] - want[a:b]).max() / scale if scale else np.abs(got[a:b]).max()
            misses += [(name, dev, d32)] if dev > 4 * d32 else []
        assert not misses, misses

    half = np.float32(0.5)
    bufs = [Buf("x", "in", data=x, decoy=x[::-1]), Buf("weights", "in", data=w, decoy=w * half),
            Buf("grad_r", "in", data=grad_r, decoy=grad_r[::-1]), Buf("grad_w", "out", nbytes=4 * NP, elem=4),
            Buf("ws", "ws", nbytes=need, elem=16)]
    case = Case(bufs, call, {"grad_w": (np.float32, (NP,))}, check, entries=(BACKWARD,))
    case.oracle_on = oracle_on
    return case


# id: (the header's entries the call goes through, builder(env) -> Case, options): the format of
# tests/test_gpu_stream_contract.CASES
CASES = {
    "hinge-fixture": ((HINGE,), lambda e: hinge(e, 1), {}),
    "hinge-run": ((HINGE,), lambda e: hinge(e, 1, first=1, count=2), {}),
    "hinge-wide-margin": ((HINGE,), lambda e: hinge(e, 2), {}),
    "backward-P65": ((BACKWARD,), lambda e: backward(e, 65), {}),
    "backward-P32833": ((BACKWARD,), lambda e: backward(e, plan_p32833(e[0])), {}),
}
