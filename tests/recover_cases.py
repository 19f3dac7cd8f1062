"""Inputs and cases of the three device entries of librf_recover_hip.so (include/reflectance_filtering_recover.h).

fixture_cases(): the eight cases of tests/golden/recover.npz in the entries' layout (x [P,3] B G R, e [P]) with
the reference's tops, losses and diff.  seeded(): inputs of any size with the fixture's ranges and its three
planted pixels.  CASES: the entries in the Case / Buf format of tests/abi_cases.py, run by
tests/test_gpu_recover_contract.py under the buffer, stream and capture runners; the oracle is the float32
restatement (tests/recover_numpy.py), bit for bit.

    forward-list   rf_recover_forward_f32 at 300 listed pixels of 1,000 (first and last among them), all outputs
    boundary-P777  rf_recover_boundary_backward_f32, Y norm, L2: four passes, the last of 9 pixels
    scatter-list   rf_recover_hinge_scatter_f32 at the same list; grad_e is input and output

Decoys: x, e, grad_l and grad_e are the same floats in another order.  The pixel list is index-like (named
"points"): whatever a call reads of it is valid.  Residues: float32 buffers 4 and 12, int64 and float64 8 and 24.
"""
import os

import numpy as np

from reflectance_filtering_amd import _ffi_recover
from tests import recover_numpy as restate
from tests.abi_cases import Buf, Case, _once

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FORWARD, BOUNDARY, SCATTER = ("rf_recover_forward_f32", "rf_recover_boundary_backward_f32",
                              "rf_recover_hinge_scatter_f32")
PENALTIES = {"L1": 1, "L2": 2}
_cache = {}


def fixture_cases(golden_dir=GOLDEN):
    """A list of dicts: mode, norm, penalty (1 / 2), scale, x, e, refl [P,3] R G B, shading [P,3], losses
    float32 [2], mean_distance [2], diff [P]."""
    if "fixture" not in _cache:
        data = np.load(os.path.join(golden_dir, "recover.npz"))
        cases = []
        for c in range(int(data["n_cases"])):
            get = (lambda name: data["case%d_%s" % (c, name)])
            mode, image = str(get("mode")), get("image")
            pixels = (lambda blob: np.ascontiguousarray(blob.transpose(0, 2, 3, 1)).reshape(-1, blob.shape[1]))
            cases.append({"mode": mode, "norm": restate.NORMS.index(mode[4:]),
                          "penalty": PENALTIES[str(get("penalty"))], "scale": float(data["scale"]),
                          "x": np.ascontiguousarray(pixels(image)[:, ::-1]), "e": pixels(get("e")).reshape(-1),
                          "refl": pixels(get("reflectance")), "shading": pixels(get("shading")),
                          "losses": get("losses"), "mean_distance": get("mean_distance"),
                          "diff": pixels(get("diff")).reshape(-1)})
        _cache["fixture"] = cases
    return _cache["fixture"]


def seeded(npixels, seed):
    """(x [P,3], e [P]) float32 in the fixture's ranges; where there is room, a pixel with e = 0, a black pixel
    and a pixel with a negative channel."""
    rng = np.random.RandomState(seed)
    x = rng.uniform(0.02, 1.0, size=(npixels, 3)).astype(np.float32)
    e = rng.uniform(0.01, 1.3, size=npixels).astype(np.float32)
    if npixels >= 8:
        e[npixels // 2] = 0.0
        x[npixels // 3] = 0.0
        x[npixels - 2] = (0.2, 0.1, -0.9)
    return x, e


def pixel_list(npixels, count, seed):
    """`count` distinct pixels in random order, the first and the last pixel among them."""
    rng = np.random.RandomState(seed)
    inner = rng.choice(np.arange(1, npixels - 1), count - 2, replace=False)
    return rng.permutation(np.concatenate([[0, npixels - 1], inner])).astype(np.int64)


def _same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = np.flatnonzero(got.reshape(-1).view(np.uint8) != want.reshape(-1).view(np.uint8))
    assert bad.size == 0, "%s: %d bytes differ from the restatement, the first in element %d" % (
        what, bad.size, bad[0] // got.dtype.itemsize)


def forward_oracle(x, e, pixel, norm):
    rec = restate.recover32(x[pixel], e[pixel], norm)
    return {"lightness": rec["lightness"], "reflectance": np.ascontiguousarray(rec["refl"][:, ::-1]),
            "shading": rec["s"]}


def forward(env, npixels=1000, count=300, norm=0):
    x, e = seeded(npixels, 11)
    pixel = pixel_list(npixels, count, 12)

    def oracle_on(data):
        return forward_oracle(data["x"], data["e"], pixel, norm)
    oracle = _once(lambda: oracle_on({"x": x, "e": e}))

    def call(lib, p, stream):
        return lib.rf_recover_forward_f32(p["x"], p["e"], npixels, p["points"], count, norm, p["lightness"],
                                          p["reflectance"], p["shading"], stream)

    def check(outs):
        for name, want in oracle().items():
            _same_bits(outs[name], want, name)

    bufs = [Buf("x", "in", data=x, decoy=x[::-1]), Buf("e", "in", data=e, decoy=e[::-1]),
            Buf("points", "in", data=pixel), Buf("lightness", "out", nbytes=4 * count, elem=4),
            Buf("reflectance", "out", nbytes=12 * count, elem=4), Buf("shading", "out", nbytes=4 * count, elem=4)]
    outputs = {"lightness": (np.float32, (count,)), "reflectance": (np.float32, (count, 3)),
               "shading": (np.float32, (count,))}
    case = Case(bufs, call, outputs, check, entries=(FORWARD,))
    case.oracle_on = oracle_on
    return case


def boundary_oracle(rf, x, e, norm, penalty, scale_r, scale_s):
    loss_r, loss_s, grad = restate.boundary_backward32(x, e, norm, penalty, scale_r, scale_s)
    plan = _ffi_recover.boundary_plan(len(e))
    means = np.array([restate.ordered_mean(loss_r, len(e), plan), restate.ordered_mean(loss_s, len(e), plan)])
    return {"loss_out": means, "grad_e": grad}


def boundary(env, npixels=777, norm=2, penalty=2, scales=(0.1, 0.25)):
    rf = env[0]
    x, e = seeded(npixels, 21)
    need = _ffi_recover.boundary_workspace_bytes(npixels)
    assert need > 0

    def oracle_on(data):
        return boundary_oracle(rf, data["x"], data["e"], norm, penalty, scales[0], scales[1])
    oracle = _once(lambda: oracle_on({"x": x, "e": e}))

    def call(lib, p, stream):
        return lib.rf_recover_boundary_backward_f32(p["x"], p["e"], npixels, norm, penalty, scales[0], scales[1],
                                                    p["loss_out"], p["grad_e"], p["ws"], need, stream)

    def check(outs):
        for name, want in oracle().items():
            _same_bits(outs[name], want, name)

    bufs = [Buf("x", "in", data=x, decoy=x[::-1]), Buf("e", "in", data=e, decoy=e[::-1]),
            Buf("loss_out", "out", nbytes=16, elem=8), Buf("grad_e", "out", nbytes=4 * npixels, elem=4),
            Buf("ws", "ws", nbytes=need, elem=16)]
    case = Case(bufs, call, {"loss_out": (np.float64, (2,)), "grad_e": (np.float32, (npixels,))}, check,
                entries=(BOUNDARY,))
    case.oracle_on = oracle_on
    return case


def scatter(env, npixels=1000, count=300, norm=1, scale=10.0):
    x, e = seeded(npixels, 31)
    pixel = pixel_list(npixels, count, 32)
    rng = np.random.RandomState(33)
    grad_l = rng.uniform(-1, 1, count).astype(np.float32)
    grad_e = rng.uniform(-1e-3, 1e-3, npixels).astype(np.float32)

    def oracle_on(data):
        return {"grad_e": restate.hinge_scatter32(data["x"], data["e"], data["grad_l"], pixel, norm, scale,
                                                  data["grad_e"])}
    oracle = _once(lambda: oracle_on({"x": x, "e": e, "grad_l": grad_l, "grad_e": grad_e}))

    def call(lib, p, stream):
        return lib.rf_recover_hinge_scatter_f32(p["x"], p["e"], p["grad_l"], p["points"], count, npixels, norm,
                                                scale, p["grad_e"], stream)

    def check(outs):
        _same_bits(outs["grad_e"], oracle()["grad_e"], "grad_e")

    bufs = [Buf("x", "in", data=x, decoy=x[::-1]), Buf("e", "in", data=e, decoy=e[::-1]),
            Buf("grad_l", "in", data=grad_l, decoy=grad_l[::-1]), Buf("points", "in", data=pixel),
            Buf("grad_e", "out", data=grad_e, decoy=grad_e[::-1])]
    case = Case(bufs, call, {"grad_e": (np.float32, (npixels,))}, check, entries=(SCATTER,))
    case.oracle_on = oracle_on
    return case


# id: (the header's entries the call goes through, builder(env) -> Case, options): the format of
# tests/test_gpu_stream_contract.CASES
CASES = {
    "forward-list": ((FORWARD,), forward, {}),
    "boundary-P777": ((BOUNDARY,), boundary, {}),
    "scatter-list": ((SCATTER,), scatter, {}),
}
