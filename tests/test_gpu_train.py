"""Training ops library on the device: the hinge entry against the float64 restatement, the backward
entry against torch CPU float64 autograd, and five full-batch SGD steps end to end."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import synth, whdr_hinge_numpy as restate
from tests.test_train_host import H, W, distance, fixture_cases

pytestmark = pytest.mark.gpu
NP = 4513
BLOCKS = (("W0", 0, 96), ("b0", 96, 128), ("W1", 128, 1152), ("b1", 1152, 1184), ("W2", 1184, 2208),
          ("b2", 2208, 2240), ("W3", 2240, 3264), ("b3", 3264, 3296), ("W4", 3296, 4320),
          ("b4", 4320, 4352), ("wf", 4352, 4512), ("bf", 4512, 4513))


# ---- plain-torch statements (the oracles) ----------------------------------------------------------

def net(x_bgr, w):
    """The network on [P,3] B,G,R inputs with the flat parameter vector w: r [P] and the 160
    pre-activations [P,160]."""
    h = x_bgr.flip(1)
    pre, acts = [], []
    h = h @ w[0:96].view(32, 3).t() + w[96:128]
    pre.append(h)
    h = torch.relu(h)
    acts.append(h)
    for l in range(4):
        base = 128 + l * 1056
        h = h @ w[base:base + 1024].view(32, 32).t() + w[base + 1024:base + 1056]
        pre.append(h)
        h = torch.relu(h)
        acts.append(h)
    z = torch.cat(acts, 1) @ w[4352:4512] + w[4512]
    return torch.sigmoid(z), torch.cat(pre, 1)


def hinge_torch(r, po, cp, wt, co, delta, margin):
    """Mean over images of the weighted hinge loss (margin <= delta), differentiable; the floor does
    not zero the derivative."""
    eps = float(np.finfo(np.float32).eps)
    light = r + (r.clamp(min=eps) - r).detach()
    total = 0
    n = len(co) - 1
    for i in range(n):
        c = torch.from_numpy(cp[co[i]:co[i + 1]].astype(np.int64))
        w = torch.from_numpy(wt[co[i]:co[i + 1]]).to(r.dtype)
        y = light[po[i] + c[:, 0]] / light[po[i] + c[:, 1]]
        up, b = 1 + delta + margin, 1 + delta - margin
        loss = torch.where(c[:, 2] == 1, (y - 1 / up).clamp(min=0),
                           torch.where(c[:, 2] == 2, (up - y).clamp(min=0),
                                       torch.maximum((y - b).clamp(min=0), (1 / b - y).clamp(min=0))))
        total = total + (w * loss).sum() / w.sum()
    return total / n


# ---- helpers -------------------------------------------------------------------------------------------

GUARD = 256


class Guarded(object):
    """A device buffer with 256 guard bytes of 0xA5 on both sides."""

    def __init__(self, array=None, nbytes=None, fill=None):
        nbytes = array.nbytes if array is not None else nbytes
        self.raw = torch.full((nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        self.body = self.raw[GUARD:GUARD + nbytes]
        if array is not None:
            self.body.copy_(torch.from_numpy(np.ascontiguousarray(array).view(np.uint8).reshape(-1)))
        elif fill is not None:
            self.body.fill_(fill)
        self.ptr = self.raw.data_ptr() + GUARD

    def host(self, dtype):
        return self.body.cpu().numpy().view(dtype)

    def intact(self):
        raw = self.raw.cpu().numpy()
        return (raw[:GUARD] == 0xA5).all() and (raw[-GUARD:] == 0xA5).all()


def run_hinge(lib, r, po, cp, wt, co, inc_off, inc, delta, margin, first=0, count=None):
    from reflectance_filtering_amd import _ffi, _ffi_train
    count = len(co) - 1 if count is None else count
    pad = (lambda a: a if a.size else np.zeros((1,) + a.shape[1:], a.dtype))
    bufs = [Guarded(pad(np.ascontiguousarray(a, dtype=dt))) for a, dt in
            ((r, np.float32), (po, np.int32), (cp, np.int32), (wt, np.float64), (co, np.int32),
             (inc_off, np.int32), (inc, np.int32))]
    losses = Guarded(nbytes=8 * max(count, 1), fill=0xFF)
    grad = Guarded(nbytes=4 * max(len(r), 1), fill=0xFF)
    rc = lib.rf_train_whdr_hinge_points_f32(bufs[0].ptr, bufs[1].ptr + 4 * first, bufs[2].ptr,
                                            bufs[3].ptr, bufs[4].ptr + 4 * first, bufs[5].ptr,
                                            bufs[6].ptr, count, float(delta), float(margin),
                                            losses.ptr, grad.ptr, _ffi.current_stream_ptr(torch))
    _ffi_train.check(rc, "hinge")
    torch.cuda.synchronize()
    assert all(b.intact() for b in bufs + [losses, grad])
    return losses.host(np.float64)[:count].copy(), grad.host(np.float32)[:len(r)].copy()


# ---- hinge entry ---------------------------------------------------------------------------------------

def test_hinge_entry_on_the_fixture_cases(built, golden_dir):
    from reflectance_filtering_amd import _ffi_train, train
    lib = _ffi_train.load_library()
    figures = []
    for case in fixture_cases(golden_dir):
        po, cp, wt, co = case["arrays"]
        inc_off, inc = train.point_incidence(po, cp, co)
        want_l, want_g = restate.hinge_points(case["r"], po, cp, wt, co, case["delta"], case["margin"])
        losses, grad = run_hinge(lib, case["r"], po, cp, wt, co, inc_off, inc, case["delta"],
                                 case["margin"])
        dg, dl = distance(grad.astype(np.float64), losses, want_g, want_l, po)
        print("delta %g margin %g: device-to-restatement gradient %.3g loss %.3g; recorded "
              "reference-to-restatement %s" % (case["delta"], case["margin"], dg, dl, case["distance"]))
        figures.append((dg, dl, case["distance"]))
        again_l, again_g = run_hinge(lib, case["r"], po, cp, wt, co, inc_off, inc, case["delta"],
                                     case["margin"])
        assert np.array_equal(again_l, losses) and np.array_equal(again_g.view(np.uint32),
                                                                  grad.view(np.uint32))
        # images 1..2 as a sliced run == that run packed alone; nothing written outside the run
        sl, sg = run_hinge(lib, case["r"], po, cp, wt, co, inc_off, inc, case["delta"],
                           case["margin"], first=1, count=2)
        sub_po, sub_co = po[1:] - po[1], co[1:] - co[1]
        sub_off, sub_inc = train.point_incidence(sub_po, cp[co[1]:], sub_co)
        al, ag = run_hinge(lib, case["r"][po[1]:], sub_po, cp[co[1]:], wt[co[1]:], sub_co, sub_off,
                           sub_inc, case["delta"], case["margin"])
        assert np.array_equal(sl, al)
        assert np.array_equal(sg[po[1]:].view(np.uint32), ag.view(np.uint32))
        assert (sg[:po[1]].view(np.uint32) == 0xFFFFFFFF).all()
    for dg, dl, recorded in figures:
        assert dg <= 4 * recorded[0] and dl <= 4 * recorded[1]


def test_hinge_entry_empty_and_weightless_images(built):
    from reflectance_filtering_amd import _ffi_train, train
    lib = _ffi_train.load_library()
    rng = np.random.RandomState(4)
    po = np.array([0, 6, 9, 14, 20])           # image 1 has points but no comparisons
    co = np.array([0, 10, 10, 14, 30])
    cp = np.concatenate([np.stack([rng.randint(0, s, m), rng.randint(0, s, m), rng.randint(0, 3, m)], 1)
                         for s, m in ((6, 10), (5, 4), (6, 16))])
    wt = rng.uniform(0.1, 1.0, 30)
    wt[10:14] = 0.0                            # image 2 is weightless
    r = rng.uniform(0.05, 1.0, 20).astype(np.float32)
    inc_off, inc = train.point_incidence(po, cp, co)
    want_l, want_g = restate.hinge_points(r, po, cp, wt, co, 0.1, 0.05)
    losses, grad = run_hinge(lib, r, po, cp, wt, co, inc_off, inc, 0.1, 0.05)
    assert losses[1] == 0 and losses[2] == 0 and not grad[6:14].any()
    scale = np.abs(want_g).max()
    assert np.abs(grad - want_g).max() <= 8e-7 * scale      # 4 x the largest recorded fixture distance
    assert np.abs(losses - want_l).max() <= 8e-7 * want_l.max()


# ---- backward entry -------------------------------------------------------------------------------------

def backward_case(npoints, seed):
    from reflectance_filtering_amd import image_utils as iu, weights as wmod
    rng = np.random.RandomState(seed)
    w = wmod.load_weights() * (1 + 0.05 * rng.standard_normal(NP)).astype(np.float32)
    lut = iu.srgb_byte_lut()
    w64 = torch.from_numpy(w.astype(np.float64))

    def draw(k):
        x = rng.uniform(0, 1, (k, 3)).astype(np.float32)
        half = rng.rand(k) < 0.5
        x[half] = lut[rng.randint(0, 256, (int(half.sum()), 3))]
        return x
    x = draw(npoints)
    redrawn = 0
    for _ in range(20):
        _, pre = net(torch.from_numpy(x.astype(np.float64)), w64)
        close = (pre.abs() < 1e-4).any(1).numpy()
        if not close.any():
            break
        redrawn += int(close.sum())
        x[close] = draw(int(close.sum()))
    assert not close.any() and redrawn <= max(1, 0.02 * npoints)
    grad_r = rng.standard_normal(npoints).astype(np.float32)
    grad_r[rng.rand(npoints) < 0.5] = 0
    return x, w, grad_r


def autograd(x, w, grad_r, dtype):
    wt = torch.from_numpy(w.astype(dtype)).requires_grad_(True)
    r, _ = net(torch.from_numpy(x.astype(dtype)), wt)
    (r * torch.from_numpy(grad_r.astype(dtype))).sum().backward()
    return wt.grad.numpy().astype(np.float64)


def run_backward(lib, x, w, grad_r, dirty=None, stream=None):
    from reflectance_filtering_amd import _ffi, _ffi_train
    npoints = x.shape[0]
    need = _ffi_train.cnn_points_workspace_bytes(npoints)
    bx, bw, bg = Guarded(x), Guarded(w), Guarded(grad_r)
    out = Guarded(nbytes=4 * NP, fill=0xFF)
    ws = Guarded(nbytes=need, fill=dirty)
    torch.cuda.synchronize()
    s = stream if stream is not None else torch.cuda.current_stream()
    rc = lib.rf_train_cnn_points_backward_f32(bx.ptr, bw.ptr, bg.ptr, npoints, out.ptr, ws.ptr, need,
                                              ctypes.c_void_p(s.cuda_stream))
    _ffi_train.check(rc, "backward")
    s.synchronize()
    assert all(b.intact() for b in (bx, bw, bg, out, ws))
    return out.host(np.float32).copy()


def plan_points(label):
    """A point count on the kernel's own boundaries (rf_train_cnn_points_plan).  Workgroup g takes the
    passes g, g + G, ... with G = min(passes, the most a launch takes), so no point count leaves a
    workgroup without a pass; the nearest cases are a last pass of one point and one workgroup with
    a pass more than the others."""
    from reflectance_filtering_amd import _ffi_train
    per = _ffi_train.cnn_points_plan(1)[0]
    most = _ffi_train.cnn_points_plan(2 ** 31 - 1)[1]
    return {"pass-1": per - 1, "pass": per, "pass+1": per + 1, "every-workgroup-one-pass": most * per,
            "one-point-more": most * per + 1, "one-pass-more": (most + 1) * per}.get(label) or int(label)


@pytest.mark.parametrize("label", ["1", "2", "63", "64", "65", "pass-1", "pass", "pass+1",
                                   "every-workgroup-one-pass", "one-point-more", "one-pass-more"])
def test_backward_entry_against_float64_autograd(built, label):
    from reflectance_filtering_amd import _ffi_train
    npoints = plan_points(label)
    lib = _ffi_train.load_library()
    x, w, grad_r = backward_case(npoints, 100 + npoints % 97)
    want = autograd(x, w, grad_r, np.float64)
    f32 = autograd(x, w, grad_r, np.float32)
    got = run_backward(lib, x, w, grad_r)
    misses = []
    for name, a, b in BLOCKS:
        scale = np.abs(want[a:b]).max()
        d32 = np.abs(f32[a:b] - want[a:b]).max() / scale if scale else 0.0
        dev = np.abs(got[a:b] - want[a:b]).max() / scale if scale else np.abs(got[a:b]).max()
        print("P %d %s: float32 autograd %.3g, device %.3g (relative to %.3g)"
              % (npoints, name, d32, dev, scale))
        misses += [name] if dev > 4 * d32 else []
    assert not misses
    bits = got.view(np.uint32)
    assert np.array_equal(run_backward(lib, x, w, grad_r, dirty=0xFF).view(np.uint32), bits)
    assert np.array_equal(run_backward(lib, x, w, grad_r, dirty=0x00).view(np.uint32), bits)
    side = torch.cuda.Stream()
    assert np.array_equal(run_backward(lib, x, w, grad_r, dirty=0xFF, stream=side).view(np.uint32), bits)


# ---- end to end -----------------------------------------------------------------------------------------

STEPS, LR, MOMENTUM, DELTA, MARGIN = 5, 0.05, 0.9, 0.1, 0.05


def end_to_end_inputs():
    rng = np.random.RandomState(21)
    images = [synth.scene_u8(48, 64, seed=30 + i) for i in range(6)]
    comps = []
    for _ in images:
        rows = np.zeros((40, 6))
        rows[:, 0], rows[:, 2] = rng.randint(0, 64, 40), rng.randint(0, 64, 40)
        rows[:, 1], rows[:, 3] = rng.randint(0, 48, 40), rng.randint(0, 48, 40)
        rows[:, 4], rows[:, 5] = rng.randint(0, 3, 40), rng.uniform(0.2, 1.5, 40)
        comps.append(rows)
    return images, comps


def trajectory(x, arrays, w0, dtype):
    """STEPS full-batch steps of Caffe's SGD with momentum in plain torch on the CPU: the weights
    after the last step and the loss before every step and after the last."""
    po, cp, wt, co = arrays
    w = torch.from_numpy(w0.astype(dtype))
    v = torch.zeros_like(w)
    xt = torch.from_numpy(x.astype(dtype))
    losses = []
    for step in range(STEPS + 1):
        wt_ = w.clone().requires_grad_(True)
        loss = hinge_torch(net(xt, wt_)[0], po, cp, wt, co, DELTA, MARGIN)
        losses.append(loss.item())
        if step == STEPS:
            break
        loss.backward()
        v = MOMENTUM * v + LR * wt_.grad
        w = w - v
    return w.numpy().astype(np.float64), losses


def test_five_full_batch_sgd_steps_end_to_end(built, tmp_path):
    import reflectance_filtering_amd as rf
    from reflectance_filtering_amd import train, weights as wmod
    images, comps = end_to_end_inputs()
    packed = train.pack(images, comps, order_seed=5)
    assert packed.n == 6 and packed.comps.shape[0] == 240
    arrays = (packed.point_offsets, packed.comps, packed.weights, packed.comp_offsets)
    x = packed.x.cpu().numpy()
    w0 = wmod.load_weights()
    want, want_losses = trajectory(x, arrays, w0, np.float64)
    f32, _ = trajectory(x, arrays, w0, np.float32)
    assert want_losses[-1] < want_losses[0]
    final, history = train.fit(packed, w0, iterations=STEPS, base_lr=LR, solver="sgd",
                               momentum=MOMENTUM, full_batch=True, delta=DELTA, margin=MARGIN,
                               report_every=STEPS)
    scale = np.abs(want - w0).max()
    d32 = np.abs(f32 - want).max() / scale
    dev = np.abs(final - want).max() / scale
    print("oracle losses %s; device hinge %.6g -> %.6g; float32 trajectory %.3g, device %.3g of the "
          "largest weight change %.3g" % (want_losses, history[0]["train"]["hinge"],
                                          history[-1]["train"]["hinge"], d32, dev, scale))
    assert dev <= 4 * d32
    assert history[-1]["iteration"] == STEPS
    assert history[-1]["train"]["hinge"] < history[0]["train"]["hinge"]
    assert abs(history[0]["train"]["hinge"] - want_losses[0]) <= 1e-5 * want_losses[0]
    assert 0 <= history[-1]["train"]["whdr"] <= 1
    path = str(tmp_path / "trained.caffemodel")
    wmod.write_caffemodel(path, final)
    batch = torch.from_numpy(np.stack(images)).cuda()
    _, shipped8 = rf.get_reflectance_batch(batch)
    _, trained8 = rf.get_reflectance_batch(batch, weights=wmod.load_weights(path))
    assert not torch.equal(shipped8, trained8)
