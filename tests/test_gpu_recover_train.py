"""GPU suite: the dense training step of the rRel* modes end to end (train.loss_and_grad, train.fit on
train.pack_dense) against a float64 torch-autograd restatement of the whole loss on the CPU: the network
(tests/test_gpu_train.net), the recover layer and both boundary means (tests/recover_numpy.dense_loss), the hinge
loss (tests/test_gpu_train.hinge_torch) at the judgement points.  The yardstick is that of tests/test_gpu_train.py:
per weight block the device may be at most 4 x as far from float64 as the same graph in float32 autograd is.

Three images of different sizes (9 x 7, 24 x 40, 33 x 65), so count is the run's pixel total.  Where a branch is
chosen by a comparison, float32 and float64 must choose alike for the distance to mean anything: comparisons
are drawn so that no lightness ratio lies within 1e-3 of a hinge border under the first weights (as the hinge
fixture does), and a pixel whose reflectance or shading intensity lies within 1e-3 of 1 is repainted (the L1
slope jumps there).  The five-step trajectory takes the L2 penalty, whose slope is continuous at the borders, since
pixels move across them as the weights change.  A sigmoid output keeps the reflectance intensity below 1, so of
the two boundary losses only the shading one is live here; tests/test_gpu_recover.py has both, and the branch
below 0, bit for bit.
"""
import numpy as np
import pytest
import torch

from tests import recover_numpy as restate
from tests import synth, whdr_hinge_numpy as hinge_restate
from tests.test_gpu_train import BLOCKS, hinge_torch, net

pytestmark = pytest.mark.gpu

SIZES = ((9, 7), (24, 40), (33, 65))
COUNTS = (30, 60, 80)
DELTA, MARGIN, GAP = 0.1, 0.05, 1e-3
SCALE_WHDR, SCALE_BOUNDARIES = 1.0, 0.5
CASES = (("rRelMean", "L1"), ("rRelMax", "L2"), ("rRelY", "L1"), ("rRelNorm", "L2"))
STEPS, LR, MOMENTUM = 5, 0.05, 0.9
_cache = {}


def first_weights():
    """The shipped weights with the fuse bias lowered by 2.5: the shipped network's shading stays below 1 on nearly
    every pixel of these scenes, which would leave the boundary loss without a live pixel."""
    from reflectance_filtering_amd import weights as wmod
    w = wmod.load_weights().copy()
    w[4512] -= np.float32(2.5)
    return w


def recovered64(x, w, norm):
    """(reflectance intensity, shading, lightness) of [Q,3] inputs in float64."""
    ops = restate.TorchOps(torch)
    e = net(torch.from_numpy(x.astype(np.float64)), torch.from_numpy(w.astype(np.float64)))[0]
    r0, r1, r2, shading, light = restate.recover_any(ops, torch.from_numpy(x.astype(np.float64)), e, norm)
    return (((r0 + r1) + r2) / 3).numpy(), shading.numpy(), light.numpy()


def inputs(norm):
    """Three images and their comparisons, safe under the first weights (module docstring)."""
    from reflectance_filtering_amd import image_utils as iu
    if norm in _cache:
        return _cache[norm]
    lut, w0 = iu.srgb_byte_lut(), first_weights()
    rng = np.random.RandomState(300 + norm)
    limits = hinge_restate.borders(DELTA, MARGIN)
    images, comps, repainted = [], [], 0
    for i, ((h, w), m) in enumerate(zip(SIZES, COUNTS)):
        image = synth.scene_u8(h, w, seed=60 + i).copy()
        flat = image.reshape(-1, 3)
        for _ in range(20):
            v, s, light = recovered64(lut[flat], w0, norm)
            near = (np.abs(v - 1) <= GAP) | (np.abs(s - 1) <= GAP)
            if not near.any():
                break
            repainted += int(near.sum())
            flat[near] = rng.randint(0, 256, (int(near.sum()), 3))
        assert not near.any()
        light = light.reshape(h, w)
        rows = np.zeros((m, 6))
        k = 0
        while k < m:
            x1, x2 = rng.randint(0, w, 2)
            y1, y2 = rng.randint(0, h, 2)
            if k == 0:
                x1, y1, x2, y2 = 0, 0, w - 1, h - 1                   # the first and the last pixel of the image
            y = light[y1, x1] / light[y2, x2]
            if (x1, y1) == (x2, y2) or any(abs(y - lim) <= GAP * lim for lim in limits):
                assert k > 0
                continue
            rows[k] = (x1, y1, x2, y2, rng.randint(0, 3), rng.uniform(0.2, 1.5))
            k += 1
        images.append(image)
        comps.append(rows)
    assert repainted <= 0.05 * sum(h * w for h, w in SIZES)
    live = sum(int((recovered64(lut[im.reshape(-1, 3)], w0, norm)[1] > 1).sum()) for im in images)
    assert live >= 0.1 * sum(h * w for h, w in SIZES), "the shading boundary is nearly dead: %d pixels" % live
    _cache[norm] = images, comps
    return _cache[norm]


def total_loss(packed, x_dense, w, norm, penalty, dtype, first=0, count=None):
    """(loss, its three parts) of the images [first, first + count) as one differentiable torch expression."""
    count = packed.n - first if count is None else count
    ops = restate.TorchOps(torch)
    q0, q1 = int(packed.pixel_offsets[first]), int(packed.pixel_offsets[first + count])
    x = torch.from_numpy(x_dense[q0:q1].astype(dtype))
    e = net(x, w)[0]
    b_refl, b_shad, light = restate.dense_loss(ops, x, e, norm, penalty)
    p0, p1 = int(packed.point_offsets[first]), int(packed.point_offsets[first + count])
    at = torch.from_numpy(packed.point_pixel[p0:p1] - q0)
    po = packed.point_offsets[first:first + count + 1] - p0
    hinge = hinge_torch(light[at], po, packed.comps, packed.weights, packed.comp_offsets[first:first + count + 1],
                        DELTA, MARGIN)
    return SCALE_WHDR * hinge + SCALE_BOUNDARIES * (b_refl + b_shad), (hinge, b_refl, b_shad)


def autograd(packed, x_dense, w, norm, penalty, dtype):
    wt = torch.from_numpy(w.astype(dtype)).requires_grad_(True)
    loss, parts = total_loss(packed, x_dense, wt, norm, penalty, dtype)
    loss.backward()
    return wt.grad.numpy().astype(np.float64), loss.item(), [p.item() for p in parts]


def block_misses(got, want, f32, what):
    misses = []
    for name, a, b in BLOCKS:
        scale = np.abs(want[a:b]).max()
        d32 = np.abs(f32[a:b] - want[a:b]).max() / scale if scale else 0.0
        dev = np.abs(got[a:b] - want[a:b]).max() / scale if scale else np.abs(got[a:b]).max()
        print("%s %s: float32 autograd %.3g, device %.3g (relative to %.3g)" % (what, name, d32, dev, scale))
        misses += [(name, dev, d32)] if dev > 4 * d32 else []
    return misses


@pytest.mark.parametrize("mode,penalty", CASES)
def test_one_step_against_float64_autograd(built, mode, penalty):
    from reflectance_filtering_amd import train
    norm, code = train.rs_norm(mode), {"L1": 1, "L2": 2}[penalty]
    images, comps = inputs(norm)
    packed = train.pack_dense(images, comps, order_seed=3)
    assert packed.n == 3 and packed.pixels == sum(h * w for h, w in SIZES)
    x_dense = packed.x_dense.cpu().numpy()
    assert np.array_equal(x_dense[packed.point_pixel].view(np.uint32), packed.x.cpu().numpy().view(np.uint32))
    w0 = first_weights()
    want, want_loss, want_parts = autograd(packed, x_dense, w0, norm, code, np.float64)
    f32, _, _ = autograd(packed, x_dense, w0, norm, code, np.float32)
    loss, per_image, grad_w, parts = train.loss_and_grad(
        w0, packed, 0, 3, DELTA, MARGIN, rs_mode=mode, loss_scale_whdr=SCALE_WHDR,
        loss_scale_boundaries=SCALE_BOUNDARIES, boundary_penalty=penalty)
    got = grad_w.cpu().numpy().astype(np.float64)
    got_parts = [parts["hinge"], parts["boundary_reflectance"], parts["boundary_shading"]]
    print("%s %s: loss %.9g (float64 %.9g), parts %s (float64 %s)" % (mode, penalty, loss, want_loss, got_parts,
                                                                      want_parts))
    assert np.isfinite(got).all() and per_image.shape == (3,)
    assert want_parts[0] > 0 and want_parts[2] > 0                          # hinge and shading boundary are live
    assert abs(loss - want_loss) <= 1e-5 * want_loss
    for g, w in zip(got_parts, want_parts):
        assert abs(g - w) <= 1e-5 * max(w, 1e-3)
    assert loss == SCALE_WHDR * parts["hinge"] + SCALE_BOUNDARIES * (parts["boundary_reflectance"]
                                                                      + parts["boundary_shading"])
    assert not block_misses(got, want, f32, "%s %s" % (mode, penalty))
    # the boundary part reaches the weights: without it the gradient is another one
    _, _, hinge_only, _ = train.loss_and_grad(w0, packed, 0, 3, DELTA, MARGIN, rs_mode=mode,
                                              loss_scale_whdr=SCALE_WHDR, loss_scale_boundaries=0.0,
                                              boundary_penalty=penalty)
    assert not torch.equal(hinge_only, grad_w)
    # a run inside the packed set: images 1..2, count = their pixels
    wt = torch.from_numpy(w0.astype(np.float64)).requires_grad_(True)
    run_loss, _ = total_loss(packed, x_dense, wt, norm, code, np.float64, first=1, count=2)
    loss_run, _, _, _ = train.loss_and_grad(w0, packed, 1, 2, DELTA, MARGIN, rs_mode=mode,
                                            loss_scale_whdr=SCALE_WHDR, loss_scale_boundaries=SCALE_BOUNDARIES,
                                            boundary_penalty=penalty)
    assert abs(loss_run - run_loss.item()) <= 1e-5 * run_loss.item()


def trajectory(packed, x_dense, w0, norm, penalty, dtype):
    w = torch.from_numpy(w0.astype(dtype))
    v = torch.zeros_like(w)
    losses = []
    for step in range(STEPS + 1):
        wt = w.clone().requires_grad_(True)
        loss, _ = total_loss(packed, x_dense, wt, norm, penalty, dtype)
        losses.append(loss.item())
        if step == STEPS:
            break
        loss.backward()
        v = MOMENTUM * v + LR * wt.grad
        w = w - v
    return w.numpy().astype(np.float64), losses


def test_five_full_batch_sgd_steps_in_rrelmean(built):
    from reflectance_filtering_amd import train
    images, comps = inputs(0)
    packed = train.pack_dense(images, comps, order_seed=3)
    held = train.pack(images[:2], comps[:2])
    x_dense = packed.x_dense.cpu().numpy()
    w0 = first_weights()
    want, want_losses = trajectory(packed, x_dense, w0, 0, 2, np.float64)
    f32, _ = trajectory(packed, x_dense, w0, 0, 2, np.float32)
    final, history = train.fit(packed, w0, iterations=STEPS, base_lr=LR, solver="sgd", momentum=MOMENTUM,
                               full_batch=True, delta=DELTA, margin=MARGIN, report_every=STEPS, held_out=held,
                               rs_mode="rRelMean", loss_scale_whdr=SCALE_WHDR,
                               loss_scale_boundaries=SCALE_BOUNDARIES, boundary_penalty="L2")
    scale = np.abs(want - w0).max()
    d32 = np.abs(f32 - want).max() / scale
    dev = np.abs(final - want).max() / scale
    # per weight block, on the weight change: a small block does not hide behind a large one
    assert not block_misses(final.astype(np.float64) - w0, want - w0, f32 - w0, "five steps")
    print("oracle losses %s; float32 trajectory %.3g, device %.3g of the largest weight change %.3g; history %s"
          % (want_losses, d32, dev, scale, history))
    assert want_losses[-1] < want_losses[0]
    assert dev <= 4 * d32
    first, last = history[0], history[-1]
    assert last["iteration"] == STEPS and first["batch_loss"] is None
    for entry in history:
        assert sorted(entry["train"]) == ["boundary_reflectance", "boundary_shading", "hinge", "whdr"]
        assert sorted(entry["held_out"]) == ["hinge", "whdr"] and 0 <= entry["train"]["whdr"] <= 1
    total = (lambda t: SCALE_WHDR * t["hinge"] + SCALE_BOUNDARIES * (t["boundary_reflectance"]
                                                                      + t["boundary_shading"]))
    assert abs(total(first["train"]) - want_losses[0]) <= 1e-5 * want_losses[0]
    assert abs(total(last["train"]) - want_losses[-1]) <= 1e-4 * want_losses[-1]
    assert sorted(last["batch_parts"]) == ["boundary_reflectance", "boundary_shading", "hinge"]


def test_rdirectly_through_the_new_keywords_is_the_old_call(built):
    from reflectance_filtering_amd import train
    images, comps = inputs(0)
    w0 = first_weights()
    plain = train.pack(images, comps, order_seed=3)
    dense = train.pack_dense(images, comps, order_seed=3)
    old = train.loss_and_grad(w0, plain, 0, 3, DELTA, MARGIN)
    for packed in (plain, dense):
        new = train.loss_and_grad(w0, packed, 0, 3, DELTA, MARGIN, None, rs_mode="rDirectly", loss_scale_whdr=10.0,
                                  loss_scale_boundaries=7.0, boundary_penalty="L2")
        assert len(new) == 3 and new[0] == old[0]
        assert np.array_equal(new[1].view(np.uint64), old[1].view(np.uint64))
        assert torch.equal(new[2].view(torch.int32), old[2].view(torch.int32))
    a = train.evaluate(w0, plain, DELTA, MARGIN)
    assert a == train.evaluate(w0, dense, DELTA, MARGIN, rs_mode="rDirectly")
    b = train.evaluate(w0, dense, DELTA, MARGIN, rs_mode="rRelMean")
    assert sorted(b) == ["hinge", "whdr"] and b != a
    assert b == train.evaluate(w0, plain, DELTA, MARGIN, rs_mode="rRelMean")      # the points route alone
