"""Restatements of the rRel* training modes' per-pixel arithmetic (include/reflectance_filtering_recover.h).

float32: every line is one correctly rounded float32 numpy operation in the order the header pins, so the
result equals the reference's layers (tests/golden/recover.npz) and the device entries bit for bit.  The loss
mean is the header's ordered float64 sum (ordered_mean).

float64 / autograd: dense_loss() is written once over a small adapter so that numpy float64 arrays and torch
tensors (any dtype, with autograd) go through the same lines; it is the yardstick of the end-to-end tests.

x is [P,3] interleaved B, G, R everywhere; the reference's channel order in its sums is R, G, B.
"""
import numpy as np

F = np.float32
EPS = F(np.finfo(np.float32).eps)
NORMS = ("Mean", "Max", "Y", "Norm")
THREE = F(3)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def norm32(r, g, b, norm):
    if norm == 0:
        return ((r + g) + b) / THREE
    if norm == 1:
        return np.maximum(np.maximum(r, g), b)
    if norm == 2:
        return (F(0.299) * r + F(0.587) * g) + F(0.114) * b
    if norm == 3:
        return np.sqrt((r * r + g * g) + b * b)
    raise ValueError("unknown norm")


def recover32(x, e, norm):
    """dict of float32 arrays: n [P,3] and refl [P,3] in R, G, B order, s, ds (d s / d e), lightness."""
    x, e = _f32(x).reshape(-1, 3), _f32(e).ravel()
    b, g, r = x[:, 0], x[:, 1], x[:, 2]
    ri = np.maximum(e, EPS)
    m = np.maximum(norm32(r, g, b, norm), EPS)
    f = F(1) / m
    n = np.stack([f * r, f * g, f * b], axis=1)
    refl = ri[:, None] * n
    ri_inv = F(1) / ri
    s = m * ri_inv
    ds = -ri_inv * s
    lightness = np.maximum(EPS, ((refl[:, 0] + refl[:, 1]) + refl[:, 2]) / THREE)
    for a in (n, refl, s, ds, lightness):
        assert a.dtype == np.float32
    return {"n": n, "refl": refl, "s": s, "ds": ds, "lightness": lightness}


def boundary_term32(v, penalty):
    """(loss, slope) float32 of the blob intensity v; penalty 1 L1, 2 L2."""
    loss, slope = np.zeros_like(v), np.zeros_like(v)
    low, high = v < 0, v > 1
    if penalty == 1:
        loss[low], slope[low] = -v[low], F(-1)
        loss[high], slope[high] = v[high] - F(1), F(1)
    elif penalty == 2:
        loss[low], slope[low] = v[low] * v[low], F(2) * v[low]
        t = v[high] - F(1)
        loss[high], slope[high] = t * t, F(2) * t
    else:
        raise ValueError("unknown penalty")
    return loss, slope


def boundary_backward32(x, e, norm, penalty, scale_r, scale_s, count=None):
    """(per-pixel reflectance losses, per-pixel shading losses, grad_e), all float32 [P]."""
    rec = recover32(x, e, norm)
    refl, s, n = rec["refl"], rec["s"], rec["n"]
    count = F(refl.shape[0] if count is None else count)
    loss_r, slope_r = boundary_term32(((refl[:, 0] + refl[:, 1]) + refl[:, 2]) / THREE, penalty)
    loss_s, slope_s = boundary_term32(((s + s) + s) / THREE, penalty)
    dr = ((slope_r / count) / THREE) * F(scale_r)
    ds = ((slope_s / count) / THREE) * F(scale_s)
    shade = ds * rec["ds"]
    grad = ((((dr * n[:, 0] + dr * n[:, 1]) + dr * n[:, 2]) + shade) + shade) + shade
    assert grad.dtype == np.float32
    return loss_r, loss_s, grad


def ordered_mean(losses, npixels, plan, index=None):
    """The header's float64 sum of float32 per-pixel losses, divided by npixels.  plan = (pixels per pass,
    workgroups, rows).  index: the pixels the losses belong to (ascending), every other pixel's loss being
    +0.0; None = all pixels."""
    per, groups, rows = plan
    assert rows == groups and per & (per - 1) == 0
    losses = np.asarray(losses, dtype=np.float32).astype(np.float64)
    npasses = (npixels + per - 1) // per
    assert groups == min(npasses, groups)
    acc = np.zeros((groups, per), dtype=np.float64)
    if index is None:
        assert losses.shape == (npixels,)
        padded = np.zeros(npasses * per, dtype=np.float64)
        padded[:npixels] = losses
        padded = padded.reshape(npasses, per)
        for first in range(0, npasses, groups):          # pass k of every workgroup, ascending
            part = padded[first:first + groups]
            acc[:part.shape[0]] += part
    else:
        index = np.asarray(index, dtype=np.int64)
        assert (np.diff(index) > 0).all() and index.shape == losses.shape
        for q, value in zip(index.tolist(), losses.tolist()):
            acc[(q // per) % groups, q % per] += value
    width = per // 2
    while width:
        acc[:, :width] += acc[:, width:2 * width]
        width //= 2
    total = np.float64(0)
    for g in range(groups):
        total = total + acc[g, 0]
    return total / np.float64(npixels)


def hinge_scatter32(x, e, grad_l, pixel, norm, scale, grad_e):
    """grad_e with the hinge gradient added at the listed (distinct) pixels; a copy."""
    pixel = np.asarray(pixel, dtype=np.int64)
    assert np.unique(pixel).size == pixel.size
    n = recover32(_f32(x).reshape(-1, 3)[pixel], _f32(e).ravel()[pixel], norm)["n"]
    g = (F(scale) * _f32(grad_l)) / THREE
    out = _f32(grad_e).copy()
    out[pixel] = out[pixel] + ((g * n[:, 0] + g * n[:, 1]) + g * n[:, 2])
    return out


# ---- one text for numpy float64 and torch autograd ---------------------------------------------------

class NumpyOps(object):
    sqrt = staticmethod(np.sqrt)
    maximum = staticmethod(np.maximum)

    @staticmethod
    def floor(v):
        return np.maximum(v, float(EPS))

    @staticmethod
    def where(c, a, b):
        return np.where(c, a, b)


class TorchOps(object):
    def __init__(self, torch):
        self.torch = torch
        self.sqrt, self.maximum = torch.sqrt, torch.maximum

    def floor(self, v):
        """max(v, EPS) whose derivative stays 1 below the floor, as the layers keep it."""
        return v + (float(EPS) - v).clamp(min=0).detach()

    def where(self, c, a, b):
        return self.torch.where(c, a, b)


def recover_any(ops, x, e, norm):
    """(refl_R, refl_G, refl_B, shading, lightness) in the precision of x and e."""
    b, g, r = x[:, 0], x[:, 1], x[:, 2]
    if norm == 0:
        v = ((r + g) + b) / 3
    elif norm == 1:
        v = ops.maximum(ops.maximum(r, g), b)
    elif norm == 2:
        v = (float(F(0.299)) * r + float(F(0.587)) * g) + float(F(0.114)) * b
    else:
        v = ops.sqrt((r * r + g * g) + b * b)
    ri, m = ops.floor(e), ops.floor(v)
    refl = [ri * (c / m) for c in (r, g, b)]
    shading = m / ri
    lightness = ops.floor(((refl[0] + refl[1]) + refl[2]) / 3)
    return refl[0], refl[1], refl[2], shading, lightness


def boundary_any(ops, v, penalty):
    """The mean boundary loss of the intensity v."""
    zero = v * 0
    if penalty == 1:
        loss = ops.where(v < 0, -v, ops.where(v > 1, v - 1, zero))
    else:
        loss = ops.where(v < 0, v * v, ops.where(v > 1, (v - 1) * (v - 1), zero))
    return loss.sum() / v.shape[0]


def dense_loss(ops, x, e, norm, penalty):
    """(mean reflectance boundary loss, mean shading boundary loss, lightness [P]) over all pixels of x."""
    r0, r1, r2, shading, lightness = recover_any(ops, x, e, norm)
    return boundary_any(ops, ((r0 + r1) + r2) / 3, penalty), boundary_any(ops, shading, penalty), lightness
