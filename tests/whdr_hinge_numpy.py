"""Float64 numpy restatement of the WHDR hinge loss and its gradient in point-array form: the
reference value of the device entry rf_train_whdr_hinge_points_f32 (tests/test_gpu_train_hinge.py).
Its distance from the reference's own layer is recorded in tests/golden/whdr_hinge.npz
(tests/golden/make_whdr_hinge.py) and held by tests/test_train_hinge_fixture.py.

All arithmetic is float64 and nothing is rounded to float32: the lightness floor is
float32's epsilon as a double, the borders are the doubles formed from delta and margin.
"""
import numpy as np

EPS = float(np.finfo(np.float32).eps)


def comparison_terms(l1, l2, darker, delta, margin):
    """(loss, dl/dL1, dl/dL2) per comparison, unweighted; l1, l2 float64 arrays (floored already)."""
    inv = 1.0 / l2
    y = l1 * inv
    dy1, dy2 = inv, -y * inv
    loss = np.zeros_like(y)
    slope = np.zeros_like(y)
    d1, d2, d0 = darker == 1, darker == 2, darker == 0
    if ((darker < 0) | (darker > 2)).any():
        raise Exception("darker is neither 0(=E), 1, 2")
    b = 1.0 / (1.0 + delta + margin)
    on = d1 & (y > b)
    loss[on], slope[on] = y[on] - b, 1.0
    b = 1.0 + delta + margin
    on = d2 & (y < b)
    loss[on], slope[on] = b - y[on], -1.0
    b = 1.0 + delta - margin
    if margin <= delta:
        on = d0 & (y > b)
        loss[on], slope[on] = y[on] - b, 1.0
        on = d0 & ~(y > b) & (y < 1.0 / b)
        loss[on], slope[on] = 1.0 / b - y[on], -1.0
    else:
        loss[d0] = np.maximum(1.0 / b - y[d0], y[d0] - b)
        slope[d0] = np.where(y[d0] > 1.0, 1.0, -1.0)
    return loss, slope * dy1, slope * dy2


def hinge_points(r, point_offsets, comps, weights, comp_offsets, delta, margin):
    """r: [total] reflectance at the packed points; the other arrays as whdr.dedup_points returns
    them.  Returns (per-image losses float64 [n], gradient of the MEAN of them w.r.t. r float64
    [total]); an image without comparisons or with a zero weight sum has loss 0 and gradient 0."""
    r = np.asarray(r, dtype=np.float64)
    comps = np.asarray(comps, dtype=np.int64).reshape(-1, 3)
    weights = np.asarray(weights, dtype=np.float64)
    n = len(comp_offsets) - 1
    losses = np.zeros(n, dtype=np.float64)
    grad = np.zeros(r.shape[0], dtype=np.float64)
    for i in range(n):
        p0, k0, k1 = int(point_offsets[i]), int(comp_offsets[i]), int(comp_offsets[i + 1])
        wsum = weights[k0:k1].sum()
        if k1 == k0 or not wsum:
            continue
        i1, i2, darker = p0 + comps[k0:k1, 0], p0 + comps[k0:k1, 1], comps[k0:k1, 2]
        loss, g1, g2 = comparison_terms(np.maximum(EPS, r[i1]), np.maximum(EPS, r[i2]), darker,
                                        float(delta), float(margin))
        w = weights[k0:k1]
        losses[i] = (w * loss).sum() / wsum
        np.add.at(grad, i1, w * g1 / wsum / n)
        np.add.at(grad, i2, w * g2 / wsum / n)
    return losses, grad


def ratios(r, point_offsets, comps, comp_offsets):
    """y = L1 / L2 of every comparison (float64): what the fixture keeps away from the borders."""
    r = np.asarray(r, dtype=np.float64)
    comps = np.asarray(comps, dtype=np.int64).reshape(-1, 3)
    base = np.repeat(np.asarray(point_offsets[:-1], dtype=np.int64), np.diff(comp_offsets))
    return np.maximum(EPS, r[base + comps[:, 0]]) / np.maximum(EPS, r[base + comps[:, 1]])


def borders(delta, margin):
    """Every ratio at which some comparison's loss or slope changes."""
    out = [1.0 / (1.0 + delta + margin), 1.0 + delta + margin]
    b = 1.0 + delta - margin
    out += [b, 1.0 / b] if margin <= delta else [1.0]
    return out
