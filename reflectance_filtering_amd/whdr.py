"""WHDR (weighted human disagreement rate) of reflectance predictions against IIW judgements.

Mirrors the evaluation arithmetic of the reference's training layer
(/root/reference/training/layers/whdr_layer.py:180-196 `_lightness`,
:239-250 `_extract_valid_comparisons_with_actual_size`, :253-287 `whdr`) and the JSON reading of
/root/reference/training/createNumpyArrayWithComparisonsForIIW.py:320-347,613-645.

    comparisons[k] = (x1, y1, x2, y2, darker, weight)   x, y normalised to [0,1);
                     darker: 0 = 'E' (about equal), 1 = point 1 darker, 2 = point 2 darker

`whdr` is the per-image host form: one fancy-indexed gather and vectorised decisions over all
judgements of an image, with the dtype promotions the reference's scalar loop would go through
under the installed numpy (pinned on the reference's own values, tests/golden/whdr.npz);
`whdr_batch` evaluates many device-resident predictions in one launch (rf_whdr_f32).
"""
from __future__ import division, print_function

import json

import numpy as np

from . import _ffi

EPS = np.finfo(np.float32).eps  # lightness floor, whdr_layer.py:177
DARKER_CODE = {"1": 1, "2": 2, "E": 0}


def load_judgements(json_path):
    """IIW `<id>.json` -> float64 [n,6] rows (x1, y1, x2, y2, darker, darker_score) with
    normalised coordinates (createNumpyArrayWithComparisonsForIIW.py:320-347, 628-641)."""
    with open(json_path) as fh:
        data = json.load(fh)
    points = {p["id"]: (p["x"], p["y"]) for p in data["intrinsic_points"]}
    rows = []
    for c in data["intrinsic_comparisons"]:
        x1, y1 = points[c["point1"]]
        x2, y2 = points[c["point2"]]
        rows.append([x1, y1, x2, y2, DARKER_CODE[c["darker"]], c["darker_score"]])
    return np.array(rows, dtype=np.float64).reshape(-1, 6)


def to_pixels(comparisons, height, width):
    """Normalised -> pixel coordinates (x * width, y * height, truncated toward zero), stored
    back in the array's own dtype; the judgement and weight columns are untouched
    (contract: whdr_layer.py:239-250)."""
    px = np.array(comparisons, copy=True)
    # the products are formed in the array's own dtype (float32 blobs stay float32: for a
    # coordinate k / width the float32 product rounds to k, the float64 one truncates to k - 1)
    for cols, size in (([0, 2], int(width)), ([1, 3], int(height))):
        px[:, cols] = np.trunc(px[:, cols] * size)
    return px


SPLIT_SCHEMES = ("train_test", "train_val_test", "big_train_mini_val")
_VAL_PERIOD = {"train_val_test": 10, "big_train_mini_val": 100}


def iiw_split(stems, scheme="train_val_test"):
    """The reference's IIW splits (training/createNumpyArrayWithComparisonsForIIW.py:689-728
    narihiraSplitIntoTwoLists, narihiraSplitIntoThreeLists, splitIntoBigTrainMiniVal, over the list
    sorted at :745): {split name: indices into `stems`}, every list in the sorted order, so
    [stems[i] for i in result[name]] is the list the reference's function returns.  The stems (file
    names without directory and extension) are sorted with Python's plain string order; position k
    is `test` if k % 5 == 0, else `val` if k % 10 == 6 (train_val_test) or k % 100 == 6
    (big_train_mini_val), else `train`; train_test has no `val`.  The order is that of the stems,
    not of the file names (`10-x.png` sorts before `10.png`, the stem `10-x` after `10`).  Two
    equal stems make the positions ambiguous and are refused."""
    if scheme not in SPLIT_SCHEMES:
        raise ValueError("scheme must be one of %s" % ", ".join(SPLIT_SCHEMES))
    stems = [str(s) for s in stems]
    order = sorted(range(len(stems)), key=lambda i: stems[i])
    for a, b in zip(order, order[1:]):
        if stems[a] == stems[b]:
            raise ValueError("duplicate stem %r (items %d and %d): its position in the split is "
                             "ambiguous" % (stems[a], a, b))
    period = _VAL_PERIOD.get(scheme)
    split = {"train": [], "test": []}
    if period:
        split["val"] = []
    for k, i in enumerate(order):
        if k % 5 == 0:
            split["test"].append(i)
        elif period and k % period == 6:
            split["val"].append(i)
        else:
            split["train"].append(i)
    return split


def _point_lightness(reflectance, ys, xs):
    """Lightness of the pixels (ys[i], xs[i]) of a [c,h,w] image, one gather for all points:
    the channel mean (3 channels, in the image's dtype like np.mean of one pixel) or the value
    itself (1 channel), floored at EPS.  A NaN fails `> EPS` and becomes EPS, as it does through
    Python's max() in the reference (whdr_layer.py:180-196)."""
    channels = reflectance.shape[0]
    if channels not in (1, 3):
        raise Exception("Expecting 1 or 3 channels to compute lightness!")
    picked = reflectance[:, ys, xs]                       # [c, n]
    value = picked[0] if channels == 1 else picked.mean(axis=0)
    return np.where(value > EPS, value, EPS)


def whdr(reflectance, comparisons, delta=0.1):
    """WHDR of one [c,h,w] reflectance image against judgements in pixel coordinates: the
    weight of the judgements the image disagrees with over the weight of all of them
    (arithmetic contract: whdr_layer.py:253-287).  No judgements -> 0.0.

    All judgements are decided at once: the image says "point 1 darker" (1) when l2/l1 exceeds
    1 + delta, else "point 2 darker" (2) when l1/l2 does, else "about equal" (0).  The two
    weight totals are running sums in judgement order (np.cumsum adds sequentially) in the
    dtype `0.0 + weight` has under the installed numpy, and the threshold is compared in the
    dtype `lightness ratio > python float` is compared in under it - the same promotions the
    reference's scalar loop goes through."""
    reflectance = np.asarray(reflectance)
    judgements = np.asarray(comparisons)
    if judgements.shape[0] == 0:
        if reflectance.shape[0] not in (1, 3):
            raise Exception("Expecting 1 or 3 channels to compute lightness!")
        return 0.0
    pts = judgements[:, :5].astype(int)
    first = _point_lightness(reflectance, pts[:, 1], pts[:, 0])
    second = _point_lightness(reflectance, pts[:, 3], pts[:, 2])
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        up, down = second / first, first / second
    # scalar-vs-python-float promotion of the installed numpy (float32 under NumPy >= 2)
    cmp_t = (first.dtype.type(1) * 1.5).dtype
    limit = cmp_t.type(1 + delta)
    verdict = np.where(up.astype(cmp_t) > limit, 1, np.where(down.astype(cmp_t) > limit, 2, 0))
    weights = judgements[:, 5]
    acc_t = (0.0 + weights.dtype.type(0)).dtype
    weights = weights.astype(acc_t)
    total = np.cumsum(weights)[-1]
    if not total:
        return 0.0
    wrong = np.cumsum(np.where(verdict != pts[:, 4], weights, acc_t.type(0)))[-1]
    return wrong / total


def whdr_batch(reflectances, comparisons_px, delta=0.1):
    """WHDR of N device-resident predictions in one launch.
    reflectances: CUDA float32 [N,C,H,W] (C = 1 or 3) or [N,H,W];
    comparisons_px: list of N arrays [n_i,6] in pixel coordinates (to_pixels), any n_i >= 0.
    Returns float64 [N] (host).  Lightness, ratios and the decision are float32 like the
    reference's blobs, compared against float32(1 + delta) (NumPy >= 2 scalar promotion; NumPy 1
    compared in float64, a difference confined to ratios within one float32 ulp above
    1 + delta); the weighted sums are float64, accumulated in comparison order."""
    torch = _ffi.require_gpu()
    lib = _ffi.load_library()
    r = reflectances
    if not (torch.is_tensor(r) and r.is_cuda and r.dtype == torch.float32 and r.is_contiguous()
            and r.dim() in (3, 4)):
        raise ValueError("reflectances must be a contiguous CUDA float32 tensor [N,C,H,W] or [N,H,W]")
    if r.dim() == 3:
        r = r.unsqueeze(1)
    n, c, h, w = r.shape
    if c not in (1, 3):
        raise Exception("Expecting 1 or 3 channels to compute lightness!")
    if len(comparisons_px) != n:
        raise ValueError("one comparison array per image")
    offsets = np.zeros(n + 1, dtype=np.int32)
    rows = []
    for i, comp in enumerate(comparisons_px):
        comp = np.asarray(comp, dtype=np.float64).reshape(-1, 6)
        xy = comp[:, :4].astype(np.int64)
        if comp.shape[0] and (xy.min() < 0 or xy[:, [0, 2]].max() >= w or xy[:, [1, 3]].max() >= h):
            raise IndexError("comparison point outside the %dx%d image %d" % (w, h, i))
        rows.append(comp)
        offsets[i + 1] = offsets[i] + comp.shape[0]
    allc = np.concatenate(rows, axis=0) if rows else np.zeros((0, 6))
    pts = np.ascontiguousarray(allc[:, :5].astype(np.int32))
    wts = np.ascontiguousarray(allc[:, 5].astype(np.float64))
    dev = r.device
    d_pts = torch.from_numpy(pts).to(dev) if pts.size else torch.zeros((1, 5), dtype=torch.int32, device=dev)
    d_wts = torch.from_numpy(wts).to(dev) if wts.size else torch.zeros(1, dtype=torch.float64, device=dev)
    d_off = torch.from_numpy(offsets).to(dev)
    out = torch.empty(n, dtype=torch.float64, device=dev)
    if n:
        rc = lib.rf_whdr_f32(r.data_ptr(), n, c, h, w, d_pts.data_ptr(), d_wts.data_ptr(),
                             d_off.data_ptr(), float(delta), out.data_ptr(),
                             _ffi.current_stream_ptr(torch))
        _ffi.check(rc, "rf_whdr_f32")
    return out.cpu().numpy()


def dedup_points(comparisons_px, height, width):
    """The point lists of rf_jbf_points_u8 / rf_whdr_points_u8 for judgements in pixel
    coordinates (IIW comparisons share points): per image the distinct (x, y) of its comparisons,
    sorted by (x, y), and each comparison re-indexed into them.  Coordinates are truncated to int
    like whdr_batch does, and checked against the image size.
    Returns (points int32 [total,2] (x, y), point_offsets int32 [n+1], comps int32 [m,3]
    (index 1, index 2, darker), weights float64 [m], comp_offsets int32 [n+1])."""
    n = len(comparisons_px)
    point_offsets = np.zeros(n + 1, dtype=np.int64)
    comp_offsets = np.zeros(n + 1, dtype=np.int64)
    pts, comps, wts = [], [], []
    for i, comp in enumerate(comparisons_px):
        comp = np.asarray(comp, dtype=np.float64).reshape(-1, 6)
        xy = comp[:, :4].astype(np.int64)
        if comp.shape[0] and (xy.min() < 0 or xy[:, [0, 2]].max() >= width
                              or xy[:, [1, 3]].max() >= height):
            raise IndexError("comparison point outside the %dx%d image %d" % (width, height, i))
        both = np.concatenate([xy[:, 0:2], xy[:, 2:4]], axis=0)
        uniq, inverse = np.unique(both, axis=0, return_inverse=True)
        inverse = inverse.reshape(-1)
        m = comp.shape[0]
        pts.append(uniq.reshape(-1, 2))
        comps.append(np.stack([inverse[:m], inverse[m:], comp[:, 4].astype(np.int64)], axis=1))
        wts.append(comp[:, 5])
        point_offsets[i + 1] = point_offsets[i] + uniq.shape[0]
        comp_offsets[i + 1] = comp_offsets[i] + m
    cat = (lambda parts, shape: np.concatenate(parts, axis=0) if parts else np.zeros(shape))
    if comp_offsets[-1] >= 2 ** 31 or point_offsets[-1] >= 2 ** 31:
        raise ValueError("too many comparisons")
    return (cat(pts, (0, 2)).astype(np.int32), point_offsets.astype(np.int32),
            cat(comps, (0, 3)).astype(np.int32), cat(wts, (0,)).astype(np.float64),
            comp_offsets.astype(np.int32))


def _check_point_arrays(torch, samples, point_offsets, comps, weights, comp_offsets):
    """The checks of whdr_points_u8 and whdr_points_values_u8, before any device work: samples is a
    contiguous CUDA uint8 [S, total, C] with C of 1 or 3, the arrays agree with each other, and every
    comparison index stays inside its image's points (the device entries cannot check that).
    Returns (point_offsets int64, comps int64 [m,3], weights float64, comp_offsets int64)."""
    if not (torch.is_tensor(samples) and samples.is_cuda and samples.dtype == torch.uint8
            and samples.is_contiguous() and samples.dim() == 3):
        raise ValueError("samples must be a contiguous CUDA uint8 tensor [S, total, C]")
    n_sets, total, c = samples.shape
    if c not in (1, 3):
        raise Exception("Expecting 1 or 3 channels to compute lightness!")
    point_offsets = np.asarray(point_offsets, dtype=np.int64).ravel()
    comp_offsets = np.asarray(comp_offsets, dtype=np.int64).ravel()
    comps = np.asarray(comps, dtype=np.int64).reshape(-1, 3)
    weights = np.asarray(weights, dtype=np.float64).ravel()
    n = comp_offsets.shape[0] - 1
    if n < 0 or point_offsets.shape[0] < n or comps.shape[0] != weights.shape[0] \
            or comp_offsets[-1] != comps.shape[0]:
        raise ValueError("inconsistent point / comparison arrays")
    for i in range(n):
        k0, k1 = comp_offsets[i], comp_offsets[i + 1]
        size = (point_offsets[i + 1] if i + 1 < point_offsets.shape[0] else total) - point_offsets[i]
        if k1 > k0 and (comps[k0:k1, :2].min() < 0 or comps[k0:k1, :2].max() >= size):
            raise IndexError("comparison index outside the points of image %d" % i)
    return point_offsets, comps, weights, comp_offsets


def whdr_points_u8(samples, point_offsets, comps, weights, comp_offsets, delta=0.1):
    """WHDR of uint8 predictions sampled at points (rf_whdr_points_u8): samples is CUDA uint8
    [S, total, C] (C = 1 or 3; e.g. ops.joint_bilateral_points_u8's output), the other arrays as
    dedup_points returns them.  Each byte counts as float32(byte) / 255; returns float64 [S, n]
    (host), equal bit for bit to whdr_batch on the float32 images bytes / 255."""
    torch = _ffi.require_gpu()
    lib = _ffi.load_library()
    point_offsets, comps, weights, comp_offsets = _check_point_arrays(
        torch, samples, point_offsets, comps, weights, comp_offsets)
    n_sets, total, c = samples.shape
    n = comp_offsets.shape[0] - 1
    out = np.zeros((n_sets, n), dtype=np.float64)
    if n == 0 or n_sets == 0 or total == 0 or comps.shape[0] == 0:
        return out
    dev = samples.device
    up = (lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev))
    d_po, d_co = up(point_offsets[:n], np.int32), up(comp_offsets, np.int32)
    d_comps, d_wts = up(comps, np.int32), up(weights, np.float64)
    d_out = torch.empty(n_sets * n, dtype=torch.float64, device=dev)
    rc = lib.rf_whdr_points_u8(samples.data_ptr(), n_sets, total, c, n, d_po.data_ptr(),
                               d_comps.data_ptr(), d_wts.data_ptr(), d_co.data_ptr(), float(delta),
                               d_out.data_ptr(), _ffi.current_stream_ptr(torch))
    _ffi.check(rc, "rf_whdr_points_u8")
    return d_out.cpu().numpy().reshape(n_sets, n)


CODINGS = ("linear", "srgb")


def value_table(coding):
    """float32[256]: the value a stored byte stands for when a result is scored.  "linear" is
    byte / 255 in float32 (what whdr_points_u8 computes), "srgb" image_utils.srgb_byte_lut() (a
    result saved as sRGB, the reference's load_image(..., is_srgb=True)); a caller's own float32[256]
    array is taken as it is.  Anything else - another name, shape or dtype, a non-finite entry -
    is a ValueError."""
    if isinstance(coding, str):
        if coding == "linear":
            return np.arange(256, dtype=np.float32) / np.float32(255)
        if coding == "srgb":
            from .image_utils import srgb_byte_lut
            return srgb_byte_lut()
        raise ValueError("coding must be one of %s or a float32[256] array (got %r)"
                         % (", ".join(CODINGS), coding))
    if not (isinstance(coding, np.ndarray) and coding.dtype == np.float32 and coding.shape == (256,)):
        raise ValueError("a value table is a float32 array of shape (256,)")
    if not np.isfinite(coding).all():
        raise ValueError("a value table holds finite values only")
    return coding


# bytes of float32 values staged by one rf_whdr_f32 call of whdr_points_values_u8, and the images one
# launch of it accepts (one 64-lane workgroup per image, below 2^32 work-items)
WHDR_VALUES_BYTES = 1 << 28
WHDR_VALUES_IMAGES = (1 << 26) - 1


def plan_value_chunks(counts, n_sets, channels):
    """The rf_whdr_f32 calls of whdr_points_values_u8: counts[i] = distinct referenced points of
    image i.  Returns [(i0, i1, s0, s1)]: images i0..i1-1 of sets s0..s1-1 as (s1 - s0) * (i1 - i0)
    rows of channels * max(counts[i0:i1]) floats.  Images are taken in order while all sets of them
    stay under WHDR_VALUES_BYTES and WHDR_VALUES_IMAGES rows; an image that alone exceeds either has
    its sets cut (one set of one image over the byte limit is a call of its own).  Host only."""
    counts = [int(k) for k in counts]
    chunks, i0 = [], 0

    def fits(rows, width):
        return rows <= WHDR_VALUES_IMAGES and rows * channels * max(1, width) * 4 <= WHDR_VALUES_BYTES

    while i0 < len(counts):
        i1, width = i0 + 1, counts[i0]
        while i1 < len(counts) and fits(n_sets * (i1 + 1 - i0), max(width, counts[i1])):
            width = max(width, counts[i1])
            i1 += 1
        per = n_sets
        while per > 1 and not fits(per * (i1 - i0), width):
            per = (per + 1) // 2
        chunks.extend((i0, i1, s0, min(s0 + per, n_sets)) for s0 in range(0, n_sets, per))
        i0 = i1
    return chunks


def whdr_points_values_u8(samples, point_offsets, comps, weights, comp_offsets, values, delta=0.1):
    """whdr_points_u8 with a value table: each byte counts as values[byte] (value_table).  Arguments,
    checks and result are whdr_points_u8's; the value for set s, image i equals host `whdr` on the
    float32 image values[bytes] (planar), bit for bit - with the "linear" table whdr_points_u8's value.

    rf_whdr_points_u8 has no table argument, so the bytes go through the float entry: the points
    that the comparisons reference are gathered (device work per distinct referenced point, whatever
    `total` is - a guided sweep passes whole images), looked up in the table on the device, laid out
    per (set, image) as a [C, 1, Pmax] float32 image padded to the call's largest point count, and
    scored by whdr_batch (rf_whdr_f32) with comparisons (index 1, 0, index 2, 0, darker, weight).
    plan_value_chunks cuts the call so that the floats stay under WHDR_VALUES_BYTES."""
    torch = _ffi.require_gpu()
    table = value_table(values)
    point_offsets, comps, weights, comp_offsets = _check_point_arrays(
        torch, samples, point_offsets, comps, weights, comp_offsets)
    n_sets, total, c = samples.shape
    n = comp_offsets.shape[0] - 1
    out = np.zeros((n_sets, n), dtype=np.float64)
    if n == 0 or n_sets == 0 or total == 0 or comps.shape[0] == 0:
        return out
    # distinct referenced points per image: keys sort by image, then by the point's place in a set
    image = np.repeat(np.arange(n, dtype=np.int64), np.diff(comp_offsets))
    place = point_offsets[image][:, None] + comps[:, :2]
    if place.min() < 0 or place.max() >= total:
        raise IndexError("comparison index outside the samples")
    keys, inverse = np.unique(image[:, None] * total + place, return_inverse=True)
    first = np.searchsorted(keys, np.arange(n + 1, dtype=np.int64) * total)
    local = inverse.reshape(-1, 2) - first[image][:, None]
    counts = np.diff(first)
    rows = np.zeros((comps.shape[0], 6), dtype=np.float64)
    rows[:, 0], rows[:, 2], rows[:, 4], rows[:, 5] = local[:, 0], local[:, 1], comps[:, 2], weights
    chunks = plan_value_chunks(counts, n_sets, c)
    # a call's comparisons are repeated per set behind rf_whdr_f32's int32 offsets
    if any((s1 - s0) * (comp_offsets[i1] - comp_offsets[i0]) >= 2 ** 31 for i0, i1, s0, s1 in chunks):
        raise ValueError("too many comparisons")
    d_table = torch.from_numpy(table).to(samples.device)
    for i0, i1, s0, s1 in chunks:
        if comp_offsets[i1] == comp_offsets[i0]:
            continue
        width = int(counts[i0:i1].max())
        gather = np.zeros((i1 - i0, width), dtype=np.int64)     # padding reads the set's first sample
        for i in range(i0, i1):
            gather[i - i0, :counts[i]] = keys[first[i]:first[i + 1]] - i * total
        picked = samples[s0:s1].index_select(1, _index(gather.ravel(), samples))
        planar = picked.view(s1 - s0, i1 - i0, width, c).permute(0, 1, 3, 2).contiguous()
        floats = d_table.index_select(0, planar.view(-1).int()).view(-1, c, 1, width)
        per_image =[rows[comp_offsets[i]:comp_offsets[i + 1]] for i in range(i0, i1)]
        out[s0:s1, i0:i1] = whdr_batch(floats, per_image * (s1 - s0), delta).reshape(s1 - s0, i1 - i0)
    return out


def _score(samples, point_offsets, comps, weights, comp_offsets, delta, values):
    """The WHDR call of a sweep: whdr_points_u8 as ever, whdr_points_values_u8 with a value table."""
    if values is None:
        return whdr_points_u8(samples, point_offsets, comps, weights, comp_offsets, delta)
    return whdr_points_values_u8(samples, point_offsets, comps, weights, comp_offsets, values, delta)


# bytes of filtered images held at once by the guided half of a sweep (one group of pairs)
SWEEP_GUIDED_BYTES = 1 << 30


def _sweep_batch(filter_type, src, joint, comparisons_px, pairs, delta, grey_as_bgr, values=None):
    """sweep() on one device batch of equal-size images: float64 [P, N]."""
    import torch
    from . import ops
    n, h, w, c = src.shape
    pts, point_offsets, comps, weights, comp_offsets = dedup_points(comparisons_px, h, w)
    out = np.zeros((pairs.shape[0], n), dtype=np.float64)
    if comps.shape[0] == 0:
        return out
    if filter_type == "bilateral":
        samples = ops.joint_bilateral_points_u8(joint, src, pts, point_offsets, pairs, d=-1,
                                                grey_as_bgr=grey_as_bgr)
        return _score(samples, point_offsets, comps, weights, comp_offsets, delta, values)
    # guided: full passes (its window sums are sequential chains by contract, a point cannot be
    # evaluated on its own); the whole images are the point lists: pixel index y * w + x
    npx = h * w
    image_offsets = np.arange(n + 1, dtype=np.int64) * npx
    px_comps = comps.copy()
    for i in range(n):
        k0, k1 = comp_offsets[i], comp_offsets[i + 1]
        own = pts[point_offsets[i]:point_offsets[i + 1]].astype(np.int64)
        for col in (0, 1):
            q = own[comps[k0:k1, col]]
            px_comps[k0:k1, col] = q[:, 1] * w + q[:, 0]
    per = max(1, SWEEP_GUIDED_BYTES // max(1, n * npx * c))
    for p0 in range(0, pairs.shape[0], per):
        chunk = pairs[p0:p0 + per]
        filtered = torch.empty((chunk.shape[0], n, h, w, c), dtype=torch.uint8, device=src.device)
        for j, (sc, ss) in enumerate(chunk):
            ops.guided_filter_u8(joint, src, int(ss), float(sc), out=filtered[j],
                                 grey_as_bgr=grey_as_bgr)
        out[p0:p0 + chunk.shape[0]] = _score(
            filtered.view(chunk.shape[0], n * npx, c), image_offsets, px_comps, weights,
            comp_offsets, delta, values)
    return out


# a ragged bilateral call holds at most this many pixels and this many output bytes
SWEEP_PACK_PIXELS = 1 << 30
SWEEP_PACK_OUT_BYTES = 1 << 30


def join_dedup(parts):
    """dedup_points results of single images joined into the arrays of one call over all of them
    (comparison indices are relative to their image's points, so only the offsets accumulate)."""
    ends = (lambda k: np.concatenate([[0], np.cumsum([p[k][1] for p in parts], dtype=np.int64)]))
    point_offsets, comp_offsets = ends(1), ends(4)
    if comp_offsets[-1] >= 2 ** 31 or point_offsets[-1] >= 2 ** 31:
        raise ValueError("too many comparisons")
    cat = (lambda k, shape, dt: np.concatenate([p[k] for p in parts], axis=0).astype(dt)
           if parts else np.zeros(shape, dt))
    return (cat(0, (0, 2), np.int32), point_offsets.astype(np.int32), cat(2, (0, 3), np.int32),
            cat(3, (0,), np.float64), comp_offsets.astype(np.int32))


def dedup_points_ragged(comparisons_px, sizes):
    """dedup_points for images of different sizes: sizes[i] = (h_i, w_i), and the points of image i
    are deduplicated and checked with its own size.  Returns what dedup_points returns."""
    return join_dedup([dedup_points([comp], int(h), int(w))
                       for comp, (h, w) in zip(comparisons_px, sizes)])


def plan_packs(keys, pixels, points, n_pairs, src_cn):
    """The ragged calls of a bilateral sweep over a list: image indices grouped by key (the channel
    counts) wherever they stand in the list, each group cut so that a pack stays under
    SWEEP_PACK_PIXELS pixels and n_pairs * points * src_cn[key] under SWEEP_PACK_OUT_BYTES output
    bytes (an image over a limit on its own is a pack of one).  Host only."""
    packs = []
    for key in sorted(set(keys), key=keys.index):
        per_point = n_pairs * src_cn(key)
        cur, npx, npt = [], 0, 0
        for i in (i for i, k in enumerate(keys) if k == key):
            if cur and (npx + pixels[i] > SWEEP_PACK_PIXELS
                        or (npt + points[i]) * per_point > SWEEP_PACK_OUT_BYTES):
                packs.append(cur)
                cur, npx, npt = [], 0, 0
            cur.append(i)
            npx += pixels[i]
            npt += points[i]
        if cur:
            packs.append(cur)
    return packs


def sweep_packed(src, joint, sizes, dedup, pairs, delta=0.1, grey_as_bgr=False, values=None):
    """The bilateral sweep on one pack: images of sizes[i] = (h_i, w_i) packed one after another in
    the CUDA uint8 tensors src / joint [total pixels, C], dedup = dedup_points_ragged of their
    comparisons.  One ragged filter call and one WHDR call: float64 [P, n]."""
    from . import ops
    pts, point_offsets, comps, weights, comp_offsets = dedup
    if comps.shape[0] == 0:
        return np.zeros((np.asarray(pairs).reshape(-1, 2).shape[0], len(sizes)), dtype=np.float64)
    samples = ops.joint_bilateral_points_ragged_u8(joint, src, pts, point_offsets, pairs, d=-1,
                                                   grey_as_bgr=grey_as_bgr, sizes=sizes)
    return _score(samples, point_offsets, comps, weights, comp_offsets, delta, values)


def sweep_guided_packed(src, joint, sizes, dedup, pairs, delta=0.1, grey_as_bgr=False, values=None):
    """The guided sweep on one pack: one-channel images of sizes[i] = (h_i, w_i) packed one after
    another in the CUDA uint8 tensors src [total pixels, 1] / joint [total pixels, C], dedup =
    dedup_points_ragged of their comparisons.  Pairs are
    grouped by radius, equal (radius, eps) pairs computed once: per radius one
    ops.guided_filter_ragged_sweep_u8 call (one ragged filter call per eps; a radius outside 1..128
    falls back inside the entry, to the same bytes) for as many eps as keep the
    filtered bytes under SWEEP_GUIDED_BYTES, and one WHDR call on the packed results - the packed
    images are the point list, pixel index y * w_i + x behind the image's first pixel.
    float64 [P, n]."""
    from . import ops
    pts, point_offsets, comps, weights, comp_offsets = dedup
    pairs = np.asarray(pairs, dtype=np.float64).reshape(-1, 2)
    out = np.zeros((pairs.shape[0], len(sizes)), dtype=np.float64)
    if comps.shape[0] == 0:
        return out
    image_offsets = np.concatenate([[0], np.cumsum([int(h) * int(w) for h, w in sizes],
                                                   dtype=np.int64)])
    px_comps = comps.copy()
    for i, (_, w) in enumerate(sizes):
        k0, k1 = comp_offsets[i], comp_offsets[i + 1]
        own = pts[point_offsets[i]:point_offsets[i + 1]].astype(np.int64)
        for col in (0, 1):
            q = own[comps[k0:k1, col]]
            px_comps[k0:k1, col] = q[:, 1] * int(w) + q[:, 0]
    by_radius = {}      # radius -> {eps: [rows of pairs]}, both in order of first appearance
    for p, (sc, ss) in enumerate(pairs):
        by_radius.setdefault(int(ss), {}).setdefault(float(sc), []).append(p)
    per = max(1, SWEEP_GUIDED_BYTES // max(1, int(image_offsets[-1])))
    for radius, rows in by_radius.items():
        eps = list(rows)
        for e0 in range(0, len(eps), per):
            chunk = eps[e0:e0 + per]
            filtered = ops.guided_filter_ragged_sweep_u8(joint, src, radius, chunk,
                                                         grey_as_bgr=grey_as_bgr, sizes=sizes)
            res = _score(filtered, image_offsets, px_comps, weights, comp_offsets, delta, values)
            for j, e in enumerate(chunk):
                out[rows[e]] = res[j]
    return out


# bytes of full-pass results held at once by the bilateral half of a chain (two buffers per pair)
SWEEP_CHAIN_BYTES = 1 << 30


def _empty(shape, like):
    """An uninitialised uint8 tensor of `shape` on the device of `like`."""
    import torch
    return torch.empty(tuple(shape), dtype=torch.uint8, device=like.device)


def _sample(results, index):
    """The pixels `index` (device int64 [total]) of every result (tensors of equal shape whose last
    dimension is the channel): uint8 [len(results), total, C]."""
    import torch
    return torch.stack([r.view(-1, r.shape[-1])[index] for r in results]).contiguous()


def _index(values, like):
    """Host int64 indices on the device of `like`."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(values, dtype=np.int64)).to(like.device)


def _cat(parts):
    import torch
    return torch.cat(list(parts)).contiguous()


def _point_pixels(dedup, sizes):
    """Where the deduplicated points of images packed one after another lie: (image_offsets int64
    [n+1], the first pixel of every image; pixels int64 [total points], y * w_i + x behind it)."""
    pts, point_offsets = dedup[0], np.asarray(dedup[1], dtype=np.int64)
    image_offsets = np.concatenate([[0], np.cumsum([int(h) * int(w) for h, w in sizes],
                                                   dtype=np.int64)])
    widths = np.repeat(np.array([int(w) for _, w in sizes], dtype=np.int64), np.diff(point_offsets))
    return image_offsets, pts[:, 1].astype(np.int64) * widths + pts[:, 0].astype(np.int64)


def _pixel_comps(dedup, pixels):
    """The comparisons re-indexed from their image's points to its pixels (the whole image as the
    point list, as sweep_guided_packed scores a full pass)."""
    point_offsets, comps, comp_offsets = (np.asarray(dedup[k], dtype=np.int64) for k in (1, 2, 4))
    first = np.repeat(point_offsets[:-1], np.diff(comp_offsets))    # first point of a comparison's image
    px = dedup[2].copy()
    px[:, :2] = pixels[first[:, None] + comps[:, :2]]
    return px


def _chain_guided(src, sizes, dedup, pairs, iterations, delta, one_pass, values=None):
    """The guided chain on images that lie one after another in `src` (a packed list [total pixels,
    C], or a batch [N,H,W,C] with sizes = N x (H, W)): float64 [K, P, n].  Pairs are grouped by radius
    and equal (radius, eps) pairs computed once, as in sweep_guided_packed;
    one_pass(cur, radius, eps, out) filters cur into out once and returns the result, which is the
    src of that pair's next pass.  Every pass of a chunk of eps is scored by one WHDR call on the
    filtered images as point lists; a chunk's filtered bytes - the pass being written and the one it
    reads - stay under SWEEP_GUIDED_BYTES."""
    pts, point_offsets, comps, weights, comp_offsets = dedup
    out = np.zeros((iterations, pairs.shape[0], len(sizes)), dtype=np.float64)
    if comps.shape[0] == 0:
        return out
    image_offsets, pixels = _point_pixels(dedup, sizes)
    px_comps = _pixel_comps(dedup, pixels)
    by_radius = {}      # radius -> {eps: [rows of pairs]}, both in order of first appearance
    for p, (sc, ss) in enumerate(pairs):
        by_radius.setdefault(int(ss), {}).setdefault(float(sc), []).append(p)
    shape = tuple(src.shape)
    per = max(1, SWEEP_GUIDED_BYTES // max(1, 2 * int(np.prod(shape))))
    for radius, rows in by_radius.items():
        eps = list(rows)
        for e0 in range(0, len(eps), per):
            chunk = eps[e0:e0 + per]
            cur = [src] * len(chunk)
            for k in range(iterations):
                filtered = _empty((len(chunk),) + shape, src)
                cur = [one_pass(cur[j], radius, e, filtered[j]) for j, e in enumerate(chunk)]
                res = _score(filtered.view(len(chunk), -1, shape[-1]), image_offsets, px_comps,
                             weights, comp_offsets, delta, values)
                for j, e in enumerate(chunk):
                    out[k, rows[e]] = res[j]
    return out


def _chain_bilateral(src, sizes, dedup, pairs, iterations, delta, full_pass, point_pass,
                     values=None):
    """The bilateral chain on images that lie one after another in `src` (as in _chain_guided):
    float64 [K, P, n].  full_pass(cur, sigma_color, sigma_space, out) filters cur into out and returns
    the result; point_pass(cur, sigma_color, sigma_space) evaluates one more pass at the deduplicated
    points only: uint8 [1, total points, C].  Passes 1..K-1 of a pair ping-pong between two buffers
    and are scored on their samples at the points, pass K is the point pass on the result of pass
    K-1; the pairs of a group share each pass's WHDR call, and a group's buffers stay under
    SWEEP_CHAIN_BYTES."""
    pts, point_offsets, comps, weights, comp_offsets = dedup
    out = np.zeros((iterations, pairs.shape[0], len(sizes)), dtype=np.float64)
    if comps.shape[0] == 0:
        return out
    image_offsets, pixels = _point_pixels(dedup, sizes)
    index = _index(pixels + np.repeat(image_offsets[:-1],
                                      np.diff(np.asarray(point_offsets, dtype=np.int64))), src)
    shape = tuple(src.shape)
    n_bufs = min(iterations - 1, 2)
    per = max(1, SWEEP_CHAIN_BYTES // max(1, n_bufs * int(np.prod(shape))))
    for p0 in range(0, pairs.shape[0], per):
        group = [(float(sc), float(ss)) for sc, ss in pairs[p0:p0 + per]]
        rows = slice(p0, p0 + len(group))
        bufs = _empty((len(group), n_bufs) + shape, src)
        cur = [src] * len(group)
        for k in range(iterations - 1):
            cur = [full_pass(cur[g], sc, ss, bufs[g, k % 2]) for g, (sc, ss) in enumerate(group)]
            out[k, rows] = _score(_sample(cur, index), point_offsets, comps, weights, comp_offsets,
                                  delta, values)
        last = _cat(point_pass(cur[g], sc, ss) for g, (sc, ss) in enumerate(group))
        out[iterations - 1, rows] = _score(last, point_offsets, comps, weights, comp_offsets, delta,
                                           values)
    return out


def chain_packed(src, joint, sizes, dedup, pairs, iterations, delta=0.1, grey_as_bgr=False,
                 values=None):
    """sweep_packed for a chain of `iterations` >= 2 passes with the joint held fixed: float64
    [K, P, n], slice k the WHDR after pass k + 1.  Per pair K - 1 full ragged passes
    (ops.joint_bilateral_ragged_u8, the uint8 result of one the src of the next) and one point pass
    (ops.joint_bilateral_points_ragged_u8 on the result of pass K - 1)."""
    from . import ops
    pairs = np.asarray(pairs, dtype=np.float64).reshape(-1, 2)
    return _chain_bilateral(
        src, sizes, dedup, pairs, iterations, delta,
        lambda cur, sc, ss, out: ops.joint_bilateral_ragged_u8(
            joint, cur, -1, sc, ss, grey_as_bgr=grey_as_bgr, sizes=sizes, out=out)[0],
        lambda cur, sc, ss: ops.joint_bilateral_points_ragged_u8(
            joint, cur, dedup[0], dedup[1], [(sc, ss)], d=-1, grey_as_bgr=grey_as_bgr, sizes=sizes),
        values=values)


def chain_guided_packed(src, joint, sizes, dedup, pairs, iterations, delta=0.1, grey_as_bgr=False,
                        values=None):
    """sweep_guided_packed for a chain of `iterations` >= 2 passes with the guide held fixed: float64
    [K, P, n], slice k the WHDR after pass k + 1.  Per distinct (radius, eps) one
    ops.guided_filter_ragged_u8 call per pass, the packed result of one the src of the next."""
    from . import ops
    pairs = np.asarray(pairs, dtype=np.float64).reshape(-1, 2)
    return _chain_guided(
        src, sizes, dedup, pairs, iterations, delta,
        lambda cur, radius, eps, out: ops.guided_filter_ragged_u8(
            joint, cur, radius, eps, iterations=1, grey_as_bgr=grey_as_bgr, sizes=sizes, out=out)[0],
        values=values)


def _chain_batch(filter_type, src, joint, comparisons_px, pairs, iterations, delta, grey_as_bgr,
                 values=None):
    """The chain on one device batch of equal-size images, through the uniform ops: float64
    [K, P, N]."""
    from . import ops
    n, h, w, _ = src.shape
    dedup = dedup_points(comparisons_px, h, w)
    sizes = [(h, w)] * n
    if filter_type == "bilateral":
        return _chain_bilateral(
            src, sizes, dedup, pairs, iterations, delta,
            lambda cur, sc, ss, out: ops.joint_bilateral_u8(joint, cur, -1, sc, ss, out=out,
                                                            grey_as_bgr=grey_as_bgr),
            lambda cur, sc, ss: ops.joint_bilateral_points_u8(joint, cur, dedup[0], dedup[1],
                                                              [(sc, ss)], d=-1,
                                                              grey_as_bgr=grey_as_bgr),
            values=values)
    return _chain_guided(
        src, sizes, dedup, pairs, iterations, delta,
        lambda cur, radius, eps, out: ops.guided_filter_u8(joint, cur, radius, eps, out=out,
                                                           grey_as_bgr=grey_as_bgr),
        values=values)


def _as3(image):
    return image.unsqueeze(-1) if image.dim() == 2 else image


def _pack_list(images, torch):
    """Images (CUDA tensors or numpy arrays [H,W,C] / [H,W]) packed on the device as
    [total pixels, C]: host arrays are joined on the host and uploaded with one copy."""
    if not any(torch.is_tensor(im) for im in images):
        arrs = [np.asarray(im) for im in images]
        c = arrs[0].shape[2] if arrs[0].ndim == 3 else 1
        return torch.from_numpy(np.concatenate([a.reshape(-1, c) for a in arrs])).cuda()
    parts = [_as3(im if torch.is_tensor(im) else torch.as_tensor(np.asarray(im))).cuda().contiguous()
             for im in images]
    return torch.cat([p.view(-1, p.shape[2]) for p in parts])


def _stack(images):
    """Equal-size images (CUDA tensors or numpy arrays) as one device batch [N,H,W,C]."""
    import torch
    parts = [_as3(torch.as_tensor(np.asarray(im)) if not torch.is_tensor(im) else im)
             for im in images]
    return torch.stack([p.cuda() for p in parts]).contiguous()


def sweep(filter_type, src, joint, comparisons_px, sigma_pairs, delta=0.1, grey_as_bgr=False,
          iterations=1, values=None):
    """WHDR of filter(joint, src) for every (sigma_color, sigma_space) pair: float64 [P, N] on the
    host, row p = pair p, column i = image i in the caller's order.

    iterations = K > 1 scores a chain: float64 [K, P, N], slice k the WHDR after the filter has been
    applied k + 1 times with the joint held fixed and the uint8 result of one pass the src of the
    next (the rule of filter_reflectance.apply_filter_batch(iterations=)).  A chain takes the routes
    described below pass by pass: 'guided' one full pass per distinct (radius, eps) at a time
    (ops.guided_filter_ragged_u8(iterations=1) on a packed list, ops.guided_filter_u8 on a batch),
    every pass scored; 'bilateral' K - 1 full passes per pair (ops.joint_bilateral_ragged_u8 /
    ops.joint_bilateral_u8, two ping-pong buffers per pair, scored on their samples at the judgement
    points) and pass K at the points only.

    src / joint: CUDA uint8 batches [N,H,W,C], or lists of N images (CUDA tensors or numpy
    arrays [H,W,C]) that may differ in size.  comparisons_px: N arrays [n_i,6] in pixel coordinates
    (to_pixels).  grey_as_bgr: the joint has one channel and counts as three equal ones (as in
    ops.joint_bilateral_u8).
      'bilateral'  joint_bilateral_u8(joint, src, -1, sigma_color, sigma_space) evaluated at the
                   judgement points only, points deduplicated per image.  A batch goes through
                   ops.joint_bilateral_points_u8; a list is packed, whatever its sizes and their
                   order, into ragged calls (ops.joint_bilateral_points_ragged_u8: the same bytes)
                   of equal channel counts and at most SWEEP_PACK_PIXELS pixels, one filter launch
                   and one WHDR launch per pack;
      'guided'     guided_filter_u8(joint, src, int(sigma_space), sigma_color), full passes.  A
                   one-channel list of device tensors of more than one shape is packed (packs of
                   filter_reflectance.guided_ragged_packs) and, for the pairs with int(sigma_space)
                   in 1..128, filtered by one ragged call per pack and distinct pair
                   (ops.guided_filter_ragged_sweep_u8 per pack and radius; equal pairs are computed
                   once; the same bytes).  Any other list, and any other pair, batches the images of equal
                   shapes wherever they stand in the list.
    Each result equals whdr_batch on the filtered bytes as float32 / 255 (planar), bit for bit.

    values: a value table (value_table: "linear", "srgb" or a float32[256] array).  The filters see the
    bytes as ever; every pass is then scored by whdr_points_values_u8, each filtered byte counting as
    values[byte] - a stored result that is sRGB-coded.  None scores through whdr_points_u8."""
    from . import filter_reflectance as fr
    from .batch import group_by_shape
    import torch
    pairs = np.asarray(sigma_pairs, dtype=np.float64).reshape(-1, 2)
    if pairs.shape[0] == 0:
        raise ValueError("sigma_pairs is empty")
    for sc, ss in pairs:
        fr._check_params(filter_type, sc, ss)
    iterations = int(iterations)
    if iterations < 1:
        raise ValueError("iterations must be >= 1")
    chain = iterations > 1
    # the linear path makes its calls without the keyword
    coded = {} if values is None else {"values": value_table(values)}
    if torch.is_tensor(src):
        if not torch.is_tensor(joint) or src.dim() != 4:
            raise ValueError("src and joint must both be CUDA batches [N,H,W,C] or both lists")
        if len(comparisons_px) != src.shape[0]:
            raise ValueError("one comparison array per image")
        _ffi.require_gpu()
        if chain:
            return _chain_batch(filter_type, src, joint, comparisons_px, pairs, iterations, delta,
                                grey_as_bgr, **coded)
        return _sweep_batch(filter_type, src, joint, comparisons_px, pairs, delta, grey_as_bgr, **coded)
    src, joint = list(src), list(joint)
    if len(src) != len(joint) or len(src) != len(comparisons_px):
        raise ValueError("src, joint and comparisons_px must have one entry per image")
    # points are deduplicated and checked with each image's own size, before any device work
    dedup = [dedup_points([comp], img.shape[0], img.shape[1])
             for img, comp in zip(src, comparisons_px)]
    for s_img, j_img in zip(src, joint):
        if tuple(s_img.shape[:2]) != tuple(j_img.shape[:2]):
            raise ValueError("src and joint images must have the same size")
    _ffi.require_gpu()

    # [K, P, N] throughout; a single pass hands back its only slice
    out = np.zeros((iterations, pairs.shape[0], len(src)), dtype=np.float64)

    def key(i):   # (H, W, src channels, joint channels): equal keys batch together
        s_shape, j_shape = tuple(src[i].shape), tuple(joint[i].shape)
        return s_shape[:2] + ((s_shape + (1,))[2], (j_shape + (1,))[2])

    if filter_type == "bilateral":
        keys = [key(i)[2:] for i in range(len(src))]
        sizes = [key(i)[:2] for i in range(len(src))]
        packs = plan_packs(keys, [h * w for h, w in sizes], [int(d[1][-1]) for d in dedup],
                           pairs.shape[0], lambda k: k[0])
        for pack in packs:
            psizes = [sizes[i] for i in pack]
            pdedup = join_dedup([dedup[i] for i in pack])
            if pdedup[2].shape[0] == 0:
                continue
            s_p = _pack_list([src[i] for i in pack], torch)
            j_p = s_p if all(joint[i] is src[i] for i in pack) else \
                _pack_list([joint[i] for i in pack], torch)
            out[:, :, pack] = chain_packed(s_p, j_p, psizes, pdedup, pairs, iterations, delta,
                                           grey_as_bgr, **coded) if chain else \
                sweep_packed(s_p, j_p, psizes, pdedup, pairs, delta, grey_as_bgr, **coded)[None]
        return out if chain else out[0]
    # guided, a one-channel device list of more than one shape (the conditions of
    # filter_reflectance.apply_filter_list's ragged route): the pairs whose radius the ragged guided
    # filter takes run pack by pack, one ragged call per pack and distinct pair
    keys = [key(i) for i in range(len(src))]
    rows = [p for p, (_, ss) in enumerate(pairs) if 1 <= int(ss) <= fr.GF_RAGGED_MAX_RADIUS]
    if (rows and len(set(k[:2] for k in keys)) > 1 and all(k[2] == 1 for k in keys)
            and len(set(k[3] for k in keys)) == 1
            and all(getattr(t, "is_cuda", False) for t in src + joint)):
        from . import ops
        sizes = [k[:2] for k in keys]
        cap = ops.gf_workspace_cap(src[0].device, torch)
        for pack in fr.guided_ragged_packs(sizes, fr.GF_RAGGED_MAX_BYTES, cap):
            pdedup = join_dedup([dedup[i] for i in pack])
            if pdedup[2].shape[0] == 0:
                continue
            s_p = _pack_list([src[i] for i in pack], torch)
            j_p = s_p if all(joint[i] is src[i] for i in pack) else \
                _pack_list([joint[i] for i in pack], torch)
            psizes = [sizes[i] for i in pack]
            out[(slice(None),) + np.ix_(rows, pack)] = \
                chain_guided_packed(s_p, j_p, psizes, pdedup, pairs[rows], iterations, delta,
                                    grey_as_bgr, **coded) if chain else \
                sweep_guided_packed(s_p, j_p, psizes, pdedup, pairs[rows], delta, grey_as_bgr,
                                    **coded)[None]
        rest = [p for p in range(pairs.shape[0]) if p not in rows]
        if not rest:
            return out if chain else out[0]
    else:
        rest = list(range(pairs.shape[0]))
    # everything else: equal shapes per pass, grouped wherever they stand in the list
    # (1 GiB runs: the guided half addresses a run's pixels with int32 offsets)
    order = sorted(range(len(src)), key=key)
    for run in group_by_shape(order, key, max_bytes=1 << 30):
        s_b = _stack([src[i] for i in run])
        j_b = _stack([joint[i] for i in run])
        if s_b.shape[:3] != j_b.shape[:3]:
            raise ValueError("src and joint images must have the same size")
        run_comps = [comparisons_px[i] for i in run]
        out[(slice(None),) + np.ix_(rest, run)] = \
            _chain_batch(filter_type, s_b, j_b, run_comps, pairs[rest], iterations, delta,
                         grey_as_bgr, **coded) if chain else \
            _sweep_batch(filter_type, s_b, j_b, run_comps, pairs[rest], delta, grey_as_bgr,
                         **coded)[None]
    return out if chain else out[0]


def score_list(images, comparisons_px, coding="linear", delta=0.1):
    """WHDR of stored uint8 results as they are, no filter applied: float64 [N] on the host, the
    baseline row of a sweep.  images: N uint8 images (CUDA tensors or numpy arrays, [H,W] or [H,W,C]
    with C of 1 or 3, taken as given) that may differ in size; comparisons_px: N arrays [n_i,6] in
    pixel coordinates.  coding: what a byte stands for (value_table).  Points are deduplicated and
    checked with each image's own size and the images packed by channel count as `sweep` packs a
    list; a pack is scored with its packed pixels as the point lists.  An image without judgements
    scores 0.0.  Each value equals host `whdr` on the float32 image values[bytes] (planar)."""
    import torch
    values = None if isinstance(coding, str) and coding == "linear" else value_table(coding)
    images = list(images)
    if len(images) != len(comparisons_px):
        raise ValueError("images and comparisons_px must have one entry per image")
    shapes = [tuple(im.shape) for im in images]
    for i, (im, shape) in enumerate(zip(images, shapes)):
        is_u8 = im.dtype == torch.uint8 if torch.is_tensor(im) else np.asarray(im).dtype == np.uint8
        if not is_u8 or len(shape) not in (2, 3):
            raise ValueError("image %d is not a uint8 image [H,W] or [H,W,C]" % i)
        if (shape + (1,))[2] not in (1, 3):
            raise Exception("Expecting 1 or 3 channels to compute lightness!")
    dedup = [dedup_points([comp], shape[0], shape[1]) for comp, shape in zip(comparisons_px, shapes)]
    out = np.zeros(len(images), dtype=np.float64)
    if not images:
        return out
    _ffi.require_gpu()
    keys = [(shape + (1,))[2] for shape in shapes]
    sizes = [shape[:2] for shape in shapes]
    for pack in plan_packs(keys, [h * w for h, w in sizes], [int(d[1][-1]) for d in dedup], 1,
                           lambda k: k):
        pdedup = join_dedup([dedup[i] for i in pack])
        if pdedup[2].shape[0] == 0:
            continue
        psizes = [sizes[i] for i in pack]
        packed = _pack_list([images[i] for i in pack], torch)
        image_offsets, pixels = _point_pixels(pdedup, psizes)
        out[pack] = _score(packed.view(1, -1, packed.shape[-1]), image_offsets,
                           _pixel_comps(pdedup, pixels), pdedup[3], pdedup[4], delta, values)[0]
    return out
