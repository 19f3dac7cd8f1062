"""Fine-tune the shipped 1x1 reflectance CNN on the WHDR hinge loss at judgement points.

The reference trains the network in Caffe on whole 256x256 images with a Python loss layer
(training/layers/whdr_hinge_loss_layer.py of the reference).  Every layer of the network is a 1x1
convolution with pad 0 and the loss reads the reflectance at judgement points only, so a forward and
backward pass over the de-duplicated points of a photo IS that gradient.  Per
step:

    r      = ops.cnn_reflectance_f32 at the packed points        (the forward pass `decompose` runs)
    loss   = rf_train_whdr_hinge_points_f32 -> per-image losses, d loss / d r
    grad_w = rf_train_cnn_points_backward_f32
    w      = SGD with momentum, or Adam, in plain torch on the 4,513 floats

    python -m reflectance_filtering_amd.train --inputs 'iiw/*.png' --split train --report_split val \
        --iterations 2000 --batch_size 10 --base_lr 1e-3 --out weights.caffemodel --log train.json

`--comparisons augmented` trains on the transitive hull of every photo's judgements (augment.py, the
reference's --comparisonsType augmented) and, like the reference's layer, evaluates a random
`--max_evaluated` (1,500) of an image's comparisons per step; the true WHDR is still that of the
original judgements.

`--RS_est_mode rRelMean` (or rRelMax, rRelY, rRelNorm) trains the network's output as the factor of
image / norm(image), the reference's colour modes, with both of its boundary losses (reflectance and
shading inside [0, 1]).  Those are means over EVERY pixel, so the step is dense:

    e      = ops.cnn_reflectance_f32 over all pixels of the minibatch (pack_dense)
    L      = rf_recover_forward_f32 at the judgement points -> the hinge entry as above
    grad_e = rf_recover_boundary_backward_f32 over all pixels, then rf_recover_hinge_scatter_f32
    grad_w = rf_train_cnn_points_backward_f32 over all pixels

Single process, single GPU.  There is no CPU fallback.
"""
from __future__ import division, print_function

import argparse
import json
import math
import sys

import numpy as np

from . import _ffi, _ffi_recover, _ffi_train
from . import whdr as whdr_mod

SOLVERS = ("sgd", "adam")
DENSE_COMPARISONS = 300     # whdr_hinge_loss_layer.py:136: above this an image is "densely annotated"
MAX_EVALUATED_COMPARISONS = 1500    # whdr_hinge_loss_layer.py: a random subsample above this many
COMPARISON_TYPES = ("comparisons", "augmented")
RS_MODES = ("rDirectly", "rRelMean", "rRelMax", "rRelY", "rRelNorm")    # networks.py: the one-channel r modes
BOUNDARY_PENALTIES = ("L1", "L2")


def rs_norm(rs_mode):
    """The norm code of the recover entries for an rRel* mode, None for rDirectly."""
    if rs_mode not in RS_MODES:
        raise ValueError("rs_mode must be one of %s" % ", ".join(RS_MODES))
    return None if rs_mode == "rDirectly" else _ffi_recover.NORMS[rs_mode[4:]]


def select_comparisons(comparisons, ratio=1.0, eval_dense=True):
    """The reference's choice of an image's evaluated comparisons (whdr_hinge_loss_layer.py:135-140):
    one comparison for an image with more than 300 when eval_dense is false, then the first
    ceil(ratio * count).  Its random subsample above 1,500 comparisons is drawn per step
    (subsample_weights)."""
    if not 0 < ratio <= 1:
        raise ValueError("ratio must be in (0, 1]")
    comparisons = np.asarray(comparisons, dtype=np.float64).reshape(-1, 6)
    count = comparisons.shape[0]
    if not eval_dense and count > DENSE_COMPARISONS:
        count = 1
    if ratio < 1.0:
        count = int(np.ceil(ratio * count))
    return comparisons[:count]


def point_incidence(point_offsets, comps, comp_offsets):
    """The incidence lists rf_train_whdr_hinge_points_f32 walks: (inc_offsets int32 [total+1], inc
    int32 [2m]).  inc[inc_offsets[p]:inc_offsets[p+1]] holds, for the point at absolute position p,
    its comparisons in ascending order, each as 2 * (k - comp_offsets[image]) + side (side 0: the
    point is index 1 of the comparison, side 1: index 2); a comparison whose two ends are the same
    point appears twice, side 0 first."""
    point_offsets = np.asarray(point_offsets, dtype=np.int64).ravel()
    comp_offsets = np.asarray(comp_offsets, dtype=np.int64).ravel()
    comps = np.asarray(comps, dtype=np.int64).reshape(-1, 3)
    n = comp_offsets.shape[0] - 1
    total, m = int(point_offsets[-1]), comps.shape[0]
    if n < 0 or point_offsets.shape[0] != n + 1 or comp_offsets[-1] != m:
        raise ValueError("inconsistent point / comparison arrays")
    counts = np.diff(comp_offsets)
    image = np.repeat(np.arange(n), counts)
    local = np.arange(m) - comp_offsets[image]
    size = (point_offsets[1:] - point_offsets[:-1])[image]
    if m and (comps[:, :2].min() < 0 or (comps[:, :2] >= size[:, None]).any()):
        raise IndexError("comparison index outside the points of its image")
    ends = (point_offsets[image][:, None] + comps[:, :2]).reshape(-1)         # k0s0 k0s1 k1s0 ...
    entries = (2 * local[:, None] + np.arange(2)[None, :]).reshape(-1)
    order = np.argsort(ends, kind="stable")
    inc_offsets = np.concatenate([[0], np.cumsum(np.bincount(ends, minlength=total))])
    if 2 * m >= 2 ** 31:
        raise ValueError("too many comparisons")
    return inc_offsets.astype(np.int32), entries[order].astype(np.int32)


class Packed(object):
    """What pack() returns: the host arrays (numpy), their device copies (d_*), the network inputs
    at the points (x, CUDA float32 [total, 3], B G R) and per-call scratch."""


def _device_array(torch, dev, array):
    """A host array on the device, never of zero length (the entries refuse NULL pointers)."""
    array = np.ascontiguousarray(array)
    if array.size == 0:
        array = np.zeros((1,) + array.shape[1:], dtype=array.dtype)
    return torch.from_numpy(array).to(dev)


def _inputs_at(image, xs, ys, lut):
    """float32 [k,3] (B, G, R) network inputs of pixels (xs, ys) of one image: uint8 sRGB photos go
    through the table of the CNN entry, float32 images are linear already."""
    if hasattr(image, "is_cuda"):
        image = image.cpu().numpy()
    image = np.asarray(image)
    if image.ndim != 3 or image.shape[2] != 3:
        raise ValueError("an image must be [H,W,3]")
    picked = image[ys, xs, :]
    if image.dtype == np.uint8:
        return lut[picked]
    if image.dtype == np.float32:
        return picked
    raise ValueError("an image must be uint8 (sRGB) or float32 (linear)")


def pack(images, comparisons_px, order_seed=None, ratio=1.0, eval_dense=True, device=None,
         hinge_comparisons_px=None):
    """The training set on the device.  images: [H,W,3] BGR arrays, uint8 sRGB or float32 linear, of
    any sizes; comparisons_px: per image float [m,6] judgements in pixel coordinates
    (whdr.to_pixels).  The image order is shuffled once (order_seed; None keeps it), the
    comparisons are selected (select_comparisons), de-duplicated (whdr.dedup_points) and given
    incidence lists, and the network inputs at the points are gathered into one [total,3] buffer:
    they never change during training.
    hinge_comparisons_px: a second comparison set per image (the augmented one), same format.  When
    given, the hinge arrays (comps, weights, comp_offsets, the incidence lists) come from IT, selected
    as the reference applies ratio / eval_dense to its `augmented` blob, the true WHDR of evaluate()
    comes from ALL of comparisons_px (whdr_comps, whdr_weights, whdr_comp_offsets), and the points are
    the de-duplicated union of both sets.  Without it nothing changes: whdr_* are the hinge arrays."""
    torch = _ffi.require_gpu()
    from . import image_utils as iu
    if len(images) != len(comparisons_px):
        raise ValueError("one comparison array per image")
    n = len(images)
    order = (np.arange(n) if order_seed is None
             else np.random.RandomState(order_seed).permutation(n))
    images = [images[i] for i in order]
    comps_px = [select_comparisons(comparisons_px[i], ratio, eval_dense) for i in order]
    sizes = [tuple(int(v) for v in im.shape[:2]) for im in images]
    if hinge_comparisons_px is None:
        points, point_offsets, comps, weights, comp_offsets = whdr_mod.dedup_points_ragged(comps_px, sizes)
        whdr_px, whdr_arrays = comps_px, (comps, weights, comp_offsets)
    else:
        if len(hinge_comparisons_px) != n:
            raise ValueError("one second comparison array per image")
        whdr_px = [np.asarray(comparisons_px[i], dtype=np.float64).reshape(-1, 6) for i in order]
        comps_px = [select_comparisons(hinge_comparisons_px[i], ratio, eval_dense) for i in order]
        points, point_offsets, both, both_w, both_off = whdr_mod.dedup_points_ragged(
            [np.concatenate([h, o], axis=0) for h, o in zip(comps_px, whdr_px)], sizes)
        parts = [[], []]        # per image the first rows are the hinge set, the rest the judgements
        for i in range(n):
            cut = both_off[i] + comps_px[i].shape[0]
            parts[0].append(slice(both_off[i], cut))
            parts[1].append(slice(cut, both_off[i + 1]))
        split = []
        for rows in parts:
            offsets = np.concatenate([[0], np.cumsum([r.stop - r.start for r in rows])]).astype(np.int32)
            split.append((np.concatenate([both[r] for r in rows] + [both[:0]], axis=0),
                          np.concatenate([both_w[r] for r in rows] + [both_w[:0]], axis=0), offsets))
        (comps, weights, comp_offsets), whdr_arrays = split
    if (comps.shape[0] and ((comps[:, 2] < 0) | (comps[:, 2] > 2)).any()):
        raise ValueError("darker is neither 0 (=E), 1, 2")
    inc_offsets, inc = point_incidence(point_offsets, comps, comp_offsets)
    lut = iu.srgb_byte_lut()
    x = np.zeros((points.shape[0], 3), dtype=np.float32)
    for i, image in enumerate(images):
        p0, p1 = point_offsets[i], point_offsets[i + 1]
        if p1 > p0:
            x[p0:p1] = _inputs_at(image, points[p0:p1, 0], points[p0:p1, 1], lut)
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    packed = Packed()
    packed.n, packed.total, packed.order, packed.sizes = n, int(points.shape[0]), order, sizes
    packed.comparisons_px, packed.whdr_comparisons_px = comps_px, whdr_px
    packed.whdr_comps, packed.whdr_weights, packed.whdr_comp_offsets = whdr_arrays
    packed.points, packed.point_offsets, packed.comps = points, point_offsets, comps
    packed.weights, packed.comp_offsets = weights, comp_offsets
    packed.inc_offsets, packed.inc = inc_offsets, inc
    packed.x = _device_array(torch, dev, x)
    packed.d_point_offsets = _device_array(torch, dev, point_offsets)
    packed.d_comps = _device_array(torch, dev, comps)
    packed.d_weights = _device_array(torch, dev, weights)
    packed.d_comp_offsets = _device_array(torch, dev, comp_offsets)
    packed.d_inc_offsets = _device_array(torch, dev, inc_offsets)
    packed.d_inc = _device_array(torch, dev, inc)
    packed.r = torch.zeros(max(packed.total, 1), dtype=torch.float32, device=dev)
    packed.grad_r = torch.zeros(max(packed.total, 1), dtype=torch.float32, device=dev)
    packed.workspace = None
    return packed


def check_distinct_pixels(point_pixel):
    """rf_recover_hinge_scatter_f32 adds into grad_e at the listed pixels without atomics: two equal
    indices would race, so a list with a repeated pixel is refused here."""
    point_pixel = np.asarray(point_pixel, dtype=np.int64).ravel()
    if np.unique(point_pixel).size != point_pixel.size:
        raise ValueError("the packed points are not pairwise distinct pixels")
    return point_pixel


def pack_dense(images, comparisons_px, order_seed=None, ratio=1.0, eval_dense=True, device=None,
               hinge_comparisons_px=None):
    """pack() for the dense modes (rRel*): the same Packed plus
        x_dense        CUDA float32 [T,3] (B, G, R): every pixel of every image in packed order,
                       row-major, through the same sRGB table as x
        pixel_offsets  int64 [n+1] (host): image i owns the pixels [pixel_offsets[i], pixel_offsets[i+1])
        point_pixel    int64 [total] (host; d_point_pixel on the device): the absolute dense index of
                       every packed point, so that x_dense[point_pixel] is x bit for bit
    Memory: 12 bytes per pixel stay on the device for the whole training, about 2 MB per IIW photo
    (341 x 512), 2 GB for a thousand; a step adds 8 bytes per pixel of its minibatch (e and grad_e)."""
    torch = _ffi.require_gpu()
    from . import image_utils as iu
    packed = pack(images, comparisons_px, order_seed, ratio, eval_dense, device, hinge_comparisons_px)
    images = [images[i] for i in packed.order]
    dev = packed.x.device
    areas = [h * w for h, w in packed.sizes]
    pixel_offsets = np.concatenate([[0], np.cumsum(areas)]).astype(np.int64)
    image_of = np.repeat(np.arange(packed.n), np.diff(packed.point_offsets))
    widths = np.array([w for _, w in packed.sizes] + [0], dtype=np.int64)[image_of]
    points = packed.points.astype(np.int64).reshape(-1, 2)
    point_pixel = check_distinct_pixels(pixel_offsets[image_of] + points[:, 1] * widths + points[:, 0])
    lut = iu.srgb_byte_lut()
    x_dense = torch.empty((max(int(pixel_offsets[-1]), 1), 3), dtype=torch.float32, device=dev)
    for i, image in enumerate(images):      # one image on the host at a time
        if areas[i]:
            h, w = packed.sizes[i]
            ys, xs = np.divmod(np.arange(areas[i]), w)
            x_dense[pixel_offsets[i]:pixel_offsets[i + 1]] = torch.from_numpy(
                np.ascontiguousarray(_inputs_at(image, xs, ys, lut))).to(dev)
    packed.x_dense, packed.pixel_offsets, packed.point_pixel = x_dense, pixel_offsets, point_pixel
    packed.pixels = int(pixel_offsets[-1])
    packed.d_point_pixel = _device_array(torch, dev, point_pixel)
    packed.recover_workspace = None
    return packed


def _host_weights(weights):
    if hasattr(weights, "is_cuda"):
        weights = weights.detach().cpu().numpy()
    weights = np.ascontiguousarray(weights, dtype=np.float32).ravel()
    if weights.size != _ffi.CNN_NPARAMS:
        raise ValueError("weights must hold %d floats" % _ffi.CNN_NPARAMS)
    return weights


def _run(packed, first, count):
    if not (0 <= first and 0 <= count and first + count <= packed.n):
        raise ValueError("images [%d, %d) are outside the %d packed ones" % (first, first + count,
                                                                             packed.n))
    return int(packed.point_offsets[first]), int(packed.point_offsets[first + count])


def forward(weights, packed, first, count):
    """r at the points of images [first, first + count), written into packed.r at their absolute
    positions by the forward pass every other part of the package runs (ops.cnn_reflectance_f32)."""
    from . import ops
    p0, p1 = _run(packed, first, count)
    if p1 > p0:
        r, _ = ops.cnn_reflectance_f32(packed.x[p0:p1].view(1, 1, p1 - p0, 3), layout="nhwc_bgr",
                                       weights=_host_weights(weights), want_u8=False)
        packed.r[p0:p1] = r.view(-1)
    return packed.r[p0:p1]


def subsample_weights(packed, first, count, max_evaluated, generator):
    """The reference layer's random subsample (whdr_hinge_loss_layer.py, MAX_EVALUATED_COMPARISONS): a
    copy of the packed weights (CUDA float64 [m]) in which every image of [first, first + count) with
    more than max_evaluated hinge comparisons keeps max_evaluated of them, chosen without replacement
    by `generator` (a torch generator on the device), and the rest have weight 0 - exact zeros in the
    entry's loss, weight sum and gradient, which leaves the reference's arithmetic on the chosen ones.
    None where nothing is to be dropped (max_evaluated 0 = all): no draw is made then."""
    torch = _ffi.require_gpu()
    _run(packed, first, count)
    if not max_evaluated:
        return None
    sizes = np.diff(packed.comp_offsets[first:first + count + 1].astype(np.int64))
    if not (sizes > max_evaluated).any():
        return None
    weights = packed.d_weights.clone()
    for i in np.nonzero(sizes > max_evaluated)[0]:
        k0 = int(packed.comp_offsets[first + i])
        order = torch.randperm(int(sizes[i]), generator=generator, device=weights.device)
        weights[k0 + order[int(max_evaluated):]] = 0
    return weights


def hinge(packed, first, count, delta, margin, weights=None):
    """rf_train_whdr_hinge_points_f32 on packed.r for images [first, first + count): the per-image
    losses (CUDA float64 [count]); d mean-loss / d r is left in packed.grad_r.  weights: this call's
    weight array (subsample_weights) in place of the packed one."""
    torch = _ffi.require_gpu()
    lib = _ffi_train.load_library()
    _run(packed, first, count)
    losses = torch.zeros(max(count, 1), dtype=torch.float64, device=packed.x.device)
    rc = lib.rf_train_whdr_hinge_points_f32(
        packed.r.data_ptr(), packed.d_point_offsets.data_ptr() + 4 * first,
        packed.d_comps.data_ptr(), (packed.d_weights if weights is None else weights).data_ptr(),
        packed.d_comp_offsets.data_ptr() + 4 * first, packed.d_inc_offsets.data_ptr(),
        packed.d_inc.data_ptr(), int(count), float(delta), float(margin), losses.data_ptr(),
        packed.grad_r.data_ptr(), _ffi.current_stream_ptr(torch))
    _ffi_train.check(rc, "rf_train_whdr_hinge_points_f32")
    return losses[:count]


def backward(weights, packed, first, count):
    """rf_train_cnn_points_backward_f32 with packed.grad_r at the points of images [first, first +
    count): grad_w, CUDA float32 [4513]."""
    p0, p1 = _run(packed, first, count)
    return _backward_at(weights, packed, packed.x[p0:p1], packed.grad_r[p0:p1])


def _backward_at(weights, packed, x, grad):
    """The backward entry over the rows of x [P,3] with d loss / d output in grad [P]."""
    torch = _ffi.require_gpu()
    lib = _ffi_train.load_library()
    p0, p1 = 0, int(grad.shape[0])
    dev = packed.x.device
    grad_w = torch.zeros(_ffi.CNN_NPARAMS, dtype=torch.float32, device=dev)
    if p1 == p0:
        return grad_w
    if not (hasattr(weights, "is_cuda") and weights.is_cuda and weights.dtype == torch.float32
            and weights.is_contiguous() and weights.numel() == _ffi.CNN_NPARAMS):
        weights = torch.from_numpy(_host_weights(weights)).to(dev)
    need = _ffi_train.cnn_points_workspace_bytes(p1 - p0)
    if packed.workspace is None or packed.workspace.numel() < need:
        packed.workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    rc = lib.rf_train_cnn_points_backward_f32(
        x.data_ptr(), weights.data_ptr(), grad.data_ptr(), p1 - p0, grad_w.data_ptr(),
        packed.workspace.data_ptr(), packed.workspace.numel(), _ffi.current_stream_ptr(torch))
    _ffi_train.check(rc, "rf_train_cnn_points_backward_f32")
    return grad_w


def _dense_run(packed, first, count):
    if not hasattr(packed, "x_dense"):
        raise ValueError("the rRel* modes need every pixel: pack with pack_dense()")
    _run(packed, first, count)
    return int(packed.pixel_offsets[first]), int(packed.pixel_offsets[first + count])


def forward_dense(weights, packed, first, count):
    """The network's output e at every pixel of images [first, first + count): (x of the run [Q,3],
    e CUDA float32 [Q]), by the forward pass every other part of the package runs."""
    from . import ops
    q0, q1 = _dense_run(packed, first, count)
    x = packed.x_dense[q0:q1]
    e, _ = ops.cnn_reflectance_f32(x.view(1, 1, q1 - q0, 3), layout="nhwc_bgr",
                                   weights=_host_weights(weights), want_u8=False)
    return x, e.view(-1)


def recover_points(x, e, pixel, norm, lightness):
    """rf_recover_forward_f32: the recovered lightness at the listed pixels (CUDA int64, or None =
    all rows of x in order) of x [P,3] / e [P], written into `lightness`."""
    torch = _ffi.require_gpu()
    lib = _ffi_recover.load_library()
    listed = int(e.shape[0] if pixel is None else pixel.shape[0])
    rc = lib.rf_recover_forward_f32(x.data_ptr(), e.data_ptr(), int(e.shape[0]),
                                    None if pixel is None else pixel.data_ptr(), listed, int(norm),
                                    lightness.data_ptr(), None, None, _ffi.current_stream_ptr(torch))
    _ffi_recover.check(rc, "rf_recover_forward_f32")
    return lightness


def boundary(packed, x, e, norm, penalty, scale_reflectance, scale_shading):
    """rf_recover_boundary_backward_f32 over all rows of x / e: (the unscaled means of the reflectance
    and the shading boundary loss, CUDA float64 [2]; grad_e CUDA float32 [Q], the scaled losses'
    gradient)."""
    torch = _ffi.require_gpu()
    lib = _ffi_recover.load_library()
    npixels, dev = int(e.shape[0]), x.device
    means = torch.zeros(2, dtype=torch.float64, device=dev)
    grad_e = torch.empty(max(npixels, 1), dtype=torch.float32, device=dev)
    need = _ffi_recover.boundary_workspace_bytes(npixels)
    if packed.recover_workspace is None or packed.recover_workspace.numel() < need:
        packed.recover_workspace = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    rc = lib.rf_recover_boundary_backward_f32(
        x.data_ptr(), e.data_ptr(), npixels, int(norm), _ffi_recover.PENALTIES[penalty],
        float(scale_reflectance), float(scale_shading), means.data_ptr(), grad_e.data_ptr(),
        packed.recover_workspace.data_ptr(), packed.recover_workspace.numel(),
        _ffi.current_stream_ptr(torch))
    _ffi_recover.check(rc, "rf_recover_boundary_backward_f32")
    return means, grad_e[:npixels]


def hinge_scatter(x, e, grad_l, pixel, norm, scale, grad_e):
    """rf_recover_hinge_scatter_f32: scale * d hinge / d e added into grad_e at the listed pixels."""
    torch = _ffi.require_gpu()
    lib = _ffi_recover.load_library()
    rc = lib.rf_recover_hinge_scatter_f32(x.data_ptr(), e.data_ptr(), grad_l.data_ptr(),
                                          pixel.data_ptr(), int(pixel.shape[0]), int(e.shape[0]),
                                          int(norm), float(scale), grad_e.data_ptr(),
                                          _ffi.current_stream_ptr(torch))
    _ffi_recover.check(rc, "rf_recover_hinge_scatter_f32")
    return grad_e


def _loss_and_grad_dense(weights, packed, first, count, delta, margin, hinge_weights, norm,
                         loss_scale_whdr, loss_scale_boundaries, boundary_penalty):
    if boundary_penalty not in BOUNDARY_PENALTIES:
        raise ValueError("boundary_penalty must be L1 or L2")
    p0, p1 = _run(packed, first, count)
    q0, q1 = _dense_run(packed, first, count)
    if q1 == q0:        # no pixels: nothing to average over
        torch = _ffi.require_gpu()
        parts = {"hinge": 0.0, "boundary_reflectance": 0.0, "boundary_shading": 0.0}
        return 0.0, np.zeros(count), torch.zeros(_ffi.CNN_NPARAMS, dtype=torch.float32,
                                                 device=packed.x.device), parts
    x, e = forward_dense(weights, packed, first, count)
    pixel = (packed.d_point_pixel[p0:p1] - int(packed.pixel_offsets[first])).contiguous()
    if p1 > p0:
        recover_points(x, e, pixel, norm, packed.r[p0:p1])
    losses = hinge(packed, first, count, delta, margin, hinge_weights)
    means, grad_e = boundary(packed, x, e, norm, boundary_penalty, loss_scale_boundaries,
                             loss_scale_boundaries)
    if p1 > p0:
        hinge_scatter(x, e, packed.grad_r[p0:p1], pixel, norm, loss_scale_whdr, grad_e)
    grad_w = _backward_at(weights, packed, x, grad_e)
    per_image = losses.cpu().numpy()
    b_refl, b_shad = (float(v) for v in means.cpu().numpy())
    parts = {"hinge": float(per_image.mean()) if count else 0.0, "boundary_reflectance": b_refl,
             "boundary_shading": b_shad}
    loss = loss_scale_whdr * parts["hinge"] + loss_scale_boundaries * (b_refl + b_shad)
    return loss, per_image, grad_w, parts


def loss_and_grad(weights, packed, first, count, delta=0.1, margin=0.0, hinge_weights=None,
                  rs_mode="rDirectly", loss_scale_whdr=1.0, loss_scale_boundaries=0.1,
                  boundary_penalty="L1"):
    """(loss, per-image losses float64 [count] (host), grad_w CUDA float32 [4513]) of the mean hinge
    loss over the packed images [first, first + count) - a minibatch is a run of consecutive images
    and needs no repacking.  The loss is that of exactly the reflectance `decompose` would output
    for these weights.  hinge_weights: the comparison weights of this step (subsample_weights).
    rs_mode rRelMean / rRelMax / rRelY / rRelNorm (packed by pack_dense): the network's output is the
    factor of image / norm(image); the hinge loss reads the recovered lightness, both boundary losses
    (boundary_penalty L1 or L2) are means over every pixel of the run (count = the run's pixels, the
    reference's N H W for images of one size), and the result has a fourth element:
    loss = loss_scale_whdr * hinge + loss_scale_boundaries * (boundary_reflectance +
    boundary_shading), grad_w its gradient, and {"hinge", "boundary_reflectance",
    "boundary_shading"} the three unscaled parts.  In rDirectly the three scales are not used."""
    norm = rs_norm(rs_mode)
    if norm is not None:
        return _loss_and_grad_dense(weights, packed, first, count, delta, margin, hinge_weights, norm,
                                    float(loss_scale_whdr), float(loss_scale_boundaries),
                                    boundary_penalty)
    forward(weights, packed, first, count)
    losses = hinge(packed, first, count, delta, margin, hinge_weights)
    grad_w = backward(weights, packed, first, count)
    per_image = losses.cpu().numpy()
    return (float(per_image.mean()) if count else 0.0), per_image, grad_w


def whdr_at_points(packed, delta=0.1):
    """The true WHDR of packed.r per packed image (host, whdr.whdr: each image's points as a
    one-row image, its comparisons re-addressed into it), float64 [n].  The comparisons are the
    packed judgements: the hinge set itself unless pack() was given a second set."""
    r = packed.r.cpu().numpy()
    out = np.zeros(packed.n, dtype=np.float64)
    for i in range(packed.n):
        p0, p1 = packed.point_offsets[i], packed.point_offsets[i + 1]
        k0, k1 = packed.whdr_comp_offsets[i], packed.whdr_comp_offsets[i + 1]
        if k1 == k0:
            continue
        rows = np.zeros((k1 - k0, 6), dtype=np.float64)
        rows[:, 0], rows[:, 2] = packed.whdr_comps[k0:k1, 0], packed.whdr_comps[k0:k1, 1]
        rows[:, 4], rows[:, 5] = packed.whdr_comps[k0:k1, 2], packed.whdr_weights[k0:k1]
        out[i] = whdr_mod.whdr(r[p0:p1].reshape(1, 1, -1), rows, delta)
    return out


def evaluate(weights, packed, delta=0.1, margin=0.0, rs_mode="rDirectly"):
    """{"hinge": mean hinge loss, "whdr": mean true WHDR (threshold delta)} over all packed images.
    In an rRel* mode both are those of the recovered lightness; only the points are evaluated."""
    norm = rs_norm(rs_mode)
    if packed.n == 0:
        return {"hinge": 0.0, "whdr": 0.0}
    forward(weights, packed, 0, packed.n)
    if norm is not None and packed.total:
        recover_points(packed.x, packed.r[:packed.total].clone(), None, norm, packed.r)
    losses = hinge(packed, 0, packed.n, delta, margin).cpu().numpy()
    return {"hinge": float(losses.mean()), "whdr": float(whdr_at_points(packed, delta).mean())}


def boundary_means(weights, packed, rs_mode, boundary_penalty="L1", batch_size=10):
    """{"boundary_reflectance", "boundary_shading"}: both boundary means over every pixel of the
    packed set (pack_dense), taken in runs of batch_size images and weighted by their pixels."""
    norm = rs_norm(rs_mode)
    if norm is None:
        raise ValueError("rDirectly has no boundary loss")
    sums = np.zeros(2)
    for first, count in batch_runs(packed.n, batch_size):
        x, e = forward_dense(weights, packed, first, count)
        means, _ = boundary(packed, x, e, norm, boundary_penalty, 0.0, 0.0)
        sums += means.cpu().numpy() * int(e.shape[0])
    total = max(int(packed.pixels), 1)
    return {"boundary_reflectance": float(sums[0] / total), "boundary_shading": float(sums[1] / total)}


def batch_runs(n, batch_size, full_batch=False):
    """The minibatches as (first, count) runs of consecutive packed images."""
    if full_batch or batch_size >= n:
        return [(0, n)]
    return [(first, min(batch_size, n - first)) for first in range(0, n, batch_size)]


def fit(packed, weights=None, iterations=100, batch_size=10, base_lr=1e-3, solver="sgd",
        momentum=0.9, momentum2=0.999, adam_eps=1e-8, full_batch=False, delta=0.1, margin=0.0,
        seed=0, report_every=0, held_out=None, log=None, max_evaluated=0, rs_mode="rDirectly",
        loss_scale_whdr=1.0, loss_scale_boundaries=0.1, boundary_penalty="L1"):
    """Train for `iterations` steps.  Minibatches are runs of `batch_size` consecutive images of the
    packed order, and the order of the batches is reshuffled every epoch from `seed`; full_batch
    takes all images every step.  solver: "sgd" (v = momentum v + lr g; w -= v, Caffe's SGD) or
    "adam" (Caffe's Adam).  Every report_every steps (and after the last) the mean hinge loss and
    true WHDR of the whole training set and of `held_out` (another pack()) are recorded, over all
    their comparisons.  max_evaluated > 0: every step evaluates a random max_evaluated of the hinge
    comparisons of an image that has more (subsample_weights, drawn on the device from `seed`).
    rs_mode and the three options behind it: loss_and_grad; in an rRel* mode `packed` comes from
    pack_dense, every report adds both boundary means over the training set to its "train" entry
    (held_out needs its points only) and "batch_parts" holds the step's three unscaled parts.
    Returns (weights float32 [4513] (host), history: list of dicts)."""
    torch = _ffi.require_gpu()
    from . import weights as wmod
    if solver not in SOLVERS:
        raise ValueError("solver must be one of %s" % ", ".join(SOLVERS))
    if packed.n == 0:
        raise ValueError("no images to train on")
    if iterations < 0 or batch_size < 1:
        raise ValueError("iterations must be >= 0 and batch_size >= 1")
    dense = rs_norm(rs_mode) is not None
    if dense:
        _dense_run(packed, 0, packed.n)
    mode = {"rs_mode": rs_mode} if dense else {}
    dev = packed.x.device
    w = torch.from_numpy(_host_weights(wmod.load_weights() if weights is None else weights).copy()).to(dev)
    m1, m2 = torch.zeros_like(w), torch.zeros_like(w)
    runs = batch_runs(packed.n, batch_size, full_batch)
    history, queue, epoch = [], [], 0
    chooser = torch.Generator(device=dev)
    chooser.manual_seed(int(seed))

    def record(step, batch_loss):
        entry = {"iteration": step, "batch_loss": batch_loss,
                 "train": evaluate(w, packed, delta, margin, **mode)}
        if dense:
            entry["batch_parts"] = batch_parts
            entry["train"].update(boundary_means(w, packed, rs_mode, boundary_penalty, batch_size))
        if held_out is not None:
            entry["held_out"] = evaluate(w, held_out, delta, margin, **mode)
        history.append(entry)
        if log is not None:
            log(entry)

    batch_loss = batch_parts = None
    mode_options = dict(rs_mode=rs_mode, loss_scale_whdr=loss_scale_whdr,
                        loss_scale_boundaries=loss_scale_boundaries,
                        boundary_penalty=boundary_penalty)
    if report_every:
        record(0, None)
    for step in range(1, iterations + 1):
        if not queue:
            queue = [runs[i] for i in np.random.RandomState(seed + epoch).permutation(len(runs))]
            epoch += 1
        first, count = queue.pop(0)
        step_weights = subsample_weights(packed, first, count, max_evaluated, chooser)
        if dense:
            batch_loss, _, grad, batch_parts = loss_and_grad(w, packed, first, count, delta, margin,
                                                             step_weights, **mode_options)
        else:
            batch_loss, _, grad = loss_and_grad(w, packed, first, count, delta, margin, step_weights)
        if solver == "sgd":
            m1.mul_(momentum).add_(grad, alpha=base_lr)
            w.sub_(m1)
        else:
            m1.mul_(momentum).add_(grad, alpha=1 - momentum)
            m2.mul_(momentum2).addcmul_(grad, grad, value=1 - momentum2)
            rate = base_lr * math.sqrt(1 - momentum2 ** step) / (1 - momentum ** step)
            w.addcdiv_(m1, m2.sqrt().add_(adam_eps), value=-rate)
        if report_every and (step % report_every == 0 or step == iterations):
            record(step, batch_loss)
    return w.cpu().numpy(), history


# ---- command line -----------------------------------------------------------------------------------

def _positive(kind):
    def parse(text):
        value = kind(text)
        if not value > 0:
            raise argparse.ArgumentTypeError("must be > 0")
        return value
    return parse


def _non_negative(text):
    value = float(text)
    if not (value >= 0 and math.isfinite(value)):
        raise argparse.ArgumentTypeError("must be finite and >= 0")
    return value


def _count(text):
    value = int(text)
    if value < 0:
        raise argparse.ArgumentTypeError("must be >= 0")
    return value


def build_parser():
    from . import sweep
    p = argparse.ArgumentParser(description="Fine-tune the 1x1 reflectance CNN on the WHDR hinge loss "
                                            "at IIW judgement points (one process, one GPU).")
    p.add_argument("--inputs", nargs="+", required=True,
                   help="photos (files or glob patterns), IIW <stem>.json beside each")
    sweep.add_split_options(p)
    p.add_argument("--report_split", choices=sweep.SPLITS[1:], default=argparse.SUPPRESS, metavar="NAME",
                   help="also report hinge loss and WHDR on the photos of split NAME (held out)")
    p.add_argument("--init", default=None, metavar="CAFFEMODEL",
                   help="start from these weights (default: the shipped ones)")
    p.add_argument("--delta", type=_non_negative, default=0.1)
    p.add_argument("--margin", type=_non_negative, default=0.0)
    p.add_argument("--ratio", type=float, default=1.0, help="evaluate the first ceil(ratio * m) comparisons")
    p.add_argument("--eval_dense", type=int, choices=(0, 1), default=1,
                   help="0: one comparison for images with more than %d" % DENSE_COMPARISONS)
    p.add_argument("--comparisons", choices=COMPARISON_TYPES, default="comparisons",
                   help="augmented: the hinge loss takes the transitive hull of each photo's judgements")
    p.add_argument("--max_evaluated", type=_count, default=MAX_EVALUATED_COMPARISONS, metavar="K",
                   help="per step a random K of an image's comparisons when it has more (0 = all)")
    p.add_argument("--RS_est_mode", choices=RS_MODES, default="rDirectly",
                   help="rDirectly: the output is the reflectance intensity; rRelMean / rRelMax / rRelY / "
                        "rRelNorm: it is the factor of image / norm(image) (colour reflectance and shading; "
                        "dense steps).  The reference trainer's own default is rRelMax")
    p.add_argument("--loss_scale_whdr", type=_non_negative, default=1.0,
                   help="weight of the hinge loss outside rDirectly (the reference's default: 10)")
    p.add_argument("--loss_scale_boundaries01", type=_non_negative, default=0.1,
                   help="weight of both boundary losses outside rDirectly (the reference's default: 0.1)")
    p.add_argument("--boundary_penalty", choices=BOUNDARY_PENALTIES, default="L1",
                   help="penalty on reflectance and shading outside [0, 1] (outside rDirectly)")
    p.add_argument("--solver", choices=SOLVERS, default="sgd")
    p.add_argument("--base_lr", type=_positive(float), default=1e-3)
    p.add_argument("--momentum", type=_non_negative, default=0.9)
    p.add_argument("--iterations", type=_positive(int), default=1000)
    p.add_argument("--batch_size", type=_positive(int), default=10)
    p.add_argument("--full_batch", action="store_true", help="every step takes all training images")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--report_every", type=_positive(int), default=100)
    p.add_argument("--out", default="weights.caffemodel")
    p.add_argument("--log", default="train.json")
    return p


def parse_args(argv):
    from . import sweep
    parser = build_parser()
    args = sweep.fill_defaults(parser.parse_args(argv))
    sweep.check_split(parser, args.split, args.split_scheme)
    if not 0 < args.ratio <= 1:
        parser.error("--ratio must be in (0, 1]")
    if args.report_split:
        sweep.check_split(parser, args.report_split, args.split_scheme, "--report_split")
        if args.split == "all":
            parser.error("--report_split needs a --split to train on: all holds every split")
        if args.report_split == args.split:
            parser.error("--report_split %s is the split the network is trained on" % args.split)
    return parser, args


def load_packed(photos, args, order_seed, dense=False):
    """pack() - pack_dense() when dense - of photos read by sweep.load (host decode), judgements
    scaled to each photo's size."""
    from . import sweep
    packer = pack_dense if dense else pack
    images, _, _, judgements, _ = sweep.load(photos)
    comps = [whdr_mod.to_pixels(j, im.shape[0], im.shape[1]) for j, im in zip(judgements, images)]
    if args.comparisons != "augmented":
        return packer(images, comps, order_seed, args.ratio, bool(args.eval_dense))
    from . import augment
    lists, points = augment.augment_files([sweep.judgements_for(f) for f in photos], seed=args.seed)
    hull = [whdr_mod.to_pixels(augment.to_rows(a, p), im.shape[0], im.shape[1])
            for a, p, im in zip(lists, points, images)]
    return packer(images, comps, order_seed, args.ratio, bool(args.eval_dense), hinge_comparisons_px=hull)


def main(argv=None):
    from . import sweep
    from . import weights as wmod
    from .batch import expand_inputs
    parser, args = parse_args(sys.argv[1:] if argv is None else argv)
    photos = expand_inputs(args.inputs)
    if not photos:
        raise SystemExit("no input photos")
    selected, split = sweep.select_split(photos, args.split, args.split_scheme)
    if not selected:
        raise SystemExit("no input photos in split %s" % args.split)
    held = None
    if args.report_split:
        held, _ = sweep.select_split(photos, args.report_split, args.split_scheme)
        if not held:
            parser.error("--report_split: no photo in split %s" % args.report_split)
    init = wmod.load_weights(args.init)
    dense = args.RS_est_mode != "rDirectly"
    mode = dict(rs_mode=args.RS_est_mode, loss_scale_whdr=args.loss_scale_whdr,
                loss_scale_boundaries=args.loss_scale_boundaries01,
                boundary_penalty=args.boundary_penalty) if dense else {}
    packed = load_packed(selected, args, args.seed, dense)
    held_packed = load_packed(held, args, None) if held else None

    def say(entry):
        line = "iteration %d: train hinge %.6f whdr %.4f" % (
            entry["iteration"], entry["train"]["hinge"], entry["train"]["whdr"])
        if "boundary_shading" in entry["train"]:
            line += " boundaries %.6g %.6g" % (entry["train"]["boundary_reflectance"],
                                               entry["train"]["boundary_shading"])
        if "held_out" in entry:
            line += "; %s hinge %.6f whdr %.4f" % (args.report_split, entry["held_out"]["hinge"],
                                                   entry["held_out"]["whdr"])
        print(line)

    final, history = fit(packed, init, iterations=args.iterations, batch_size=args.batch_size,
                         base_lr=args.base_lr, solver=args.solver, momentum=args.momentum,
                         full_batch=args.full_batch, delta=args.delta, margin=args.margin,
                         seed=args.seed, report_every=args.report_every, held_out=held_packed,
                         log=say, max_evaluated=args.max_evaluated, **mode)
    wmod.write_caffemodel(args.out, final)
    result = {"delta": args.delta, "margin": args.margin, "ratio": args.ratio,
              "eval_dense": args.eval_dense, "comparisons_type": args.comparisons,
              "max_evaluated": args.max_evaluated, "solver": args.solver, "base_lr": args.base_lr,
              "momentum": args.momentum, "iterations": args.iterations,
              "batch_size": args.batch_size, "full_batch": bool(args.full_batch), "seed": args.seed,
              "images": packed.n, "points": packed.total, "comparisons": int(packed.comps.shape[0]),
              "init": args.init, "out": args.out, "history": history}
    if dense:
        result.update({"RS_est_mode": args.RS_est_mode, "loss_scale_whdr": args.loss_scale_whdr,
                       "loss_scale_boundaries01": args.loss_scale_boundaries01,
                       "boundary_penalty": args.boundary_penalty, "pixels": packed.pixels})
    if split:
        result["split"] = split
    if args.report_split:
        result["report_split"] = args.report_split
    with open(args.log, "w") as fh:
        json.dump(result, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
