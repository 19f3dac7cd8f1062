#!/usr/bin/env python
"""Intrinsic decomposition with the shipped 1x1 reflectance CNN, on the MI355X.

Same functions, outputs and command line as the reference's ``decompose_with_trained_CNN.py``
(/root/reference/decompose_with_trained_CNN.py:57-148).  The Caffe net is replaced by
``ReflectanceNet``, a small object with pycaffe's surface (``blobs[name].reshape/.data``,
``forward()``) whose forward pass is the HIP kernel behind ``rf_cnn_reflectance_u8``.

Image convention on the blob side: linear RGB, channels x height x width, range 0..1.
"""
from __future__ import division, print_function

import argparse
import collections
import sys
import os

import numpy as np

from . import image_utils as iu
from . import ops, _ffi
from . import weights as _weights


def imgCV2_to_caffeBlob(img):
    """uint8 BGR HxWx3 -> float64 blob [1,3,H,W] in linear RGB
    (/root/reference/decompose_with_trained_CNN.py:57-69)."""
    rgb01 = (img / 255.0)[:, :, ::-1]
    linear = iu.srgb_to_rgb(rgb01)
    return np.transpose(linear, (2, 0, 1))[np.newaxis, :, :, :]


def caffeBlob_to_imgGrayLinear(blob):
    """[1,1,H,W] blob -> HxW image; anything else is an error
    (/root/reference/decompose_with_trained_CNN.py:72-79)."""
    b, c = blob.shape[:2]
    if b != 1 or c != 1:
        raise ValueError("Expecting to get 1 image in mini-batch having 1 channel, "
                         "but got batch size of {} and {} channels".format(b, c))
    return blob[0, 0, :, :]


class _Blob(object):
    def __init__(self, shape):
        self.data = np.zeros(shape, dtype=np.float32)

    def reshape(self, *shape):
        self.data = np.zeros(shape, dtype=np.float32)


class _NotByteLevels(ValueError):
    """_blob_to_bytes: the blob is well formed but holds values between the sRGB byte levels."""


class ReflectanceNet(object):
    """pycaffe-shaped wrapper of the HIP forward pass.

    ``blobs['images'].data`` holds the float32 linear-RGB blob [N,3,H,W] exactly as the reference
    fills it, and forward() runs whatever floats are there, as Caffe does, for any N.  When every
    blob value is ``float32(srgb_to_rgb(v/255))`` for a byte v - what imgCV2_to_caffeBlob makes of
    8-bit pixels - forward() recovers the bytes through the same 256-entry table and hands uint8
    BGR to the kernel (3 B/pixel over PCIe instead of 12).  Any other blob (linear data deeper
    than 8 bits: MIT Intrinsic, MPI Sintel, HDR, the trainer's npz and movie inputs) is uploaded
    as it is and takes the float entry (ops.cnn_reflectance_f32, layout "nchw_rgb"), which on byte
    levels computes the same bits as the byte route.
    """

    def __init__(self, caffemodel=None):
        self.weights = _weights.load_weights(caffemodel)
        self.blobs = {"images": _Blob((1, 3, 256, 256)),
                      "reflectance_intensity": _Blob((1, 1, 256, 256))}
        self._lut = iu.srgb_byte_lut()

    def _blob_to_bytes(self):
        x = self.blobs["images"].data
        if x.ndim != 4 or x.shape[1] != 3:
            raise ValueError("blob 'images' must be [N,3,H,W]")
        idx = np.searchsorted(self._lut, x)
        idx = np.clip(idx, 0, 255)
        if not np.array_equal(self._lut[idx], x):
            raise _NotByteLevels("blob 'images' does not hold sRGB byte levels; "
                                 "use get_reflectance_batch() on uint8 images instead")
        # blob is RGB, channel-first -> BGR, channel-last
        return np.ascontiguousarray(idx.astype(np.uint8).transpose(0, 2, 3, 1)[:, :, :, ::-1])

    def forward(self):
        torch = _ffi.require_gpu()
        try:                                    # (a blob that is not [N,3,H,W] stays an error)
            bgr = torch.from_numpy(self._blob_to_bytes()).cuda()
        except _NotByteLevels:
            blob = np.ascontiguousarray(self.blobs["images"].data, dtype=np.float32)
            r, _ = ops.cnn_reflectance_f32(torch.from_numpy(blob).cuda(), layout="nchw_rgb",
                                           weights=self.weights, want_u8=False)
        else:
            r, _ = ops.cnn_reflectance_u8(bgr, weights=self.weights, want_u8=False)
        self.blobs["reflectance_intensity"].data = r.cpu().numpy()[:, np.newaxis, :, :]
        return {"reflectance_intensity": self.blobs["reflectance_intensity"].data}


def get_reflectance_caffe(net, image):
    """Run one uint8 BGR image through ``net`` and return the HxW float32 reflectance
    intensity (/root/reference/decompose_with_trained_CNN.py:82-95)."""
    height, width = image.shape[:2]
    net.blobs["images"].reshape(1, 3, height, width)
    net.blobs["images"].data[...] = imgCV2_to_caffeBlob(image)
    net.forward()
    return caffeBlob_to_imgGrayLinear(net.blobs["reflectance_intensity"].data)


def _cnn_batch(images, weights, **want):
    """The network on a device batch [N,H,W,3], routed by dtype: uint8 sRGB BGR (cv2.imread) or
    float32 linear BGR."""
    dtype = str(getattr(images, "dtype", None))
    if dtype == "torch.uint8":
        return ops.cnn_reflectance_u8(images, weights=weights, **want)
    if dtype == "torch.float32":
        return ops.cnn_reflectance_f32(images, layout="nhwc_bgr", weights=weights, **want)
    raise ValueError("images must be uint8 sRGB BGR [N,H,W,3] or float32 linear BGR [N,H,W,3], "
                     "got dtype {}".format(dtype))


def get_reflectance_batch(images, weights=None):
    """Device-resident batch form: CUDA uint8 BGR [N,H,W,3] (sRGB, as cv2.imread returns it) or
    CUDA float32 BGR [N,H,W,3] (linear, 0..1: data deeper than 8 bits) -> (r float32 [N,H,W],
    r_u8 uint8 [N,H,W] = the `-r.png` bytes).  Any other dtype is a ValueError."""
    return _cnn_batch(images, weights)


def decompose_and_filter_batch(images, sigma_color=20.0, sigma_spatial=22.0, weights=None,
                               filter_type="bilateral"):
    """CNN -> filter(CNN, CNN) on the device, the reference tool's two self-guided recipes:
    'bilateral' BF(CNN, CNN) (the paper's headline pipeline, README.md:56 of the reference;
    jointBilateralFilter with d = -1) or 'guided' GF(CNN, CNN) (guidedFilter with
    radius = int(sigma_spatial), eps = sigma_color; the tool suggests sigma_color=7,
    sigma_spatial=52).  CUDA uint8 BGR [N,H,W,3] -> (r_u8 [N,H,W], filtered [N,H,W]) with
    `filtered` bit-identical to what the two CLIs produce through `<base>-r.png` (grey PNG re-read
    as 3 equal channels, filtered with itself as guidance, any channel of the result).  A float32
    linear BGR batch [N,H,W,3] is accepted as by get_reflectance_batch: the filter consumes r_u8
    and nothing else here reads the photo."""
    if filter_type not in ("bilateral", "guided"):
        raise ValueError("filter_type must be 'bilateral' or 'guided'.")
    _, r8 = _cnn_batch(images, weights, want_float=False)
    r1 = r8.unsqueeze(-1)
    if filter_type == "guided":
        out = ops.guided_filter_u8(r1, r1, int(sigma_spatial), sigma_color, grey_as_bgr=True)
    else:
        out = ops.joint_bilateral_u8(r1, r1, -1, sigma_color, sigma_spatial, grey_as_bgr=True)
    return r8, out.squeeze(-1)


def decompose_and_filter_list(images, sigma_color=20.0, sigma_spatial=22.0, weights=None,
                              filter_type="bilateral"):
    """decompose_and_filter_batch for photos of different sizes: a list of CUDA uint8 BGR tensors
    [H_i,W_i,3] -> (list of r_u8 [H_i,W_i], list of filtered [H_i,W_i]), each byte for byte what
    decompose_and_filter_batch makes of that photo alone.  The network is per pixel, so the packed
    photos go through it once as one image [1, 1, total pixels, 3]; 'bilateral' then filters the
    packed grey maps in one ragged call (ops.joint_bilateral_ragged_u8), 'guided' through
    filter_reflectance.apply_filter_list: one ragged call (ops.guided_filter_ragged_u8) for photos of
    more than one shape at int(sigma_spatial) 1..128, else one batch per group of equal shapes."""
    from . import filter_reflectance as fr
    if filter_type not in ("bilateral", "guided"):
        raise ValueError("filter_type must be 'bilateral' or 'guided'.")
    torch = _ffi.require_gpu()
    bgr, sizes = ops.pack_images(images, "images", torch)
    if bgr.shape[1] != 3:
        raise ValueError("images must have 3 channels")
    _, r8 = ops.cnn_reflectance_u8(bgr.view(1, 1, -1, 3), weights=weights, want_float=False)
    r1 = r8.view(-1, 1)
    maps = ops.split_packed(r1, sizes)
    if filter_type == "guided":
        out = fr.apply_filter_list("guided", maps, maps, sigma_color, sigma_spatial,
                                   grey_as_bgr=True)
    else:
        _, out = ops.joint_bilateral_ragged_u8(r1, r1, -1, sigma_color, sigma_spatial,
                                               grey_as_bgr=True, sizes=sizes)
    return [m.squeeze(-1) for m in maps], [o.squeeze(-1) for o in out]


def decompose_batch(images, weights=None):
    """Everything decompose_image writes, for a device-resident batch: CUDA uint8 BGR
    [N,H,W,3] -> (r float32 [N,H,W], r_u8 [N,H,W] = `-r.png`, reflectance bytes [N,H,W,3] =
    `-r_colorized.png`, shading bytes [N,H,W] = `-s_colorized.png`), no host arithmetic
    (/root/reference/decompose_with_trained_CNN.py:113-128)."""
    r, r8 = ops.cnn_reflectance_u8(images, weights=weights)
    refl, shad = ops.colorize_srgb_u8(images, r)
    return r, r8, refl, shad


def decompose_packed(images, weights=None):
    """The device work of decompose_list with the results left packed, photo after photo: a list of
    CUDA uint8 BGR tensors [H_i,W_i,3] -> (sizes int64 [n,2] (h, w), r float32 [total pixels], r_u8
    [total pixels], reflectance bytes [total pixels, 3], shading bytes [total pixels]).  One pack,
    one pass of the packed photos through the per-pixel network as one image [1, 1, total pixels, 3],
    one ragged colourise (ops.colorize_ragged_srgb_u8: percentile and `max > 1` test per photo)."""
    torch = _ffi.require_gpu()
    bgr, sizes = ops.pack_images(images, "images", torch)
    if bgr.shape[1] != 3:
        raise ValueError("images must have 3 channels")
    r, r8 = ops.cnn_reflectance_u8(bgr.view(1, 1, -1, 3), weights=weights)
    r, r8 = r.view(-1), r8.view(-1)
    refl, shad, _, _ = ops.colorize_ragged_srgb_u8(bgr, r, sizes=sizes)
    return sizes, r, r8, refl, shad


def decompose_list(images, weights=None):
    """decompose_batch for photos of different sizes: a list of CUDA uint8 BGR tensors [H_i,W_i,3] ->
    (list of r float32 [H_i,W_i], list of r_u8 [H_i,W_i], list of reflectance bytes [H_i,W_i,3], list
    of shading bytes [H_i,W_i]), each bit for bit (r) and byte for byte what decompose_batch makes of
    that photo alone; the views of one kind share one packed tensor (decompose_packed)."""
    sizes, r, r8, refl, shad = decompose_packed(images, weights=weights)
    grey = lambda t: [v.squeeze(-1) for v in ops.split_packed(t.view(-1, 1), sizes)]
    return grey(r), grey(r8), ops.split_packed(refl, sizes), grey(shad)


DecomposeFilter = collections.namedtuple(
    "DecomposeFilter", "sizes r r_u8 reflectance shading filtered filtered_reflectance filtered_shading")


def _packed_views(views, torch):
    """The packed tensor [total pixels, C] behind a list of [H_i,W_i,C] results: the views of the
    ragged operators lie one after another in one buffer, which is handed back as it is; results of
    separate batches are joined with one torch.cat (a copy, no arithmetic)."""
    c = views[0].shape[2]
    base = views[0]._base
    total = 0
    for v in views:
        if base is None or v._base is not base or v.data_ptr() != base.data_ptr() + total * c:
            return torch.cat([t.reshape(-1, c) for t in views])
        total += v.shape[0] * v.shape[1]
    if tuple(base.shape) != (total, c) or not base.is_contiguous():
        return torch.cat([t.reshape(-1, c) for t in views])
    return base


def decompose_filter_packed(images, sigma_color=20.0, sigma_spatial=22.0, filter_type="bilateral",
                            guidance=None, iterations=1, weights=None, colorize_filtered=True):
    """The paper's whole result for a list of photos, left packed photo after photo: the CNN map, its
    filtered form and the decomposition derived from each.  images: a list of CUDA uint8 BGR tensors
    [H_i,W_i,3] of any sizes.  Returns a DecomposeFilter: sizes int64 [n,2] (h, w); r float32, r_u8,
    reflectance [.., 3] and shading as decompose_packed; filtered uint8 [total pixels], the bytes
    filter_reflectance makes of `<base>-r.png`; filtered_reflectance [total pixels, 3] and
    filtered_shading [total pixels], the bytes of imwrite(colorize(float32(filtered) / 255, photo),
    sRGB=True) (None with colorize_filtered=False).
    guidance: None - the CNN map guides itself (the bytes of decompose_and_filter_list); "image" - the
    photos guide; or a list of CUDA uint8 tensors [H_i,W_i,1 or 3] of the photos' sizes, e.g. `flat`
    images (one channel stands for three equal ones).  iterations >= 1 chains the filter under the
    same guidance as apply_filter_list does.  One pack, one pass through the network, the ragged
    filter routes of apply_filter_list, one ops.colorize_ragged_srgb_u8 and one
    ops.colorize_ragged_r8_srgb_u8, which reads the filtered bytes as they are: no host arithmetic and
    no torch arithmetic on pixel values."""
    from . import filter_reflectance as fr
    fr._check_params(filter_type, sigma_color, sigma_spatial)
    if iterations < 1:
        raise ValueError("iterations must be >= 1")
    torch = _ffi.require_gpu()
    images = list(images)
    bgr, sizes = ops.pack_images(images, "images", torch)
    if bgr.shape[1] != 3:
        raise ValueError("images must have 3 channels")
    if guidance is not None and not isinstance(guidance, str):
        guidance = list(guidance)
        if len(guidance) != len(images):
            raise ValueError("guidance must hold one image per photo")
        for i, (g, (h, w)) in enumerate(zip(guidance, sizes.tolist())):
            if not torch.is_tensor(g) or g.dim() != 3 or tuple(g.shape[:2]) != (h, w):
                raise ValueError("guidance of image {} is not a tensor of its size {}x{}".format(i, h, w))
            if g.shape[2] not in (1, 3) or g.shape[2] != guidance[0].shape[2]:
                raise ValueError("guidance of image {} must have 1 or 3 channels, the same for the "
                                 "whole list".format(i))
    elif guidance not in (None, "image"):
        raise ValueError("guidance must be None, 'image' or a list of device tensors")
    r, r8 = ops.cnn_reflectance_u8(bgr.view(1, 1, -1, 3), weights=weights)
    r, r8 = r.view(-1), r8.view(-1)
    refl, shad, _, _ = ops.colorize_ragged_srgb_u8(bgr, r, sizes=sizes)
    r1 = r8.view(-1, 1)
    if guidance is None and filter_type == "bilateral":
        filtered = r1
        bufs = [torch.empty_like(r1) for _ in range(min(iterations, 2))]
        for it in range(iterations):
            filtered, _ = ops.joint_bilateral_ragged_u8(r1, filtered, -1, sigma_color, sigma_spatial,
                                                        grey_as_bgr=True, sizes=sizes, out=bufs[it % 2])
    else:
        maps = ops.split_packed(r1, sizes)
        if guidance is None:
            joints, grey = maps, True
        elif isinstance(guidance, str):
            joints, grey = images, False
        else:
            joints, grey = guidance, guidance[0].shape[2] == 1
        filtered = _packed_views(fr.apply_filter_list(filter_type, maps, joints, sigma_color, sigma_spatial,
                                                      iterations=iterations, grey_as_bgr=grey), torch)
    filtered = filtered.view(-1)
    f_refl = f_shad = None
    if colorize_filtered:
        f_refl, f_shad, _, _ = ops.colorize_ragged_r8_srgb_u8(bgr, filtered, sizes=sizes)
    return DecomposeFilter(sizes, r, r8, refl, shad, filtered, f_refl, f_shad)


def decompose_filter_list(images, sigma_color=20.0, sigma_spatial=22.0, filter_type="bilateral",
                          guidance=None, iterations=1, weights=None, colorize_filtered=True):
    """decompose_filter_packed split photo by photo: the same DecomposeFilter with a list of views
    [H_i,W_i] (reflectance and filtered_reflectance [H_i,W_i,3]) in every field but sizes; the views of
    one field share one packed tensor."""
    p = decompose_filter_packed(images, sigma_color, sigma_spatial, filter_type, guidance, iterations,
                                weights, colorize_filtered)
    grey = lambda t: None if t is None else [v.squeeze(-1) for v in ops.split_packed(t.view(-1, 1), p.sizes)]
    colour = lambda t: None if t is None else ops.split_packed(t, p.sizes)
    return DecomposeFilter(p.sizes, grey(p.r), grey(p.r_u8), colour(p.reflectance), grey(p.shading),
                           grey(p.filtered), colour(p.filtered_reflectance), grey(p.filtered_shading))


def decompose_image(filename_in, path_out, caffemodel=None):
    """Predict reflectance intensity for one image file and write `<base>-r.png`,
    `<base>-r_colorized.png`, `<base>-s_colorized.png`
    (/root/reference/decompose_with_trained_CNN.py:98-130)."""
    net = ReflectanceNet(caffemodel)
    image = iu.imread(filename_in)
    basename = os.path.splitext(os.path.basename(filename_in))[0]
    reflectance_gray = get_reflectance_caffe(net, image)
    iu.imwrite(os.path.join(path_out, basename + "-r.png"), reflectance_gray)
    reflectance, shading = iu.colorize(reflectance_gray, image)
    iu.imwrite(os.path.join(path_out, basename + "-r_colorized.png"), reflectance, sRGB=True)
    iu.imwrite(os.path.join(path_out, basename + "-s_colorized.png"), shading, sRGB=True)
    return reflectance_gray


def build_parser():
    parser = argparse.ArgumentParser(
        description="Decompose an image with the direct reflectance prediction CNN "
                    "(MI355X build).")
    parser.add_argument("--filename_in", help="image that should be decomposed")
    parser.add_argument("--path_out", help="existing folder that receives the decomposition")
    return parser


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(sys.argv[1:] if argv is None else argv)
    if args.filename_in and args.path_out:
        decompose_image(args.filename_in, args.path_out)
    else:
        parser.print_help()
    return 0


if __name__ == "__main__":
    sys.exit(main())
