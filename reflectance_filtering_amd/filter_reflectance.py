#!/usr/bin/env python
"""Reflectance filtering: joint-bilateral / guided filter of a reflectance estimate.

Same operator API and command line as the reference's ``filter_reflectance.py``
(/root/reference/filter_reflectance.py:49-139); the two OpenCV-ximgproc calls are served by
hand-written HIP kernels on the MI355X (``reflectance_filtering_amd.ximgproc``).

    python filter_reflectance.py --filter_type=bilateral --sigma_color=20 --sigma_spatial=22 \
        --filename_in=x-r.png --guidance_in=x.png --path_out=out/
"""
from __future__ import division, print_function

import argparse
import os
import sys

from . import image_utils as iu
from . import _ffi, ops, ximgproc

FILTER_TYPES = ("bilateral", "guided")

PARAMETER_HINTS = (
    # CNN prediction filtered with itself as guidance
    "--filter_type=bilateral --sigma_color=20 --sigma_spatial=22",
    "--filter_type=guided --sigma_color=7 --sigma_spatial=52",
    # CNN prediction filtered with an L1-flattened image ('flat') as guidance
    "--filter_type=guided --sigma_color=3 --sigma_spatial=45",
)


def _check_params(filter_type, sigma_color, sigma_spatial):
    """Validation order of /root/reference/filter_reflectance.py:56-57,71-72: sigmas first."""
    if sigma_color <= 0 or sigma_spatial <= 0:
        raise ValueError("Parameters are expected to be positive.")
    if filter_type not in FILTER_TYPES:
        raise ValueError("filter_type must be 'bilateral' or 'guided'.")


def apply_filter(filter_type, image, joint, sigma_color, sigma_spatial):
    """Filter ``image`` (uint8 HxWx3) guided by ``joint``.

    'bilateral': jointBilateralFilter(joint, image, d=-1, sigmaColor=sigma_color,
                 sigmaSpace=sigma_spatial);
    'guided':    guidedFilter(guide=joint, src=image, radius=int(sigma_spatial), eps=sigma_color)
    -- the parameter mapping of /root/reference/filter_reflectance.py:58-70.
    """
    _check_params(filter_type, sigma_color, sigma_spatial)
    if filter_type == "bilateral":
        return ximgproc.jointBilateralFilter(joint, image, d=-1, sigmaColor=sigma_color,
                                             sigmaSpace=sigma_spatial)
    return ximgproc.guidedFilter(guide=joint, src=image, radius=int(sigma_spatial),
                                 eps=sigma_color)


def apply_filter_batch(filter_type, images, joints, sigma_color, sigma_spatial, iterations=1,
                       grey_as_bgr=False):
    """Device-resident batch form: ``images``/``joints`` are CUDA uint8 tensors [N,H,W,C];
    returns a CUDA uint8 tensor.  ``iterations`` > 1 chains the filter with the same guidance
    (the uint8 result of one pass is the input of the next), e.g. the reference's 3x GF.
    ``grey_as_bgr``: ``joints`` is [N,H,W,1] and counts as three equal channels (a grey PNG as
    cv2.imread reads it), in either filter."""
    _check_params(filter_type, sigma_color, sigma_spatial)
    if iterations < 1:
        raise ValueError("iterations must be >= 1")
    if filter_type == "guided":
        return ops.guided_filter_u8(joints, images, int(sigma_spatial), sigma_color,
                                    iterations=iterations, grey_as_bgr=grey_as_bgr)
    out = images
    for _ in range(iterations):
        out = ops.joint_bilateral_u8(joints, out, -1, sigma_color, sigma_spatial,
                                     grey_as_bgr=grey_as_bgr)
    return out


GF_RAGGED_MAX_RADIUS = 128        # the radii rf_gf_ragged_u8 runs as one launch set (kGfMaxRadiusU8)
GF_RAGGED_MAX_BYTES = 1 << 30     # src bytes of one ragged guided call (as a shape group's)


def guided_ragged_packs(sizes, max_bytes, workspace_cap):
    """Consecutive runs of a list of (h, w) one-channel images, cut so that a run's bytes stay under
    max_bytes and the workspace of its ragged guided call under workspace_cap.  The workspace is
    bounded from above without asking the library: per image its record (48 B), an item record
    (16 B) per stage-1 workgroup (at most ceil(w / 512) strips x h segments), 64-row block and
    16-column block (+ 8 of padding), the row states (32 B per 16-column block and row) and
    alpha/beta (16 B per pixel); 256 B of rounding per call."""
    packs, cur, cur_bytes, cur_ws = [], [], 0, 256
    for i, (h, w) in enumerate(sizes):
        h, w = int(h), int(w)
        nb = -(-w // 16)
        ws = 48 + 16 * (-(-w // 512) * h + -(-h // 64) + nb + 8) + 32 * nb * h + 16 * h * w
        if cur and (cur_bytes + h * w > max_bytes or cur_ws + ws > workspace_cap):
            packs.append(cur)
            cur, cur_bytes, cur_ws = [], 0, 256
        cur.append(i)
        cur_bytes += h * w
        cur_ws += ws
    if cur:
        packs.append(cur)
    return packs


def _stack(images):
    import torch
    return torch.stack(list(images))


def apply_filter_list(filter_type, images, joints, sigma_color, sigma_spatial, iterations=1,
                      grey_as_bgr=False):
    """apply_filter_batch for images of different sizes: ``images``/``joints`` are lists of CUDA
    uint8 tensors [H_i,W_i,C] (equal C within a list, image i of both of one size); returns the
    list of filtered images in the caller's order, each byte for byte what apply_filter_batch
    makes of that image alone.  'bilateral' packs the list and runs it as one ragged call per
    pass (ops.joint_bilateral_ragged_u8), the passes of ``iterations`` > 1 ping-ponging between
    two packed buffers.  'guided' with a one-channel list of device tensors of more than one shape and
    int(sigma_spatial) in 1..128 runs one ragged call for all passes (ops.guided_filter_ragged_u8),
    a long list in packs of at most 2^30 bytes whose scratch stays under the guided filter's
    workspace cap; any other guided list runs one batch per group of equal shapes, wherever its
    members stand in the list."""
    _check_params(filter_type, sigma_color, sigma_spatial)
    if iterations < 1:
        raise ValueError("iterations must be >= 1")
    same = joints is images                  # self-guided: one list, packed once
    images = list(images)
    joints = images if same else list(joints)
    if len(images) != len(joints):
        raise ValueError("images and joints must have the same length")
    for i, (im, jt) in enumerate(zip(images, joints)):
        if tuple(im.shape[:2]) != tuple(jt.shape[:2]):
            raise ValueError("image {} and its joint differ in size".format(i))
    if not images:
        return []
    torch = _ffi.require_gpu()
    if (filter_type == "guided" and images[0].shape[2] == 1
            and 1 <= int(sigma_spatial) <= GF_RAGGED_MAX_RADIUS
            and len(set(tuple(im.shape[:2]) for im in images)) > 1
            # the ragged op packs device tensors (ops.pack_images); whatever else a caller hands in
            # stays with the stacked batches, which say what is wrong with it
            and all(getattr(t, "is_cuda", False) for t in images + joints)):
        out = []
        cap = ops.gf_workspace_cap(images[0].device, torch)
        for pack in guided_ragged_packs([im.shape[:2] for im in images], GF_RAGGED_MAX_BYTES, cap):
            srcs = [images[i] for i in pack]
            out.extend(ops.guided_filter_ragged_u8(srcs if same else [joints[i] for i in pack], srcs,
                                                   int(sigma_spatial), sigma_color,
                                                   iterations=iterations, grey_as_bgr=grey_as_bgr)[1])
        return out
    if filter_type == "guided":
        from .batch import group_by_shape
        # (a flat key: group_by_shape takes its product as the bytes of an item)
        key = lambda i: tuple(images[i].shape) + (joints[i].shape[2],)
        out = [None] * len(images)
        for run in group_by_shape(sorted(range(len(images)), key=key), key, max_bytes=1 << 30):
            res = apply_filter_batch(filter_type, _stack([images[i] for i in run]),
                                     _stack([joints[i] for i in run]), sigma_color, sigma_spatial,
                                     iterations=iterations, grey_as_bgr=grey_as_bgr)
            for i, r in zip(run, res):
                out[i] = r
        return out
    src, sizes = ops.pack_images(images, "images", torch)
    joint = src if joints is images else ops.pack_images(joints, "joints", torch)[0]
    bufs = [torch.empty_like(src) for _ in range(min(iterations, 2))]
    views = None
    for it in range(iterations):
        src, views = ops.joint_bilateral_ragged_u8(joint, src, -1, sigma_color, sigma_spatial,
                                                   grey_as_bgr=grey_as_bgr, sizes=sizes,
                                                   out=bufs[it % 2])
    return views


def output_filename(filename_in, path_out, filter_type, sigma_color, sigma_spatial):
    """<path_out>/<basename>_<type>_c<sigma_color>s<sigma_spatial>.png with the parameters
    formatted by str.format (floats keep their '.0'): /root/reference/filter_reflectance.py:81-93."""
    basename = os.path.splitext(os.path.basename(filename_in))[0]
    suffix = "_{}_c{}s{}".format(filter_type, sigma_color, sigma_spatial)
    return os.path.join(path_out, basename + suffix + ".png")


def read_filter_write(filter_type, filename_in, guidance_in, sigma_color, sigma_spatial,
                      path_out):
    """Read the image and its guidance, filter, write the PNG, return the filtered image."""
    image = iu.imread(filename_in)
    joint = iu.imread(guidance_in)
    filtered = apply_filter(filter_type, image, joint, sigma_color, sigma_spatial)
    iu.imwrite(output_filename(filename_in, path_out, filter_type, sigma_color, sigma_spatial),
               filtered)
    return filtered


def build_parser():
    parser = argparse.ArgumentParser(
        description="Filter a reflectance prediction with a joint bilateral or guided filter "
                    "to strengthen the piecewise-constant reflectance prior (MI355X build).")
    parser.add_argument("--filename_in", help="image to be filtered")
    parser.add_argument("--guidance_in", help="guidance (joint) image steering the filter")
    parser.add_argument("--path_out", help="existing folder that receives the result")
    parser.add_argument("--sigma_color", type=float, help="color parameter")
    parser.add_argument("--sigma_spatial", type=float, help="spatial parameter")
    parser.add_argument("--filter_type",
                        help="'guided' (guided filter) or 'bilateral' (joint bilateral filter)")
    return parser


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    parser = build_parser()
    args = parser.parse_args(argv)
    if len(argv) > 0:
        read_filter_write(args.filter_type, args.filename_in, args.guidance_in,
                          args.sigma_color, args.sigma_spatial, args.path_out)
    else:
        parser.print_help()
        print("If you do not have any idea what parameters to choose, "
              "try one of the following combinations:")
        for hint in PARAMETER_HINTS:
            print(hint)
    return 0


if __name__ == "__main__":
    sys.exit(main())
