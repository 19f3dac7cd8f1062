#!/usr/bin/env python
"""WHDR parameter sweep of the reflectance filters: the loop the reference tool's docstring
describes ("Go through color and spatial parameters and evaluate filter",
the reference's filter_reflectance.py:1) over IIW photos and their judgements, on one device.

    python -m reflectance_filtering_amd.sweep --inputs 'iiw/*.png' --filter_type bilateral \\
        --sigma_color 10,15,20,25 --sigma_spatial 16,22,28 --out sweep.json [--per_image sweep.npz]

Each photo `<stem>.png` comes with IIW judgements `<stem>.json` beside it.  The CNN predicts the
reflectance bytes (`<stem>-r.png` of decompose_with_trained_CNN); the grid is the outer product
of the two sigma lists; every pair filters the prediction and scores it with WHDR
(the bilateral filter evaluated at the judgement points only, all photos of whatever sizes in one
ragged call per pack of 2^30 pixels; the guided filter in full passes, all photos of a pack in one
ragged call per pair).  --guidance cnn filters the prediction with itself as guidance (BF/GF(CNN, CNN),
the bytes of decompose_and_filter_batch), --guidance image with the photo (the reference
README's example call).  The JSON holds the grid, the mean WHDR per pair over the images that
have judgements, the best pair and the image count; the npz the per-image matrix.
"""
from __future__ import division, print_function

import argparse
import json
import os
import sys

import numpy as np

FILTER_TYPES = ("bilateral", "guided")
GUIDANCE = ("cnn", "image")


def parse_grid(text):
    """'10,15,20.5' -> [10.0, 15.0, 20.5]: positive numbers, in the order given."""
    values = [float(v) for v in str(text).split(",") if v.strip()]
    if not values:
        raise ValueError("empty sigma list %r" % text)
    if any(not (v > 0) for v in values):
        raise ValueError("Parameters are expected to be positive.")
    return values


def grid_pairs(sigma_color, sigma_spatial):
    """Outer product, sigma_color major: float64 [len(c) * len(s), 2] (sigma_color, sigma_space)."""
    return np.array([(c, s) for c in sigma_color for s in sigma_spatial], dtype=np.float64)


def judgements_for(photo):
    """IIW judgement file of a photo: `<stem>.json` beside it."""
    return os.path.splitext(photo)[0] + ".json"


def summarise(pairs, per_image, has_judgements):
    """Mean WHDR per pair over the images with judgements, and the best (lowest) pair."""
    use = np.asarray(has_judgements, dtype=bool)
    mean = per_image[:, use].mean(axis=1) if use.any() else np.zeros(pairs.shape[0])
    best = int(np.argmin(mean))
    return mean, best


def run(photos, filter_type, sigma_color, sigma_spatial, guidance="cnn", delta=0.1):
    """The sweep over a list of photo files: returns (pairs [P,2], per_image float64 [P,N],
    has_judgements bool [N])."""
    import torch
    from . import ops, whdr
    from . import image_utils as iu
    pairs = grid_pairs(sigma_color, sigma_spatial)
    images, comps = [], []
    for f in photos:
        img = iu.imread(f)
        images.append(img)
        comps.append(whdr.to_pixels(whdr.load_judgements(judgements_for(f)), img.shape[0],
                                    img.shape[1]))
    per_image = np.zeros((pairs.shape[0], len(photos)), dtype=np.float64)
    if filter_type == "bilateral":
        # The network is per pixel, so the photos of a pack - whatever their sizes - go through
        # it as one image [1, 1, total pixels, 3], and the point sweep takes the packed bytes as
        # they come out.  A pack stays under whdr.SWEEP_PACK_PIXELS = 2^30 pixels, inside the
        # width rf_cnn_reflectance_packed_u8 accepts (a positive int).
        sizes = [img.shape[:2] for img in images]
        dedup = [whdr.dedup_points([c], h, w) for c, (h, w) in zip(comps, sizes)]
        packs = whdr.plan_packs([0] * len(photos), [h * w for h, w in sizes],
                                [int(d[1][-1]) for d in dedup], pairs.shape[0], lambda k: 1)
        for pack in packs:
            joined = whdr.join_dedup([dedup[i] for i in pack])
            if joined[2].shape[0] == 0:
                continue
            bgr = torch.from_numpy(np.concatenate([images[i].reshape(-1, 3) for i in pack])).cuda()
            _, r8 = ops.cnn_reflectance_u8(bgr.view(1, 1, -1, 3), want_float=False)
            r1 = r8.view(-1, 1)
            psizes = [sizes[i] for i in pack]
            if guidance == "cnn":
                res = whdr.sweep_packed(r1, r1, psizes, joined, pairs, delta, grey_as_bgr=True)
            else:
                res = whdr.sweep_packed(r1, bgr, psizes, joined, pairs, delta)
            per_image[:, pack] = res
        return pairs, per_image, np.array([c.shape[0] > 0 for c in comps], dtype=bool)
    # guided: full passes.  The photos of a pack - whatever their sizes - go through the network as
    # one image [1, 1, total pixels, 3], like the bilateral branch, and the packed bytes go to the
    # ragged guided filter (whdr.sweep_guided_packed: one ragged call per distinct pair; a radius
    # outside 1..128 falls back inside the entry, to the same bytes).
    from . import filter_reflectance as fr
    sizes = [img.shape[:2] for img in images]
    dedup = [whdr.dedup_points([c], h, w) for c, (h, w) in zip(comps, sizes)]
    cap = ops.gf_workspace_cap(torch.device("cuda", torch.cuda.current_device()), torch)
    for pack in fr.guided_ragged_packs(sizes, fr.GF_RAGGED_MAX_BYTES, cap):
        joined = whdr.join_dedup([dedup[i] for i in pack])
        if joined[2].shape[0] == 0:
            continue
        bgr = torch.from_numpy(np.concatenate([images[i].reshape(-1, 3) for i in pack])).cuda()
        _, r8 = ops.cnn_reflectance_u8(bgr.view(1, 1, -1, 3), want_float=False)
        r1 = r8.view(-1, 1)
        psizes = [sizes[i] for i in pack]
        if guidance == "cnn":
            res = whdr.sweep_guided_packed(r1, r1, psizes, joined, pairs, delta, grey_as_bgr=True)
        else:
            res = whdr.sweep_guided_packed(r1, bgr, psizes, joined, pairs, delta)
        per_image[:, pack] = res
    return pairs, per_image, np.array([c.shape[0] > 0 for c in comps], dtype=bool)


def build_parser():
    p = argparse.ArgumentParser(description="WHDR over a grid of filter parameters (one device).")
    p.add_argument("--inputs", nargs="+", required=True,
                   help="photos (files or glob patterns), IIW <stem>.json beside each")
    p.add_argument("--filter_type", choices=FILTER_TYPES, default="bilateral")
    p.add_argument("--sigma_color", type=parse_grid, required=True, help="comma-separated list")
    p.add_argument("--sigma_spatial", type=parse_grid, required=True, help="comma-separated list")
    p.add_argument("--guidance", choices=GUIDANCE, default="cnn")
    p.add_argument("--delta", type=float, default=0.1)
    p.add_argument("--out", default="sweep.json")
    p.add_argument("--per_image", default=None, help="npz with the per-image WHDR matrix")
    return p


def main(argv=None):
    args = build_parser().parse_args(sys.argv[1:] if argv is None else argv)
    from .batch import expand_inputs
    photos = expand_inputs(args.inputs)
    if not photos:
        raise SystemExit("no input photos")
    pairs, per_image, has = run(photos, args.filter_type, args.sigma_color, args.sigma_spatial,
                                args.guidance, args.delta)
    mean, best = summarise(pairs, per_image, has)
    result = {
        "filter_type": args.filter_type, "guidance": args.guidance, "delta": args.delta,
        "sigma_color": args.sigma_color, "sigma_spatial": args.sigma_spatial,
        "pairs": pairs.tolist(), "mean_whdr": mean.tolist(),
        "best": {"sigma_color": float(pairs[best, 0]), "sigma_spatial": float(pairs[best, 1]),
                 "mean_whdr": float(mean[best])},
        "images": len(photos), "images_with_judgements": int(has.sum()),
    }
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    if args.per_image:
        np.savez(args.per_image, whdr=per_image, pairs=pairs, has_judgements=has,
                 files=np.array(photos))
    print("best: sigma_color %g sigma_spatial %g mean WHDR %.6f over %d image(s)"
          % (pairs[best, 0], pairs[best, 1], mean[best], int(has.sum())))
    return 0


if __name__ == "__main__":
    sys.exit(main())
