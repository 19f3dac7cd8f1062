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

    ... --src_files '{dir}/zoran/{stem}.png' --guidance_files '{dir}/flat/{stem}.png' \\
        --filter_type guided --sigma_color 3 --sigma_spatial 45 --iterations 3

--src_files filters the stored decomposition of another method instead of the CNN's prediction (the
network is not called; a file with three equal channels is filtered and scored as one channel, any
other as three), --guidance_files guides with a stored image such as the reference README's `flat`
(it overrides --guidance; with --src_files and --guidance cnn the source guides itself), and
--iterations K chains the filter K times with the guidance held fixed and scores every pass (the
JSON gains `passes`, the npz matrix a leading pass axis).  Photos, stored files and judgement files
are read on batch.IO_THREADS threads; --png_decoder device leaves only inflate to them.

run(..., src_coding="srgb") scores stored sources that are sRGB-coded (whdr.value_table); its command
line, with the unfiltered row beside the sweep, is reflectance_filtering_amd.score.
"""
from __future__ import division, print_function

import argparse
import json
import os
import sys

import numpy as np

FILTER_TYPES = ("bilateral", "guided")
GUIDANCE = ("cnn", "image")
PNG_DECODERS = ("host", "device")      # batch.PNG_DECODERS (batch imports the device ops)
SRC_CODINGS = ("linear", "srgb")       # whdr.CODINGS: what a byte of a stored source stands for


def _positive_int(text):
    value = int(text)
    if value < 1:
        raise argparse.ArgumentTypeError("must be at least 1")
    return value


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


def file_for(photo, pattern):
    """The stored source or guidance file of a photo under a --src_files / --guidance_files pattern:
    batch.guidance_for's fields {path} {dir} {name} {stem} {ext} {base}."""
    from .batch import guidance_for
    return guidance_for(photo, pattern)


# pixels decoded by one device decode call of the loader
DECODE_PACK_PIXELS = 1 << 28


def _read_all(jobs):
    """Every (function, file name) job on a pool of batch.IO_THREADS threads (image decode and JSON
    parsing spend their time in zlib and the file system with the GIL released): the results in the
    order of the jobs, each file read once."""
    from concurrent.futures import ThreadPoolExecutor
    from .batch import IO_THREADS
    with ThreadPoolExecutor(max_workers=IO_THREADS) as pool:
        futures = [pool.submit(fn, name) for fn, name in jobs]
        return [f.result() for f in futures]


def _size(item):
    """(h, w) of what a loader thread handed over: a parsed PNG or a decoded array."""
    return (int(item[0]), int(item[1])) if isinstance(item, tuple) else tuple(item.shape[:2])


def _decode_on_device(items):
    """batch._read_for_device results as (CUDA uint8 [H,W,3] tensor, its three channels are equal)
    pairs, in packs of at most DECODE_PACK_PIXELS pixels per batch._decode_step call (one device
    decode for the parsed files of a pack; what the parser declined arrives decoded and is uploaded
    as it is)."""
    import torch
    from .batch import _decode_step
    out, first, npx = [], 0, 0
    for i, item in enumerate(items):
        h, w = _size(item)
        if i > first and npx + h * w > DECODE_PACK_PIXELS:
            out.extend(_decode_step(items[first:i], torch))
            first, npx = i, 0
        npx += h * w
    if items:
        out.extend(_decode_step(items[first:], torch))
    return out


def load(photos, src_files=None, guidance_files=None, png_decoder="host", photo_pixels=True):
    """Everything a sweep reads, on one thread pool: the photos, their judgement files and - with
    the patterns - their stored sources and guidance images.  Returns (images, sources, guides,
    judgements, grey): lists in the order of `photos` (sources / guides None without their pattern;
    grey[i]: the three channels of source i are equal at every pixel, None without sources).  An
    image is what image_utils.imread returns, uint8 [H,W,3] BGR - a host array with the host decoder,
    a CUDA tensor of the same bytes with png_decoder="device" (batch._read_for_device on the threads,
    the parser's declines read by imread as in batch.py, and one device decode per pack).  A source
    or guidance file whose size differs from its photo's is refused before any device work;
    photo_pixels=False leaves the photos undecoded on the device route (only their sizes are used:
    the list holds the parsed files)."""
    from . import batch, whdr
    from . import image_utils as iu
    device = batch._check_png_decoder(png_decoder)
    read = batch._read_for_device if device else (lambda name: iu.imread(name))
    photos = list(photos)
    n = len(photos)
    kinds = ["photo"] + [kind for kind, pattern in (("source", src_files), ("guidance", guidance_files))
                         if pattern]
    lists = [photos] + [[file_for(f, pattern) for f in photos]
                        for pattern in (src_files, guidance_files) if pattern]
    done = _read_all([(read, name) for names in lists for name in names]
                     + [(whdr.load_judgements, judgements_for(f)) for f in photos])
    judgements = done[len(lists) * n:]
    loaded = [done[k * n:(k + 1) * n] for k in range(len(lists))]
    for kind, names, items in list(zip(kinds, lists, loaded))[1:]:
        for photo, name, item, ref in zip(photos, names, items, loaded[0]):
            if _size(item) != _size(ref):
                raise ValueError("{} file {} is {}x{}, its photo {} is {}x{}".format(
                    kind, name, _size(item)[1], _size(item)[0], photo, _size(ref)[1], _size(ref)[0]))
    flags = None
    if device:
        skip = 0 if photo_pixels else n
        flat = [item for items in loaded for item in items]
        decoded = _decode_on_device(flat[skip:])
        flat[skip:] = [img for img, _ in decoded]
        flags = [None] * skip + [bool(grey) for _, grey in decoded]
        loaded = [flat[k * n:(k + 1) * n] for k in range(len(lists))]
    images = loaded.pop(0)
    sources = loaded.pop(0) if src_files else None
    guides = loaded.pop(0) if guidance_files else None
    grey = None
    if sources is not None:     # the device decoder says it per file, a host array is compared here
        grey = flags[n:2 * n] if device else [bool(batch._is_grey(im)) for im in sources]
    return images, sources, guides, judgements, grey


def _device_list(images, channels=3):
    """Images [H,W,3] (host arrays or CUDA tensors) as contiguous CUDA uint8 tensors [H,W,channels]
    (channels = 1 keeps the first channel of a grey image): host arrays are joined on the host,
    uploaded with one copy and handed back as views of it."""
    import torch
    from . import ops
    if all(isinstance(im, np.ndarray) for im in images):
        packed = torch.from_numpy(np.concatenate([im[:, :, :channels].reshape(-1, channels)
                                                  for im in images])).cuda()
        return ops.split_packed(packed, [im.shape[:2] for im in images])
    return [(im if torch.is_tensor(im) else torch.from_numpy(im).cuda())[:, :, :channels].contiguous()
            for im in images]


def _sweep_stored(filter_type, pairs, comps, images, sources, grey_sources, guides, guidance, delta,
                  iterations, values=None):
    """The sweep over stored sources: float64 [K, P, N].  Grey sources (three equal channels) are
    filtered and scored as one channel, the others as three; a list that mixes them is split by that
    signature into one whdr.sweep call each, and the columns go back in the caller's order.  values:
    the value table the passes are scored with (whdr.sweep(values=)); None makes the calls of ever."""
    coded = {} if values is None else {"values": values}
    from . import whdr
    out = np.zeros((iterations, pairs.shape[0], len(sources)), dtype=np.float64)
    groups = {}         # grey signature -> photo indices, in order of first appearance
    for i, grey in enumerate(grey_sources):
        groups.setdefault(bool(grey), []).append(i)
    for grey, idx in groups.items():
        srcs = _device_list([sources[i] for i in idx], 1 if grey else 3)
        if guides is not None:
            joints, grey_as_bgr = _device_list([guides[i] for i in idx]), False
        elif guidance == "image":
            joints, grey_as_bgr = _device_list([images[i] for i in idx]), False
        else:       # the source guides itself
            joints, grey_as_bgr = srcs, grey
        res = whdr.sweep(filter_type, srcs, joints, [comps[i] for i in idx], pairs, delta,
                         grey_as_bgr=grey_as_bgr, iterations=iterations, **coded)
        out[:, :, idx] = res if iterations > 1 else res[None]
    return out


def run(photos, filter_type, sigma_color, sigma_spatial, guidance="cnn", delta=0.1, src_files=None,
        guidance_files=None, iterations=1, png_decoder="host", src_coding="linear"):
    """The sweep over a list of photo files: returns (pairs [P,2], per_image float64 [P,N],
    has_judgements bool [N]); with iterations = K > 1 per_image is [K,P,N], slice k the WHDR after
    pass k + 1 of the chain (whdr.sweep).  src_files: a pattern (file_for) naming the stored
    reflectance of every photo, filtered instead of the CNN's prediction - the network is not
    called.  guidance_files: a pattern naming the image that guides, as it is read (three channels);
    it overrides `guidance`.  With src_files and guidance "cnn" the source guides itself.
    png_decoder: "host" or "device" (load).  src_coding: "linear" or "srgb", what a byte of a stored
    source stands for when a pass is scored (whdr.value_table); the filters see the stored bytes
    either way.  "srgb" needs src_files: the CNN's own prediction is linear."""
    import torch
    from . import ops, whdr
    pairs = grid_pairs(sigma_color, sigma_spatial)
    iterations = int(iterations)
    if iterations < 1:
        raise ValueError("iterations must be >= 1")
    if src_coding not in SRC_CODINGS:
        raise ValueError("src_coding must be one of %s" % ", ".join(SRC_CODINGS))
    if src_coding != "linear" and not src_files:
        raise ValueError("src_coding %r needs src_files: the CNN's prediction is linear" % src_coding)
    photos = list(photos)
    need_photos = not src_files or (not guidance_files and guidance == "image")
    images, sources, guides, judgements, grey_sources = load(photos, src_files, guidance_files,
                                                             png_decoder, photo_pixels=need_photos)
    sizes = [_size(img) for img in images]
    comps = [whdr.to_pixels(j, h, w) for j, (h, w) in zip(judgements, sizes)]
    has = np.array([c.shape[0] > 0 for c in comps], dtype=bool)
    if sources is not None:
        coded = {} if src_coding == "linear" else {"values": whdr.value_table(src_coding)}
        per_image = _sweep_stored(filter_type, pairs, comps, images, sources, grey_sources, guides,
                                  guidance, delta, iterations, **coded)
        return pairs, (per_image if iterations > 1 else per_image[0]), has
    # The network is per pixel, so the photos of a pack - whatever their sizes - go through it as
    # one image [1, 1, total pixels, 3], and the filters take the packed bytes as they come out.
    per_image = np.zeros((iterations, pairs.shape[0], len(photos)), dtype=np.float64)
    dedup = [whdr.dedup_points([c], h, w) for c, (h, w) in zip(comps, sizes)]
    if filter_type == "bilateral":
        # the point sweep: a pack stays under whdr.SWEEP_PACK_PIXELS = 2^30 pixels, inside the width
        # rf_cnn_reflectance_packed_u8 accepts (a positive int)
        packs = whdr.plan_packs([0] * len(photos), [h * w for h, w in sizes],
                                [int(d[1][-1]) for d in dedup], pairs.shape[0], lambda k: 1)
        single, chain = whdr.sweep_packed, whdr.chain_packed
    else:
        # guided: full passes, the packed bytes go to the ragged guided filter (one ragged call per
        # distinct pair and pass; a radius outside 1..128 falls back inside the entry, to the same
        # bytes)
        from . import filter_reflectance as fr
        cap = ops.gf_workspace_cap(torch.device("cuda", torch.cuda.current_device()), torch)
        packs = fr.guided_ragged_packs(sizes, fr.GF_RAGGED_MAX_BYTES, cap)
        single, chain = whdr.sweep_guided_packed, whdr.chain_guided_packed
    for pack in packs:
        joined = whdr.join_dedup([dedup[i] for i in pack])
        if joined[2].shape[0] == 0:
            continue
        bgr = whdr._pack_list([images[i] for i in pack], torch)
        _, r8 = ops.cnn_reflectance_u8(bgr.view(1, 1, -1, 3), want_float=False)
        r1 = r8.view(-1, 1)
        psizes = [sizes[i] for i in pack]
        if guides is not None:
            joint, grey_as_bgr = whdr._pack_list([guides[i] for i in pack], torch), False
        elif guidance == "cnn":
            joint, grey_as_bgr = r1, True
        else:
            joint, grey_as_bgr = bgr, False
        if iterations > 1:
            per_image[:, :, pack] = chain(r1, joint, psizes, joined, pairs, iterations, delta,
                                          grey_as_bgr=grey_as_bgr)
        else:
            per_image[0][:, pack] = single(r1, joint, psizes, joined, pairs, delta,
                                           grey_as_bgr=grey_as_bgr)
    return pairs, (per_image if iterations > 1 else per_image[0]), has


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
    p.add_argument("--src_files", default=None, metavar="PATTERN",
                   help="filter the stored reflectance this pattern names per photo instead of the "
                        "CNN's prediction; fields {path} {dir} {name} {stem} {ext} {base}")
    p.add_argument("--guidance_files", default=None, metavar="PATTERN",
                   help="guide with the image this pattern names per photo (overrides --guidance)")
    p.add_argument("--iterations", type=_positive_int, default=1, metavar="K",
                   help="apply the filter K times with the guidance held fixed; every pass is scored")
    p.add_argument("--png_decoder", choices=PNG_DECODERS, default="host",
                   help="device: the threads inflate, the device reconstructs the PNG rows")
    return p


def report(filter_type, guidance, delta, sigma_color, sigma_spatial, pairs, per_image, has,
           iterations=1, src_files=None, guidance_files=None):
    """What the tool writes about a run(): the JSON dictionary and the line it prints."""
    def best_of(mean, best):
        return {"sigma_color": float(pairs[best, 0]), "sigma_spatial": float(pairs[best, 1]),
                "mean_whdr": float(mean[best])}

    # a chain reports every pass; the keys of a single pass then hold the last one, the chain's result
    passes = [summarise(pairs, m, has) for m in (per_image if iterations > 1 else [per_image])]
    mean, best = passes[-1]
    result = {
        "filter_type": filter_type, "guidance": guidance, "delta": delta,
        "sigma_color": sigma_color, "sigma_spatial": sigma_spatial,
        "pairs": pairs.tolist(), "mean_whdr": mean.tolist(),
        "best": best_of(mean, best),
        "images": len(has), "images_with_judgements": int(has.sum()),
    }
    if iterations > 1:
        result["iterations"] = iterations
        result["passes"] = [{"pass": k + 1, "mean_whdr": m.tolist(), "best": best_of(m, b)}
                            for k, (m, b) in enumerate(passes)]
    if src_files:
        result["src_files"] = src_files
    if guidance_files:
        result["guidance_files"] = guidance_files
    line = ("best: sigma_color %g sigma_spatial %g mean WHDR %.6f over %d image(s)"
            % (pairs[best, 0], pairs[best, 1], mean[best], int(has.sum())))
    return result, line


def main(argv=None):
    args = build_parser().parse_args(sys.argv[1:] if argv is None else argv)
    from .batch import expand_inputs
    photos = expand_inputs(args.inputs)
    if not photos:
        raise SystemExit("no input photos")
    pairs, per_image, has = run(photos, args.filter_type, args.sigma_color, args.sigma_spatial,
                                args.guidance, args.delta, src_files=args.src_files,
                                guidance_files=args.guidance_files, iterations=args.iterations,
                                png_decoder=args.png_decoder)
    result, line = report(args.filter_type, args.guidance, args.delta, args.sigma_color,
                          args.sigma_spatial, pairs, per_image, has, args.iterations, args.src_files,
                          args.guidance_files)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    if args.per_image:
        np.savez(args.per_image, whdr=per_image, pairs=pairs, has_judgements=has,
                 files=np.array(photos))
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
