#!/usr/bin/env python
"""Batch front-end: the reference's two tools over many files, one process per GPU.

The reference handles one image per invocation (/root/reference/filter_reflectance.py:76-96,
/root/reference/decompose_with_trained_CNN.py:98-130).  Every image is independent, so a list of
files shards embarrassingly: each rank (torchrun sets RANK/WORLD_SIZE/LOCAL_RANK) takes a
contiguous slice of the sorted file list and works through it in steps of 16 files as a pipeline
- a thread pool decodes the next step and encodes the previous one while the device filters the
current one - and writes the same output files the single-image tools would write.  A step whose
images all have one size goes through the device-resident batch operators as one batch.  A step
whose images differ in size goes through the list forms, one call for the whole step: `decompose`
through decompose_with_trained_CNN.decompose_packed (the device work of decompose_list: one CNN pass
over the packed photos, one ragged colourise), a bilateral `filter` through
filter_reflectance.apply_filter_list (one ragged call per pass), and so does a guided `filter` step
whose sources are all grey (one ragged call for all passes); only a guided step with a colour source
is still cut into runs of equal size, one batch per run.  No collective is involved.

    python -m reflectance_filtering_amd.batch filter --filter_type=bilateral --sigma_color=20 \
        --sigma_spatial=22 --inputs 'out/*-r.png' --guidance 'photos/{stem}.png' --path_out out
    python -m torch.distributed.run --nproc-per-node 8 -m reflectance_filtering_amd.batch \
        decompose --inputs 'photos/*.png' --path_out out

    python -m reflectance_filtering_amd.batch decompose_filter --inputs 'photos/*.png' \
        --path_out out --filter_type=bilateral --sigma_color=20 --sigma_spatial=22

`decompose_filter` is both tools in one pass over the photos: a step goes through
decompose_with_trained_CNN.decompose_filter_packed (one CNN pass, the ragged filter routes, two ragged
colourises) and writes what `decompose` writes, what `filter` makes of its `-r.png` outputs, and the
colour reflectance and shading derived from the filtered map (`<filtered stem>-r_colorized.png`,
`-s_colorized.png`).  Every photo is decoded once and no `-r.png` is read back.  Its `--guidance` is
omitted (the CNN map guides itself), `image` (the photo guides) or a pattern evaluated on the photo's
path.

`--png_encoder device` deflates the `.png` outputs on the device and `--png_decoder device` leaves
only parsing and inflate of the `.png` inputs to the I/O threads (the device undoes the row filters
and unpacks the samples); both default to `host`, and the pixels are the same either way.

`--guidance` is a pattern evaluated per input: {path} {dir} {name} {stem} {ext}; `{stem}` of
`x-r.png` is `x-r`, `{base}` strips a trailing `-r` as well, so `photos/{base}.png` pairs a CNN
prediction with its photo.  Omit it to use each input as its own guidance (BF(CNN,CNN)).
"""
from __future__ import division, print_function

import argparse
import glob
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import filter_reflectance as fr
from . import ops
from . import image_utils as iu
from . import sharding

MAX_BATCH_BYTES = 2 << 30  # per group of equal-size images kept on the device at once
STEP_FILES = 16            # files per pipeline step (decode k+1 | device k | encode k-1)
IO_THREADS = max(1, min(16, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity")
                        else (os.cpu_count() or 1)))


def pipeline(items, load, compute, step=None):
    """Three-stage pipeline over `items` in steps of `step` files: while the device works on step
    k (in the calling thread: `compute(list of load() results)` returns a list of
    (file name, payload) pairs to write), the thread pool decodes step k+1 and encodes what step k-1
    produced: an array payload goes through image_utils.imwrite, a `bytes` payload - a file encoded
    on the device already - is written as it is.  Image decode / encode spend their time in zlib with
    the GIL released and the device calls release it too, so the three stages overlap; at most two
    decoded steps and two steps of pending writes are alive at a time.  Returns the names written,
    in order."""
    step = step or STEP_FILES
    items = list(items)
    steps = [items[i:i + step] for i in range(0, len(items), step)]
    written = []
    if not steps:
        return written
    with ThreadPoolExecutor(max_workers=IO_THREADS) as pool:
        loads = [pool.submit(load, it) for it in steps[0]]
        pending = []                       # write futures of the previous steps, oldest first
        for k, _ in enumerate(steps):
            nxt = [pool.submit(load, it) for it in steps[k + 1]] if k + 1 < len(steps) else []
            loaded = [f.result() for f in loads]
            jobs = compute(loaded)
            while len(pending) > 1:        # writes of step k-2 must be done before step k's start
                for f in pending.pop(0):
                    f.result()
            pending.append([pool.submit(_write_job, name, payload) for name, payload in jobs])
            written.extend(name for name, _ in jobs)
            loads = nxt
        for futs in pending:
            for f in futs:
                f.result()
    return written


def _write_job(name, payload):
    if isinstance(payload, (bytes, bytearray, memoryview)):
        try:
            with open(name, "wb") as fh:
                fh.write(payload)
        except OSError:
            raise Exception("Not able to write {}, does the folder exist?".format(name))
    else:
        iu.imwrite(name, payload)


PNG_ENCODERS = ("host", "device")


def _check_png_encoder(png_encoder):
    if png_encoder not in PNG_ENCODERS:
        raise ValueError("png_encoder must be one of {}".format(", ".join(PNG_ENCODERS)))
    return png_encoder == "device"


PNG_DECODERS = ("host", "device")


def _check_png_decoder(png_decoder):
    if png_decoder not in PNG_DECODERS:
        raise ValueError("png_decoder must be one of {}".format(", ".join(PNG_DECODERS)))
    return png_decoder == "device"


def _is_png(name):
    return os.path.splitext(name)[1].lower() == ".png"


def _read_for_device(name):
    """What an I/O thread hands over for the device decoder: the parsed file (image_utils.png_parse:
    inflated, not reconstructed) of a `.png` name, or the decoded array where the parser declines the
    file (interlace, a bit depth below 8, damage: imread says what is wrong) or it is no PNG."""
    if _is_png(name):
        try:
            with open(name, "rb") as fh:
                parsed = iu.png_parse(fh.read())
        except OSError:
            parsed = None
        if parsed is not None:
            return parsed
    return iu.imread(name)


def _decode_step(items, torch):
    """The files of one step on the device: `items` holds _read_for_device results (None stands for
    "the item before", a guidance file that is the input itself).  All parsed files are decoded in one
    ops.png_decode_ragged_u8 call, the arrays are uploaded as they are.  Returns one (CUDA uint8
    [H,W,3] tensor, all three channels equal) pair per item."""
    parsed = [i for i, it in enumerate(items) if isinstance(it, tuple)]
    images, grey = ops.png_decode_ragged_u8([items[i] for i in parsed])
    out = [None] * len(items)
    for i, img, g in zip(parsed, images, grey):
        out[i] = (img, g)
    for i, it in enumerate(items):
        if it is None:
            out[i] = out[i - 1]
        elif out[i] is None:
            out[i] = (torch.from_numpy(it).cuda(), _is_grey(it))
    return out


def expand_inputs(patterns):
    """Sorted, de-duplicated list of files matched by the patterns (a literal path matches itself)."""
    files = []
    for pat in patterns:
        hits = sorted(glob.glob(pat))
        files.extend(hits if hits else ([pat] if os.path.exists(pat) else []))
    seen, out = set(), []
    for f in files:
        if f not in seen:
            seen.add(f)
            out.append(f)
    return out


def guidance_for(path, pattern):
    """File name of the guidance image of `path` under `pattern` (None -> the input itself)."""
    if not pattern:
        return path
    d, name = os.path.split(path)
    stem, ext = os.path.splitext(name)
    base = stem[:-2] if stem.endswith("-r") else stem
    return pattern.format(path=path, dir=d, name=name, stem=stem, ext=ext, base=base)


def my_slice(files, rank=None, world=None):
    """The contiguous part of `files` this rank owns."""
    if rank is None:
        rank = int(os.environ.get("RANK", "0"))
    if world is None:
        world = int(os.environ.get("WORLD_SIZE", "1"))
    lo, hi = sharding.shard_range(len(files), world, rank)
    return files[lo:hi]


def group_by_shape(items, shape_of, max_bytes=MAX_BATCH_BYTES):
    """Consecutive runs of `items` with equal shape, cut so that a run stays under max_bytes."""
    groups, cur, cur_shape = [], [], None
    for it in items:
        shp = shape_of(it)
        per = int(np.prod(shp))
        if cur and (shp != cur_shape or (len(cur) + 1) * per > max_bytes):
            groups.append(cur)
            cur = []
        cur.append(it)
        cur_shape = shp
    if cur:
        groups.append(cur)
    return groups


def _is_grey(batch):
    """All images of a [N,H,W,3] uint8 batch have three equal channels."""
    return (batch.shape[-1] == 3 and np.array_equal(batch[..., 0], batch[..., 1])
            and np.array_equal(batch[..., 1], batch[..., 2]))


def filter_files(filter_type, inputs, guidance_pattern, sigma_color, sigma_spatial, path_out,
                 iterations=1, rank=None, world=None, png_encoder="host", png_decoder="host"):
    """filter_reflectance.read_filter_write over this rank's share of `inputs`; returns the
    list of files written.  png_encoder="device" deflates the `.png` outputs on the device
    (ops.png_encode_ragged_u8: the same pixels in files of other bytes); any other extension keeps
    the host writer.  png_decoder="device": the I/O threads only parse and inflate the `.png` inputs
    (image_utils.png_parse) and the device undoes the row filters and unpacks the samples, one
    ops.png_decode_ragged_u8 call per step; a file the parser declines and any other extension keep
    imread.  The pixels, and so the files written, are the same."""
    import torch
    fr._check_params(filter_type, sigma_color, sigma_spatial)
    on_device = _check_png_encoder(png_encoder)
    decode_on_device = _check_png_decoder(png_decoder)
    mine = my_slice(inputs, rank, world)

    def load(f):
        img, gui = iu.imread(f), iu.imread(guidance_for(f, guidance_pattern))
        if img.shape[:2] != gui.shape[:2]:
            raise ValueError("input {} and its guidance differ in size".format(f))
        return f, img, gui

    def out_name(f):
        name = f
        for _ in range(iterations):  # the chained CLI runs append the suffix once per pass
            name = fr.output_filename(name, path_out, filter_type, sigma_color, sigma_spatial)
        return name

    def device_jobs(names, results, grey_src):
        """The jobs of one device result per name ([H,W,C] tensors): files encoded on the device for
        the `.png` names (one call for all of them; a grey source as three equal samples, which is
        what the host path replicates), arrays for the others."""
        jobs = [None] * len(names)
        png = [i for i, name in enumerate(names) if _is_png(name)]
        if png:
            files = ops.png_encode_ragged_u8([results[i] for i in png], grey_as_rgb=grey_src)
            for i, data in zip(png, files):
                jobs[i] = (names[i], data)
        for i, name in enumerate(names):
            if jobs[i] is None:
                res = results[i].cpu().numpy()
                jobs[i] = (name, np.repeat(res, 3, axis=2) if grey_src else res)
        return jobs

    def compute_ragged(loaded):
        """A bilateral step whose images differ in shape - or a guided one whose sources are all
        grey: one ragged call over the whole step (fr.apply_filter_list; one per pass for the
        bilateral filter) instead of one launch per run of equal shapes.  The grey reductions of
        `compute` below, judged over the step: identical bytes."""
        grey_src = all(_is_grey(t[1]) for t in loaded)
        grey_gui = grey_src and all(_is_grey(t[2]) for t in loaded)
        cut = lambda a, grey: np.ascontiguousarray(a[..., :1]) if grey else a
        images = [torch.from_numpy(cut(t[1], grey_src)).cuda() for t in loaded]
        joints = [torch.from_numpy(cut(t[2], grey_gui)).cuda() for t in loaded]
        outs = fr.apply_filter_list(filter_type, images, joints, sigma_color, sigma_spatial,
                                    iterations=iterations, grey_as_bgr=grey_gui)
        if on_device:
            return device_jobs([out_name(t[0]) for t in loaded], list(outs), grey_src)
        jobs = []
        for (f, _, _), res in zip(loaded, outs):
            res = res.cpu().numpy()
            jobs.append((out_name(f), np.repeat(res, 3, axis=2) if grey_src else res))
        return jobs

    def compute(loaded):
        if len(set(t[1].shape for t in loaded)) > 1 and (
                filter_type == "bilateral" or all(_is_grey(t[1]) for t in loaded)):
            return compute_ragged(loaded)
        jobs = []
        for group in group_by_shape(loaded, lambda t: t[1].shape):
            imgs = np.stack([t[1] for t in group])
            guis = np.stack([t[2] for t in group])
            # A grey PNG comes back from imread as three equal channels (the CNN's `-r.png` always
            # does).  The channels never mix in either filter, so such a group is filtered as one
            # channel - a third of the transfers and of the guided filter's scratch, all tile
            # shapes of the bilateral kernel - and replicated afterwards: identical bytes.
            grey_src = _is_grey(imgs)
            if grey_src:
                imgs = imgs[..., :1]
            images = torch.from_numpy(np.ascontiguousarray(imgs)).cuda()
            if filter_type == "bilateral" and grey_src and _is_grey(guis):
                joints = torch.from_numpy(np.ascontiguousarray(guis[..., :1])).cuda()
                out = images
                for _ in range(iterations):
                    out = ops.joint_bilateral_u8(joints, out, -1, sigma_color, sigma_spatial,
                                                 grey_as_bgr=True)
            elif filter_type == "guided" and _is_grey(guis):
                # grey guidance (GF(CNN, CNN)): uploaded as one byte per pixel, read as three equal
                # channels by the grey-guide kernels - identical bytes
                joints = torch.from_numpy(np.ascontiguousarray(guis[..., :1])).cuda()
                out = fr.apply_filter_batch(filter_type, images, joints, sigma_color,
                                            sigma_spatial, iterations=iterations, grey_as_bgr=True)
            else:
                joints = torch.from_numpy(guis).cuda()
                out = fr.apply_filter_batch(filter_type, images, joints, sigma_color,
                                            sigma_spatial, iterations=iterations)
            if on_device:
                jobs.extend(device_jobs([out_name(t[0]) for t in group], list(out), grey_src))
                continue
            out = out.cpu().numpy()
            if grey_src:
                out = np.repeat(out, 3, axis=3)
            for (f, _, _), res in zip(group, out):
                jobs.append((out_name(f), res))
        return jobs

    def load_parsed(f):
        g = guidance_for(f, guidance_pattern)
        # a guidance file that is the input itself is read and decoded once
        return f, _read_for_device(f), (None if g == f else _read_for_device(g))

    def filter_on_device(filter_type, images, joints, grey_src, grey_gui):
        """One group of equal shapes, [N,H,W,C] on the device: the branches of `compute`."""
        if filter_type == "bilateral" and grey_src and grey_gui:
            out = images
            for _ in range(iterations):
                out = ops.joint_bilateral_u8(joints, out, -1, sigma_color, sigma_spatial,
                                             grey_as_bgr=True)
            return out
        return fr.apply_filter_batch(filter_type, images, joints, sigma_color, sigma_spatial,
                                     iterations=iterations,
                                     **({"grey_as_bgr": True} if grey_gui else {}))

    def compute_decoded(loaded):
        """`compute` for the device decoder: the step's files become device tensors and grey flags
        in one call (_decode_step), the grey reductions take channel 0 as a device slice, and a
        uniform group stacks device tensors.  The same operators on the same pixels: identical
        bytes."""
        flat = []
        for _, img, gui in loaded:
            flat.extend((img, gui))
        dec = _decode_step(flat, torch)
        step = []
        for k, (f, _, _) in enumerate(loaded):
            (img, img_grey), (gui, gui_grey) = dec[2 * k], dec[2 * k + 1]
            if img.shape[:2] != gui.shape[:2]:
                raise ValueError("input {} and its guidance differ in size".format(f))
            step.append((f, img, gui, img_grey, gui_grey))
        cut = lambda a, grey: a[..., :1].contiguous() if grey else a

        def finish(names, results, grey_src):
            if on_device:
                return device_jobs(names, results, grey_src)
            jobs = []
            for name, res in zip(names, results):
                res = res.cpu().numpy()
                jobs.append((name, np.repeat(res, 3, axis=2) if grey_src else res))
            return jobs

        all_grey = all(t[3] for t in step)
        if len(set(tuple(t[1].shape) for t in step)) > 1 and (filter_type == "bilateral" or all_grey):
            grey_src = all_grey
            grey_gui = grey_src and all(t[4] for t in step)
            outs = fr.apply_filter_list(filter_type, [cut(t[1], grey_src) for t in step],
                                        [cut(t[2], grey_gui) for t in step], sigma_color,
                                        sigma_spatial, iterations=iterations, grey_as_bgr=grey_gui)
            return finish([out_name(t[0]) for t in step], list(outs), grey_src)
        jobs = []
        for group in group_by_shape(step, lambda t: tuple(t[1].shape)):
            grey_src = all(t[3] for t in group)
            guis_grey = all(t[4] for t in group)
            # the guidance is cut to one channel where `compute` cuts it: for the bilateral filter
            # with a grey source, for the guided filter always
            grey_gui = guis_grey and (grey_src if filter_type == "bilateral" else filter_type == "guided")
            images = torch.stack([cut(t[1], grey_src) for t in group])
            joints = torch.stack([cut(t[2], grey_gui) for t in group])
            out = filter_on_device(filter_type, images, joints, grey_src, grey_gui)
            jobs.extend(finish([out_name(t[0]) for t in group], list(out), grey_src))
        return jobs

    if decode_on_device:
        return pipeline(mine, load_parsed, compute_decoded)
    return pipeline(mine, load, compute)


def decompose_files(inputs, path_out, rank=None, world=None, png_encoder="host", png_decoder="host"):
    """decompose_image over this rank's share of `inputs`: CNN, colourisation, percentile
    normalisation and the sRGB byte conversion all run batched on the device; the host only
    decodes and encodes the image files - or, with png_encoder="device", only decodes them: the
    three outputs of a step are deflated on the device (ops.png_encode_ragged_u8, three calls) and
    come back as finished files with the same pixels in other bytes.  png_decoder="device": the
    I/O threads only parse and inflate the `.png` inputs and the device reconstructs and unpacks them
    (see filter_files): the same pixels, the same files."""
    import torch
    from . import decompose_with_trained_CNN as dc
    on_device = _check_png_encoder(png_encoder)
    decode_on_device = _check_png_decoder(png_decoder)
    mine = my_slice(inputs, rank, world)
    firsts = []

    def add_encoded(jobs, loaded, sizes, r8, refl, shad):
        """The step's jobs from its packed device outputs ([total pixels], [total pixels, 3],
        [total pixels]), encoded there."""
        files = [ops.png_encode_ragged_u8(t, sizes=sizes) for t in (r8, refl, shad)]
        for i, t in enumerate(loaded):
            add(jobs, t[0], files[0][i], files[1][i], files[2][i])

    def add(jobs, f, r8, refl, shad):
        base = os.path.splitext(os.path.basename(f))[0]
        jobs.append((os.path.join(path_out, base + "-r.png"), r8))
        jobs.append((os.path.join(path_out, base + "-r_colorized.png"), refl))
        jobs.append((os.path.join(path_out, base + "-s_colorized.png"), shad))
        firsts.append(os.path.join(path_out, base + "-r.png"))

    def compute_ragged(loaded):
        """A step whose images differ in shape: the device work of dc.decompose_list over the whole
        step (one CNN pass, one ragged colourise) instead of one decompose_batch per run of equal
        shapes, then three copies of the packed outputs to the host, split there: identical bytes."""
        sizes, _, r8, refl, shad = dc.decompose_packed([on_gpu(t[1]) for t in loaded])
        if on_device:
            jobs = []
            add_encoded(jobs, loaded, sizes, r8.reshape(-1), refl.reshape(-1, 3), shad.reshape(-1))
            return jobs
        r8, refl, shad = r8.cpu().numpy(), refl.cpu().numpy(), shad.cpu().numpy()
        jobs, first = [], 0
        for (f, _), (h, w) in zip(loaded, sizes.tolist()):
            px = slice(first, first + h * w)
            add(jobs, f, r8[px].reshape(h, w), refl[px].reshape(h, w, 3), shad[px].reshape(h, w))
            first += h * w
        return jobs

    def on_gpu(image):
        return image if torch.is_tensor(image) else torch.from_numpy(image).cuda()

    def compute(loaded):
        if decode_on_device:   # the step's files as device tensors, decoded there in one call
            decoded = _decode_step([t[1] for t in loaded], torch)
            loaded = [(t[0], d[0]) for t, d in zip(loaded, decoded)]
        if len(set(tuple(t[1].shape) for t in loaded)) > 1:
            return compute_ragged(loaded)
        jobs = []
        for group in group_by_shape(loaded, lambda t: tuple(t[1].shape)):
            if decode_on_device:
                images = torch.stack([t[1] for t in group])
            else:
                images = torch.from_numpy(np.stack([t[1] for t in group])).cuda()
            _, r8, refl, shad = dc.decompose_batch(images)
            if on_device:   # a uniform step goes through the same op, as a list of equal sizes
                add_encoded(jobs, group, [t[1].shape[:2] for t in group], r8.reshape(-1),
                            refl.reshape(-1, 3), shad.reshape(-1))
                continue
            r8, refl, shad = r8.cpu().numpy(), refl.cpu().numpy(), shad.cpu().numpy()
            for i, (f, _) in enumerate(group):
                add(jobs, f, r8[i], refl[i], shad[i])
        return jobs

    pipeline(mine, (lambda f: (f, _read_for_device(f))) if decode_on_device
             else (lambda f: (f, iu.imread(f))), compute)
    return firsts


def decompose_filter_names(filename_in, path_out, filter_type, sigma_color, sigma_spatial, iterations=1):
    """The six files decompose_filter_files writes for one photo, in the order it writes them: the
    three of `decompose`, the file `filter` makes of `<base>-r.png` in `iterations` chained runs (the
    suffix once per pass), and that file's stem + `-r_colorized.png` / `-s_colorized.png`."""
    base = os.path.splitext(os.path.basename(filename_in))[0]
    first = os.path.join(path_out, base + "-r.png")
    filtered = first
    for _ in range(iterations):
        filtered = fr.output_filename(filtered, path_out, filter_type, sigma_color, sigma_spatial)
    stem = os.path.splitext(filtered)[0]
    return (first, os.path.join(path_out, base + "-r_colorized.png"),
            os.path.join(path_out, base + "-s_colorized.png"), filtered,
            stem + "-r_colorized.png", stem + "-s_colorized.png")


def decompose_filter_files(inputs, path_out, filter_type, sigma_color, sigma_spatial,
                           guidance_pattern=None, iterations=1, rank=None, world=None,
                           png_encoder="host", png_decoder="host", colorize_filtered=True):
    """`decompose` and `filter` of its `-r.png` outputs in one pass over this rank's share of the
    photos `inputs`, plus the decomposition derived from the filtered map
    (decompose_with_trained_CNN.decompose_filter_packed, one call per step): every photo - and
    guidance file - is decoded once and no `-r.png` is read back.  guidance_pattern: None - the CNN
    map guides itself; "image" - the photo guides; anything else is a guidance_for pattern evaluated
    on the photo's path.  Writes the files of decompose_filter_names per photo: the first three are
    the bytes of decompose_files, the fourth those of filter_files on `<base>-r.png` with the same
    guidance (the grey map as three equal channels), the last two
    imwrite(colorize(float32(filtered) / 255, photo), sRGB=True) (left out with
    colorize_filtered=False).  png_encoder / png_decoder as in filter_files.  Returns the names of the
    filtered files."""
    import torch
    from . import decompose_with_trained_CNN as dc
    fr._check_params(filter_type, sigma_color, sigma_spatial)
    if iterations < 1:
        raise ValueError("iterations must be >= 1")
    on_device = _check_png_encoder(png_encoder)
    decode_on_device = _check_png_decoder(png_decoder)
    mine = my_slice(inputs, rank, world)
    read = _read_for_device if decode_on_device else iu.imread
    filtered_names = []

    def load(f):
        g = None if guidance_pattern in (None, "image") else guidance_for(f, guidance_pattern)
        # a guidance file that is the photo itself is read and decoded once
        return f, read(f), (None if g is None or g == f else read(g)), g == f

    def compute(loaded):
        if decode_on_device:
            flat = []
            for _, img, gui, _ in loaded:
                flat.extend((img,) if gui is None else (img, gui))
            dec = iter(_decode_step(flat, torch))
            step = []
            for f, _, gui, own in loaded:
                img = next(dec)[0]
                step.append((f, img, None if gui is None else next(dec), own))
            greys = [t[2][1] for t in step if t[2] is not None]
            step = [(f, img, None if gui is None else gui[0], own) for f, img, gui, own in step]
        else:
            greys = [_is_grey(t[2]) for t in loaded if t[2] is not None]
            step = [(f, torch.from_numpy(img).cuda(), None if gui is None else torch.from_numpy(gui).cuda(),
                     own) for f, img, gui, own in loaded]
        photos = [t[1] for t in step]
        if guidance_pattern is None:
            guidance = None
        elif guidance_pattern == "image":
            guidance = "image"
        else:
            # as filter_files: a step of grey guidance files is read as one channel standing for three
            grey_gui = all(greys) and not any(t[3] for t in step)
            guidance = []
            for f, photo, gui, own in step:
                gui = photo if own else gui
                if tuple(gui.shape[:2]) != tuple(photo.shape[:2]):
                    raise ValueError("input {} and its guidance differ in size".format(f))
                guidance.append(gui[..., :1].contiguous() if grey_gui else gui)
        res = dc.decompose_filter_packed(photos, sigma_color, sigma_spatial, filter_type, guidance,
                                         iterations, colorize_filtered=colorize_filtered)
        names = [decompose_filter_names(t[0], path_out, filter_type, sigma_color, sigma_spatial, iterations)
                 for t in step]
        filtered_names.extend(n[3] for n in names)
        kinds = [res.r_u8, res.reflectance, res.shading, res.filtered]
        if colorize_filtered:
            kinds += [res.filtered_reflectance, res.filtered_shading]
        jobs = []
        if on_device:
            files = [ops.png_encode_ragged_u8(t, sizes=res.sizes, grey_as_rgb=(k == 3))
                     for k, t in enumerate(kinds)]
            for i, n in enumerate(names):
                jobs.extend((n[k], files[k][i]) for k in range(len(kinds)))
            return jobs
        kinds = [t.cpu().numpy() for t in kinds]
        first = 0
        for n, (h, w) in zip(names, res.sizes.tolist()):
            px = slice(first, first + h * w)
            for k, a in enumerate(kinds):
                a = a[px].reshape((h, w, 3) if a.ndim == 2 else (h, w))
                # the filtered grey map as three equal channels, as filter_files writes it
                jobs.append((n[k], np.repeat(a[:, :, None], 3, axis=2) if k == 3 else a))
            first += h * w
        return jobs

    pipeline(mine, load, compute)
    return filtered_names


def build_parser():
    parser = argparse.ArgumentParser(description="Batched, multi-GPU front-end of the two tools.")
    sub = parser.add_subparsers(dest="command")
    f = sub.add_parser("filter", help="filter_reflectance over many files")
    f.add_argument("--inputs", nargs="+", required=True, help="files or glob patterns")
    f.add_argument("--guidance", default=None, help="pattern for the guidance file (see module doc)")
    f.add_argument("--path_out", required=True)
    f.add_argument("--sigma_color", type=float, required=True)
    f.add_argument("--sigma_spatial", type=float, required=True)
    f.add_argument("--filter_type", required=True)
    f.add_argument("--iterations", type=int, default=1)
    f.add_argument("--png_encoder", choices=PNG_ENCODERS, default="host",
                   help="who deflates the .png outputs: zlib on the I/O threads, or the device")
    d = sub.add_parser("decompose", help="decompose_with_trained_CNN over many files")
    d.add_argument("--inputs", nargs="+", required=True)
    d.add_argument("--path_out", required=True)
    d.add_argument("--png_encoder", choices=PNG_ENCODERS, default="host",
                   help="who deflates the three .png outputs per photo")
    c = sub.add_parser("decompose_filter", help="decompose, filter the CNN map and colourise the "
                                                "filtered map: every photo decoded once")
    c.add_argument("--inputs", nargs="+", required=True, help="photos: files or glob patterns")
    c.add_argument("--path_out", required=True)
    c.add_argument("--filter_type", default="bilateral")
    c.add_argument("--sigma_color", type=float, default=20.0)
    c.add_argument("--sigma_spatial", type=float, default=22.0)
    c.add_argument("--guidance", default=None,
                   help="omitted: the CNN map guides itself; `image`: the photo guides; anything else: "
                        "a pattern for the guidance file, evaluated on the photo's path")
    c.add_argument("--iterations", type=int, default=1)
    c.add_argument("--png_encoder", choices=PNG_ENCODERS, default="host",
                   help="who deflates the six .png outputs per photo")
    for p in (f, d, c):
        p.add_argument("--png_decoder", choices=PNG_DECODERS, default="host",
                       help="who undoes the row filters of the .png inputs and unpacks them: the I/O "
                            "threads, or the device (the threads then only parse and inflate)")
    return parser


def main(argv=None):
    args = build_parser().parse_args(sys.argv[1:] if argv is None else argv)
    if args.command is None:
        build_parser().print_help()
        return 0
    import torch
    local = int(os.environ.get("LOCAL_RANK", os.environ.get("RANK", "0")))
    if torch.cuda.is_available():
        torch.cuda.set_device(local % torch.cuda.device_count())
    files = expand_inputs(args.inputs)
    if args.command == "filter":
        out = filter_files(args.filter_type, files, args.guidance, args.sigma_color,
                           args.sigma_spatial, args.path_out, iterations=args.iterations,
                           png_encoder=args.png_encoder, png_decoder=args.png_decoder)
    elif args.command == "decompose_filter":
        out = decompose_filter_files(files, args.path_out, args.filter_type, args.sigma_color,
                                     args.sigma_spatial, guidance_pattern=args.guidance,
                                     iterations=args.iterations, png_encoder=args.png_encoder,
                                     png_decoder=args.png_decoder)
    else:
        out = decompose_files(files, args.path_out, png_encoder=args.png_encoder,
                              png_decoder=args.png_decoder)
    print("rank {}: wrote {} file(s)".format(os.environ.get("RANK", "0"), len(out)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
