#!/usr/bin/env python
"""WHDR of stored decompositions as they are, and of their filtered forms: on one device, or under
torchrun one process per GPU, each on a contiguous slice of the photos (sweep.run_sharded).

    python -m reflectance_filtering_amd.score --inputs 'iiw/*.png' --results '{dir}/zoran/{stem}.png' \\
        --coding srgb --out score.json [--per_image score.npz]

Each photo `<stem>.png` comes with IIW judgements `<stem>.json` beside it (as for sweep.py); --results
names the stored reflectance of every photo (sweep.file_for's fields {path} {dir} {name} {stem} {ext}
{base}).  --coding says what a stored byte stands for: `linear` is byte / 255, `srgb` a result saved
as sRGB (the reference README's load_image(..., is_srgb=True); whdr.value_table).  Without filter
options the files are scored unfiltered - the baseline row every filtered row is compared against.

    ... --filter_type guided --sigma_color 3 --sigma_spatial 45 [--guidance image]
        [--guidance_files '{dir}/flat/{stem}.png'] [--iterations 3]

--filter_type, --sigma_color and --sigma_spatial, given together, also run the sweep of sweep.py over
the stored files (sweep.run(src_files=..., src_coding=...)): the filters see the stored bytes, every
pass is scored under the coding.  --guidance self lets each file guide itself, image the photo.  A file
with three equal channels is scored as one channel, any other as three - sweep.py's rule, so the
unfiltered row and the filtered ones agree in kind.

The JSON holds `coding`, `delta`, `images`, `images_with_judgements`, `results` and `source`
(`mean_whdr` over the images with judgements); with a filter also the keys sweep.py writes for the
same run (`src_files` is the --results pattern, `guidance` sweep.py's name: `cnn` for self).  The npz holds `source` [N], `has_judgements` and `files`, with a filter `whdr` and `pairs`.

--split and --split_scheme score one of the reference's IIW splits (sweep.py: the position is taken
over all photos --inputs names; the JSON gains `split`, `files` hold the selected photos).  Under
RANK / WORLD_SIZE / LOCAL_RANK every rank loads, scores and filters its slice; rank 0 gathers `source`,
`has_judgements` and `whdr` and writes the files of one process (sweep.py; --io_threads, --group_timeout).
"""
from __future__ import division, print_function

import argparse
import json
import os
import sys

import numpy as np

from . import sweep

CODINGS = sweep.SRC_CODINGS
GUIDANCE = ("self", "image")        # sweep.run's "cnn" with stored sources: the source guides itself
FILTER_OPTIONS = ("filter_type", "sigma_color", "sigma_spatial")
FILTER_ONLY = ("guidance", "guidance_files", "iterations")


def build_parser():
    p = argparse.ArgumentParser(description="WHDR of stored decompositions (under torchrun one process per GPU).")
    p.add_argument("--inputs", nargs="+", required=True,
                   help="photos (files or glob patterns), IIW <stem>.json beside each")
    p.add_argument("--results", required=True, metavar="PATTERN",
                   help="the stored reflectance per photo; fields {path} {dir} {name} {stem} {ext} {base}")
    p.add_argument("--coding", choices=CODINGS, default="linear",
                   help="what a stored byte stands for: byte / 255, or an sRGB-coded value")
    p.add_argument("--delta", type=float, default=0.1)
    p.add_argument("--out", default="score.json")
    p.add_argument("--per_image", default=None, help="npz with the per-image WHDR values")
    p.add_argument("--png_decoder", choices=sweep.PNG_DECODERS, default="host",
                   help="device: the threads inflate, the device reconstructs the PNG rows")
    f = p.add_argument_group("filter (optional; the first three are given together)")
    f.add_argument("--filter_type", choices=sweep.FILTER_TYPES, default=None)
    f.add_argument("--sigma_color", type=sweep.parse_grid, default=None, help="comma-separated list")
    f.add_argument("--sigma_spatial", type=sweep.parse_grid, default=None, help="comma-separated list")
    f.add_argument("--guidance", choices=GUIDANCE, default=None,
                   help="self (the default): each stored file guides itself; image: its photo")
    f.add_argument("--guidance_files", default=None, metavar="PATTERN",
                   help="guide with the image this pattern names per photo (overrides --guidance)")
    f.add_argument("--iterations", type=sweep._positive_int, default=None, metavar="K",
                   help="apply the filter K times with the guidance held fixed; every pass is scored")
    sweep.add_split_options(p)
    sweep.add_rank_options(p)
    return p


def parse_args(argv):
    """The options, with the filter's checked as a group: all three of FILTER_OPTIONS or none, and
    those of FILTER_ONLY only beside them.  `filtered` says whether a filter runs; guidance and
    iterations then hold their defaults ("self", 1)."""
    parser = build_parser()
    args = parser.parse_args(argv)
    given = [name for name in FILTER_OPTIONS if getattr(args, name) is not None]
    if given and len(given) != len(FILTER_OPTIONS):
        parser.error("--filter_type, --sigma_color and --sigma_spatial are given together (got only %s)"
                     % ", ".join("--" + name for name in given))
    args.filtered = bool(given)
    extra = [name for name in FILTER_ONLY if getattr(args, name) is not None]
    if extra and not args.filtered:
        parser.error("%s needs --filter_type, --sigma_color and --sigma_spatial"
                     % ", ".join("--" + name for name in extra))
    if args.filtered:
        args.guidance = args.guidance or "self"
        args.iterations = args.iterations or 1
    sweep.fill_defaults(args)
    sweep.check_split(parser, args.split, args.split_scheme)
    return args


def score_sources(sources, grey, comps, coding="linear", delta=0.1):
    """The stored sources as they are: float64 [N].  A grey source (three equal channels) is scored
    as its first channel, any other as three - the rule of sweep._sweep_stored."""
    from . import whdr
    return whdr.score_list([src[:, :, :1] if g else src for src, g in zip(sources, grey)], comps,
                           coding, delta)


def main(argv=None):
    args = parse_args(sys.argv[1:] if argv is None else argv)
    from . import whdr
    from .batch import expand_inputs
    photos = expand_inputs(args.inputs)
    if not photos:
        raise SystemExit("no input photos")
    selected, split = sweep.select_split(photos, args.split, args.split_scheme)
    if not selected:
        raise SystemExit("no input photos in split %s" % args.split)
    guidance = "cnn" if args.guidance == "self" else args.guidance

    def work(part):
        """A rank's slice: the stored files as they are and, with a filter, sweep.run over them."""
        if not part:
            out = {"source": np.zeros(0, dtype=np.float64), "has": np.zeros(0, dtype=bool)}
            if args.filtered:
                pairs, per_image, _ = sweep.empty_result(args.sigma_color, args.sigma_spatial,
                                                         args.iterations)
                out.update(whdr=per_image, pairs=pairs)
            return out
        images, sources, _, judgements, grey = sweep.load(part, args.results, None, args.png_decoder,
                                                          photo_pixels=False)
        comps = [whdr.to_pixels(j, *sweep._size(img)) for j, img in zip(judgements, images)]
        out = {"source": score_sources(sources, grey, comps, args.coding, args.delta),
               "has": np.array([c.shape[0] > 0 for c in comps], dtype=bool)}
        if args.filtered:
            pairs, per_image, _ = sweep.run(part, args.filter_type, args.sigma_color,
                                            args.sigma_spatial, guidance, args.delta,
                                            src_files=args.results, guidance_files=args.guidance_files,
                                            iterations=args.iterations, png_decoder=args.png_decoder,
                                            src_coding=args.coding)
            out.update(whdr=per_image, pairs=pairs)
        return out

    rank = int(os.environ.get("RANK", "0"))
    try:
        rank, merged = sweep.run_sharded(selected, work, args.io_threads, args.group_timeout)
    except sweep.ShardError as error:
        return sweep.fail(rank, error)
    finally:
        sweep.leave_group()
    if rank:
        return 0
    source, has = merged["source"], merged["has"]
    result = {
        "coding": args.coding, "delta": args.delta, "images": len(selected),
        "images_with_judgements": int(has.sum()), "results": args.results,
        "source": {"mean_whdr": float(source[has].mean()) if has.any() else 0.0},
    }
    saved = {"source": source, "has_judgements": has, "files": np.array(selected)}
    line = "source: mean WHDR %.6f over %d image(s)" % (result["source"]["mean_whdr"], int(has.sum()))
    if args.filtered:
        pairs, per_image = merged["pairs"], merged["whdr"]
        filtered, best = sweep.report(args.filter_type, guidance, args.delta, args.sigma_color,
                                      args.sigma_spatial, pairs, per_image, has, args.iterations,
                                      args.results, args.guidance_files)
        filtered.update(result)
        result = filtered
        saved.update(whdr=per_image, pairs=pairs)
        line += "\n" + best
    if split:
        result["split"] = split
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    if args.per_image:
        np.savez(args.per_image, **saved)
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
