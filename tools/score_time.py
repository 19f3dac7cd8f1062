#!/usr/bin/env python
"""What the coded WHDR path costs: whdr_points_values_u8 with the linear table against whdr_points_u8.

64 synthetic grey CNN-like maps of the three common IIW shapes (341x512, 512x341, 384x512) in the
seeded order of tools/ragged_filter_time.py, each with about 300 judged points in 450 comparisons, as
8 sets of device-resident uint8 samples - the call a sweep of 8 pairs makes per pass.  Two forms of it:
    points  the samples are the deduplicated judgement points [8, total points, 1] (what a bilateral
            sweep scores)
    images  the samples are the packed maps themselves [8, total pixels, 1], comparisons indexed by
            pixel (what a guided sweep scores)
Two routes, the same scores (asserted equal bit for bit):
    u8      whdr.whdr_points_u8: one rf_whdr_points_u8 launch on the bytes (unchanged by the value
            tables, so this is the code before them)
    values  whdr.whdr_points_values_u8 with value_table("linear"): host remap of the comparisons to
            the distinct referenced points, device gather and table look-up, rf_whdr_f32
After a warm-up of both, the routes alternate --reps times, --passes calls per timed span that ends
in a device synchronise (both routes end in a copy of the result to the host); the line gives median,
min and max ms per call.  The ratio is recorded, not bounded: the linear path stays the default.

Each case runs in a child process under its own time limit; a child that fails ends the run.  Prints
one JSON line per case; --out also appends the readable lines to a file.

    python tools/score_time.py [--reps 5] [--passes 3] [--limit 300] [--cases points,images] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ("points", "images")
N_SETS = 8


def case(name, reps, passes, out):
    import numpy as np
    import torch
    from reflectance_filtering_amd import whdr
    from tests import synth
    from tools.gf_sweep_time import comparisons
    from tools.ragged_filter_time import list_shapes
    assert torch.cuda.is_available(), "score_time.py needs a HIP device"
    shapes = list_shapes()
    rng = np.random.default_rng(11)
    comps = [comparisons(h, w, rng) for h, w in shapes]
    dedup = whdr.dedup_points_ragged(comps, shapes)
    image_offsets, pixels = whdr._point_pixels(dedup, shapes)
    # set s: the maps with s added to every byte (wrapping), so the sets differ
    packed = np.concatenate([synth.reflectance_like_u8(h, w, 100 + i)[:, :, :1].reshape(-1, 1)
                             for i, (h, w) in enumerate(shapes)])
    sets = torch.from_numpy(np.stack([packed + np.uint8(17 * s) for s in range(N_SETS)])).cuda()
    if name == "points":
        index = whdr._index(pixels + np.repeat(image_offsets[:-1], np.diff(dedup[1].astype(np.int64))),
                            sets)
        args = (sets[:, index].contiguous(), dedup[1], dedup[2], dedup[3], dedup[4])
    else:
        args = (sets, image_offsets, whdr._pixel_comps(dedup, pixels), dedup[3], dedup[4])
    table = whdr.value_table("linear")
    routes = (("u8", lambda: whdr.whdr_points_u8(*args, delta=0.1)),
              ("values", lambda: whdr.whdr_points_values_u8(*args, values=table, delta=0.1)))
    first = {r: fn() for r, fn in routes}          # warm-up of both routes, and the scores
    assert first["u8"].shape == (N_SETS, len(shapes)) and np.any(first["u8"] > 0)
    assert np.array_equal(first["u8"], first["values"]), "the coded route differs from the byte route"
    times = {r: [] for r, _ in routes}
    for _ in range(reps):
        for r, fn in routes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(passes):
                fn()
            torch.cuda.synchronize()
            times[r].append((time.perf_counter() - t0) / passes)
    line = {"tool": "score_time", "case": name, "n": len(shapes), "sets": N_SETS,
            "samples_per_set": int(args[0].shape[1]), "distinct_points": int(dedup[1][-1]),
            "comparisons": int(dedup[4][-1]), "reps": reps, "passes": passes, "routes": {}}
    text = []
    for r, _ in routes:
        med = statistics.median(times[r])
        line["routes"][r] = {"median_ms": 1e3 * med, "min_ms": 1e3 * min(times[r]),
                             "max_ms": 1e3 * max(times[r])}
        text.append("%-6s %-6s median %8.3f ms (min %.3f max %.3f) per call: %d sets x %d maps, %d samples "
                    "per set, %d distinct points, %d comparisons"
                    % (name, r, 1e3 * med, 1e3 * min(times[r]), 1e3 * max(times[r]), N_SETS, len(shapes),
                       args[0].shape[1], dedup[1][-1], dedup[4][-1]))
    line["values_over_u8"] = line["routes"]["values"]["median_ms"] / line["routes"]["u8"]["median_ms"]
    text.append("%-6s values / u8 = %.2f (medians)" % (name, line["values_over_u8"]))
    print("\n".join(text), file=sys.stderr)
    if out:
        with open(out, "a") as fh:
            fh.write("\n".join(text) + "\n")
    print(json.dumps(line))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--passes", type=int, default=3, help="calls per timed span")
    ap.add_argument("--limit", type=int, default=300, help="seconds a case may take")
    ap.add_argument("--case", choices=CASES, help="run one case in this process")
    ap.add_argument("--cases", default=",".join(CASES), help="comma-separated cases to run")
    ap.add_argument("--out", default=None, help="append the readable lines to this file")
    args = ap.parse_args()
    if args.case:
        return case(args.case, args.reps, args.passes, args.out)
    names = [c for c in args.cases.split(",") if c]
    if any(c not in CASES for c in names):
        ap.error("--cases: choose from %s" % ", ".join(CASES))
    for name in names:     # each GPU step in a fresh process under its own limit; a failure ends the run
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__),
               "--case", name, "--reps", str(args.reps), "--passes", str(args.passes)]
        rc = subprocess.call(cmd + (["--out", args.out] if args.out else []))
        if rc != 0:
            print("score_time: case %s ended with status %d; stopping" % (name, rc), file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
