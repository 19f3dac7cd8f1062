#!/usr/bin/env python
"""Decompose over a list of mixed sizes: one decompose_batch per equal-shape run against decompose_list.

64 synthetic photos of the three common IIW shapes (341x512, 512x341, 384x512) in the seeded order
of tools/ragged_filter_time.py, whose equal-shape runs are 1 to 4 images long (a sorted IIW listing:
no long run of one shape), device-resident.  Two paths, in steps of 16 images (batch.py's step) and
over the whole list at once:
    runs    one decompose_batch call per run of equal shapes (batch.group_by_shape), the way
            batch.decompose_files takes a step whose images differ in shape without the list form:
            one CNN launch and the 18 colourise launches per run
    list    one decompose_list call per step: one pack, one CNN launch, 18 ragged colourise launches
The stacked batches of `runs` are built before the timed span; the pack of `list` is part of
decompose_list and is timed with it.  The span ends in a device synchronise.  The two results are
asserted equal, r bit for bit.  After a warm-up of every shape, the paths alternate --reps times,
--passes passes over the list per timed span; the line gives median, min and max ms per pass over
the list, MP/s of the median, calls and kernel launches per pass (torch.cat of the pack included).

--chunk-px times decompose_list again under each listed value of the debug option
"colorize_chunk_px" (pixels per workgroup chunk of the ragged colourise; 0 = the plan rule), in the
same alternation.  Runs in a child process under a time limit; writes the JSON line to --out too.

    python tools/decompose_list_time.py [--reps 9] [--passes 3] [--chunk-px 512,1024,4096]
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

from tools.ragged_filter_time import STEP, list_shapes  # noqa: E402

COLORIZE_LAUNCHES = 18          # init, 8 x (histogram + pick), write: uniform and ragged entry alike


def measure(reps, passes, chunks):
    import numpy as np
    import torch
    from reflectance_filtering_amd import _ffi, batch
    from reflectance_filtering_amd import decompose_with_trained_CNN as dc
    from tests import synth
    assert torch.cuda.is_available(), "decompose_list_time.py needs a HIP device"
    shapes = list_shapes()
    photos = [torch.from_numpy(synth.scene_u8(h, w, 200 + i)).cuda() for i, (h, w) in enumerate(shapes)]
    pixels = sum(h * w for h, w in shapes)
    line = {"tool": "decompose_list_time", "n": len(shapes), "pixels": pixels, "reps": reps,
            "passes": passes, "shape_runs": 1 + sum(a != b for a, b in zip(shapes, shapes[1:])),
            "paths": {}}

    for step_name, step in (("step16", STEP), ("one_call", len(shapes))):
        steps = [list(range(i, min(i + step, len(shapes)))) for i in range(0, len(shapes), step)]
        run_idx = [batch.group_by_shape(s, lambda i: shapes[i]) for s in steps]
        run_batches = [[torch.stack([photos[i] for i in run]) for run in runs] for runs in run_idx]
        lists = [[photos[i] for i in s] for s in steps]
        plans = [_ffi.colorize_ragged_plan([shapes[i] for i in s]) for s in steps]

        def by_runs():
            return [[dc.decompose_batch(b) for b in runs] for runs in run_batches]

        def as_list(chunk_px=0):
            with _ffi.debug_options(colorize_chunk_px=chunk_px):
                return [dc.decompose_list(p) for p in lists]

        a, b = by_runs(), as_list()             # warm-up of every shape, and the results
        for runs, outs, got, s in zip(run_idx, a, b, steps):
            flat = {i: [t[k] for t in outs[r]] for r, run in enumerate(runs) for k, i in enumerate(run)}
            for pos, i in enumerate(s):
                want_r, want_r8, want_refl, want_shad = flat[i]
                assert torch.equal(got[0][pos].view(torch.int32), want_r.view(torch.int32)), "r differs"
                assert torch.equal(got[1][pos], want_r8) and torch.equal(got[2][pos], want_refl)
                assert torch.equal(got[3][pos], want_shad), "list differs from runs"
        del a, b
        paths = [("runs", by_runs), ("list", as_list)]
        for c in chunks:
            paths.append(("list_chunk%d" % c, lambda c=c: as_list(c)))
            paths[-1][1]()                      # (same bytes under every chunk length: tests)
        times = {name: [] for name, _ in paths}
        for _ in range(reps):
            for name, fn in paths:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(passes):
                    fn()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) / passes)
        n_runs = sum(len(r) for r in run_idx)
        for name, _ in paths:
            calls = n_runs if name == "runs" else len(steps)
            # per call: the CNN, the colourise launches; the list form also packs (one torch.cat)
            launches = calls * (1 + COLORIZE_LAUNCHES) + (0 if name == "runs" else calls)
            med = statistics.median(times[name])
            row = {"median_ms": 1e3 * med, "min_ms": 1e3 * min(times[name]),
                   "max_ms": 1e3 * max(times[name]), "mp_per_s": pixels / med / 1e6, "calls": calls,
                   "launches": launches}
            if name == "list":
                row["chunk_px"] = [p[0] for p in plans]
                row["workgroups"] = [p[1] for p in plans]
            line["paths"]["%s_%s" % (step_name, name)] = row
            print("%-8s %-16s median %8.3f ms (min %.3f max %.3f) %7.1f MP/s, %d call(s), %d launch(es)"
                  % (step_name, name, 1e3 * med, 1e3 * min(times[name]), 1e3 * max(times[name]),
                     pixels / med / 1e6, calls, launches), file=sys.stderr)
        line["paths"]["%s_ratio_runs_over_list" % step_name] = (
            statistics.median(times["runs"]) / statistics.median(times["list"]))
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--passes", type=int, default=3, help="passes over the list per timed span")
    ap.add_argument("--limit", type=int, default=300, help="seconds the measurement may take")
    ap.add_argument("--chunk-px", default="", help="comma-separated colorize_chunk_px values to time too")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decompose_list_time.json"))
    ap.add_argument("--child", action="store_true", help="measure in this process")
    args = ap.parse_args()
    chunks = [int(c) for c in args.chunk_px.split(",") if c]
    if any(c <= 0 or c % 256 for c in chunks):
        ap.error("--chunk-px: positive multiples of 256")
    if args.child:
        text = json.dumps(measure(args.reps, args.passes, chunks))
        print(text)
        with open(args.out, "w") as f:
            f.write(text + "\n")
        return 0
    # the GPU step in a fresh process under its own limit
    rc = subprocess.call(["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__),
                          "--child", "--reps", str(args.reps), "--passes", str(args.passes),
                          "--chunk-px", args.chunk_px, "--out", args.out])
    if rc != 0:
        print("decompose_list_time: ended with status %d" % rc, file=sys.stderr)
    return rc


if __name__ == "__main__":
    sys.exit(main())
