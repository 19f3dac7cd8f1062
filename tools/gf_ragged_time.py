#!/usr/bin/env python
"""Guided filter over a list of mixed sizes: equal-shape runs against the ragged call.

64 synthetic grey CNN-like maps of the three common IIW shapes (341x512, 512x341, 384x512) in the
seeded order of tools/ragged_filter_time.py, whose equal-shape runs are 1 to 4 images long, device-
resident, through the reference's two guided recipes: GF(CNN, CNN) at c7 s52 (the maps guide
themselves, grey_as_bgr) and GF(CNN, flat) at c3 s45 (a colour guide per map), 1 and 3 iterations.
Two paths, in steps of 16 images (batch.py's step) and over the whole list at once:
    runs    one filter_reflectance.apply_filter_batch call per run of equal shapes
            (batch.group_by_shape): what a guided list cost before the ragged entry
    ragged  one ops.guided_filter_ragged_u8 call per step
The batches of `runs` and the packs of `ragged` are built before the timed span: the span holds the
filter calls alone and ends in a device synchronise.  The two results are asserted equal.  After a
warm-up of every shape, the paths alternate --reps times, --passes passes over the list per timed
span; the line gives median, min and max ms per pass over the list, MP/s of the median, calls and
kernel launches per pass (3 per iteration for a ragged call by its plan and for a batch of fewer than
eight one-channel images by the launches of rf_gf_ex_u8: stage 1, row walk, column walk).

Each case runs in a child process under its own time limit; a child that fails ends the run.  Prints
one JSON line per case.

    python tools/gf_ragged_time.py [--reps 9] [--passes 3] [--limit 300] [--cases c7s52x1,c3s45x3]
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

# name: (sigma_color = eps, sigma_spatial = radius, guide, iterations)
CASES = {"c7s52x1": (7.0, 52.0, "self", 1), "c7s52x3": (7.0, 52.0, "self", 3),
         "c3s45x1": (3.0, 45.0, "colour", 1), "c3s45x3": (3.0, 45.0, "colour", 3)}
STEP = 16


def case(name, reps, passes):
    import numpy as np
    import torch
    from reflectance_filtering_amd import _ffi, batch, ops
    from reflectance_filtering_amd import filter_reflectance as fr
    from tests import synth
    from tools.ragged_filter_time import list_shapes
    assert torch.cuda.is_available(), "gf_ragged_time.py needs a HIP device"
    sc, ss, guide_kind, iterations = CASES[name]
    grey = guide_kind == "self"
    shapes = list_shapes()
    maps = [torch.from_numpy(np.ascontiguousarray(synth.reflectance_like_u8(h, w, 100 + i)[:, :, :1])).cuda()
            for i, (h, w) in enumerate(shapes)]
    guides = maps if grey else [torch.from_numpy(synth.flat_guide_u8(h, w, 300 + i, cells=9)).cuda()
                                for i, (h, w) in enumerate(shapes)]
    gcn = 1 if grey else 3
    pixels = sum(h * w for h, w in shapes)
    line = {"tool": "gf_ragged_time", "case": name, "sigma_color": sc, "sigma_spatial": ss,
            "guide": guide_kind, "iterations": iterations, "n": len(shapes), "pixels": pixels,
            "reps": reps, "passes": passes,
            "shape_runs": 1 + sum(a != b for a, b in zip(shapes, shapes[1:])), "paths": {}}

    for step_name, step in (("step16", STEP), ("one_call", len(shapes))):
        steps = [list(range(i, min(i + step, len(shapes)))) for i in range(0, len(shapes), step)]
        run_idx = [batch.group_by_shape(s, lambda i: shapes[i]) for s in steps]
        run_batches = [[(torch.stack([maps[i] for i in run]), torch.stack([guides[i] for i in run]))
                        for run in runs] for runs in run_idx]
        packs = []
        for s in steps:
            src = torch.cat([maps[i].view(-1, 1) for i in s])
            gui = src if grey else torch.cat([guides[i].view(-1, 3) for i in s])
            packs.append((gui, src, [shapes[i] for i in s]))

        def by_runs():
            return [[fr.apply_filter_batch("guided", m, g, sc, ss, iterations=iterations, grey_as_bgr=grey)
                     for m, g in runs] for runs in run_batches]

        def ragged():
            return [ops.guided_filter_ragged_u8(g, p, int(ss), sc, iterations=iterations,
                                                grey_as_bgr=grey, sizes=sizes)[1]
                    for g, p, sizes in packs]

        a, b = by_runs(), ragged()              # warm-up of every shape, and the bytes
        for runs, outs, views, s in zip(run_idx, a, b, steps):
            flat = {i: outs[r][k] for r, run in enumerate(runs) for k, i in enumerate(run)}
            assert all(torch.equal(flat[i], v) for i, v in zip(s, views)), "ragged differs from runs"
        del a, b
        times = {"runs": [], "ragged": []}
        for _ in range(reps):
            for path, fn in (("runs", by_runs), ("ragged", ragged)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(passes):
                    fn()
                torch.cuda.synchronize()
                times[path].append((time.perf_counter() - t0) / passes)
        for g, p, sizes in packs:
            plan = _ffi.gf_ragged_plan(sizes, gcn, 1, int(ss), _ffi.GF_GREY_AS_BGR if grey else 0)
            assert plan is not None and plan["launches"] == 3, "the list did not take the ragged route"
        calls = {"runs": sum(len(r) for r in run_idx), "ragged": len(steps)}
        launches = {"runs": 3 * iterations * calls["runs"], "ragged": 3 * iterations * calls["ragged"]}
        for path in ("runs", "ragged"):
            med = statistics.median(times[path])
            line["paths"]["%s_%s" % (step_name, path)] = {
                "median_ms": 1e3 * med, "min_ms": 1e3 * min(times[path]),
                "max_ms": 1e3 * max(times[path]), "mp_per_s": pixels / med / 1e6,
                "calls": calls[path], "launches": launches[path]}
            print("%s %-8s %-6s median %8.3f ms (min %.3f max %.3f) %7.1f MP/s, %d call(s), %d launch(es)"
                  % (name, step_name, path, 1e3 * med, 1e3 * min(times[path]), 1e3 * max(times[path]),
                     pixels / med / 1e6, calls[path], launches[path]), file=sys.stderr)
    print(json.dumps(line))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--passes", type=int, default=3, help="passes over the list per timed span")
    ap.add_argument("--limit", type=int, default=300, help="seconds a case may take")
    ap.add_argument("--case", choices=sorted(CASES), help="run one case in this process")
    ap.add_argument("--cases", default=",".join(CASES), help="comma-separated cases to run")
    args = ap.parse_args()
    if args.case:
        return case(args.case, args.reps, args.passes)
    names = [c for c in args.cases.split(",") if c]
    if any(c not in CASES for c in names):
        ap.error("--cases: choose from %s" % ", ".join(CASES))
    for name in names:     # each GPU step in a fresh process under its own limit; a failure ends the run
        rc = subprocess.call(["timeout", "-k", "10", str(args.limit), sys.executable,
                              os.path.abspath(__file__), "--case", name, "--reps", str(args.reps),
                              "--passes", str(args.passes)])
        if rc != 0:
            print("gf_ragged_time: case %s ended with status %d; stopping" % (name, rc),
                  file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
