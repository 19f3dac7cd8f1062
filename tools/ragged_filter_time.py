#!/usr/bin/env python
"""Joint bilateral over a list of mixed sizes: equal-shape runs against the ragged call.

64 synthetic grey CNN-like maps of the three common IIW shapes (341x512, 512x341, 384x512) in a
seeded order whose equal-shape runs are 1 to 4 images long (a sorted IIW listing: no long run of
one shape), device-resident, BF(CNN, CNN) with grey_as_bgr at the paper's two bilateral recipes,
c20 s22 (radius 33) and c15 s28 (radius 42), and at two wider sigma_spatial of the slab kernel,
c20 s36 (radius 54) and c20 s66 (radius 99).  Two paths, in steps of 16 images (batch.py's step)
and over the whole list at once:
    runs    one ops.joint_bilateral_u8 call per run of equal shapes (batch.group_by_shape), the way
            batch.filter_files takes a step whose images differ in shape without the ragged entry
    ragged  one ops.joint_bilateral_ragged_u8 call per step
The batches of `runs` and the packs of `ragged` are built before the timed span: the span holds
the filter calls alone and ends in a device synchronise.  The two results are asserted equal.
After a warm-up of every shape, the paths alternate --reps times, --passes passes over the list
per timed span; the line gives median, min and max ms per pass over the list, MP/s of the median,
calls and kernel launches per pass (from the launch plan).

Each parameter set runs in a child process under its own time limit; a child that fails ends the
run.  Prints one JSON line per parameter set.

    python tools/ragged_filter_time.py [--reps 9] [--passes 3] [--limit 300] [--cases c20s36,c20s66]
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

CASES = {"c20s22": (20.0, 22.0), "c15s28": (15.0, 28.0), "c20s36": (20.0, 36.0), "c20s66": (20.0, 66.0)}
SHAPES = ((341, 512), (512, 341), (384, 512))
STEP = 16


def list_shapes(n=64, seed=3):
    """n shapes in runs of 1..4 equal ones, neighbouring runs of different shapes."""
    import numpy as np
    rng = np.random.default_rng(seed)
    out, last = [], -1
    while len(out) < n:
        k = int(rng.choice([i for i in range(len(SHAPES)) if i != last]))
        out.extend([SHAPES[k]] * int(rng.integers(1, 5)))
        last = k
    return out[:n]


def case(name, reps, passes):
    import numpy as np
    import torch
    from reflectance_filtering_amd import _ffi, batch, ops
    from tests import synth
    assert torch.cuda.is_available(), "ragged_filter_time.py needs a HIP device"
    sc, ss = CASES[name]
    shapes = list_shapes()
    maps = [torch.from_numpy(np.ascontiguousarray(synth.reflectance_like_u8(h, w, 100 + i)[:, :, :1])).cuda()
            for i, (h, w) in enumerate(shapes)]
    pixels = sum(h * w for h, w in shapes)
    line = {"tool": "ragged_filter_time", "case": name, "sigma_color": sc, "sigma_spatial": ss,
            "n": len(shapes), "pixels": pixels, "reps": reps, "passes": passes,
            "shape_runs": 1 + sum(a != b for a, b in zip(shapes, shapes[1:])), "paths": {}}

    def launches_of(sizes):
        plan = _ffi.jbf_ragged_plan(sizes, 1, 1, -1, sc, ss, _ffi.JBF_GREY_AS_BGR)
        if plan is not None:
            return len(plan)
        # no tile class: one slab launch over all images, or one launch per image
        slab = _ffi.jbf_ragged_slab_plan(sizes, 1, 1, -1, sc, ss, _ffi.JBF_GREY_AS_BGR)
        return len(sizes) if slab is None else 1

    for step_name, step in (("step16", STEP), ("one_call", len(shapes))):
        steps = [list(range(i, min(i + step, len(shapes)))) for i in range(0, len(shapes), step)]
        run_idx = [batch.group_by_shape(s, lambda i: shapes[i]) for s in steps]
        run_batches = [[torch.stack([maps[i] for i in run]) for run in runs] for runs in run_idx]
        packs = [(torch.cat([maps[i].view(-1, 1) for i in s]), [shapes[i] for i in s]) for s in steps]

        def by_runs():
            return [[ops.joint_bilateral_u8(b, b, -1, sc, ss, grey_as_bgr=True) for b in runs]
                    for runs in run_batches]

        def ragged():
            return [ops.joint_bilateral_ragged_u8(p, p, -1, sc, ss, grey_as_bgr=True, sizes=sizes)[1]
                    for p, sizes in packs]

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
        calls = {"runs": sum(len(r) for r in run_idx), "ragged": len(steps)}
        launches = {"runs": sum(launches_of([shapes[run[0]]]) for runs in run_idx for run in runs),
                    "ragged": sum(launches_of(sizes) for _, sizes in packs)}
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
    ap.add_argument("--limit", type=int, default=300, help="seconds a parameter set may take")
    ap.add_argument("--case", choices=sorted(CASES), help="run one parameter set in this process")
    ap.add_argument("--cases", default=",".join(CASES), help="comma-separated parameter sets to run")
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
            print("ragged_filter_time: case %s ended with status %d; stopping" % (name, rc),
                  file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
