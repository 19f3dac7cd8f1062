#!/usr/bin/env python
"""Guided WHDR sweep over a list of mixed sizes: shape groups against one ragged call per pair.

64 synthetic grey CNN-like maps of the three common IIW shapes (341x512, 512x341, 384x512) in the
seeded order of tools/ragged_filter_time.py, device-resident, each with about 300 judged points, through
whdr.sweep('guided') over the grid eps {1, 3, 5, 7} x radius {45, 52}: GF(CNN, CNN) (the maps guide
themselves, grey_as_bgr) and a colour guide per map.  Two routes, the same scores (asserted equal):
    groups  whdr._sweep_batch per group of equal shapes (batch.group_by_shape), one uniform
            guided_filter_u8 batch per group and pair: the route a list took before the ragged sweep
            (that function is unchanged)
    pairs   whdr.sweep as it is: the list packed once, one ops.guided_filter_ragged_u8 call per pair
(A third route, one stage 1 shared by the eps of a radius, was timed with this tool and taken out:
profiles/gf_sweep_time.txt.)
Stacking / packing and the WHDR calls are inside the timed span for both: it is the sweep a caller
pays for.  After a warm-up of every route, the routes alternate --reps times, --passes sweeps per
timed span that ends in a device synchronise; the line gives median, min and max ms per sweep, filter
calls and filter-kernel launches per sweep (3 per uniform batch of one-channel images and per ragged
call, by the plan query).

Each case runs in a child process under its own time limit; a child that fails ends the run.  Prints
one JSON line per case.

    python tools/gf_sweep_time.py [--reps 9] [--passes 3] [--limit 300] [--cases self,colour]
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

CASES = ("self", "colour")
EPS = (1.0, 3.0, 5.0, 7.0)
RADII = (45, 52)
POINTS, COMPARISONS = 300, 450


def comparisons(h, w, rng):
    """IIW-like judgements in pixel coordinates over a pool of POINTS points."""
    import numpy as np
    pool = np.stack([rng.integers(0, w, POINTS), rng.integers(0, h, POINTS)], axis=1)
    a = pool[rng.integers(0, POINTS, COMPARISONS)]
    b = pool[rng.integers(0, POINTS, COMPARISONS)]
    return np.concatenate([a, b, rng.integers(0, 3, (COMPARISONS, 1)),
                           rng.random((COMPARISONS, 1)) + 0.05], axis=1).astype(np.float64)


def case(name, reps, passes):
    import numpy as np
    import torch
    from reflectance_filtering_amd import _ffi, batch, ops, whdr
    from tests import synth
    from tools.ragged_filter_time import list_shapes
    assert torch.cuda.is_available(), "gf_sweep_time.py needs a HIP device"
    grey = name == "self"
    shapes = list_shapes()
    rng = np.random.default_rng(11)
    maps = [torch.from_numpy(np.ascontiguousarray(synth.reflectance_like_u8(h, w, 100 + i)[:, :, :1])).cuda()
            for i, (h, w) in enumerate(shapes)]
    guides = maps if grey else [torch.from_numpy(synth.flat_guide_u8(h, w, 300 + i, cells=9)).cuda()
                                for i, (h, w) in enumerate(shapes)]
    comps = [comparisons(h, w, rng) for h, w in shapes]
    pairs = np.array([(e, r) for r in RADII for e in EPS], dtype=np.float64)
    gcn = 1 if grey else 3
    flags = _ffi.GF_GREY_AS_BGR if grey else 0
    pixels = sum(h * w for h, w in shapes)

    def groups():
        out = np.zeros((pairs.shape[0], len(shapes)))
        key = lambda i: tuple(maps[i].shape) + (gcn,)
        for run in batch.group_by_shape(sorted(range(len(shapes)), key=key), key, max_bytes=1 << 30):
            out[:, run] = whdr._sweep_batch("guided", torch.stack([maps[i] for i in run]),
                                            torch.stack([guides[i] for i in run]),
                                            [comps[i] for i in run], pairs, 0.1, grey)
        return out

    def per_pair():
        return whdr.sweep("guided", maps, guides, comps, pairs, grey_as_bgr=grey)

    routes = (("groups", groups), ("pairs", per_pair))
    first = {r: fn() for r, fn in routes}          # warm-up of every route, and the scores
    assert np.array_equal(first["groups"], first["pairs"]), "the ragged route differs from the shape groups"
    times = {r: [] for r, _ in routes}
    for _ in range(reps):
        for r, fn in routes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(passes):
                fn()
            torch.cuda.synchronize()
            times[r].append((time.perf_counter() - t0) / passes)
    plan = _ffi.gf_ragged_plan(shapes, gcn, 1, RADII[0], flags)
    assert plan is not None and plan["launches"] == 3, "the list did not take the ragged route"
    n_groups = len(set(shapes))
    calls = {"groups": n_groups * len(pairs), "pairs": len(pairs)}
    launches = {"groups": 3 * calls["groups"], "pairs": 3 * calls["pairs"]}
    line = {"tool": "gf_sweep_time", "case": name, "n": len(shapes), "pixels": pixels, "eps": list(EPS),
            "radii": list(RADII), "points_per_image": POINTS, "reps": reps, "passes": passes,
            "mean_whdr": first["pairs"].mean(axis=1).tolist(), "routes": {}}
    for r, _ in routes:
        med = statistics.median(times[r])
        line["routes"][r] = {"median_ms": 1e3 * med, "min_ms": 1e3 * min(times[r]),
                             "max_ms": 1e3 * max(times[r]), "filter_calls": calls[r],
                             "filter_launches": launches[r]}
        print("%-6s %-6s median %8.3f ms (min %.3f max %.3f) per sweep of %d pairs, %d filter call(s), "
              "%d filter launch(es)" % (name, r, 1e3 * med, 1e3 * min(times[r]), 1e3 * max(times[r]),
                                        len(pairs), calls[r], launches[r]), file=sys.stderr)
    print(json.dumps(line))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--passes", type=int, default=3, help="sweeps per timed span")
    ap.add_argument("--limit", type=int, default=300, help="seconds a case may take")
    ap.add_argument("--case", choices=CASES, help="run one case in this process")
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
            print("gf_sweep_time: case %s ended with status %d; stopping" % (name, rc), file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
