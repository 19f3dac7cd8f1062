#!/usr/bin/env python
"""WHDR sweep, bilateral half: the point path against full passes.

On N synthetic photo-size grey CNN-like maps (default 8 x 384x512, about an IIW photo) with a few
hundred random judgement points each (IIW-like: comparisons sharing points), two grids:
    s22    sigma_color 10,15,20,25 x sigma_spatial 22          (radius 33)
    s66_88 sigma_color 10,15,20,25 x sigma_spatial 66,77,88    (radii 99 .. 132)
and two ways to get the WHDR of every (image, pair), BF(CNN, CNN):
    points  whdr.sweep('bilateral', ...): rf_jbf_points_u8 at the deduplicated points + rf_whdr_points_u8
    full    per pair one rf_jbf_u8 pass over the batch (grey_as_bgr) + whdr_batch on float bytes / 255
            (the float conversion is done on the host, outside the timed span, as a plain user would
            not do it on the device either: the span is filter + metric launches only)
The two WHDR matrices are asserted equal.  Wall time per sweep (median of --reps after a warm-up,
each ending in a device synchronise).  Prints one JSON line.

--mixed times the list path instead: 64 grey maps alternating 341x512 and 512x341 in list order
with a few 384x512 among them (a sorted IIW listing: no long run of one shape), the same points
per image and the same two grids, through whdr.sweep on the list.  Beside the time it prints how
many point-filter calls the sweep made (one per pack with the ragged entry, one per equal-shape
run without it) and the points per wave of every chunk of every call, from the launch plan.  It
uses nothing newer than whdr.sweep on lists, so one copy of it times any two commits.

    python tools/sweep_time.py [--n 8] [--h 384] [--w 512] [--points 300] [--reps 5] [--mixed]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GRIDS = {"s22": ([10, 15, 20, 25], [22]), "s66_88": ([10, 15, 20, 25], [66, 77, 88])}


def judgements(rng, h, w, points):
    """IIW-like comparisons in pixel coordinates: 2 * points comparisons sharing `points` points."""
    import numpy as np
    pool = np.stack([rng.integers(0, w, points), rng.integers(0, h, points)], axis=1)
    m = 2 * points
    a, b = pool[rng.integers(0, points, m)], pool[rng.integers(0, points, m)]
    return np.concatenate([a, b, rng.integers(0, 3, (m, 1)), rng.random((m, 1))],
                          axis=1).astype(np.float64)


def mixed_shapes(n=64):
    """Alternating 341x512 / 512x341, every 16th image 384x512."""
    return [(384, 512) if i % 16 == 7 else ((341, 512), (512, 341))[i % 2] for i in range(n)]


def mixed(args):
    import numpy as np
    import torch
    from reflectance_filtering_amd import _ffi, ops, whdr
    from tests import synth
    assert torch.cuda.is_available(), "sweep_time.py needs a HIP device"
    rng = np.random.default_rng(1)
    shapes = mixed_shapes()
    maps = [np.ascontiguousarray(synth.reflectance_like_u8(h, w, 100 + i)[:, :, :1])
            for i, (h, w) in enumerate(shapes)]
    comps = [judgements(rng, h, w, args.points) for h, w in shapes]
    dev = [torch.from_numpy(m).cuda() for m in maps]
    calls = []                               # points of every point-filter call of a sweep

    def counted(name):
        real = getattr(ops, name, None)
        if real is not None:
            def wrapper(joint, src, points, *a, **kw):
                calls.append(int(np.asarray(points).reshape(-1, 2).shape[0]))
                return real(joint, src, points, *a, **kw)
            setattr(ops, name, wrapper)

    counted("joint_bilateral_points_u8")
    counted("joint_bilateral_points_ragged_u8")

    def run(pairs):
        return whdr.sweep("bilateral", dev, dev, comps, pairs, grey_as_bgr=True)

    line = {"tool": "sweep_time", "case": "mixed", "n": len(shapes), "points_per_image": args.points,
            "shape_runs": 1 + sum(a != b for a, b in zip(shapes, shapes[1:])), "grids": {}}
    for name, (cs, ss) in GRIDS.items():
        pairs = [(c, s) for c in cs for s in ss]
        got = run(pairs)
        del calls[:]
        one = np.stack([whdr.sweep("bilateral", d[None], d[None], [c], pairs, grey_as_bgr=True)[:, 0]
                        for d, c in zip(dev[:6], comps[:6])], axis=1)
        assert np.array_equal(got[:, :6], one), "list sweep differs from per-image sweeps"
        del calls[:]
        run(pairs)
        per_sweep = list(calls)
        ppw = sorted({c[2] for total in per_sweep
                      for c in _ffi.jbf_points_plan([s for _, s in pairs], -1, 1,
                                                    _ffi.JBF_GREY_AS_BGR, total)})
        ts = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(pairs)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        line["grids"][name] = {"pairs": len(pairs), "list_s": statistics.median(ts),
                               "min_s": min(ts), "max_s": max(ts), "calls": len(per_sweep),
                               "points": sum(per_sweep), "ppw": ppw}
        print("%-7s %2d pairs: list sweep %.4f s in %d call(s), %d points, ppw %s"
              % (name, len(pairs), statistics.median(ts), len(per_sweep), sum(per_sweep), ppw),
              file=sys.stderr)
    print(json.dumps(line))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8)
    ap.add_argument("--h", type=int, default=384)
    ap.add_argument("--w", type=int, default=512)
    ap.add_argument("--points", type=int, default=300, help="distinct judgement points per image")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--mixed", action="store_true", help="the mixed-size list case (64 maps)")
    args = ap.parse_args()
    if args.mixed:
        return mixed(args)
    import numpy as np
    import torch
    from reflectance_filtering_amd import ops, whdr
    from tests import synth
    assert torch.cuda.is_available(), "sweep_time.py needs a HIP device"
    rng = np.random.default_rng(0)
    n, h, w = args.n, args.h, args.w
    maps = np.stack([synth.reflectance_like_u8(h, w, 100 + i)[:, :, :1] for i in range(n)])
    comps = []
    for _ in range(n):
        pool = np.stack([rng.integers(0, w, args.points), rng.integers(0, h, args.points)], axis=1)
        m = 2 * args.points
        a, b = pool[rng.integers(0, args.points, m)], pool[rng.integers(0, args.points, m)]
        comps.append(np.concatenate([a, b, rng.integers(0, 3, (m, 1)), rng.random((m, 1))],
                                    axis=1).astype(np.float64))
    r1 = torch.from_numpy(np.ascontiguousarray(maps)).cuda()
    distinct = whdr.dedup_points(comps, h, w)[1][-1]

    def points(pairs):
        return whdr.sweep("bilateral", r1, r1, comps, pairs, grey_as_bgr=True)

    def full(pairs):
        res = []
        for sc, ss in pairs:
            f = ops.joint_bilateral_u8(r1, r1, -1, sc, ss, grey_as_bgr=True).cpu().numpy()
            planar = np.ascontiguousarray(np.transpose(f, (0, 3, 1, 2)))
            refl = torch.from_numpy(planar.astype(np.float32) / np.float32(255)).cuda()
            res.append(whdr.whdr_batch(refl, comps))
        return np.stack(res)

    def full_device_span(pairs):
        """Filter + metric launches only (the float images are prepared outside the span)."""
        spans, res = 0.0, []
        for sc, ss in pairs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f = ops.joint_bilateral_u8(r1, r1, -1, sc, ss, grey_as_bgr=True)
            torch.cuda.synchronize()
            spans += time.perf_counter() - t0
            planar = np.ascontiguousarray(np.transpose(f.cpu().numpy(), (0, 3, 1, 2)))
            refl = torch.from_numpy(planar.astype(np.float32) / np.float32(255)).cuda()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res.append(whdr.whdr_batch(refl, comps))
            spans += time.perf_counter() - t0
        return spans, np.stack(res)

    def timed(fn, pairs):
        fn(pairs)
        ts = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(pairs)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts)

    line = {"tool": "sweep_time", "n": n, "h": h, "w": w, "points_per_image": args.points,
            "distinct_points": int(distinct), "pixels": n * h * w, "grids": {}}
    for name, (cs, ss) in GRIDS.items():
        pairs = [(c, s) for c in cs for s in ss]
        a, b = points(pairs), full(pairs)
        assert np.array_equal(a, b), "point sweep differs from the full-pass pipeline"
        t_points = timed(points, pairs)
        full_device_span(pairs)
        spans = statistics.median(full_device_span(pairs)[0] for _ in range(args.reps))
        line["grids"][name] = {"pairs": len(pairs), "points_s": t_points, "full_s": spans,
                               "speedup": spans / t_points}
        print("%-7s %2d pairs: points %.4f s, full passes %.4f s (x%.1f)"
              % (name, len(pairs), t_points, spans, spans / t_points), file=sys.stderr)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
