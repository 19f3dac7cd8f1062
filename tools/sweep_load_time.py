#!/usr/bin/env python
"""WHDR sweep from files, end to end: what the loader costs, and what a chain saves.

64 synthetic photos of the three IIW shapes of tools/sweep_time.py --mixed (341x512 and 512x341
alternating, every 16th 384x512) are written as PNG files with an IIW-style judgement file beside
each (--points distinct points, twice as many comparisons).  Two sweeps, each one pair, each timed
from the file names to the WHDR matrix on the host:
    bilateral  sigma_color 20, sigma_spatial 22    BF(CNN, CNN)
    guided     sigma_color 3,  sigma_spatial 45    GF(CNN, CNN)
through three loaders:
    serial   sweep.run of the parent commit, imported from --parent (a checkout of it that holds a
             built librf_hip.so): one image_utils.imread after another on the main thread
    threads  sweep.run, png_decoder="host": the same reads on batch.IO_THREADS threads
    device   sweep.run, png_decoder="device": the threads inflate, the device reconstructs the rows
The three matrices are asserted equal.  After one warm-up each, --reps alternating repeats
(serial, threads, device, serial, ...): median and min-max per loader.

The chain: 64 stored grey sources, the photos as guidance files, guided c3 s45 three times.
    chain   sweep.run(src_files, guidance_files, iterations=3): one read, three passes, every pass scored
    files   three single-pass `batch.py filter` runs (batch.filter_files), each reading the PNGs the run
            before wrote - the reference's chain of CLI runs; no pass is scored
The third slice of the chain is asserted equal to a single-pass sweep.run over the files the second
run wrote.  Same repeats.

Prints a table on stdout and one JSON line last.

    python tools/sweep_load_time.py --parent ../parent_checkout [--n 64] [--points 300] [--reps 5]
"""
import argparse
import importlib.util
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SWEEPS = (("bilateral", 20.0, 22.0), ("guided", 3.0, 45.0))


def parent_sweep(path):
    """The parent commit's sweep module, from a checkout at `path`, under a package name of its own
    (its relative imports stay inside that checkout, its library is the one built there)."""
    pkg = os.path.join(os.path.abspath(path), "reflectance_filtering_amd")
    spec = importlib.util.spec_from_file_location("rf_parent", os.path.join(pkg, "__init__.py"),
                                                  submodule_search_locations=[pkg])
    module = importlib.util.module_from_spec(spec)
    sys.modules["rf_parent"] = module
    spec.loader.exec_module(module)
    return importlib.import_module("rf_parent.sweep")


def write_inputs(work, n, points):
    import numpy as np
    from reflectance_filtering_amd import image_utils as iu
    from tests import synth
    from tools.sweep_time import judgements, mixed_shapes
    rng = np.random.default_rng(2)
    for d in ("photos", "src"):
        os.makedirs(os.path.join(work, d))
    photos = []
    for i, (h, w) in enumerate(mixed_shapes(n)):
        name = os.path.join(work, "photos", "%03d.png" % i)
        iu.imwrite(name, synth.scene_u8(h, w, 300 + i))
        iu.imwrite(os.path.join(work, "src", "%03d.png" % i), synth.reflectance_like_u8(h, w, 400 + i))
        pts, comparisons = [], []
        for row in judgements(rng, h, w, points):
            ids = []
            for x, y in ((row[0], row[1]), (row[2], row[3])):
                ids.append(len(pts))
                pts.append({"id": len(pts), "x": (x + 0.5) / w, "y": (y + 0.5) / h})
            comparisons.append({"point1": ids[0], "point2": ids[1], "darker": "E12"[int(row[4])],
                                "darker_score": float(row[5])})
        with open(os.path.splitext(name)[0] + ".json", "w") as fh:
            json.dump({"intrinsic_points": pts, "intrinsic_comparisons": comparisons}, fh)
        photos.append(name)
    return photos


def alternate(variants, reps, sync):
    """One warm-up each, then `reps` rounds over all variants in turn: {name: [seconds]}."""
    times = {name: [] for name, _ in variants}
    for name, fn in variants:
        fn()
    for _ in range(reps):
        for name, fn in variants:
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            times[name].append(time.perf_counter() - t0)
    return times


def report(title, times, line):
    print(title)
    for name, ts in times.items():
        print("    %-8s median %8.4f s   min %8.4f   max %8.4f   (%d repeats)"
              % (name, statistics.median(ts), min(ts), max(ts), len(ts)))
        line[name] = {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="checkout of the parent commit, library built")
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--points", type=int, default=300, help="distinct judgement points per image")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import numpy as np
    import torch
    from reflectance_filtering_amd import batch
    from reflectance_filtering_amd import sweep
    assert torch.cuda.is_available(), "sweep_load_time.py needs a HIP device"
    serial = parent_sweep(args.parent) if args.parent else None
    work = tempfile.mkdtemp(prefix="sweep_load_time_")
    line = {"tool": "sweep_load_time", "n": args.n, "points_per_image": args.points, "reps": args.reps,
            "io_threads": batch.IO_THREADS, "sweeps": {}}
    try:
        photos = write_inputs(work, args.n, args.points)
        print("%d photos, %d judgement points each, %d I/O threads%s"
              % (args.n, args.points, batch.IO_THREADS, "" if serial else "; no --parent: serial loader not timed"))
        for ftype, sc, ss in SWEEPS:
            got = {}

            def variant(name, fn):
                def call():
                    got[name] = fn()[1]
                return name, call

            variants = [variant("threads", lambda: sweep.run(photos, ftype, [sc], [ss])),
                        variant("device", lambda: sweep.run(photos, ftype, [sc], [ss], png_decoder="device"))]
            if serial:
                variants.insert(0, variant("serial", lambda: serial.run(photos, ftype, [sc], [ss])))
            times = alternate(variants, args.reps, torch.cuda.synchronize)
            for name in got:
                assert np.array_equal(got[name], got["threads"]), "%s loader: another matrix" % name
            entry = line["sweeps"][ftype] = {"sigma_color": sc, "sigma_spatial": ss}
            report("%s c%g s%g, from files:" % (ftype, sc, ss), times, entry)
        # the chain against chained file runs
        src, gui = os.path.join(work, "src", "{name}"), os.path.join(work, "photos", "{name}")
        sources = [sweep.file_for(f, src) for f in photos]
        # the outputs of a file run carry the parameter suffix: their guidance is found by stem
        flat = os.path.join(work, "flat")
        os.makedirs(flat)
        suffix = "_guided_c3.0s45.0"
        for f in photos:
            stem = os.path.splitext(os.path.basename(f))[0]
            for k in range(3):
                os.symlink(f, os.path.join(flat, stem + suffix * k + ".png"))
        result = {}

        def chain():
            result["chain"] = sweep.run(photos, "guided", [3.0], [45.0], src_files=src,
                                        guidance_files=gui, iterations=3)[1]

        def files():
            inputs = sources
            for k in range(3):
                out = os.path.join(work, "pass%d" % k)
                shutil.rmtree(out, ignore_errors=True)
                os.makedirs(out)
                inputs = batch.filter_files("guided", inputs, os.path.join(flat, "{name}"), 3.0, 45.0, out)

        times = alternate([("chain", chain), ("files", files)], args.reps, torch.cuda.synchronize)
        second = os.path.join(work, "pass1", "{stem}" + suffix * 2 + ".png")
        last = sweep.run(photos, "guided", [3.0], [45.0], src_files=second, guidance_files=gui)[1]
        assert np.array_equal(result["chain"][2], last), "the chain's third pass: another matrix"
        report("guided c3 s45 three times, stored sources:", times, line.setdefault("chain", {}))
    finally:
        shutil.rmtree(work, ignore_errors=True)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
