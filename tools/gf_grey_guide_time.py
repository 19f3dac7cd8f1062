#!/usr/bin/env python
"""Guided filter with a grey guide, GF(CNN, CNN): 8 x 3840x2160 grey CNN-like maps filtered with
themselves as guidance, two forms alternated in one process -
    grey    guide [N,H,W,1] with RF_GF_GREY_AS_BGR (ops.guided_filter_u8(grey_as_bgr=True))
    colour  the same guide replicated to [N,H,W,3] through rf_gf_u8
at radius 52 / eps 7 (the reference tool's GF(CNN, CNN) recipe) and radius 45 / eps 3, 1 and 3
iterations.  Median of 7 event timings per form after warm-up; the two outputs are asserted byte-equal
at the timed size.  Prints one JSON line.

    python tools/gf_grey_guide_time.py [--lib PATH] [--reps 7] [--only grey|colour] [--cases r52i1,...]
                                       [--src grey|colour] [--one-stream]
(--only / --cases: one form / some cases alone, e.g. under rocprofv3 --kernel-trace --stats, with
 --one-stream so that kernel durations are those of kernels running alone.)
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = ((52, 7.0, 1), (52, 7.0, 3), (45, 3.0, 1), (45, 3.0, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="time this librf_hip.so instead of the package's")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--n", type=int, default=8)
    ap.add_argument("--only", choices=("grey", "colour"), default=None)
    ap.add_argument("--cases", default=None, help="comma-separated r<radius>i<iterations>")
    ap.add_argument("--src", choices=("grey", "colour"), default="grey",
                    help="grey: the map filters itself (1-channel src); colour: a photo-like src")
    ap.add_argument("--one-stream", action="store_true",
                    help="the whole batch on one stream (kernel times of kernels running alone)")
    args = ap.parse_args()
    import torch
    import bench
    from reflectance_filtering_amd import _ffi, ops
    if args.lib:
        _ffi.LIB_PATH = os.path.abspath(args.lib)
        sys.stderr.write("gf_grey_guide_time: loading %s\n" % _ffi.LIB_PATH)
    dev = torch.device("cuda:0")
    n, h, w = args.n, 2160, 3840
    scene, grey3 = bench.synth_batch(torch, n, h, w, 77, dev)
    g1 = grey3[..., :1].contiguous()        # the CNN map: one byte per pixel
    g3 = g1.repeat(1, 1, 1, 3).contiguous()  # ... as cv2.imread returns its PNG
    # filtered with itself (1-channel src, as the batch CLI sends it), or a colour src
    src = g1 if args.src == "grey" else scene
    if args.one_stream:
        _ffi.load_library().rf_debug_option(b"gf_one_stream", 1)
    out_g, out_c = torch.empty_like(src), torch.empty_like(src)
    ws = ops.gf_workspace(n, h, w, src.shape[3], 52, dev, torch)
    forms = {
        "grey": lambda r, e, it: ops.guided_filter_u8(g1, src, r, e, iterations=it, out=out_g,
                                                       workspace=ws, grey_as_bgr=True),
        "colour": lambda r, e, it: ops.guided_filter_u8(g3, src, r, e, iterations=it, out=out_c,
                                                         workspace=ws),
    }
    names = [args.only] if args.only else ["grey", "colour"]
    cases = CASES
    if args.cases:
        want = set(args.cases.split(","))
        cases = [c for c in CASES if "r%di%d" % (c[0], c[2]) in want]
    res = {"n": n, "h": h, "w": w, "src": args.src, "one_stream": args.one_stream, "reps": args.reps,
           "lib": os.path.basename(_ffi.LIB_PATH), "ms": {}}
    for r, e, it in cases:
        for name in names:            # warm-up: tables, side stream, clocks
            for _ in range(2):
                forms[name](r, e, it)
        torch.cuda.synchronize()
        times = {k: [] for k in names}
        for _ in range(args.reps):    # the forms alternate
            for name in names:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                forms[name](r, e, it)
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1))
        key = "r%d_eps%g_it%d" % (r, e, it)
        res["ms"][key] = {k: round(statistics.median(v), 3) for k, v in times.items()}
        if len(names) == 2:
            assert torch.equal(out_g, out_c), "grey-guide bytes differ from the replicated guide's: %s" % key
            res["ms"][key]["colour_over_grey"] = round(res["ms"][key]["colour"] / res["ms"][key]["grey"], 3)
    res["bytes_equal"] = len(names) == 2
    print(json.dumps(res))


if __name__ == "__main__":
    main()
