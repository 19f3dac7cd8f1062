#!/usr/bin/env python
"""Time the CNN forward on uint8 input (rf_cnn_reflectance_u8) and on float32 input in both layouts
(rf_cnn_reflectance_f32: planar NCHW RGB, interleaved NHWC BGR), alternating in one process on the
shape tools/cnn_ab.py uses, and - with --parent-lib - the u8 entry of another build of librf_hip.so
(the parent commit's) in the same rounds.  Further paths after a comma are timed the same way, e.g. a
second copy of either build as a control: what two loads of the same code differ by.

    python tools/cnn_f32_time.py [--batch 256] [--repeats 5] [--rounds 12] [--calls 4] [--parent-lib old.so[,control.so...]]
                                 [--out profiles/cnn_f32_time.txt]

A repeat is `rounds` rounds of one call per variant, in turn, the round's first variant rotating; its
figure for a variant is the median time per call (device events around `calls` calls enqueued back to
back, each weight pack + forward: the device stays busy, so the host's launch latency after an idle
device is not part of the figure).  Reported per variant: the rate of
every repeat, their minimum, median and maximum.  The float inputs hold the byte levels of the u8
input, so every variant computes the same pixels: the outputs are compared bit for bit.
"""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--calls", type=int, default=4, help="calls enqueued back to back per timing")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    import bench
    from reflectance_filtering_amd import _ffi, weights as W, image_utils as iu

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    n, h, w = args.batch, 333, 500
    scene, _ = bench.synth_batch(torch, n, h, w, 5002, dev)
    wts = torch.from_numpy(np.ascontiguousarray(W.load_weights())).to(dev)
    lut = torch.from_numpy(iu.srgb_byte_lut()).to(dev)
    nhwc = torch.empty((n, h, w, 3), dtype=torch.float32, device=dev)
    for lo in range(0, n, 16):                       # (in slices: the int64 index is 8x the bytes)
        nhwc[lo:lo + 16] = lut[scene[lo:lo + 16].long()]
    nchw = nhwc.flip(-1).permute(0, 3, 1, 2).contiguous()
    lib = _ffi.load_library()
    stream = _ffi.current_stream_ptr(torch)

    def u8_call(which):
        return lambda r, r8: which.rf_cnn_reflectance_u8(scene.data_ptr(), r.data_ptr(), r8.data_ptr(),
                                                         n, h, w, wts.data_ptr(), lut.data_ptr(), stream)

    def f32_call(x, layout):
        return lambda r, r8: lib.rf_cnn_reflectance_f32(x.data_ptr(), r.data_ptr(), r8.data_ptr(), n, h, w,
                                                        layout, wts.data_ptr(), stream)

    variants = [("u8", u8_call(lib)), ("f32 nchw_rgb", f32_call(nchw, _ffi.CNN_NCHW_RGB)),
                ("f32 nhwc_bgr", f32_call(nhwc, _ffi.CNN_NHWC_BGR))]
    for k, path in enumerate(filter(None, args.parent_lib.split(","))):
        other = ctypes.CDLL(path)
        other.rf_cnn_reflectance_u8.argtypes = lib.rf_cnn_reflectance_u8.argtypes
        other.rf_cnn_reflectance_u8.restype = ctypes.c_int
        label = "u8 (parent build)" if k == 0 else "u8 (%s)" % os.path.basename(path)
        variants.insert(1 + k, (label, u8_call(other)))
    # every variant writes the same two buffers, so no figure depends on where an output lies
    out = (torch.empty((n, h, w), dtype=torch.float32, device=dev),
           torch.empty((n, h, w), dtype=torch.uint8, device=dev))
    results = {}
    mpix = n * h * w / 1e6
    rates = {name: [] for name, _ in variants}
    for rep in range(args.repeats):
        times = {name: [] for name, _ in variants}
        for rnd in range(args.rounds + 1):           # round 0 warms up
            k = rnd % len(variants)                  # every variant takes every place in a round in turn
            for name, call in variants[k:] + variants[:k]:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                rcs = [call(*out) for _ in range(args.calls)]
                e1.record()
                torch.cuda.synchronize()
                assert not any(rcs), (name, rcs, lib.rf_last_error())
                if rnd:
                    times[name].append(e0.elapsed_time(e1) / args.calls)
                elif rep == 0:
                    results[name] = (out[0].clone(), out[1].clone())
        for name, _ in variants:
            ms = sorted(times[name])[len(times[name]) // 2]
            rates[name].append(mpix / ms)            # MP/ms = GP/s
    first = results[variants[0][0]]
    lines = ["CNN forward, %d x %d x %d (%.1f MP), %d repeats of %d alternating rounds; GP/s per repeat "
             "(median of the repeat's timings, each %d calls back to back between device events, a call = "
             "weight pack + forward)" % (n, h, w, mpix, args.repeats, args.rounds, args.calls),
             "device: %s" % torch.cuda.get_device_name(0)]
    for name, _ in variants:
        same = torch.equal(results[name][0], first[0]) and torch.equal(results[name][1], first[1])
        v = rates[name]
        lines.append("%-26s min %.2f  median %.2f  max %.2f GP/s   [%s]   identical_to_u8=%s"
                     % (name, min(v), sorted(v)[len(v) // 2], max(v), " ".join("%.2f" % x for x in v), same))
    if args.parent_lib:
        p, c = rates["u8 (parent build)"], rates["u8"]
        lines.append("u8, this build against the parent build: median %.2f vs %.2f GP/s (%+.2f %%); the parent's "
                     "repeats span %.2f..%.2f, this build's %.2f..%.2f -> this build's median is %s the "
                     "parent's run-to-run spread"
                     % (sorted(c)[len(c) // 2], sorted(p)[len(p) // 2],
                        100.0 * (sorted(c)[len(c) // 2] / sorted(p)[len(p) // 2] - 1.0), min(p), max(p), min(c),
                        max(c), "inside or above" if sorted(c)[len(c) // 2] >= min(p) else "BELOW"))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
