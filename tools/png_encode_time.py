#!/usr/bin/env python
"""PNG encode on the device against the host encoder: the op alone, and the batch tools file to file.

Three steps, each in a child process of its own under its own time limit, chained (a step that
fails ends the run); every line goes to stderr and to --out:

  device     ops.png_encode_ragged_u8 between two device events (the op reads its streams back,
             so the span holds the three launches, both copies and the container) and its C entry
             alone (the table upload and the three launches), after a warm-up, --reps times: the
             three outputs of decompose_packed over the 64-photo list of
             tools/decompose_list_time.py (r8 and shading grey, reflectance colour), each in one
             call, and 16 x 1080p BGR in one call.  Beside it image_utils._png_encode of the
             same arrays on batch.IO_THREADS threads (wall clock), and the size of both outputs.
  decompose  batch.decompose_files over the 64 photos as files, --png_encoder host and device
             alternating, --reps times each in one process (wall clock, file to file)
  filter     batch.filter_files over the 96 x 1080p case of tools/batch_pipeline_time.py (bilateral
             20 / 22, grey predictions with colour guidance), alternating in the same way

Medians, and the spread of the repeats as min and max.

    python tools/png_encode_time.py [--reps 5] [--files 96] [--steps device,decompose,filter]
"""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LIMITS = {"device": 240, "decompose": 240, "filter": 420}     # seconds per step


def say(out, text):
    print(text, file=sys.stderr)
    with open(out, "a") as fh:
        fh.write(text + "\n")


def spread(times):
    return "median %9.3f ms (min %.3f max %.3f)" % (1e3 * statistics.median(times), 1e3 * min(times),
                                                    1e3 * max(times))


def step_device(reps, out):
    import numpy as np
    import torch
    from reflectance_filtering_amd import _ffi, batch, ops
    from reflectance_filtering_amd import decompose_with_trained_CNN as dc
    from reflectance_filtering_amd import image_utils as iu
    from tests import synth
    from tools.ragged_filter_time import list_shapes
    lib = _ffi.load_library()
    shapes = list_shapes()
    photos = [torch.from_numpy(synth.scene_u8(h, w, 200 + i)).cuda() for i, (h, w) in enumerate(shapes)]
    sizes, _, r8, refl, shad = dc.decompose_packed(photos)
    hd = torch.from_numpy(np.stack([synth.scene_u8(1080, 1920, 300 + i) for i in range(16)])).cuda()
    cases = [("64 photos, r8 (grey)", r8.reshape(-1, 1), sizes),
             ("64 photos, reflectance (colour)", refl.reshape(-1, 3), sizes),
             ("64 photos, shading (grey)", shad.reshape(-1, 1), sizes),
             ("16 x 1080p BGR", hd.reshape(-1, 3), np.array([(1080, 1920)] * 16))]
    with ThreadPoolExecutor(max_workers=batch.IO_THREADS) as pool:
        for name, packed, sz in cases:
            views = [v.cpu().numpy() for v in ops.split_packed(packed, sz)]
            arrays = [v[:, :, 0] if v.shape[2] == 1 else v for v in views]
            files = ops.png_encode_ragged_u8(packed, sizes=sz)                       # warm-up
            host = list(pool.map(iu._png_encode, arrays))
            for data, arr in zip(files[:4], arrays[:4]):
                want = arr if arr.ndim == 3 else np.repeat(arr[:, :, None], 3, axis=2)
                assert np.array_equal(iu._png_decode(data), want), "the device file decodes to other pixels"
            dev_t, host_t, kern_t = [], [], []
            hs = np.ascontiguousarray(np.asarray(sz)[:, 0], dtype=np.int32)
            wd = np.ascontiguousarray(np.asarray(sz)[:, 1], dtype=np.int32)
            args = (len(hs), hs.ctypes.data, wd.ctypes.data, int(packed.shape[1]), 0)
            bound, need = lib.rf_png_stream_bound(*args), lib.rf_png_workspace_bytes(*args)
            streams = torch.empty(bound, dtype=torch.uint8, device="cuda")
            offsets = torch.empty(len(hs) + 1, dtype=torch.int64, device="cuda")
            ws = torch.empty(need, dtype=torch.uint8, device="cuda")
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                ops.png_encode_ragged_u8(packed, sizes=sz)
                e1.record()
                e1.synchronize()
                dev_t.append(e0.elapsed_time(e1) / 1e3)
                t0 = time.perf_counter()
                list(pool.map(iu._png_encode, arrays))
                host_t.append(time.perf_counter() - t0)
                k0, k1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                k0.record()
                rc = lib.rf_png_deflate_ragged_u8(packed.data_ptr(), args[0], args[1], args[2], args[3], 0,
                                                  streams.data_ptr(), bound, offsets.data_ptr(),
                                                  ws.data_ptr(), need, _ffi.current_stream_ptr(torch))
                k1.record()
                k1.synchronize()
                assert rc == 0, lib.rf_last_error()
                kern_t.append(k0.elapsed_time(k1) / 1e3)
            mp = packed.shape[0] / 1e6
            say(out, "%-32s op %s %6.0f MP/s | its C entry alone %s %6.0f MP/s | host, %d threads %s %6.0f MP/s "
                     "| bytes device / host %.4f"
                % (name, spread(dev_t), mp / statistics.median(dev_t), spread(kern_t),
                   mp / statistics.median(kern_t), batch.IO_THREADS, spread(host_t),
                   mp / statistics.median(host_t), sum(map(len, files)) / sum(map(len, host))))


def alternate(out, name, pixels, reps, run):
    """run(encoder, directory) file to file, host and device alternating after a warm-up of both."""
    import torch
    from reflectance_filtering_amd import batch
    times = {"host": [], "device": []}
    dirs = {enc: tempfile.mkdtemp() for enc in times}
    for enc in times:
        run(enc, dirs[enc])
    for _ in range(reps):
        for enc in times:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(enc, dirs[enc])
            torch.cuda.synchronize()
            times[enc].append(time.perf_counter() - t0)
    for enc in times:
        say(out, "%-44s --png_encoder %-6s %s %7.1f MP/s file to file (%d I/O threads)"
            % (name, enc, spread(times[enc]), pixels / 1e6 / statistics.median(times[enc]),
               batch.IO_THREADS))
    say(out, "%-44s host / device = %.2f" % (name, statistics.median(times["host"])
                                             / statistics.median(times["device"])))


def step_decompose(reps, out):
    from reflectance_filtering_amd import batch
    from reflectance_filtering_amd import image_utils as iu
    from tests import synth
    from tools.ragged_filter_time import list_shapes
    shapes = list_shapes()
    src = tempfile.mkdtemp()
    files = []
    for i, (h, w) in enumerate(shapes):
        files.append(os.path.join(src, "p%03d.png" % i))
        iu.imwrite(files[-1], synth.scene_u8(h, w, 200 + i))
    alternate(out, "decompose_files, %d mixed-shape photos" % len(shapes), sum(h * w for h, w in shapes),
              reps, lambda enc, d: batch.decompose_files(files, d, rank=0, world=1, png_encoder=enc))


def step_filter(reps, out, n):
    import numpy as np
    from reflectance_filtering_amd import batch
    from reflectance_filtering_amd import image_utils as iu
    from tests import synth
    h, w = 1080, 1920
    src = tempfile.mkdtemp()

    def make(i):
        iu.imwrite(os.path.join(src, "p%03d.png" % i), synth.scene_u8(h, w, seed=i))
        g = synth.reflectance_like_u8(h, w, seed=100 + i)
        iu.imwrite(os.path.join(src, "p%03d-r.png" % i), np.repeat(g[..., :1], 3, axis=2))

    with ThreadPoolExecutor(max_workers=batch.IO_THREADS) as pool:
        list(pool.map(make, range(n)))
    files = batch.expand_inputs([os.path.join(src, "*-r.png")])
    pattern = os.path.join(src, "{base}.png")
    alternate(out, "filter_files bilateral, %d x %dx%d" % (n, w, h), n * h * w, reps,
              lambda enc, d: batch.filter_files("bilateral", files, pattern, 20.0, 22.0, d, rank=0,
                                                world=1, png_encoder=enc))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="repeats per encoder (at least 5)")
    ap.add_argument("--files", type=int, default=96, help="1080p files of the filter step")
    ap.add_argument("--steps", default="device,decompose,filter")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_encode_time.txt"))
    ap.add_argument("--child", default="", help="run this step in this process")
    args = ap.parse_args()
    if args.child:
        import torch
        assert torch.cuda.is_available(), "png_encode_time.py needs a HIP device"
        torch.cuda.set_device(0)
        if args.child == "device":
            step_device(args.reps, args.out)
        elif args.child == "decompose":
            step_decompose(args.reps, args.out)
        else:
            step_filter(args.reps, args.out, args.files)
        return 0
    steps = [s for s in args.steps.split(",") if s]
    if any(s not in LIMITS for s in steps) or args.reps < 5:
        ap.error("--steps: device, decompose, filter; --reps: 5 or more")
    open(args.out, "w").close()
    for s in steps:      # each GPU step in a fresh process under its own limit; the first failure ends the run
        rc = subprocess.call(["timeout", "-k", "10", str(LIMITS[s]), sys.executable, os.path.abspath(__file__),
                              "--child", s, "--reps", str(args.reps), "--files", str(args.files),
                              "--out", args.out])
        if rc != 0:
            print("png_encode_time: step %s ended with status %d" % (s, rc), file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
