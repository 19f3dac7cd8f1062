#!/usr/bin/env python
"""PNG decode with the device's help against the host decoder: the decode alone, and the batch tools
file to file.

Three steps, each in a child process of its own under its own time limit, chained (a step that
fails ends the run); every line goes to stderr and to --out:

  decode     16 x 1080p colour photos written by Pillow (Paeth rows) plus 16 x 1080p grey maps written
             by image_utils._png_encode (Up rows), as files: image_utils.imread of all 32 on
             batch.IO_THREADS threads (wall clock) against reading and image_utils.png_parse of them
             on the same threads followed by one ops.png_decode_ragged_u8 call (wall clock, both
             parts and their sum), after a warm-up, --reps times, the two routes alternating.  The
             operator alone between two device events (staging copy, upload, three launches, the
             flags' way back) and its C entry alone on raw streams that are on the device already.
  filter     batch.filter_files over the 96 x 1080p case of tools/png_encode_time.py (bilateral
             20 / 22, grey predictions with colour guidance, --png_encoder device), --png_decoder
             host and device alternating, --reps times each in one process (wall clock, file to file)
  decompose  batch.decompose_files over the 64 mixed-shape photos of tools/decompose_list_time.py as
             files (--png_encoder device), alternating in the same way

Medians, and the spread of the repeats as min and max.  A route counts as a gain only where its
median beats the other's by more than that spread.

    python tools/png_decode_time.py [--reps 5] [--files 96] [--steps decode,filter,decompose]
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

LIMITS = {"decode": 240, "filter": 420, "decompose": 240}     # seconds per step


def say(out, text):
    print(text, file=sys.stderr)
    with open(out, "a") as fh:
        fh.write(text + "\n")


def spread(times):
    return "median %9.3f ms (min %.3f max %.3f)" % (1e3 * statistics.median(times), 1e3 * min(times),
                                                    1e3 * max(times))


def read_parse(name):
    from reflectance_filtering_amd import image_utils as iu
    with open(name, "rb") as fh:
        return iu.png_parse(fh.read())


def step_decode(reps, out):
    import numpy as np
    import torch
    from PIL import Image
    from reflectance_filtering_amd import _ffi, batch, ops
    from reflectance_filtering_amd import image_utils as iu
    from tests import synth
    lib = _ffi.load_library()
    h, w = 1080, 1920
    src = tempfile.mkdtemp()

    def make(i):
        if i < 16:
            name = os.path.join(src, "photo%02d.png" % i)
            Image.fromarray(np.ascontiguousarray(synth.scene_u8(h, w, 300 + i)[:, :, ::-1])).save(name)
        else:
            name = os.path.join(src, "grey%02d.png" % i)
            iu.imwrite(name, synth.reflectance_like_u8(h, w, 400 + i)[:, :, 0])
        return name

    with ThreadPoolExecutor(max_workers=batch.IO_THREADS) as pool:
        files = list(pool.map(make, range(32)))
        want = list(pool.map(iu.imread, files))                                  # warm-up of both routes
        parsed = list(pool.map(read_parse, files))
        assert all(p is not None for p in parsed)
        images, grey = ops.png_decode_ragged_u8(parsed)
        for a, b in zip(images, want):
            assert np.array_equal(a.cpu().numpy(), b), "the device route decodes to other pixels"
        assert grey == [False] * 16 + [True] * 16
        host_t, parse_t, op_wall_t, sum_t, op_t, kern_t = [], [], [], [], [], []
        hs = np.full(32, h, np.int32)
        wd = np.full(32, w, np.int32)
        fm = np.array([(p[2] << 8) | p[3] for p in parsed], np.int32)
        offs = np.zeros(33, np.uint64)
        offs[1:] = np.cumsum([len(p[5]) for p in parsed])
        pristine = torch.from_numpy(np.frombuffer(b"".join(p[5] for p in parsed), np.uint8).copy()).cuda()
        raw = torch.empty_like(pristine)
        need = lib.rf_png_unfilter_workspace_bytes(32, hs.ctypes.data, wd.ctypes.data, fm.ctypes.data)
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        dst = torch.empty(32 * h * w * 3, dtype=torch.uint8, device="cuda")
        flags = torch.empty(32, dtype=torch.uint8, device="cuda")
        for _ in range(reps):
            t0 = time.perf_counter()
            list(pool.map(iu.imread, files))
            host_t.append(time.perf_counter() - t0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            parsed = list(pool.map(read_parse, files))
            t1 = time.perf_counter()
            ops.png_decode_ragged_u8(parsed)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            parse_t.append(t1 - t0)
            op_wall_t.append(t2 - t1)
            sum_t.append(t2 - t0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.png_decode_ragged_u8(parsed)
            e1.record()
            e1.synchronize()
            op_t.append(e0.elapsed_time(e1) / 1e3)
            raw.copy_(pristine)                                                  # the entry overwrites raw
            k0, k1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            k0.record()
            rc = lib.rf_png_unfilter_ragged_u8(raw.data_ptr(), offs.ctypes.data, 32, hs.ctypes.data,
                                               wd.ctypes.data, fm.ctypes.data, None, dst.data_ptr(),
                                               flags.data_ptr(), ws.data_ptr(), need,
                                               _ffi.current_stream_ptr(torch))
            k1.record()
            k1.synchronize()
            assert rc == 0, lib.rf_last_error()
            kern_t.append(k0.elapsed_time(k1) / 1e3)
    mp = 32 * h * w / 1e6
    name = "16 colour (Pillow) + 16 grey (_png_encode) 1080p"
    say(out, "%s  imread, %d threads                  %s %6.0f MP/s"
        % (name, batch.IO_THREADS, spread(host_t), mp / statistics.median(host_t)))
    say(out, "%s  png_parse, %d threads + device op   %s %6.0f MP/s"
        % (name, batch.IO_THREADS, spread(sum_t), mp / statistics.median(sum_t)))
    say(out, "%s    of it png_parse, %d threads       %s" % (name, batch.IO_THREADS, spread(parse_t)))
    say(out, "%s    of it png_decode_ragged_u8        %s" % (name, spread(op_wall_t)))
    say(out, "%s  the op between device events        %s %6.0f MP/s"
        % (name, spread(op_t), mp / statistics.median(op_t)))
    say(out, "%s  its C entry alone                   %s %6.0f MP/s"
        % (name, spread(kern_t), mp / statistics.median(kern_t)))
    say(out, "%s  imread / (png_parse + device op) = %.2f"
        % (name, statistics.median(host_t) / statistics.median(sum_t)))


def alternate(out, name, pixels, reps, run):
    """run(decoder, directory) file to file, host and device alternating after a warm-up of both."""
    import torch
    from reflectance_filtering_amd import batch
    times = {"host": [], "device": []}
    dirs = {dec: tempfile.mkdtemp() for dec in times}
    for dec in times:
        run(dec, dirs[dec])
    for name_ in sorted(os.listdir(dirs["host"])):
        with open(os.path.join(dirs["host"], name_), "rb") as fa, \
                open(os.path.join(dirs["device"], name_), "rb") as fb:
            assert fa.read() == fb.read(), "the two decoders wrote different files: %s" % name_
    for _ in range(reps):
        for dec in times:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(dec, dirs[dec])
            torch.cuda.synchronize()
            times[dec].append(time.perf_counter() - t0)
    for dec in times:
        say(out, "%-44s --png_decoder %-6s %s %7.1f MP/s file to file (%d I/O threads)"
            % (name, dec, spread(times[dec]), pixels / 1e6 / statistics.median(times[dec]),
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
              reps, lambda dec, d: batch.decompose_files(files, d, rank=0, world=1, png_encoder="device",
                                                         png_decoder=dec))


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
              lambda dec, d: batch.filter_files("bilateral", files, pattern, 20.0, 22.0, d, rank=0,
                                                world=1, png_encoder="device", png_decoder=dec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="repeats per decoder (at least 5)")
    ap.add_argument("--files", type=int, default=96, help="1080p files of the filter step")
    ap.add_argument("--steps", default="decode,filter,decompose")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_decode_time.txt"))
    ap.add_argument("--child", default="", help="run this step in this process")
    args = ap.parse_args()
    if args.child:
        import torch
        assert torch.cuda.is_available(), "png_decode_time.py needs a HIP device"
        torch.cuda.set_device(0)
        if args.child == "decode":
            step_decode(args.reps, args.out)
        elif args.child == "decompose":
            step_decompose(args.reps, args.out)
        else:
            step_filter(args.reps, args.out, args.files)
        return 0
    steps = [s for s in args.steps.split(",") if s]
    if any(s not in LIMITS for s in steps) or args.reps < 5:
        ap.error("--steps: decode, filter, decompose; --reps: 5 or more")
    open(args.out, "w").close()
    for s in steps:      # each GPU step in a fresh process under its own limit; the first failure ends the run
        rc = subprocess.call(["timeout", "-k", "10", str(LIMITS[s]), sys.executable, os.path.abspath(__file__),
                              "--child", s, "--reps", str(args.reps), "--files", str(args.files),
                              "--out", args.out])
        if rc != 0:
            print("png_decode_time: step %s ended with status %d" % (s, rc), file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
