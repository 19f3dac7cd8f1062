#!/usr/bin/env python
"""Decompose + filter of photos in one pass against the two commands with a PNG hand-off.

The 64 synthetic photos of the three common IIW shapes that tools/decompose_list_time.py builds
(341x512, 512x341, 384x512, equal-shape runs of 1 to 4), as PNG files in a temporary folder and as
device tensors.

File to file, per filter (bilateral c20 s22, guided c7 s52) and per codec pair (host, device):
    A       batch.decompose_files, then batch.filter_files on its `-r.png` outputs: two passes of the
            pipeline, every `-r.png` written, read back and decoded
    B_like  batch.decompose_filter_files(colorize_filtered=False): the same four files per photo
    B       batch.decompose_filter_files: six files per photo (the two colourised outputs of the
            filtered map on top)
Device-resident, in steps of 16 photos (batch.py's step):
    A       decompose_packed + decompose_and_filter_list per step
    B_like  decompose_filter_packed(colorize_filtered=False) per step
    B       decompose_filter_packed per step
with each side's operator calls and kernel launches per pass over the list (the CNN 1, a colourise 18,
a pack one torch.cat, the filters what their launch plans say).

After one warm-up of every path the paths alternate --reps times in one process; every span ends in
a device synchronise (file to file: after the last file is written).  Median, min and max per path,
and whether like-for-like B beats A by more than the min-max spread.  A's and B_like's files are
compared byte for byte once.  Runs in a child process under a time limit and writes the table to
--out.

    python tools/decompose_filter_time.py [--reps 5] [--out profiles/decompose_filter_time.txt]
"""
import argparse
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.ragged_filter_time import STEP, list_shapes  # noqa: E402

COLORIZE_LAUNCHES = 18          # init, 8 x (histogram + pick), write
RECIPES = (("bilateral", 20.0, 22.0), ("guided", 7.0, 52.0))


def _alternate(paths, reps, sync):
    times = {name: [] for name, _ in paths}
    for name, fn in paths:      # warm-up of every path
        fn()
    for _ in range(reps):
        for name, fn in paths:
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            times[name].append(time.perf_counter() - t0)
    return times


def _row(label, ts, extra=""):
    return "%-42s median %9.2f ms  (min %.2f  max %.2f)%s" % (
        label, 1e3 * statistics.median(ts), 1e3 * min(ts), 1e3 * max(ts), extra)


def _verdict(a, b):
    """Does b beat a by more than the repeats' spread: the slowest b under the fastest a."""
    gain = statistics.median(a) / statistics.median(b)
    clear = max(b) < min(a)
    return "A / B_like = %.3f of medians; %s" % (
        gain, "B_like's slowest repeat is under A's fastest: beyond the spread" if clear else
        "the min-max ranges overlap: no difference beyond the spread")


class Counter(object):
    """Counts the operator calls of one pass and the kernel launches they stand for."""

    def __init__(self, ops, _ffi):
        self.ops, self._ffi, self.calls, self.launches, self.saved = ops, _ffi, {}, 0, {}

    def _note(self, name, launches):
        self.calls[name] = self.calls.get(name, 0) + 1
        self.launches += launches

    def __enter__(self):
        ops, ffi = self.ops, self._ffi

        def sizes_of(args, kw):
            if kw.get("sizes") is not None:
                return kw["sizes"]
            return [tuple(t.shape[:2]) for t in args[1]]

        def cn(t):
            return t.shape[1] if hasattr(t, "shape") and t.dim() == 2 else t[0].shape[2]

        def jbf(args, kw):
            plan = ffi.jbf_ragged_plan(sizes_of(args, kw), cn(args[0]), cn(args[1]), args[2], args[3], args[4],
                                       ffi.JBF_GREY_AS_BGR if kw.get("grey_as_bgr") else 0)
            if plan is None:
                slab = ffi.jbf_ragged_slab_plan(sizes_of(args, kw), cn(args[0]), cn(args[1]), args[2], args[3],
                                                args[4], ffi.JBF_GREY_AS_BGR if kw.get("grey_as_bgr") else 0)
                return 1 if slab is not None else len(sizes_of(args, kw))
            return len(plan)

        def gf(args, kw):
            plan = ffi.gf_ragged_plan(sizes_of(args, kw), cn(args[0]), cn(args[1]), args[2],
                                      ffi.GF_GREY_AS_BGR if kw.get("grey_as_bgr") else 0)
            return len(sizes_of(args, kw)) if plan is None else plan["launches"] * kw.get("iterations", 1)

        rules = {"pack_images": lambda a, k: 1, "cnn_reflectance_u8": lambda a, k: 1,
                 "colorize_ragged_srgb_u8": lambda a, k: COLORIZE_LAUNCHES,
                 "colorize_ragged_r8_srgb_u8": lambda a, k: COLORIZE_LAUNCHES,
                 "joint_bilateral_ragged_u8": jbf, "guided_filter_ragged_u8": gf}
        for name, rule in rules.items():
            real = getattr(ops, name)
            self.saved[name] = real

            def wrapped(*a, _real=real, _rule=rule, _name=name, **k):
                self._note(_name, _rule(a, k))
                return _real(*a, **k)
            setattr(ops, name, wrapped)
        return self

    def __exit__(self, *exc):
        for name, real in self.saved.items():
            setattr(self.ops, name, real)
        return False

    def text(self):
        return "  %d call(s), %d launch(es): %s" % (
            sum(self.calls.values()), self.launches,
            ", ".join("%s x%d" % kv for kv in sorted(self.calls.items())))


def measure(reps, out_path):
    import torch
    from reflectance_filtering_amd import _ffi, batch, ops
    from reflectance_filtering_amd import decompose_with_trained_CNN as dc
    from reflectance_filtering_amd import image_utils as iu
    from tests import synth
    assert torch.cuda.is_available(), "decompose_filter_time.py needs a HIP device"
    shapes = list_shapes()
    scenes = [synth.scene_u8(h, w, 200 + i) for i, (h, w) in enumerate(shapes)]
    pixels = sum(h * w for h, w in shapes)
    sync = torch.cuda.synchronize
    lines = ["decompose_filter_time: %d photos, %.2f MP, %d repeats alternating in one process, %s"
             % (len(shapes), pixels / 1e6, reps, torch.cuda.get_device_name(0)),
             "(A = two commands / two calls, B_like = one pass with A's outputs, B = one pass with the two",
             " colourised outputs of the filtered map on top)", ""]
    work = tempfile.mkdtemp(prefix="decompose_filter_time_")
    try:
        src = os.path.join(work, "in")
        os.mkdir(src)
        inputs = []
        for i, scene in enumerate(scenes):
            inputs.append(os.path.join(src, "%03d.png" % i))
            iu.imwrite(inputs[-1], scene)
        lines.append("file to file (ms per pass over the %d files, %d I/O threads):" % (len(inputs), batch.IO_THREADS))
        for ft, sc, ss in RECIPES:
            for codec in ("host", "device"):
                outs = {k: os.path.join(work, "%s_%s_%s" % (ft, codec, k)) for k in ("A", "B_like", "B")}
                for d in outs.values():
                    os.mkdir(d)
                kw = {"rank": 0, "world": 1, "png_encoder": codec, "png_decoder": codec}

                def path_a():
                    firsts = batch.decompose_files(inputs, outs["A"], **kw)
                    batch.filter_files(ft, firsts, None, sc, ss, outs["A"], **kw)

                def path_b(full, key):
                    batch.decompose_filter_files(inputs, outs[key], ft, sc, ss, colorize_filtered=full, **kw)

                paths = [("A", path_a), ("B_like", lambda: path_b(False, "B_like")), ("B", lambda: path_b(True, "B"))]
                times = _alternate(paths, reps, sync)
                names = sorted(os.listdir(outs["A"]))
                assert names == sorted(os.listdir(outs["B_like"])) and len(names) == 4 * len(inputs)
                assert len(os.listdir(outs["B"])) == 6 * len(inputs)
                for name in names:
                    a, b = (iu.imread(os.path.join(outs[k], name)) for k in ("A", "B_like"))
                    assert (a == b).all(), name
                    if codec == "host":
                        with open(os.path.join(outs["A"], name), "rb") as fa, \
                                open(os.path.join(outs["B_like"], name), "rb") as fb:
                            assert fa.read() == fb.read(), name
                tag = "%s c%g s%g, %s codecs" % (ft, sc, ss, codec)
                for name, _ in paths:
                    lines.append(_row("%s  %s" % (tag, name), times[name]))
                lines.append("    " + _verdict(times["A"], times["B_like"]))
                for d in outs.values():
                    shutil.rmtree(d)
    finally:
        shutil.rmtree(work, ignore_errors=True)

    lines += ["", "device-resident, steps of %d photos (ms per pass over the list):" % STEP]
    photos = [torch.from_numpy(s).cuda() for s in scenes]
    steps = [photos[i:i + STEP] for i in range(0, len(photos), STEP)]
    for ft, sc, ss in RECIPES:
        def dev_a():
            return [(dc.decompose_packed(p), dc.decompose_and_filter_list(p, sc, ss, filter_type=ft)) for p in steps]

        def dev_b(full):
            return [dc.decompose_filter_packed(p, sc, ss, ft, colorize_filtered=full) for p in steps]

        for (packed, (_, filtered)), res in zip(dev_a(), dev_b(True)):
            assert torch.equal(packed[2], res.r_u8) and torch.equal(packed[3], res.reflectance)
            assert torch.equal(torch.cat([f.reshape(-1) for f in filtered]), res.filtered)
        paths = [("A", dev_a), ("B_like", lambda: dev_b(False)), ("B", lambda: dev_b(True))]
        counts = {}
        for name, fn in paths:
            with Counter(ops, _ffi) as c:
                fn()
            counts[name] = c.text()
        times = _alternate([(n, (lambda fn=fn: [fn() for _ in range(3)])) for n, fn in paths], reps, sync)
        for name, _ in paths:
            lines.append(_row("%s c%g s%g  %s" % (ft, sc, ss, name), [t / 3 for t in times[name]]))
            lines.append("  " + counts[name])
        lines.append("    " + _verdict(times["A"], times["B_like"]))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    with open(out_path, "w") as f:
        f.write(text)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=540, help="seconds the measurement may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decompose_filter_time.txt"))
    ap.add_argument("--child", action="store_true", help="measure in this process")
    args = ap.parse_args()
    if args.child:
        return measure(args.reps, args.out)
    # the GPU step in a fresh process under its own limit
    rc = subprocess.call(["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__),
                          "--child", "--reps", str(args.reps), "--out", args.out])
    if rc != 0:
        print("decompose_filter_time: ended with status %d" % rc, file=sys.stderr)
    return rc


if __name__ == "__main__":
    sys.exit(main())
