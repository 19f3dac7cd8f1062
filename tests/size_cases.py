"""The cases of tests/test_gpu_size_contract.py: the builders of tests/abi_cases.py over buffers in which a
byte offset passes 2^31 and 2^32 (for one-channel and float buffers: a pixel or element index as well).

Method: the far copy equals the near copy, and the near copy equals the oracle.  A call's image buffers
are built on the device: a head A - one period, the builder's own images (two 259 x 387 images for a
uniform entry, the list RAGGED for a ragged one) - repeated R times, then a tail B: the same shapes with
other images (the builder's `first`).  R is the least count with which every mark of the case lies at or
before the end of the last A, so that the buffer crosses the marks and B lies wholly behind them.

A 32-bit product in an address expression reads or writes offset mod 2^32: right bytes in front of the
mark, bytes of another period behind it.  So that a wrapped offset cannot land on identical data, the byte
length of one period is no power of two in any buffer of the call (asserted in run): then no power-of-two
wrap maps a period onto itself.  B catches the aligned wrap that this rule cannot.

find_bad_period is the comparison, a plain function over byte arrays (numpy or torch);
tests/test_size_compare.py feeds it wrapped, unwritten and clean arrays.

CASES go through run.  The point entries and the two WHDR entries have index lists beside their images
(points, comparisons): run_points, run_whdr_f32 and run_whdr_points_u8 build those on the host for the
first period, the periods around each mark and B, and compare every result with the one-period calls'.
"""
import ctypes
import time

import numpy as np
import pytest

from tests import abi_cases as C

H, W = 259, 387                                 # h % 64 = 3, w % 4 = 3, w % 64 = 3: 100,233 pixels (odd)
SHAPE = (2, H, W)
RAGGED = ((5, 7), (67, 131), (H, W))            # smaller than a tile, one with strips, 259 x 387: 42 tiles
SLICE_BYTES = 256 << 20
LIMIT_BYTES = 32 << 30                          # no case needs more device memory than this
P31, P32 = 1 << 31, 1 << 32


def where(start, stop, marks):
    """Where the bytes [start, stop) lie relative to each mark: "2^31 B: behind, 2^32 B: across"."""
    out = []
    for label, at in marks:
        out.append("%s: %s" % (label, "in front" if stop <= at else "behind" if start >= at else "across"))
    return ", ".join(out)


def find_bad_period(buf, period, count, marks=(), slice_bytes=SLICE_BYTES):
    """buf: a one-dimensional byte array (numpy or torch) that starts with `count` periods of `period`
    bytes.  None where every period equals the first; else a message that names the first period that
    differs and where it lies relative to `marks` ((label, byte offset) pairs).  Compared in slices of
    whole periods, slice_bytes at most (one period where a period is longer)."""
    assert len(buf.shape) == 1 and buf.shape[0] >= period * count and buf.itemsize == 1
    head = buf[:period]
    step = max(1, slice_bytes // period)
    k = 1
    while k < count:
        m = min(step, count - k)
        part = buf[k * period:(k + m) * period].reshape(m, period)
        if bool((part != head).any()):
            for j in range(m):
                diff = part[j] != head
                if bool(diff.any()):
                    at = (k + j) * period
                    return "period %d (bytes %d..%d) differs from period 0 in %d bytes (%s)" % (
                        k + j, at, at + period - 1, int(diff.sum()), where(at, at + period, marks))
        k += m
    return None


# ---- the cases -------------------------------------------------------------------------------------------

def byte_marks(name, *also):
    """Byte offsets 2^31 and 2^32 of buffer `name`, and further (label, offset) marks of it."""
    return [(name, "2^31 B", P31), (name, "2^32 B", P32)] + [(name, label, at) for label, at in also]


def _jbf(pair, route, two_wg=None):
    return lambda e, first: C.jbf_u8(e, pair, route, SHAPE, first=first), two_wg


def _b(build):
    return build, None


# id: ((builder(env, first) -> abi_cases.Case, the call takes the two-workgroups route), marks)
# In a one-channel u8 buffer a byte offset is the pixel index; in a float buffer element index 2^31 is byte
# 2^33 and 2^32 is byte 2^34.
F31, F32 = ("element 2^31", 1 << 33), ("element 2^32", 1 << 34)
CASES = {
    # rf_jbf_u8: bytes of a 3-channel src; the pixel index of a one-channel src
    "jbf_u8-s22-colour": (_jbf("colour_colour", "s22"), byte_marks("src")),
    "jbf_u8-s22-grey3-two-wg": (_jbf("colour_grey3", "s22", True), byte_marks("src")),
    "jbf_u8-s28-grey3": (_jbf("colour_grey3", "s28"), byte_marks("src")),
    "jbf_u8-s36-slabs": (_jbf("colour_grey3", "s36"), byte_marks("src")),
    "jbf_u8-generic-d3": (_jbf("colour_grey3", "generic_d3"), byte_marks("src")),
    "jbf_u8-d3-grey1-pixels": (_jbf("joint1_grey1", "d3"), byte_marks("src")),
    "jbf_u8-s22-grey-as-bgr-pixels": (_jbf("joint1_as_bgr", "s22"), byte_marks("src")),
    # rf_jbf_ragged_u8
    "jbf_ragged_u8-r33-colour": (_b(lambda e, f: C.jbf_ragged_u8(e, 22.0, RAGGED, "colour", f)), byte_marks("src")),
    "jbf_ragged_u8-r54-colour": (_b(lambda e, f: C.jbf_ragged_u8(e, 36.0, RAGGED, "colour", f)), byte_marks("src")),
    "jbf_ragged_u8-r33-grey1-pixels": (_b(lambda e, f: C.jbf_ragged_u8(e, 22.0, RAGGED, "grey1", f)),
                                       byte_marks("src")),
    # rf_gf_u8, rf_gf_ex_u8: two passes, the workspace of 64 images (the call runs in chunks)
    "gf_u8-r9-colour": (_b(lambda e, f: C.gf_u8(e, SHAPE, "colour", 9, 2, ws_images=64, first=f)), byte_marks("src")),
    "gf_u8-r130-colour-float": (_b(lambda e, f: C.gf_u8(e, SHAPE, "colour", 130, 2, ws_images=64, first=f)),
                                byte_marks("src")),
    "gf_u8-r9-colour-in-place": (_b(lambda e, f: C.gf_u8(e, SHAPE, "colour", 9, 2, ws_images=64, in_place=True,
                                                         first=f)), byte_marks("src")),
    "gf_u8-r9-grey1-pixels": (_b(lambda e, f: C.gf_u8(e, SHAPE, "grey1", 9, 2, ws_images=64, first=f)),
                              byte_marks("src")),
    "gf_ex_u8-r9-colour-grey-guide": (_b(lambda e, f: C.gf_u8(e, SHAPE, "colour", 9, 2, ws_images=64,
                                                              grey_guide=True, first=f)), byte_marks("src")),
    "gf_ex_u8-r130-grey1-grey-guide-pixels": (_b(lambda e, f: C.gf_u8(e, SHAPE, "grey1", 130, 2, ws_images=64,
                                                                      grey_guide=True, first=f)), byte_marks("src")),
    # rf_gf_ragged_u8 (src has one channel): its workspace holds 16 bytes and more per pixel, so under
    # LIMIT_BYTES the list stops behind byte 2^32 of the colour guide, which is pixel index 2^30.4 of src
    "gf_ragged_u8-colour-guide": (_b(lambda e, f: C.gf_ragged_u8(e, RAGGED, False, f)), byte_marks("guide")),
    "gf_ragged_u8-grey-as-bgr": (_b(lambda e, f: C.gf_ragged_u8(e, RAGGED, True, f)),
                                 [("guide", "pixel 2^30", 1 << 30)]),
    # the CNN: NHWC BGR and NCHW RGB, r and r8 together and each alone
    "cnn_u8-both": (_b(lambda e, f: C.cnn_reflectance(e, "u8", "both", SHAPE, first=f)), byte_marks("x")),
    "cnn_u8-r8-pixels": (_b(lambda e, f: C.cnn_reflectance(e, "u8", "u8", SHAPE, first=f)), byte_marks("r8")),
    "cnn_packed_u8-r-elements": (_b(lambda e, f: C.cnn_reflectance(e, "u8", "float", SHAPE, packed=True, first=f)),
                                 byte_marks("r", F31, F32)),
    "cnn_f32-nchw-both": (_b(lambda e, f: C.cnn_reflectance(e, "f32_nchw_rgb", "both", SHAPE, first=f)),
                          byte_marks("x", F31, F32)),
    "cnn_f32-nhwc-r8": (_b(lambda e, f: C.cnn_reflectance(e, "f32_nhwc_bgr", "u8", SHAPE, first=f)),
                        byte_marks("x", F31, F32)),
    "cnn_packed_f32-nhwc-both": (_b(lambda e, f: C.cnn_reflectance(e, "f32_nhwc_bgr", "both", SHAPE, packed=True,
                                                                   first=f)), byte_marks("x", F31, F32)),
    "cnn_packed_f32-nchw-r": (_b(lambda e, f: C.cnn_reflectance(e, "f32_nchw_rgb", "float", SHAPE, packed=True,
                                                                first=f)), byte_marks("x", F31, F32)),
    # colourise: bytes of refl_out; the pixel index of r and shading_out as far as LIMIT_BYTES lets it go
    # (with bgr, r and shading_out alone, pixel index 2^32 needs 8 bytes per pixel: 32 GiB and the tail)
    "colorize_srgb_u8-both": (_b(lambda e, f: C.colorize_srgb_u8(e, "both", SHAPE, f)), byte_marks("refl")),
    "colorize_srgb_u8-shading-pixels": (_b(lambda e, f: C.colorize_srgb_u8(e, "shading", SHAPE, f)),
                                        [("shad", "pixel 2^31", P31)]),
    "colorize_ragged_srgb_u8": (_b(lambda e, f: C.colorize_ragged(e, "rf_colorize_ragged_srgb_u8", RAGGED, f)),
                                byte_marks("refl")),
    "colorize_ragged_r8_srgb_u8": (_b(lambda e, f: C.colorize_ragged(e, "rf_colorize_ragged_r8_srgb_u8", RAGGED, f)),
                                   byte_marks("refl") + [("shad", "pixel 2^31", P31)]),
    # the float filters, three channels: bytes and element index 2^31
    "jbf_f32": (_b(lambda e, f: C.jbf_f32(e, 3, shape=SHAPE, first=f)), byte_marks("src", F31)),
    "gf_f32-r9": (_b(lambda e, f: C.gf_f32(e, 3, 9, SHAPE, f)), byte_marks("src", F31)),
    # rf_png_unfilter_ragged_u8: the builder's five formats, the parsed streams repeated, raw_offsets on the host
    "png_unfilter_ragged_u8": (_b(C.png_unfilter_ragged_u8), byte_marks("raw") + byte_marks("images")),
}


# ---- one run -----------------------------------------------------------------------------------------------

def _bytes(host):
    return np.frombuffer(np.ascontiguousarray(host).tobytes(), np.uint8).copy()


def _call(env, case, call, dev):
    rf, co, torch = env
    lib = rf._ffi.load_library()
    ptrs = dict((name, t.data_ptr()) for name, t in dev.items())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if case.around is not None:
        with case.around():
            rc = call(lib, ptrs, stream)
    else:
        rc = call(lib, ptrs, stream)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    assert rc == rf._ffi.RF_OK, (rc, lib.rf_last_error())
    return seconds


def _small(env, case):
    """One period through the entry: its raw output bytes by name, checked against the oracle."""
    rf, co, torch = env
    dev = {}
    for b in case.bufs:
        if b.data is not None:
            dev[b.name] = torch.from_numpy(_bytes(b.data)).cuda()
        else:
            dev[b.name] = torch.full((max(b.nbytes, 1),), 0xA5, dtype=torch.uint8, device="cuda")
    _call(env, case, case.call, dev)
    if case.after is not None:
        case.after()
    raw = dict((b.name, dev[b.name].cpu().numpy()) for b in case.bufs if b.role == "out")
    case.check(C.typed_outputs(case, raw))
    return raw


def run(env, name):
    """The case `name` of CASES; returns the line of figures that the test prints."""
    rf, co, torch = env
    lib = rf._ffi.load_library()
    (build, two_wg), marks = CASES[name]
    head = build(env, 0)
    if two_wg:
        assert head.two_wg, "the plan no longer puts this case on the two-workgroups-per-CU route"
    grows = [b for b in head.bufs if b.name not in C.PER_CALL]
    period = dict((b.name, b.nbytes) for b in grows)
    for b in grows:
        assert b.nbytes & (b.nbytes - 1), "a period of %s is %d bytes: a power of two" % (b.name, b.nbytes)
    reps = max(-(-at // period[buf]) for buf, _, at in marks)
    call, ws_bytes = head.sized(reps + 1)
    fixed = [b for b in head.bufs if b.name in C.PER_CALL and b.role != "ws"]
    need = sum((reps + 1) * period[b.name] for b in grows) + ws_bytes + sum(b.nbytes for b in fixed) + 3 * SLICE_BYTES
    assert need <= LIMIT_BYTES, "%s needs %.1f GiB" % (name, need / 2.0 ** 30)
    torch.cuda.synchronize()
    free = torch.cuda.mem_get_info()[0]
    if free < 1.25 * need:
        pytest.skip("%s needs %d bytes of device memory, times 1.25; %d are free" % (name, need, free))
    try:
        near = _small(env, head)                     # the warm-up on one period as well
        tail = build(env, 2)                         # (built here: a rf_jbf_u8 case counts its calls from its making)
        assert tail.two_wg == head.two_wg
        for b, t in zip(head.bufs, tail.bufs):
            assert (b.name, b.nbytes, b.role) == (t.name, t.nbytes, t.role)
            assert b.data is None or b.name in C.PER_CALL or not np.array_equal(b.data, t.data), b.name
        far = _small(env, tail)
        dev = {}
        for b, t in zip(head.bufs, tail.bufs):
            if b.name == "ws":
                dev[b.name] = torch.full((ws_bytes,), 0xA5, dtype=torch.uint8, device="cuda")
            elif b.name in C.PER_CALL:
                dev[b.name] = (torch.from_numpy(_bytes(b.data)).cuda() if b.data is not None else
                               torch.full((b.nbytes,), 0xA5, dtype=torch.uint8, device="cuda"))
            else:
                p = period[b.name]
                big = torch.empty((reps + 1) * p, dtype=torch.uint8, device="cuda")
                if b.data is not None:
                    one, last = torch.from_numpy(_bytes(b.data)).cuda(), torch.from_numpy(_bytes(t.data)).cuda()
                else:       # no valid result of A: the complement of the first period's
                    one = last = torch.from_numpy(255 - near[b.name]).cuda()
                big[:reps * p].view(reps, p).copy_(one.view(1, p).expand(reps, p))
                big[reps * p:].copy_(last)
                dev[b.name] = big
                del one, last
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        count = lib.rf_debug_jbf_two_wg_calls()
        seconds = _call(env, head, call, dev)
        if head.two_wg is not None:
            assert lib.rf_debug_jbf_two_wg_calls() - count == (1 if head.two_wg else 0), \
                "the call did not take the route the plan names"
        peak = torch.cuda.max_memory_allocated()
        for b in head.bufs:
            if b.role != "out":
                continue
            p, big = period[b.name], dev[b.name]
            here = [(label, at) for _, label, at in byte_marks(b.name, F31, F32) if at < big.shape[0]]
            got = big[:p].cpu().numpy()
            assert np.array_equal(got, near[b.name]), "%s: the first period differs from the one-period call's in " \
                "%d bytes" % (b.name, int(np.count_nonzero(got != near[b.name])))
            bad = find_bad_period(big, p, reps, here)
            assert bad is None, "%s: %s" % (b.name, bad)
            got = big[reps * p:].cpu().numpy()
            assert np.array_equal(got, far[b.name]), "%s: the tail B (bytes %d.., %s) differs from the call on B " \
                "alone in %d bytes" % (b.name, reps * p, where(reps * p, (reps + 1) * p, here),
                                       int(np.count_nonzero(got != far[b.name])))
        sizes = C.MIXED if name.startswith("png") else RAGGED if "ragged" in name else ((H, W),) * 2
        pixels = (reps + 1) * sum(h * w for h, w in sizes)
        return "size contract %-40s %7.3f s  peak %5.2f GiB  %d periods  %.2f Gpx  marks: %s" % (
            name, seconds, peak / 2.0 ** 30, reps + 1, pixels / 1e9,
            "; ".join("%s of %s" % (label, buf) for buf, label, _ in marks))
    finally:
        dev = near = far = None
        rf.ops.release_workspaces()
        torch.cuda.empty_cache()


# ---- WHDR: index lists built beside the images -----------------------------------------------------------------

def _around(marks, period, reps):
    """The periods of A that hold comparisons: the first, and for each mark the one it lies in with both
    neighbours."""
    out = {0}
    for _, at in marks:
        out.update(k for k in (at // period - 1, at // period, at // period + 1) if 0 <= k < reps)
    return sorted(out)


def _tiled(torch, one, last, reps):
    """[one] * reps + [last] as bytes on the device."""
    p = one.nbytes
    big = torch.empty((reps + 1) * p, dtype=torch.uint8, device="cuda")
    big[:reps * p].view(reps, p).copy_(torch.from_numpy(_bytes(one)).cuda().view(1, p).expand(reps, p))
    big[reps * p:].copy_(torch.from_numpy(_bytes(last)).cuda())
    return big


def _data(case):
    return dict((b.name, b.data) for b in case.bufs)


def _fits(torch, name, need):
    assert need <= LIMIT_BYTES
    torch.cuda.synchronize()
    free = torch.cuda.mem_get_info()[0]
    if free < 1.25 * need:
        pytest.skip("%s needs %d bytes of device memory, times 1.25; %d are free" % (name, need, free))


def run_whdr_f32(env):
    """rf_whdr_f32 on planar 3-channel images: refl passes bytes 2^31 and 2^32 and element 2^31.  Comparisons
    only for the images of the periods of _around and of B; every other image has an empty list."""
    rf, co, torch = env
    lib = rf._ffi.load_library()
    head, tail = C.whdr_f32(env, 3, SHAPE, 0), C.whdr_f32(env, 3, SHAPE, 2)
    a, b = _data(head), _data(tail)
    period, n = a["refl"].nbytes, SHAPE[0]
    assert period & (period - 1) and not np.array_equal(a["refl"], b["refl"])
    marks = [("2^31 B", P31), ("2^32 B", P32), F31]
    reps = -(-F31[1] // period)
    _fits(torch, "whdr_f32", (reps + 1) * period + 3 * SLICE_BYTES)
    try:
        near, far = _small(env, head)["out"].view(np.float64), _small(env, tail)["out"].view(np.float64)
        active = _around(marks, period, reps)
        counts = np.zeros((reps + 1) * n, np.int64)
        per = np.diff(a["offsets"])
        for k in active:
            counts[k * n:(k + 1) * n] = per
        counts[reps * n:] = np.diff(b["offsets"])
        offsets = np.zeros((reps + 1) * n + 1, np.int32)
        offsets[1:] = np.cumsum(counts)
        points = np.concatenate([a["points"]] * len(active) + [b["points"]])
        weights = np.concatenate([a["weights"]] * len(active) + [b["weights"]])
        none = np.float64(rf.whdr.whdr(a["refl"][0], np.zeros((0, 6)), 0.1))
        want = np.full((reps + 1) * n, none)
        for k in active:
            want[k * n:(k + 1) * n] = near
        want[reps * n:] = far
        dev = {"refl": _tiled(torch, a["refl"], b["refl"], reps), "points": torch.from_numpy(points).cuda(),
               "weights": torch.from_numpy(weights).cuda(), "offsets": torch.from_numpy(offsets).cuda(),
               "out": torch.full(((reps + 1) * n,), -1.0, dtype=torch.float64, device="cuda")}
        h, w = SHAPE[1:]

        def call(lib, p, stream):
            return lib.rf_whdr_f32(p["refl"], (reps + 1) * n, 3, h, w, p["points"], p["weights"], p["offsets"], 0.1,
                                   p["out"], stream)
        torch.cuda.reset_peak_memory_stats()
        seconds = _call(env, head, call, dev)
        peak = torch.cuda.max_memory_allocated()
        got = dev["out"].cpu().numpy()
        bad = np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))
        assert bad.size == 0, "image %d (period %d, refl bytes %s): %r, the call on its period alone gives %r" % (
            bad[0], bad[0] // n, where(bad[0] // n * period, (bad[0] // n + 1) * period, marks), got[bad[0]],
            want[bad[0]])
        return "size contract %-40s %7.3f s  peak %5.2f GiB  %d periods  %.2f Gpx  marks: %s of refl; lists in periods %s" % (
            "whdr_f32", seconds, peak / 2.0 ** 30, reps + 1, (reps + 1) * n * h * w / 1e9,
            "; ".join(label for label, _ in marks), active)
    finally:
        dev = None
        rf.ops.release_workspaces()
        torch.cuda.empty_cache()


def run_whdr_points_u8(env):
    """rf_whdr_points_u8 on two sets of 3-channel samples: byte 2^31 lies in set 0, byte 2^32 in set 1 (an offset
    of set * set_stride * c).  Every image of both sets has its comparisons."""
    rf, co, torch = env
    lib = rf._ffi.load_library()
    head, tail = C.whdr_points_u8(env, 3, SHAPE, 0), C.whdr_points_u8(env, 3, SHAPE, 2)
    a, b = _data(head), _data(tail)
    n, (h, w) = SHAPE[0], SHAPE[1:]
    period = n * h * w * 3                       # bytes of one period in one set
    assert period & (period - 1) and a["samples"].shape == (2, n * h * w, 3)
    reps = -(-(P32 - P32 // 4) // period)        # a set of 3/4 of 2^32 bytes and the tail
    stride = (reps + 1) * n * h * w
    assert stride * 3 > P31 and stride * 3 + reps * period > P32 > stride * 3 and stride < P31
    marks = [("2^31 B", P31), ("2^32 B", P32)]
    _fits(torch, "whdr_points_u8", 2 * stride * 3 + 3 * SLICE_BYTES)
    try:
        near, far = (_small(env, c)["out"].view(np.float64).reshape(2, n) for c in (head, tail))
        samples = torch.cat([_tiled(torch, a["samples"][s], b["samples"][s], reps) for s in range(2)])
        images = (reps + 1) * n
        per = int(a["comp_offsets"][1])
        assert np.array_equal(np.diff(a["comp_offsets"]), [per] * n) and np.array_equal(a["comp_offsets"], b["comp_offsets"])
        dev = {"samples": samples,
               "point_offsets": torch.from_numpy((np.arange(images + 1, dtype=np.int64) * h * w).astype(np.int32)).cuda(),
               "comps": torch.from_numpy(np.concatenate([a["comps"]] * reps + [b["comps"]])).cuda(),
               "weights": torch.from_numpy(np.concatenate([a["weights"]] * reps + [b["weights"]])).cuda(),
               "comp_offsets": torch.from_numpy((np.arange(images + 1, dtype=np.int64) * per).astype(np.int32)).cuda(),
               "out": torch.full((2 * images,), -1.0, dtype=torch.float64, device="cuda")}

        def call(lib, p, stream):
            return lib.rf_whdr_points_u8(p["samples"], 2, stride, 3, images, p["point_offsets"], p["comps"], p["weights"],
                                         p["comp_offsets"], 0.1, p["out"], stream)
        torch.cuda.reset_peak_memory_stats()
        seconds = _call(env, head, call, dev)
        peak = torch.cuda.max_memory_allocated()
        got = dev["out"].cpu().numpy().reshape(2, images)
        want = np.concatenate([np.tile(near, (1, reps)), far], axis=1)
        bad = np.argwhere(got != want)
        if bad.size:
            s, i = bad[0]
            at = (s * stride + i * h * w) * 3
            raise AssertionError("set %d, image %d (period %d, sample bytes %s): %r, the call on its period alone gives "
                                 "%r" % (s, i, i // n, where(at, at + h * w * 3, marks), got[s, i], want[s, i]))
        return "size contract %-40s %7.3f s  peak %5.2f GiB  %d periods  %.2f Gpx  marks: %s of samples" % (
            "whdr_points_u8", seconds, peak / 2.0 ** 30, reps + 1, 2 * stride / 1e9, "; ".join(l for l, _ in marks))
    finally:
        dev = samples = None
        rf.ops.release_workspaces()
        torch.cuda.empty_cache()


def run_points(env, ragged, jkind, skind):
    """rf_jbf_points_u8 / rf_jbf_points_ragged_u8 with POINT_PARAMS: the joint passes bytes 2^31 and 2^32 (a
    one-channel joint: pixel indices).  Points - corners among them - only in the periods of _around and in B;
    the images in between are never read."""
    rf, co, torch = env
    lib = rf._ffi.load_library()
    name = "jbf_points%s_u8-%s" % ("_ragged" if ragged else "", jkind)
    sizes = RAGGED if ragged else ((H, W),) * 2
    head = C.jbf_points(env, ragged, sizes, jkind, skind, 0)
    tail = C.jbf_points(env, ragged, sizes, jkind, skind, 2)
    a, b = _data(head), _data(tail)
    period = a["joint"].nbytes
    for key in ("joint", "src"):
        assert a[key].nbytes & (a[key].nbytes - 1) and not np.array_equal(a[key], b[key])
    marks = [("2^31 B", P31), ("2^32 B", P32)]
    reps = -(-P32 // period)
    _fits(torch, name, (reps + 1) * (period + a["src"].nbytes) + 3 * SLICE_BYTES)
    try:
        shape = head.outputs["out"][1]
        near, far = (_small(env, c)["out"].reshape(shape) for c in (head, tail))
        active = _around(marks, period, reps)
        m = len(sizes)
        counts = np.zeros((reps + 1) * m, np.int64)
        for k in active:
            counts[k * m:(k + 1) * m] = np.diff(a["offsets"])
        counts[reps * m:] = np.diff(b["offsets"])
        offsets = np.zeros((reps + 1) * m + 1, np.int32)
        offsets[1:] = np.cumsum(counts)
        points = np.concatenate([a["points"]] * len(active) + [b["points"]])
        want = np.ascontiguousarray(np.concatenate([near] * len(active) + [far], axis=1))
        jcn, scn = a["joint"].shape[-1], a["src"].shape[-1]
        call, need = C.points_call(lib, ragged, tuple(sizes) * (reps + 1), jcn, scn, points.shape[0])
        dev = {"joint": _tiled(torch, a["joint"], b["joint"], reps), "src": _tiled(torch, a["src"], b["src"], reps),
               "points": torch.from_numpy(points).cuda(), "offsets": torch.from_numpy(offsets).cuda(),
               "out": torch.from_numpy(255 - want.reshape(-1)).cuda(),
               "ws": torch.full((need,), 0xA5, dtype=torch.uint8, device="cuda")}
        torch.cuda.reset_peak_memory_stats()
        seconds = _call(env, head, call, dev)
        peak = torch.cuda.max_memory_allocated()
        got = dev["out"].cpu().numpy().reshape(want.shape)
        bad = np.argwhere(got != want)
        if bad.size:
            at = int(bad[0][1])
            k = (active + [reps])[at // near.shape[1]]
            raise AssertionError("parameter set %d, point %d (period %d, joint bytes %s): %r, the call on its period "
                                 "alone gives %r" % (bad[0][0], at, k, where(k * period, (k + 1) * period, marks),
                                                     got[tuple(bad[0])], want[tuple(bad[0])]))
        return "size contract %-40s %7.3f s  peak %5.2f GiB  %d periods  %.2f Gpx  marks: %s of joint; points in periods %s" % (
            name, seconds, peak / 2.0 ** 30, reps + 1, (reps + 1) * sum(h * w for h, w in sizes) / 1e9,
            "; ".join(l for l, _ in marks), active)
    finally:
        dev = None
        rf.ops.release_workspaces()
        torch.cuda.empty_cache()
