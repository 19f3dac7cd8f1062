"""GPU suite: the two device entries of librf_train_hip.so (include/reflectance_filtering_train.h) under the
four contracts the entries of librf_hip.so are held to, with the runners of those modules handed the train
library and rf_train_last_error.  The cases are those of tests/train_cases.py; tests/test_train_host.py
holds the class list to the header and sees every decoy fail its case's check on the host.

  Buffers  (tests/test_gpu_buffer_contract._contract) every case under the five (layout, fill) pairs: float32
           and int32 buffers at the residues 4 and 12, float64 buffers at 8 and 24, the workspace at 16; only
           outputs and workspace change, the L0 result is the oracle's, every other layout is bit-identical.
           (No train buffer is uint8, so L1, L2 and L3 are one layout and those four runs differ in the fill.)
  Stream   (tests/test_gpu_stream_contract.Flight) every case behind that module's delay on a non-blocking
           side stream: the keep-buffers hold the oracle's result, and the entry returned while the marker in
           front of it was pending - the header states no synchronisation.
  Capture  (tests/test_gpu_capture_contract.Bench) both entries are CAPTURABLE and the library has no
           refusing class: one warm call, ONE call captured with nothing run eagerly, then the replays
           true inputs / workspace 0xA5, decoys / 0xFF, true inputs / 0x00 -> oracle, not oracle, oracle, guards
           and inputs intact after each.  The library keeps no state, so there is no shutdown sequence of its
           own; the graph is replayed once more after rf_shutdown() of the MAIN library, which the header
           says does not concern this one.
  Sizes    hinge past the marks: three images whose points start at 2^30 + 5 and whose comparisons start at
           358,000,000, so r, grad_r and inc_offsets are read or written past byte 2^32 and so is comps; the
           buffers are uninitialised but for the touched tail and a 0xA5 head of 1 MiB (where an offset
           wrapped at 32 bits would land); expected is the same images packed alone, bit for bit.
           hinge at the launch limit: n = 2^24 - 1, every image empty but the last; n = 2^24 is refused with
           loss_out untouched.
           backward past byte 2^32 of x (P = 357,913,942 + 65) and of grad_r (P = 2^30 + 65): x is a short
           period of valid inputs tiled on the device, grad_r is zero except at about 200 points (all positive)
           in the first pass, in the passes around byte 2^32 and in the last pass; the oracle is float64
           autograd over the live points alone at 4 x float32 autograd per block.  The second call took 1.9 s
           on an MI355X (under the 10 s it may take), so it is kept.
           A size case skips only where free memory is below 1.25 x its need; none needs more than 32 GiB.
Printed per size case: wall time of the large call and peak device memory (profiles/train_contract_time.txt).
"""
import ctypes
import time

import numpy as np
import pytest

from tests import size_cases
from tests import train_cases as T
from tests.test_gpu_buffer_contract import _contract
from tests.test_gpu_capture_contract import Bench, _capture
from tests.test_gpu_fuzz import env  # noqa: F401  (a fixture)
from tests.test_gpu_stream_contract import Delay, Flight
from tests.test_gpu_train import BLOCKS, NP, autograd, backward_case

pytestmark = pytest.mark.gpu

CAPTURABLE = (T.HINGE, T.BACKWARD)
REFUSING = ()           # no entry of the library refuses a capturing stream ...
SYNCHRONISING = ()      # ... and none synchronises


class Ctx(object):
    pass


@pytest.fixture(scope="module")
def ctx(env):
    rf, co, torch = env
    out = Ctx()
    out.lib = rf._ffi_train.load_library()
    out.err = out.lib.rf_train_last_error
    out.main = rf._ffi.load_library()
    out.delay = Delay(torch)
    out.S = torch.cuda.Stream()
    out.cases = {}
    return out


def _case(env, ctx, name):
    """Built once per module: one oracle result serves every run of a case."""
    if name not in ctx.cases:
        entries, build, opts = T.CASES[name]
        ctx.cases[name] = build(env)
        assert ctx.cases[name].entries == entries and set(entries) <= set(CAPTURABLE)
    return ctx.cases[name]


# ---- buffers ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(T.CASES))
def test_buffer_contract(env, ctx, name):
    _contract(env, _case(env, ctx, name), ctx.lib, ctx.err)


# ---- stream -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(T.CASES))
def test_entry_on_a_busy_side_stream(env, ctx, name):
    rf, co, torch = env
    delay, S = ctx.delay, ctx.S
    flight = Flight(env, ctx.lib, _case(env, ctx, name), last_error=ctx.err)
    flight.idle_call(S)                                  # first use: the code object
    call_seconds = flight.idle_call(S)                   # the warm call
    reps, seconds, capped = delay.reps_for(call_seconds)
    rc, pending = flight.enqueue(S, delay, reps)
    S.synchronize()
    print("train stream contract %-18s warm call %7.3f ms, delay %4d passes = %5.1f ms%s; marker pending at "
          "return: %s" % (name, call_seconds * 1e3, reps, seconds * 1e3, " (capped)" if capped else "", pending))
    assert rc == rf._ffi.RF_OK, (name, rc, ctx.err())
    flight.verify(what=name)
    assert pending, ("%s returned after the work queued in front of it on its stream had finished: it waited, "
                     "and its header says it synchronises nothing" % name)


# ---- capture ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(T.CASES))
def test_case_is_captured_and_replays_also_after_rf_shutdown(env, ctx, name):
    rf, co, torch = env
    S = ctx.S
    bench = Bench(env, ctx.lib, _case(env, ctx, name), last_error=ctx.err)
    bench.idle_call(S)
    graph, rc, msg, ended = _capture(env, ctx, bench)
    assert rc == rf._ffi.RF_OK, (name, rc, msg)
    assert ended is None, "%s returned RF_OK and left a capture that cannot be ended: %s" % (name, ended)
    try:
        bench.ar.assert_only_changed(bench.regions("ws"))
    except AssertionError as err:
        raise AssertionError("%s ran work eagerly while its stream was being captured: %s" % (name, err))

    def replay(inputs, ws_byte):
        with torch.cuda.stream(S):
            bench.put(inputs)
            bench.wipe_outputs()
            if ws_byte is not None:
                bench.fill_workspace(ws_byte)
        torch.cuda.synchronize()
        bench.ar.snapshot()
        torch.cuda.synchronize()
        with torch.cuda.stream(S):
            graph.replay()
            bench.keep_outputs()
        torch.cuda.synchronize()
        try:
            bench.ar.assert_only_changed(bench.regions("out") + bench.regions("ws"))
        except AssertionError as err:
            raise AssertionError("%s, replay on %s inputs: %s" % (name, inputs, err))
        return bench.matches()

    first = replay("true", None)
    on_decoys = replay("decoy", 0xFF)
    again = replay("true", 0x00)
    torch.cuda.synchronize()
    assert ctx.main.rf_shutdown() == rf._ffi.RF_OK       # of librf_hip.so: it "does not concern" this library
    after = replay("true", 0xFF)
    print("train capture contract %-18s replays: true inputs %s, decoys over a 0xFF workspace %s, true inputs over "
          "a 0x00 workspace %s, true inputs after rf_shutdown %s"
          % (name, "match" if first is None else "DIFFER", "differ" if on_decoys is not None else "MATCH",
             "match" if again is None else "DIFFER", "match" if after is None else "DIFFER"))
    assert first is None, "%s: the first replay is not the oracle's: %s" % (name, first)
    assert on_decoys is not None, ("%s: a replay on the decoys gave the true inputs' result: it does not read its "
                                   "buffers at replay time" % name)
    assert again is None, "%s: the replay after the decoys, over a zeroed workspace, is not the oracle's: %s" % (
        name, again)
    assert after is None, "%s: the replay after rf_shutdown() of the main library is not the oracle's: %s" % (
        name, after)
    del graph


# ---- sizes ------------------------------------------------------------------------------------------------------

P32_POINTS = (1 << 30) + 5              # first point of the hinge set: byte 2^32 + 20 of r, grad_r, inc_offsets
P32_COMPS = 358000000                   # its first comparison: byte 2^32 + 1,032,704 of comps
HEAD = 1 << 20                          # bytes of 0xA5 at the start of every large buffer
MOST_IMAGES = (1 << 24) - 1             # one workgroup of 256 per image, below 2^32 work-items


def _stream(torch):
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _hinge_arrays(index, images):
    """(r, po, cp, wt, co, inc_off, inc, delta, margin) of the images `images` of fixture case `index`, packed alone."""
    from reflectance_filtering_amd import train
    fix = T._fixture(index)
    po, cp, wt, co = fix["arrays"]
    a, b = images
    sub_po, sub_co = po[a:b + 1] - po[a], co[a:b + 1] - co[a]
    sub_cp, sub_wt = cp[co[a]:co[b]], wt[co[a]:co[b]]
    inc_off, inc = train.point_incidence(sub_po, sub_cp, sub_co)
    return (np.ascontiguousarray(fix["r"][po[a]:po[b]], np.float32), sub_po.astype(np.int32),
            np.ascontiguousarray(sub_cp, np.int32), np.ascontiguousarray(sub_wt, np.float64),
            sub_co.astype(np.int32), inc_off, inc, float(fix["delta"]), float(fix["margin"]))


def _hinge_small(env, lib, err, arrays, fill=0xA5):
    """The entry on arrays packed alone: (loss_out float64 [n], grad_r float32 [total]) as the device wrote them."""
    rf, co_, torch = env
    r, po, cp, wt, co, inc_off, inc, delta, margin = arrays
    dev = [torch.from_numpy(a).cuda() for a in (r, po, cp, wt, co, inc_off, inc)]
    n = len(co) - 1
    losses = torch.full((8 * n,), fill, dtype=torch.uint8, device="cuda")
    grad = torch.full((4 * len(r),), fill, dtype=torch.uint8, device="cuda")
    rc = lib.rf_train_whdr_hinge_points_f32(*([t.data_ptr() for t in dev] + [n, delta, margin, losses.data_ptr(),
                                                                               grad.data_ptr(), _stream(torch)]))
    torch.cuda.synchronize()
    assert rc == rf._ffi.RF_OK, err()
    return losses.cpu().numpy().view(np.float64), grad.cpu().numpy().view(np.float32)


def _tail(torch, dtype, count, tail):
    """An uninitialised device buffer of `count` elements with a 0xA5 head and `tail` (host) as its last elements."""
    buf = torch.empty(count, dtype=dtype, device="cuda")
    raw = buf.view(torch.uint8)
    raw[:HEAD].fill_(0xA5)
    t = torch.from_numpy(np.ascontiguousarray(tail)).cuda()
    buf[count - t.numel():].copy_(t.view(-1))
    return buf


def _head_intact(torch, buf):
    return bool((buf.view(torch.uint8)[:HEAD] == 0xA5).all())


def test_hinge_past_the_marks(env, ctx):
    rf, co_, torch = env
    lib, err = ctx.lib, ctx.err
    arrays = _hinge_arrays(1, (0, 3))
    r, po, cp, wt, co, inc_off, inc, delta, margin = arrays
    total, m = len(r), len(wt)
    need = 4 * 3 * (P32_POINTS + total + 1) + 12 * (P32_COMPS + m) + 8 * (P32_COMPS + m)
    assert 4 * P32_POINTS > 1 << 32 and 12 * P32_COMPS > 1 << 32 and P32_POINTS + total < 1 << 31
    size_cases._fits(torch, "train hinge past the marks", need)
    dev = {}
    try:
        want_l, want_g = _hinge_small(env, lib, err, arrays)
        torch.cuda.reset_peak_memory_stats()
        dev["r"] = _tail(torch, torch.float32, P32_POINTS + total, r)
        dev["grad_r"] = _tail(torch, torch.float32, P32_POINTS + total, np.full(total, np.nan, np.float32))
        dev["inc_offsets"] = _tail(torch, torch.int32, P32_POINTS + total + 1, inc_off)
        dev["comps"] = _tail(torch, torch.int32, 3 * (P32_COMPS + m), cp.reshape(-1))
        dev["weights"] = _tail(torch, torch.float64, P32_COMPS + m, wt)
        small = [torch.from_numpy(a).cuda() for a in ((po.astype(np.int64) + P32_POINTS).astype(np.int32),
                                                      (co.astype(np.int64) + P32_COMPS).astype(np.int32), inc)]
        losses = torch.full((3,), np.nan, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = lib.rf_train_whdr_hinge_points_f32(dev["r"].data_ptr(), small[0].data_ptr(), dev["comps"].data_ptr(),
                                                dev["weights"].data_ptr(), small[1].data_ptr(),
                                                dev["inc_offsets"].data_ptr(), small[2].data_ptr(), 3, delta, margin,
                                                losses.data_ptr(), dev["grad_r"].data_ptr(), _stream(torch))
        torch.cuda.synchronize()
        seconds = time.perf_counter() - t0
        peak = torch.cuda.max_memory_allocated()
        print("\ntrain size contract %-34s %7.3f ms  peak %5.2f GiB  points from %d, comparisons from %d"
              % ("hinge past the marks", seconds * 1e3, peak / 2.0 ** 30, P32_POINTS, P32_COMPS))
        assert rc == rf._ffi.RF_OK, err()
        got_l = losses.cpu().numpy()
        got_g = dev["grad_r"][P32_POINTS:].cpu().numpy()
        assert np.array_equal(got_l.view(np.uint64), want_l.view(np.uint64)), (got_l, want_l)
        bad = np.flatnonzero(got_g.view(np.uint32) != want_g.view(np.uint32))
        assert bad.size == 0, "%d of %d gradients differ from the set packed alone, the first at point %d: %r, %r" % (
            bad.size, total, bad[0], got_g[bad[0]], want_g[bad[0]])
        for name in sorted(dev):
            assert _head_intact(torch, dev[name]), "the first MiB of %s changed" % name
    finally:
        dev = small = losses = None
        torch.cuda.empty_cache()


def test_hinge_at_the_launch_limit_and_one_image_more(env, ctx):
    """n = 2^24 - 1: every image empty but the last, loss_out pre-filled with the complement of what is expected.
    The last image's loss is that of its small call, bit for bit; its gradient is the small call's divided by n:
    each is one rounding of a double to float32 (2^-24 relative), so n x the large one is within 2^-23 of the
    small one.  n = 2^24 is refused, loss_out untouched."""
    rf, co_, torch = env
    lib, err = ctx.lib, ctx.err
    arrays = _hinge_arrays(1, (2, 3))
    r, po, cp, wt, co, inc_off, inc, delta, margin = arrays
    n, total, m = MOST_IMAGES, len(r), len(wt)
    size_cases._fits(torch, "train hinge at the launch limit", 4 * 8 * (n + 2))
    try:
        want_l, want_g = _hinge_small(env, lib, err, arrays)
        torch.cuda.reset_peak_memory_stats()
        dev = [torch.from_numpy(a).cuda() for a in (r, cp, wt, inc_off, inc)]
        d_po = torch.zeros(n + 2, dtype=torch.int32, device="cuda")
        d_co = torch.zeros(n + 2, dtype=torch.int32, device="cuda")
        d_po[n:], d_co[n:] = total, m
        expected = torch.zeros(n + 1, dtype=torch.float64, device="cuda")
        expected[n - 1] = float(want_l[0])
        fill = ~expected.view(torch.int64)
        losses = fill.clone()
        grad = torch.full((total,), np.nan, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()

        def call(count):
            return lib.rf_train_whdr_hinge_points_f32(dev[0].data_ptr(), d_po.data_ptr(), dev[1].data_ptr(),
                                                      dev[2].data_ptr(), d_co.data_ptr(), dev[3].data_ptr(),
                                                      dev[4].data_ptr(), count, delta, margin, losses.data_ptr(),
                                                      grad.data_ptr(), _stream(torch))
        assert call(n + 1) == rf._ffi.RF_E_UNSUPPORTED, err()
        assert err().endswith(b"too many images for one launch")
        torch.cuda.synchronize()
        assert bool((losses == fill).all()) and bool(torch.isnan(grad).all()), "the refused call wrote"
        t0 = time.perf_counter()
        rc = call(n)
        torch.cuda.synchronize()
        seconds = time.perf_counter() - t0
        peak = torch.cuda.max_memory_allocated()
        print("\ntrain size contract %-34s %7.3f ms  peak %5.2f GiB  %d images, the last of %d comparisons"
              % ("hinge at the launch limit", seconds * 1e3, peak / 2.0 ** 30, n, m))
        assert rc == rf._ffi.RF_OK, err()
        wrong = torch.nonzero(losses[:n] != expected[:n].view(torch.int64))
        assert wrong.numel() == 0, "%d losses are not the expected bits, the first is image %d" % (
            wrong.shape[0], int(wrong[0]))
        assert int(losses[n]) == int(fill[n])
        got = grad.cpu().numpy().astype(np.float64) * n
        ref = want_g.astype(np.float64)
        assert np.array_equal(got == 0, ref == 0)
        assert (np.abs(got - ref) <= 2.0 ** -23 * np.abs(ref)).all(), np.abs(got / np.where(ref, ref, 1) - 1).max()
    finally:
        dev = d_po = d_co = expected = fill = losses = grad = wrong = None
        torch.cuda.empty_cache()


def _live_points(npoints, per, mark_point, rng):
    """About 200 live points: 50 of the first pass, the pass that holds `mark_point` with the pass in front of
    it and every pass behind it (the last one ends with the last point)."""
    first = np.sort(rng.choice(per, 50, replace=False))
    lo = (mark_point // per - 1) * per
    assert 0 < lo and npoints - lo < 4 * per
    around = np.arange(lo, npoints)
    live = np.concatenate([first, around])
    return live


@pytest.mark.parametrize("which", ["x", "grad_r"])
def test_backward_past_byte_2_32(env, ctx, which):
    """P = 357,913,942 + 65: point 357,913,941 of x holds byte 2^32.  P = 2^30 + 65: element 2^30 of grad_r starts
    at byte 2^32 (and x passes bytes 2^32, 2^33 and 3 x 2^32)."""
    rf, co_, torch = env
    lib, err = ctx.lib, ctx.err
    mark = {"x": (1 << 32) // 12, "grad_r": 1 << 30}[which]
    npoints = mark + 1 + 65 if which == "x" else mark + 65
    per = rf._ffi_train.cnn_points_plan(npoints)[0]
    need_ws = rf._ffi_train.cnn_points_workspace_bytes(npoints)
    period = 4099                                         # points; prime, so every lane sees every input
    size_cases._fits(torch, "train backward past byte 2^32 of %s" % which, 16 * npoints + need_ws)
    try:
        px, w, _ = backward_case(period, 100 + period % 97)
        rng = np.random.RandomState(7)
        live = _live_points(npoints, per, mark, rng)
        assert live[-1] == npoints - 1 and 150 <= live.size <= 300 and live[0] < per
        # all of one sign: the bf block is ONE element, the sum of dz over the live points.  Under signed grad_r
        # it is a cancelling sum (|sum| / sum of |terms| = 1 / 27 for these points), and the float32 distance of a
        # single cancelling element is one draw of an error that can land far below its usual size - no yardstick
        values = (0.5 + rng.rand(live.size)).astype(np.float32)
        lx = px[live % period]
        want = autograd(lx, w, values, np.float64)
        f32 = autograd(lx, w, values, np.float32)
        torch.cuda.reset_peak_memory_stats()
        reps = npoints // period
        x = torch.empty((npoints, 3), dtype=torch.float32, device="cuda")
        dpx = torch.from_numpy(px).cuda()
        x[:reps * period].view(reps, period, 3).copy_(dpx.expand(reps, period, 3))
        x[reps * period:].copy_(dpx[:npoints - reps * period])
        grad_r = torch.zeros(npoints, dtype=torch.float32, device="cuda")
        grad_r[torch.from_numpy(live).cuda()] = torch.from_numpy(values).cuda()
        dw = torch.from_numpy(w).cuda()
        out = torch.full((NP,), np.nan, dtype=torch.float32, device="cuda")
        ws = torch.full((need_ws,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = lib.rf_train_cnn_points_backward_f32(x.data_ptr(), dw.data_ptr(), grad_r.data_ptr(), npoints,
                                                  out.data_ptr(), ws.data_ptr(), need_ws, _stream(torch))
        torch.cuda.synchronize()
        seconds = time.perf_counter() - t0
        peak = torch.cuda.max_memory_allocated()
        print("\ntrain size contract %-34s %7.3f s  peak %5.2f GiB  %d points, %d live"
              % ("backward past byte 2^32 of %s" % which, seconds, peak / 2.0 ** 30, npoints, live.size))
        assert rc == rf._ffi.RF_OK, err()
        got = out.cpu().numpy().astype(np.float64)
        assert np.isfinite(got).all()
        misses = []
        for name, a, b in BLOCKS:
            scale = np.abs(want[a:b]).max()
            d32 = np.abs(f32[a:b] - want[a:b]).max() / scale if scale else 0.0
            dev = np.abs(got[a:b] - want[a:b]).max() / scale if scale else np.abs(got[a:b]).max()
            misses += [(name, dev, d32)] if dev > 4 * d32 else []
        assert not misses, misses
    finally:
        x = grad_r = dpx = dw = out = ws = None
        torch.cuda.empty_cache()
