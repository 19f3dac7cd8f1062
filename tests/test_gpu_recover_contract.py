"""GPU suite: the three device entries of librf_recover_hip.so (include/reflectance_filtering_recover.h) under the
contracts the entries of the other libraries are held to, with the runners of those modules handed the recover
library and rf_recover_last_error.  The cases are those of tests/recover_cases.py; tests/test_recover_host.py sees
every decoy fail its case's check on the host.

  Buffers  (tests/test_gpu_buffer_contract._contract) every case under the five (layout, fill) pairs: float32
           buffers at the residues 4 and 12, int64 and float64 buffers at 8 and 24, the workspace at 16; only outputs
           and workspace change, the L0 result is the restatement's bit for bit, every other layout is identical.
  Stream   (tests/test_gpu_stream_contract.Flight) every case behind that module's delay on a non-blocking side
           stream: the entry returned while the marker in front of it was pending.
  Capture  (tests/test_gpu_capture_contract.Bench) all three entries are CAPTURABLE: one warm call, ONE call
           captured with nothing run eagerly, then the replays true inputs / workspace 0xA5, decoys / 0xFF, true
           inputs / 0x00 -> oracle, not oracle, oracle.  The library keeps no state and has no shutdown; the graph
           is replayed once more after rf_shutdown() of the MAIN library.  (The scatter entry's grad_e is input and
           output: the runners put its data back before every run.)
  Size     the boundary entry over 357,914,007 pixels: pixel 357,913,941 of x holds byte 2^32.  x and e are zero
           except about 200 live pixels in the first pass, in the passes around byte 2^32 and in the last pass.
           Expected: the restatement on the live pixels with count = P, and the closed form for a zero pixel
           (Ri = m = EPS, reflectance 0, shading EPS * 2^23 = 1 exactly: both losses 0, both slopes 0, grad_e +0.0),
           so the ordered sum is that of the live pixels in their slots.  Skips only where free memory is below
           1.25 x its 8.6 GB.
"""
import ctypes
import time

import numpy as np
import pytest

from tests import recover_cases as RC
from tests import recover_numpy as restate
from tests import size_cases
from tests.test_gpu_buffer_contract import _contract
from tests.test_gpu_capture_contract import Bench, _capture
from tests.test_gpu_fuzz import env  # noqa: F401  (a fixture)
from tests.test_gpu_stream_contract import Delay, Flight

pytestmark = pytest.mark.gpu

CAPTURABLE = (RC.FORWARD, RC.BOUNDARY, RC.SCATTER)


class Ctx(object):
    pass


@pytest.fixture(scope="module")
def ctx(env):
    rf, co, torch = env
    from reflectance_filtering_amd import _ffi_recover
    out = Ctx()
    out.ffi = _ffi_recover
    out.lib = _ffi_recover.load_library()
    out.err = out.lib.rf_recover_last_error
    out.main = rf._ffi.load_library()
    out.delay = Delay(torch)
    out.S = torch.cuda.Stream()
    out.cases = {}
    return out


def _case(env, ctx, name):
    if name not in ctx.cases:
        entries, build, opts = RC.CASES[name]
        ctx.cases[name] = build(env)
        assert ctx.cases[name].entries == entries and set(entries) <= set(CAPTURABLE)
    return ctx.cases[name]


@pytest.mark.parametrize("name", sorted(RC.CASES))
def test_buffer_contract(env, ctx, name):
    _contract(env, _case(env, ctx, name), ctx.lib, ctx.err)


@pytest.mark.parametrize("name", sorted(RC.CASES))
def test_entry_on_a_busy_side_stream(env, ctx, name):
    rf, co, torch = env
    delay, S = ctx.delay, ctx.S
    flight = Flight(env, ctx.lib, _case(env, ctx, name), last_error=ctx.err)
    flight.idle_call(S)                                  # first use: the code object
    call_seconds = flight.idle_call(S)                   # the warm call
    reps, seconds, capped = delay.reps_for(call_seconds)
    rc, pending = flight.enqueue(S, delay, reps)
    S.synchronize()
    print("recover stream contract %-14s warm call %7.3f ms, delay %4d passes = %5.1f ms%s; marker pending at "
          "return: %s" % (name, call_seconds * 1e3, reps, seconds * 1e3, " (capped)" if capped else "", pending))
    assert rc == rf._ffi.RF_OK, (name, rc, ctx.err())
    flight.verify(what=name)
    assert pending, ("%s returned after the work queued in front of it on its stream had finished: it waited, "
                     "and its header says it synchronises nothing" % name)


@pytest.mark.parametrize("name", sorted(RC.CASES))
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
    assert ctx.main.rf_shutdown() == rf._ffi.RF_OK       # of librf_hip.so: this library has nothing to shut down
    after = replay("true", 0xFF)
    assert first is None, "%s: the first replay is not the oracle's: %s" % (name, first)
    assert on_decoys is not None, ("%s: a replay on the decoys gave the true inputs' result: it does not read its "
                                   "buffers at replay time" % name)
    assert again is None, "%s: the replay after the decoys, over a zeroed workspace, is not the oracle's: %s" % (
        name, again)
    assert after is None, "%s: the replay after rf_shutdown() of the main library is not the oracle's: %s" % (
        name, after)
    del graph


# ---- size -----------------------------------------------------------------------------------------------------------

MARK = (1 << 32) // 12              # the pixel of x that holds byte 2^32
NPIXELS = MARK + 1 + 65


def test_boundary_past_byte_2_32_of_x(env, ctx):
    rf, co_, torch = env
    lib, err = ctx.lib, ctx.err
    assert NPIXELS == 357914007 and 12 * MARK < 1 << 32 <= 12 * (MARK + 1)
    plan = ctx.ffi.boundary_plan(NPIXELS)
    per = plan[0]
    need_ws = ctx.ffi.boundary_workspace_bytes(NPIXELS)
    size_cases._fits(torch, "recover boundary past byte 2^32 of x", 24 * NPIXELS + need_ws)
    rng = np.random.RandomState(17)
    lo = (MARK // per - 1) * per
    live = np.concatenate([np.sort(rng.choice(per, 50, replace=False)), np.arange(lo, NPIXELS)])
    assert live[-1] == NPIXELS - 1 and 150 <= live.size <= 700 and live[0] < per and lo < MARK < NPIXELS
    lx, le = RC.seeded(live.size, 18)
    norm, penalty, scales = 0, 2, (0.1, 0.25)
    loss_r, loss_s, grad = restate.boundary_backward32(lx, le, norm, penalty, scales[0], scales[1], count=NPIXELS)
    want = np.array([restate.ordered_mean(loss_r, NPIXELS, plan, index=live),
                     restate.ordered_mean(loss_s, NPIXELS, plan, index=live)])
    assert want.min() > 0 and np.count_nonzero(grad) > 100
    # the closed form of a zero pixel, by the restatement itself
    zero = restate.boundary_backward32(np.zeros((1, 3), np.float32), np.zeros(1, np.float32), norm, penalty,
                                       scales[0], scales[1], count=NPIXELS)
    assert all(a.view(np.uint32)[0] == 0 for a in zero)
    try:
        torch.cuda.reset_peak_memory_stats()
        at = torch.from_numpy(live).cuda()
        x = torch.zeros((NPIXELS, 3), dtype=torch.float32, device="cuda")
        e = torch.zeros(NPIXELS, dtype=torch.float32, device="cuda")
        x[at] = torch.from_numpy(lx).cuda()
        e[at] = torch.from_numpy(le).cuda()
        expected = torch.zeros(NPIXELS, dtype=torch.float32, device="cuda")
        expected[at] = torch.from_numpy(grad).cuda()
        got = torch.full((NPIXELS,), np.nan, dtype=torch.float32, device="cuda")
        means = torch.full((2,), np.nan, dtype=torch.float64, device="cuda")
        ws = torch.full((need_ws,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = lib.rf_recover_boundary_backward_f32(x.data_ptr(), e.data_ptr(), NPIXELS, norm, penalty, scales[0],
                                                  scales[1], means.data_ptr(), got.data_ptr(), ws.data_ptr(), need_ws,
                                                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        seconds = time.perf_counter() - t0
        peak = torch.cuda.max_memory_allocated()
        print("\nrecover size contract %-34s %7.3f ms  peak %5.2f GiB  %d pixels, %d live"
              % ("boundary past byte 2^32 of x", seconds * 1e3, peak / 2.0 ** 30, NPIXELS, live.size))
        assert rc == rf._ffi.RF_OK, err()
        wrong = torch.nonzero(got.view(torch.int32) != expected.view(torch.int32))
        assert wrong.numel() == 0, "%d gradients are not the expected bits, the first at pixel %d" % (
            wrong.shape[0], int(wrong[0]))
        got_means = means.cpu().numpy()
        assert np.array_equal(got_means.view(np.uint64), want.view(np.uint64)), (got_means, want)
    finally:
        x = e = expected = got = means = ws = at = wrong = None
        torch.cuda.empty_cache()
