"""GPU suite: the stream contract of every entry of the C ABI (include/reflectance_filtering.h) that
enqueues device work, on a busy non-blocking side stream (torch.cuda.Stream()), where neither the null
stream's implicit ordering nor an idle device hides a mistake.  The cases are those of
tests/abi_cases.py, which tests/test_gpu_buffer_contract.py places at odd addresses.

One run of a case on a stream S (Flight.enqueue), with no host synchronisation in between:
    a delay | a marker event | the true inputs copied over the decoys | the entry on S | the outputs
    copied to keep-buffers | the decoys written back and 0xA5 over the outputs
A decoy (abi_cases) is another valid input of the same kind; index-like inputs are written once and
stay, so a stale read gives wrong bytes and never an address outside a buffer.  A read that runs ahead
of S sees the decoy; work that runs behind S (a side stream that was not joined, a helper launch on
another stream) sees it again or writes after the keep copy was taken: the case's oracle check fails.

The delay is a finite chain of in-place multiplies over a 384 MiB buffer: one pass is timed with events
once per session, the entry's warm host-side call is timed on the idle stream, and the chain lasts the
larger of 50 ms and ten times that call (0.3 s at most; "capped" is printed where the rule asked for
more).  Checked per case:
  1. ordering: the keep-buffers hold the oracle's result;
  2. asynchrony: an entry whose header text states no synchronisation returns, after a warm call, while
     the marker is still pending; an entry that states one synchronisation of its stream does not wait
     for other streams' work: a longer delay started before the call on another pool stream T is still
     pending when the call returns (four hardware queues serve the pool, so T and S may share one: up
     to three T are tried in turn and one pending T is enough);
  3. the bounded per-stream tables past their bound (20 caller streams): the guided filter's side
     streams, rf_jbf_u8's vote bytes, the workspace caches of ops.py; and one stream through growing
     launches.
Printed per case: the delay, whether the marker was pending at return, which T were pending.

The module tests itself as well (test_the_runner_notices_work_on_another_stream): the same run with the
entry handed another stream - an idle one, which runs ahead, and a held-up one, which runs behind - must
fail the oracle check.  One finding of the module is kept as a test of its own: a call that finds its
parameter tables cached does not free the table set an earlier call evicted (hipFree waits for the device).

Flight and Delay also serve tests/test_gpu_train_contract.py, which holds the two entries of
librf_train_hip.so (include/reflectance_filtering_train.h) to points 1 and 2.
"""
import ctypes
import math
import time

import numpy as np
import pytest

from tests import abi_cases as C
from tests import arena as A
from tests.abi_cases import MIXED, S1, S2
from tests.test_gpu_fuzz import _jbf_f32_form, env  # noqa: F401  (env is a fixture)

pytestmark = pytest.mark.gpu

# entries whose header text states one synchronisation of the stream they are given
SYNCHRONISING = ("rf_jbf_ragged_u8", "rf_gf_ragged_u8", "rf_colorize_ragged_srgb_u8",
                 "rf_colorize_ragged_r8_srgb_u8", "rf_jbf_f32", "rf_jbf_points_u8", "rf_jbf_points_ragged_u8",
                 "rf_png_deflate_ragged_u8", "rf_png_unfilter_ragged_u8")
FORK = {"gf_force_two_streams": 1}      # the guided filter forks to its side stream from two images on
DELAY_FLOOR, DELAY_CAP = 0.05, 0.3      # seconds
# (d, sigma_color, sigma_space) that puts rf_jbf_f32 on each kernel form for the 3-channel joint of the cases
F32_FORMS = {"pair": (-1, 0.1, 4.0), "quad": (-1, 50.0, 4.0), "untiled": (83, 0.1, 4.0)}


def _case(entries, build, **opts):
    return tuple(entries), build, opts


# id: (the header's entries the call goes through, builder(env) -> abi_cases.Case, options)
#   two_wg: rf_jbf_u8's two-workgroups-per-CU route is asserted (rf_debug_jbf_two_wg_calls)
#   cold:   no warm call - the parameter table is built and uploaded while S is busy (asynchrony printed only)
#   form:   the kernel form of rf_jbf_f32 (test_gpu_fuzz._jbf_f32_form)
CASES = {
    "jbf_u8-s22-grey3": _case(["rf_jbf_u8"], lambda e: C.jbf_u8(e, "colour_grey3", "s22", S1), two_wg=True),
    "jbf_u8-s22-grey1": _case(["rf_jbf_u8"], lambda e: C.jbf_u8(e, "colour_grey1", "s22", S1), two_wg=True),
    "jbf_u8-s22-grey3-5x7": _case(["rf_jbf_u8"], lambda e: C.jbf_u8(e, "colour_grey3", "s22", S2)),
    "jbf_u8-s22-colour": _case(["rf_jbf_u8"], lambda e: C.jbf_u8(e, "colour_colour", "s22", S1)),
    "jbf_u8-s22-grey-as-bgr": _case(["rf_jbf_u8"], lambda e: C.jbf_u8(e, "joint1_as_bgr", "s22", S1)),
    "jbf_u8-s28-grey3": _case(["rf_jbf_u8"], lambda e: C.jbf_u8(e, "colour_grey3", "s28", S1)),
    "jbf_u8-s28-colour-5x7": _case(["rf_jbf_u8"], lambda e: C.jbf_u8(e, "colour_colour", "s28", S2)),
    "jbf_u8-s36-slabs": _case(["rf_jbf_u8"], lambda e: C.jbf_u8(e, "colour_grey3", "s36", S1)),
    "jbf_u8-generic": _case(["rf_jbf_u8"], lambda e: C.jbf_u8(e, "colour_grey3", "generic", S1)),
    "jbf_u8-new-table": _case(["rf_jbf_u8"], lambda e: C.jbf_u8(e, "colour_colour", "s28", S1, sigma_color=19.375),
                              cold=True),
    "jbf_ragged_u8-r33": _case(["rf_jbf_ragged_u8"], lambda e: C.jbf_ragged_u8(e, 22.0)),
    "jbf_ragged_u8-r54-slabs": _case(["rf_jbf_ragged_u8"], lambda e: C.jbf_ragged_u8(e, 36.0)),
    "gf_u8-r9-colour": _case(["rf_gf_u8"], lambda e: C.gf_u8(e, S1, "colour", 9, 1)),
    "gf_u8-r9-colour-fork": _case(["rf_gf_u8"], lambda e: C.gf_u8(e, S1, "colour", 9, 1, options=FORK)),
    "gf_u8-r9-grey1-3x-fork": _case(["rf_gf_u8"], lambda e: C.gf_u8(e, S1, "grey1", 9, 3, options=FORK)),
    "gf_u8-r45-grey3-fork": _case(["rf_gf_u8"], lambda e: C.gf_u8(e, S1, "grey3", 45, 1, options=FORK)),
    "gf_u8-r45-colour-3x-fork": _case(["rf_gf_u8"], lambda e: C.gf_u8(e, S1, "colour", 45, 3, options=FORK)),
    "gf_u8-r9-colour-5x7-fork": _case(["rf_gf_u8"], lambda e: C.gf_u8(e, S2, "colour", 9, 3, options=FORK)),
    "gf_u8-r45-chunked": _case(["rf_gf_u8"], lambda e: C.gf_u8(e, (3, 67, 131), "colour", 45, 2, ws_images=1)),
    "gf_u8-r9-in-place-fork": _case(["rf_gf_u8"],
                                    lambda e: C.gf_u8(e, S1, "colour", 9, 2, in_place=True, options=FORK)),
    "gf_u8-r129-float": _case(["rf_gf_u8"], lambda e: C.gf_u8(e, S1, "colour", 129, 1)),
    "gf_ex_u8-grey-guide": _case(["rf_gf_ex_u8"], lambda e: C.gf_u8(e, S1, "grey3", 45, 1, grey_guide=True)),
    "gf_ragged_u8": _case(["rf_gf_ragged_u8"], C.gf_ragged_u8),
    "gf_f32-r9": _case(["rf_gf_f32"], lambda e: C.gf_f32(e, 3, 9)),
    "gf_f32-r150-one-channel": _case(["rf_gf_f32"], lambda e: C.gf_f32(e, 1, 150)),
    "cnn_u8": _case(["rf_cnn_reflectance_u8"], lambda e: C.cnn_reflectance(e, "u8", "both", S1)),
    "cnn_packed_u8": _case(["rf_cnn_pack_weights", "rf_cnn_reflectance_packed_u8"],
                           lambda e: C.cnn_reflectance(e, "u8", "both", S1, packed=True)),
    "cnn_f32-nchw": _case(["rf_cnn_reflectance_f32"], lambda e: C.cnn_reflectance(e, "f32_nchw_rgb", "both", S1)),
    "cnn_f32-nhwc-5x7": _case(["rf_cnn_reflectance_f32"], lambda e: C.cnn_reflectance(e, "f32_nhwc_bgr", "both", S2)),
    "cnn_packed_f32-nchw": _case(["rf_cnn_pack_weights", "rf_cnn_reflectance_packed_f32"],
                                 lambda e: C.cnn_reflectance(e, "f32_nchw_rgb", "float", S1, packed=True)),
    "cnn_packed_f32-nhwc": _case(["rf_cnn_pack_weights", "rf_cnn_reflectance_packed_f32"],
                                 lambda e: C.cnn_reflectance(e, "f32_nhwc_bgr", "u8", S1, packed=True)),
    "colorize_srgb_u8": _case(["rf_colorize_srgb_u8"], lambda e: C.colorize_srgb_u8(e, "both", S1)),
    "colorize_ragged_srgb_u8": _case(["rf_colorize_ragged_srgb_u8"],
                                     lambda e: C.colorize_ragged(e, "rf_colorize_ragged_srgb_u8")),
    "colorize_ragged_r8_srgb_u8": _case(["rf_colorize_ragged_r8_srgb_u8"],
                                        lambda e: C.colorize_ragged(e, "rf_colorize_ragged_r8_srgb_u8")),
    "jbf_f32-pair": _case(["rf_jbf_f32"], lambda e: C.jbf_f32(e, 3, *F32_FORMS["pair"]), form="pair"),
    "jbf_f32-quad": _case(["rf_jbf_f32"], lambda e: C.jbf_f32(e, 3, *F32_FORMS["quad"]), form="quad"),
    "jbf_f32-untiled": _case(["rf_jbf_f32"], lambda e: C.jbf_f32(e, 3, *F32_FORMS["untiled"]), form="untiled"),
    "jbf_f32-one-channel": _case(["rf_jbf_f32"], lambda e: C.jbf_f32(e, 1, *F32_FORMS["pair"]), form="pair"),
    "whdr_f32": _case(["rf_whdr_f32"], lambda e: C.whdr_f32(e, 3)),
    "whdr_points_u8": _case(["rf_whdr_points_u8"], lambda e: C.whdr_points_u8(e, 3)),
    "whdr_points_u8-one-channel": _case(["rf_whdr_points_u8"], lambda e: C.whdr_points_u8(e, 1)),
    "jbf_points_u8": _case(["rf_jbf_points_u8"], lambda e: C.jbf_points(e, False)),
    "jbf_points_ragged_u8": _case(["rf_jbf_points_ragged_u8"], lambda e: C.jbf_points(e, True)),
    "png_deflate_ragged_u8": _case(["rf_png_deflate_ragged_u8"], C.png_deflate_ragged_u8),
    "png_unfilter_ragged_u8": _case(["rf_png_unfilter_ragged_u8"], C.png_unfilter_ragged_u8),
}


def covered_entries():
    """The header's entries this module runs (compared with the header by tests/test_stream_cases.py)."""
    return sorted(set(name for entries, _, _ in CASES.values() for name in entries))


# ---- the delay and the streams ---------------------------------------------------------------------------

class Delay(object):
    """A chain of in-place multiplies by one over 384 MiB, enqueued on the current stream."""

    def __init__(self, torch):
        self.torch = torch
        self.buf = torch.ones(96 << 20, dtype=torch.float32, device="cuda")
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            self.run(4)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            self.run(20)
            t1.record()
        stream.synchronize()
        self.pass_seconds = max(t0.elapsed_time(t1) / 20 / 1000, 1e-6)

    def run(self, reps):
        for _ in range(int(reps)):
            self.buf.mul_(1.0)

    def reps_for(self, call_seconds):
        """(passes, seconds, capped) of the chain for an entry whose warm host-side call takes call_seconds."""
        asked = max(DELAY_FLOOR, 10.0 * call_seconds)
        seconds = min(asked, DELAY_CAP)
        return max(1, int(math.ceil(seconds / self.pass_seconds))), seconds, asked > DELAY_CAP


class Ctx(object):
    pass


@pytest.fixture(scope="module")
def ctx(env):
    rf, co, torch = env
    out = Ctx()
    out.lib = rf._ffi.load_library()
    torch.cuda.synchronize()
    assert out.lib.rf_jbf_release_scratch() == rf._ffi.RF_OK     # S gets vote bytes of its own
    out.delay = Delay(torch)
    out.S = torch.cuda.Stream()
    out.T = [torch.cuda.Stream() for _ in range(3)]             # the next three pool streams after S
    print("\nstream contract: one delay pass takes %.3f ms" % (out.delay.pass_seconds * 1e3))
    return out


def _ptr(stream):
    return ctypes.c_void_p(stream.cuda_stream)


class Flight(object):
    """One case with buffers of its own: an arena (every base a multiple of 256, filled with 0xA5) that
    holds the decoys, the true inputs and the decoys again as separate device tensors, and `slots` sets
    of keep-buffers for the outputs.  lib is the library the case calls, last_error the getter of its error
    text (default: lib.rf_last_error; tests/test_gpu_train_contract.py passes librf_train_hip.so's)."""

    def __init__(self, env, lib, case, slots=1, last_error=None):
        rf, co, torch = env
        self.env, self.lib, self.case, self.torch = env, lib, case, torch
        self.last_error = lib.rf_last_error if last_error is None else last_error
        self.ar = A.Arena(torch, "cuda", A.arena_bytes([b.nbytes for b in case.bufs]), 0xA5)
        self.regs, self.true, self.decoy = {}, {}, {}
        for b in case.bufs:
            self.regs[b.name] = self.ar.place(b.nbytes, 0, b.elem, name=b.name)
            if b.data is None:
                continue
            if b.decoy is None:
                assert b.name in C.INDEX_LIKE, "%s holds values and has no decoy" % b.name
                self.ar.write(self.regs[b.name], b.data)
                continue
            assert not np.array_equal(b.decoy, b.data), b.name
            self.ar.write(self.regs[b.name], b.decoy)
            self.true[b.name] = self._device(b.data)
            self.decoy[b.name] = self._device(b.decoy)
        self.outs = [b.name for b in case.bufs if b.role == "out"]
        self.keep = [dict((name, torch.empty(self.regs[name].nbytes, dtype=torch.uint8, device="cuda"))
                          for name in self.outs) for _ in range(slots)]
        self.ptrs = dict((name, self.ar.ptr(r)) for name, r in self.regs.items())

    def _device(self, array):
        raw = np.ascontiguousarray(array).reshape(-1).view(np.uint8)
        return self.torch.from_numpy(raw.copy()).cuda()

    def _head(self, name, count):
        r = self.regs[name]
        return self.ar.buf[r.offset:r.offset + count]

    def _call(self, stream):
        if self.case.around is not None:
            with self.case.around():
                return self.case.call(self.lib, self.ptrs, _ptr(stream))
        return self.case.call(self.lib, self.ptrs, _ptr(stream))

    def idle_call(self, stream):
        """The entry on the idle stream with the true inputs in place: host seconds of the call."""
        torch = self.torch
        with torch.cuda.stream(stream):
            for name, t in self.true.items():
                self._head(name, t.numel()).copy_(t)
            stream.synchronize()
            t0 = time.perf_counter()
            rc = self._call(stream)
            seconds = time.perf_counter() - t0
            for name, t in self.decoy.items():            # the decoys are back before anything else runs
                self._head(name, t.numel()).copy_(t)
            for name in self.outs:
                if name not in self.decoy:                # (an output that is an input too holds its decoy)
                    self.ar.bytes(self.regs[name]).fill_(0xA5)
            stream.synchronize()
        assert rc == self.env[0]._ffi.RF_OK, (rc, self.last_error())
        return seconds

    def enqueue(self, stream, delay, reps, slot=0, call_on=None):
        """The sequence of the module docstring on `stream`: (return code, marker pending at return).
        call_on: the stream handed to the entry where that is not `stream` (the module's self-test)."""
        torch = self.torch
        with torch.cuda.stream(stream):
            delay.run(reps)
            marker = torch.cuda.Event()
            marker.record()
            for name, t in self.true.items():
                self._head(name, t.numel()).copy_(t)
            rc = self._call(stream if call_on is None else call_on)
            pending = not marker.query()
            torch.cuda.Event().record()
            for name in self.outs:
                self.keep[slot][name].copy_(self.ar.bytes(self.regs[name]))
            for name, t in self.decoy.items():
                self._head(name, t.numel()).copy_(t)
            for name in self.outs:
                if name not in self.decoy:                # (an output that is an input too holds its decoy)
                    self.ar.bytes(self.regs[name]).fill_(0xA5)
        return rc, pending

    def verify(self, slot=0, what=""):
        raw = dict((name, self.keep[slot][name].cpu().numpy().copy()) for name in self.outs)
        try:
            self.case.check(C.typed_outputs(self.case, raw))
        except AssertionError as err:
            raise AssertionError("%s: the kept outputs are not the oracle's: %s" % (what, err))


def _ok(env, lib, rc, what):
    assert rc == env[0]._ffi.RF_OK, (what, rc, lib.rf_last_error())


# ---- 1 and 2: ordering and asynchrony, every entry and route -----------------------------------------------

@pytest.mark.parametrize("name", sorted(CASES))
def test_entry_on_a_busy_side_stream(env, ctx, name):
    rf, co, torch = env
    lib, delay, S = ctx.lib, ctx.delay, ctx.S
    entries, build, opts = CASES[name]
    case = build(env)
    assert case.entries == entries, (case.entries, entries)
    sync = any(e in SYNCHRONISING for e in entries)
    assert case.sync == sync
    if opts.get("two_wg"):
        assert case.two_wg, "the plan no longer puts this case on the two-workgroups-per-CU route"
    if "form" in opts:
        joint = [b for b in case.bufs if b.name == "joint"][0].data
        assert _jbf_f32_form(joint, *F32_FORMS[opts["form"]]) == opts["form"]
    flight = Flight(env, lib, case)
    call_seconds = 0.0
    if not opts.get("cold"):
        flight.idle_call(S)                              # first use: tables, per-stream slots, code objects
        call_seconds = flight.idle_call(S)               # the warm call
    reps, seconds, capped = delay.reps_for(call_seconds)
    head = "stream contract %-28s warm call %7.3f ms, delay %4d passes = %5.1f ms%s" % (
        name, call_seconds * 1e3, reps, seconds * 1e3, " (capped)" if capped else "")
    routed = lib.rf_debug_jbf_two_wg_calls()
    if not sync:
        rc, pending = flight.enqueue(S, delay, reps)
        S.synchronize()
        print("%s; marker pending at return: %s" % (head, pending))
        _ok(env, lib, rc, name)
        flight.verify(what=name)
        if case.two_wg is not None:
            assert lib.rf_debug_jbf_two_wg_calls() - routed == (1 if case.two_wg else 0)
        if not opts.get("cold"):
            assert pending, ("%s returned after the work queued in front of it on its stream had finished: it waited "
                             "on the launch path, which its header text does not say" % "/".join(entries))
        return
    tried = []
    for T in ctx.T:
        with torch.cuda.stream(T):
            delay.run(4 * reps)                          # outlasts S's delay and the entry's wait for it
            other = torch.cuda.Event()
            other.record()
        rc, pending = flight.enqueue(S, delay, reps)
        tried.append(not other.query())
        S.synchronize()
        T.synchronize()
        _ok(env, lib, rc, name)
        flight.verify(what=name)
        if tried[-1]:
            break
    print("%s; marker pending at return: %s; T pending at return: %s" % (head, pending, tried))
    assert any(tried), ("%s waited for the work of every other stream tried: its one synchronisation is not of its "
                        "own stream alone" % "/".join(entries))


@pytest.mark.parametrize("late", [False, True], ids=["ahead_of_the_stream", "behind_the_stream"])
def test_the_runner_notices_work_on_another_stream(env, ctx, late):
    """The module's self-test: the entry is handed another stream than the one its inputs arrive on.  Ahead
    of S (an idle stream: the call runs at once) it reads the decoys; behind S (a stream held up by a longer
    delay) it runs after the keep copy was taken.  Both are valid calls on valid inputs, and the oracle check
    of the kept outputs must fail on each."""
    rf, co, torch = env
    lib, delay, S, other = ctx.lib, ctx.delay, ctx.S, ctx.T[0]
    flight = Flight(env, lib, C.gf_u8(env, S1, "colour", 9, 1))
    flight.idle_call(S)
    flight.idle_call(other)
    reps = delay.reps_for(0.0)[0]
    torch.cuda.synchronize()
    if late:
        with torch.cuda.stream(other):
            delay.run(4 * reps)
    rc, _ = flight.enqueue(S, delay, reps, call_on=other)
    torch.cuda.synchronize()
    _ok(env, lib, rc, "rf_gf_u8")
    with pytest.raises(AssertionError, match="the kept outputs are not the oracle's"):
        flight.verify(what="rf_gf_u8 on another stream")
    rc, _ = flight.enqueue(S, delay, reps)               # ... and the same flight on S itself is right
    S.synchronize()
    _ok(env, lib, rc, "rf_gf_u8")
    flight.verify(what="rf_gf_u8")


def test_a_cached_table_is_used_without_waiting_after_an_eviction(env, ctx):
    """The table cache holds 64 parameter sets.  A set that is built evicts one, whose arrays are freed
    later (hipFree waits for the whole device): by a call that builds tables and waits anyway, never by a
    call that finds its own set cached."""
    rf, co, torch = env
    lib, delay, S = ctx.lib, ctx.delay, ctx.S
    tiny = Flight(env, lib, C.jbf_u8(env, "colour_colour", "s28", S2))
    flight = Flight(env, lib, C.jbf_u8(env, "colour_colour", "s28", S1))

    def build_a_table(k):                                  # sigma pairs of this test alone
        p, (n, h, w) = tiny.ptrs, S2
        _ok(env, lib, lib.rf_jbf_u8(p["joint"], p["src"], p["dst"], n, h, w, 3, 3, -1, 51.0 + k / 64.0, 2.0, 4, 0,
                                    _ptr(S)), "rf_jbf_u8")

    for k in range(66):                                    # the cache is full and cycling
        build_a_table(k)
    flight.idle_call(S)
    call_seconds = flight.idle_call(S)
    build_a_table(66)                                      # evicts a set: its arrays wait to be freed
    S.synchronize()
    reps, seconds, capped = delay.reps_for(call_seconds)
    rc, pending = flight.enqueue(S, delay, reps)
    S.synchronize()
    print("stream contract jbf_u8 after an eviction: warm call %.3f ms, delay %d passes = %.1f ms%s; marker pending "
          "at return: %s" % (call_seconds * 1e3, reps, seconds * 1e3, " (capped)" if capped else "", pending))
    _ok(env, lib, rc, "rf_jbf_u8")
    flight.verify(what="rf_jbf_u8 after an eviction")
    assert pending, "a call whose tables are cached waited for the device (it freed an evicted table set)"


# ---- the Python wrappers: those that say nothing of a synchronisation return at once ------------------------

def test_ops_wrappers_return_while_their_stream_is_busy(env, ctx):
    rf, co, torch = env
    ops, S, delay = rf.ops, ctx.S, ctx.delay
    gcase, jcase = C.gf_u8(env, S1, "colour", 9, 1), C.jbf_u8(env, "colour_grey3", "s22", S1)
    ccase = C.colorize_srgb_u8(env, "both", S1)
    data = lambda case, name: torch.from_numpy([b for b in case.bufs if b.name == name][0].data).cuda()
    guide, gsrc = data(gcase, "guide"), data(gcase, "src")
    joint, jsrc = data(jcase, "joint"), data(jcase, "src")
    bgr, r = data(ccase, "bgr"), data(ccase, "r")
    calls = {
        "guided_filter_u8": lambda: ops.guided_filter_u8(guide, gsrc, 9, 3.0),
        "joint_bilateral_u8": lambda: ops.joint_bilateral_u8(joint, jsrc, -1, 20.0, 22.0),
        "cnn_reflectance_u8": lambda: ops.cnn_reflectance_u8(bgr),
        "colorize_srgb_u8": lambda: ops.colorize_srgb_u8(bgr, r),
    }
    torch.cuda.synchronize()
    results, pending = {}, {}
    for name in sorted(calls):
        with torch.cuda.stream(S):
            calls[name]()
            S.synchronize()
            t0 = time.perf_counter()
            calls[name]()                                 # the warm call
            seconds = time.perf_counter() - t0
            S.synchronize()
            reps, chain, capped = delay.reps_for(seconds)
            delay.run(reps)
            marker = torch.cuda.Event()
            marker.record()
            results[name] = calls[name]()
            pending[name] = not marker.query()
        S.synchronize()
        print("stream contract ops.%-20s warm call %7.3f ms, delay %4d passes = %5.1f ms%s; marker pending at "
              "return: %s" % (name, seconds * 1e3, reps, chain * 1e3, " (capped)" if capped else "", pending[name]))
    gcase.check({"dst": results["guided_filter_u8"].cpu().numpy()})
    jcase.check({"dst": results["joint_bilateral_u8"].cpu().numpy()})
    refl, shad = results["colorize_srgb_u8"]
    ccase.check({"refl": refl.cpu().numpy(), "shad": shad.cpu().numpy().reshape(S1)})
    assert all(pending.values()), pending


# ---- 3: the bounded per-stream tables, past their bound ------------------------------------------------------

def _twenty_streams(torch):
    streams = [torch.cuda.Stream() for _ in range(20)]
    distinct = len(set(s.cuda_stream for s in streams))
    assert distinct >= 17, "%d distinct handles among 20 pool streams" % distinct
    return streams, distinct


def test_guided_filter_fork_on_twenty_streams(env, ctx):
    """More caller streams than side streams are kept (16): the second round, in reverse order, recycles
    the least recently used idle side streams while others are busy (a call that finds none idle runs on
    its own stream alone)."""
    rf, co, torch = env
    lib, delay = ctx.lib, ctx.delay
    streams, distinct = _twenty_streams(torch)
    case = C.gf_u8(env, S1, "colour", 9, 1, options=FORK)
    flights = [Flight(env, lib, case, slots=2) for _ in streams]
    flights[0].idle_call(streams[0])
    reps, seconds, capped = delay.reps_for(flights[0].idle_call(streams[0]))
    torch.cuda.synchronize()
    rcs = [f.enqueue(s, delay, reps, slot=0) for s, f in zip(streams, flights)]
    rcs += [f.enqueue(s, delay, reps, slot=1) for s, f in reversed(list(zip(streams, flights)))]
    torch.cuda.synchronize()
    print("stream contract gf fork on 20 streams (%d distinct): delay %d passes = %.1f ms%s; markers pending at "
          "return: %d of %d" % (distinct, reps, seconds * 1e3, " (capped)" if capped else "",
                                sum(p for _, p in rcs), len(rcs)))
    for rc, _ in rcs:
        _ok(env, lib, rc, "rf_gf_u8")
    for i, f in enumerate(flights):
        f.verify(0, "stream %d, first round" % i)
        f.verify(1, "stream %d, second round" % i)


def test_joint_bilateral_vote_bytes_on_twenty_streams(env, ctx):
    """rf_jbf_u8 keeps vote bytes for 16 (device, stream) pairs; a further stream takes the route without
    them.  The split is counted, every result is the oracle's, also after rf_jbf_release_scratch."""
    rf, co, torch = env
    lib, delay = ctx.lib, ctx.delay
    streams, distinct = _twenty_streams(torch)
    case = C.jbf_u8(env, "colour_grey3", "s22", S1)
    assert case.two_wg
    flights = [Flight(env, lib, case, slots=3) for _ in streams]
    torch.cuda.synchronize()
    assert lib.rf_jbf_release_scratch() == rf._ffi.RF_OK          # the table of vote bytes starts empty
    flights[0].idle_call(streams[0])
    reps, seconds, capped = delay.reps_for(flights[0].idle_call(streams[0]))
    torch.cuda.synchronize()
    before = lib.rf_debug_jbf_two_wg_calls()
    rcs = [f.enqueue(s, delay, reps, slot=0) for s, f in zip(streams, flights)]
    first_round = lib.rf_debug_jbf_two_wg_calls() - before
    rcs += [f.enqueue(s, delay, reps, slot=1) for s, f in reversed(list(zip(streams, flights)))]
    torch.cuda.synchronize()
    print("stream contract jbf vote bytes on 20 streams (%d distinct): delay %d passes = %.1f ms%s; first round: "
          "%d calls on the two-workgroups-per-CU route, %d on the other; markers pending at return: %d of %d"
          % (distinct, reps, seconds * 1e3, " (capped)" if capped else "", first_round, len(streams) - first_round,
             sum(p for _, p in rcs), len(rcs)))
    for rc, _ in rcs:
        _ok(env, lib, rc, "rf_jbf_u8")
    for i, f in enumerate(flights):
        f.verify(0, "stream %d, first round" % i)
        f.verify(1, "stream %d, second round" % i)
    assert first_round == min(distinct, 16), (first_round, distinct)
    assert lib.rf_jbf_release_scratch() == rf._ffi.RF_OK          # (everything was waited for above)
    rcs = [f.enqueue(s, delay, 1, slot=2) for s, f in zip(streams, flights)]
    torch.cuda.synchronize()
    for rc, _ in rcs:
        _ok(env, lib, rc, "rf_jbf_u8")
    assert lib.rf_jbf_release_scratch() == rf._ffi.RF_OK          # the next test's stream finds room again
    for i, f in enumerate(flights):
        f.verify(2, "stream %d, after rf_jbf_release_scratch" % i)


def test_ops_workspace_caches_on_twenty_streams(env, ctx):
    """gf_workspace keeps four buffers per device and _stream_workspace clears its cache at 16 keys: a
    buffer is dropped while the kernels of another stream still use theirs."""
    rf, co, torch = env
    ops, delay = rf.ops, ctx.delay
    streams, distinct = _twenty_streams(torch)
    data = lambda case, name: torch.from_numpy([b for b in case.bufs if b.name == name][0].data).cuda()
    gcase, jcase, rcase = C.gf_u8(env, S1, "colour", 9, 1), C.jbf_ragged_u8(env), C.gf_ragged_u8(env)
    guide, gsrc = data(gcase, "guide"), data(gcase, "src")
    joint, jsrc = data(jcase, "joint"), data(jcase, "src")
    rguide, rsrc = data(rcase, "guide"), data(rcase, "src")
    reps = delay.reps_for(0.0)[0]
    torch.cuda.synchronize()
    got = {"gf": [], "jbf_ragged": [], "gf_ragged": []}
    for s in streams:
        with torch.cuda.stream(s):
            delay.run(reps)                               # its kernels are still queued when later calls drop buffers
            got["gf"].append(ops.guided_filter_u8(guide, gsrc, 9, 3.0))
    for s in streams:                                     # (these two synchronise their stream: no delay in front)
        with torch.cuda.stream(s):
            got["jbf_ragged"].append(ops.joint_bilateral_ragged_u8(joint, jsrc, -1, 20.0, 22.0, sizes=MIXED)[0])
            got["gf_ragged"].append(ops.guided_filter_ragged_u8(rguide, rsrc, 9, 3.0, iterations=2, sizes=MIXED)[0])
    torch.cuda.synchronize()
    assert len(ops._gf_workspaces) <= 4 and len(ops._jbf_ragged_workspaces) <= 16
    for i in range(len(streams)):
        for key, case in (("gf", gcase), ("jbf_ragged", jcase), ("gf_ragged", rcase)):
            try:
                case.check({"dst": got[key][i].cpu().numpy()})
            except AssertionError as err:
                raise AssertionError("%s on stream %d: %s" % (key, i, err))


def _tiled(kind, shape, distinct):
    """uint8 [n,h,w,c]: `distinct` synthetic images repeated to n, and the index of each one's original."""
    n, h, w = shape
    idx = np.arange(n) % distinct
    return C._images((distinct, h, w), kind), idx


def test_growing_launches_on_one_stream(env, ctx):
    """rf_jbf_u8 on the two-workgroups-per-CU route and ops.guided_filter_u8 through growing shapes with no
    host synchronisation in between.  One vote byte per tile in a buffer of 4 KiB at least: the first three
    shapes share it, 4100 images of one tile each outgrow it and the buffer is retired while the earlier
    launches are still queued."""
    rf, co, torch = env
    lib, delay, S = ctx.lib, ctx.delay, ctx.S
    shapes = ((3, 5, 7), (2, 67, 131), (8, 150, 200), (4100, 64, 64))
    plans = [rf._ffi.jbf_two_wg_plan(n, h, w, 3, 3, -1, 20.0, 22.0, 0) for n, h, w in shapes]
    assert all(p is not None for p in plans), plans
    assert plans[2][2] == plans[0][2] < plans[3][2], plans
    jobs = []
    for (n, h, w), distinct in zip(shapes, (3, 2, 1, 2)):
        (joint, idx), (src, _) = _tiled("colour", (n, h, w), distinct), _tiled("grey3", (n, h, w), distinct)
        want = C._jbf_oracle(co, joint, src, -1, 20.0, 22.0, 0)
        gf_want = C._gf_oracle(co, joint, src, 9, 3.0, 1) if n < 100 else None
        at = torch.from_numpy(idx).cuda()
        jobs.append((n, h, w, torch.from_numpy(joint).cuda()[at].contiguous(),
                     torch.from_numpy(src).cuda()[at].contiguous(), torch.from_numpy(want).cuda()[at], gf_want, idx))
    flight = Flight(env, lib, C.jbf_u8(env, "colour_grey3", "s22", shapes[0]))
    flight.idle_call(S)                                   # S holds its first, smallest buffer of vote bytes
    torch.cuda.synchronize()
    reps = delay.reps_for(0.0)[0]
    before = lib.rf_debug_jbf_two_wg_calls()
    dsts, gf_dsts, rcs = [], [], []
    with torch.cuda.stream(S):
        delay.run(reps)
        for n, h, w, joint, src, want, gf_want, idx in jobs:
            dsts.append(torch.full_like(src, 0xA5))
            rcs.append(lib.rf_jbf_u8(joint.data_ptr(), src.data_ptr(), dsts[-1].data_ptr(), n, h, w, 3, 3, -1, 20.0,
                                     22.0, 4, 0, _ptr(S)))
        for n, h, w, joint, src, want, gf_want, idx in jobs[:3]:
            gf_dsts.append(rf.ops.guided_filter_u8(joint, src, 9, 3.0))
    S.synchronize()
    for rc in rcs:
        _ok(env, lib, rc, "rf_jbf_u8")
    assert lib.rf_debug_jbf_two_wg_calls() - before == len(shapes)
    for (n, h, w, joint, src, want, gf_want, idx), dst in zip(jobs, dsts):
        wrong = (dst != want).reshape(n, -1).any(dim=1)
        assert not bool(wrong.any()), ("rf_jbf_u8", (n, h, w), "first wrong image", int(wrong.nonzero()[0]))
    for (n, h, w, joint, src, want, gf_want, idx), dst in zip(jobs[:3], gf_dsts):
        assert np.array_equal(dst.cpu().numpy(), gf_want[idx]), ("ops.guided_filter_u8", (n, h, w))
