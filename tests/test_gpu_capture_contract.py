"""GPU suite: the graph-capture and shutdown contract of every entry of the C ABI
(include/reflectance_filtering.h, "Graphs") that takes a stream.  The cases are CASES of
tests/test_gpu_stream_contract.py (tests/abi_cases.py), run by that module's Flight: buffers in a guarded
arena filled with 0xA5, a true form and a decoy of every value input, outputs copied to keep-buffers and
checked by the case's own oracle check.  tests/test_capture_cases.py holds the two classes to the header.

An entry is in one of two classes, and a case is refusing if any entry it goes through is:
  CAPTURABLE  the call can be captured on a side stream S (torch's default capture mode) and replayed.
              After one warm eager call on S: decoys in place, outputs and workspace at 0xA5, ONE call
              captured - RF_OK, and after a device synchronisation nothing but the workspace has changed
              (nothing ran eagerly).  Then three replays on S, serialised (the vote bytes of rf_jbf_u8
              belong to S: INTEGRATION.md), the arena's guard bytes and the inputs intact after each:
                true inputs,  workspace as the capture left it (0xA5)  -> the oracle's result
                decoys,       workspace 0xFF                          -> NOT the oracle's result
                true inputs,  workspace 0x00                          -> the oracle's result again
              A replay reads its buffers as they are at replay time and initialises whatever it reads of
              a dirty workspace.  One more case is cold: rf_jbf_u8 with a sigma_color no other module
              uses, whose tables are built inside the capture.
  REFUSING    the entries that synchronise their stream and the two raw-weight CNN entries.  After a warm
              eager call (the refusal is no first-use effect): called inside a capture the entry returns
              RF_E_UNSUPPORTED, its message names it and the capture, the capture ends without an error,
              and no byte of the arena has changed - outputs, workspace, inputs (`raw` of
              rf_png_unfilter_ragged_u8 too).  The empty graph is not replayed.  An eager call on S with
              the true inputs is right afterwards.  Three more cases are the fallback routes the header
              refuses "either way".
Printed per case: the class, the return code of the captured call, which replays matched.

Lifecycle (after the module's graphs are destroyed, as rf_shutdown asks): every case eagerly on S, checked
against the oracle; rf_shutdown(); the same call; rf_jbf_release_scratch(); the same call a third time.
Then one sequence across entries: rf_shutdown(), five cases, rf_shutdown(), the five in reverse.  The
module ends with rf_shutdown(): what it built leaves with it, and the first use of a parameter set in a
later module is a first use.

Bench and _capture also serve tests/test_gpu_train_contract.py: both entries of librf_train_hip.so are
capturable, and their graphs are replayed once more after rf_shutdown() of this library.
"""
import gc

import pytest

from tests import abi_cases as C
from tests.abi_cases import S1
from tests.test_gpu_fuzz import env  # noqa: F401  (env is a fixture)
from tests.test_gpu_stream_contract import CASES, SYNCHRONISING, Flight, _case

pytestmark = pytest.mark.gpu

REFUSING = tuple(SYNCHRONISING) + ("rf_cnn_reflectance_u8", "rf_cnn_reflectance_f32")
CAPTURABLE = ("rf_jbf_u8", "rf_gf_u8", "rf_gf_ex_u8", "rf_gf_f32", "rf_cnn_pack_weights",
              "rf_cnn_reflectance_packed_u8", "rf_cnn_reflectance_packed_f32", "rf_colorize_srgb_u8", "rf_whdr_f32",
              "rf_whdr_points_u8")

# the cases of this module alone (the format of CASES).  cold: no warm call, the parameter set's first use in
# the process is the captured call
EXTRA = {
    "jbf_u8-first-use-in-the-capture": _case(
        ["rf_jbf_u8"], lambda e: C.jbf_u8(e, "colour_colour", "s28", S1, sigma_color=19.4375), cold=True),
    "jbf_ragged_u8-force-generic": _case(
        ["rf_jbf_ragged_u8"], lambda e: C.jbf_ragged_u8(e, 22.0, flags=e[0]._ffi.JBF_FORCE_GENERIC)),
    "gf_ragged_u8-3-channel-src": _case(["rf_gf_ragged_u8"], lambda e: C.gf_ragged_u8(e, skind="grey3")),
    "gf_ragged_u8-r0": _case(["rf_gf_ragged_u8"], lambda e: C.gf_ragged_u8(e, radius=0)),
}
COLD = ("jbf_u8-first-use-in-the-capture",)


def all_cases():
    out = dict((name, (entries, build, dict(opts, cold=False))) for name, (entries, build, opts) in CASES.items())
    assert not set(out) & set(EXTRA)
    out.update(EXTRA)
    return out


def refuses(entries):
    return any(e in REFUSING for e in entries)


CAPTURABLE_CASES = sorted(name for name, (entries, _, _) in all_cases().items() if not refuses(entries))
REFUSING_CASES = sorted(name for name, (entries, _, _) in all_cases().items() if refuses(entries))
# one case each of: rf_jbf_u8 on the two-workgroups-per-CU route (vote bytes), the forked guided filter (side
# streams), the CNN on raw weights (the slot table), rf_jbf_f32 (parameter tables), the point sweep
CROSSING = ("jbf_u8-s22-grey3", "gf_u8-r9-colour-fork", "cnn_u8", "jbf_f32-pair", "jbf_points_u8")


class NoDelay(object):
    """Stands where Flight.enqueue expects the stream-contract module's delay: nothing in front of the call."""

    def run(self, reps):
        pass


class Bench(Flight):
    """Flight plus the single steps of a capture run; each is enqueued on the current stream."""

    def put(self, which):
        for name, t in (self.true if which == "true" else self.decoy).items():
            self._head(name, t.numel()).copy_(t)

    def regions(self, role):
        return [self.regs[b.name] for b in self.case.bufs if b.role == role]

    def wipe_outputs(self):
        for name in self.outs:
            if name not in self.decoy:                    # (an output that is an input too holds its decoy or its data)
                self.ar.bytes(self.regs[name]).fill_(0xA5)

    def fill_workspace(self, byte):
        for r in self.regions("ws"):
            self.ar.bytes(r).fill_(byte)

    def keep_outputs(self):
        for name in self.outs:
            self.keep[0][name].copy_(self.ar.bytes(self.regs[name]))

    def matches(self):
        """None where the kept outputs pass the case's oracle check, else the check's message."""
        try:
            self.verify()
        except AssertionError as err:
            return str(err) or "the check failed"
        return None

    def eager(self, stream, what):
        rc, _ = self.enqueue(stream, NoDelay(), 0)
        stream.synchronize()
        assert rc == self.env[0]._ffi.RF_OK, (what, rc, self.last_error())
        self.verify(what=what)


class Ctx(object):
    pass


@pytest.fixture(scope="module")
def ctx(env):
    rf, co, torch = env
    out = Ctx()
    out.lib = rf._ffi.load_library()
    torch.cuda.synchronize()
    assert out.lib.rf_jbf_release_scratch() == rf._ffi.RF_OK     # S gets vote bytes of its own
    out.S = torch.cuda.Stream()
    out.graphs, out.benches = [], {}
    yield out
    del out.graphs[:]
    gc.collect()
    torch.cuda.synchronize()
    assert out.lib.rf_shutdown() == rf._ffi.RF_OK


def _bench(env, ctx, name):
    """The case and its buffers, built once per module (one oracle result serves every run of the case)."""
    if name not in ctx.benches:
        entries, build, opts = all_cases()[name]
        case = build(env)
        assert case.entries == entries, (case.entries, entries)
        if opts.get("two_wg"):
            assert case.two_wg, "the plan no longer puts this case on the two-workgroups-per-CU route"
        ctx.benches[name] = Bench(env, ctx.lib, case)
        env[2].cuda.synchronize()
    return ctx.benches[name]


def _capture(env, ctx, bench):
    """Decoys, outputs and workspace at 0xA5, one call of the case captured on S: (graph, rc, message, the
    error that ended the capture or None).  The arena's snapshot is that of the moment before the capture."""
    rf, co, torch = env
    S = ctx.S
    with torch.cuda.stream(S):
        bench.put("decoy")
        bench.wipe_outputs()
        bench.fill_workspace(0xA5)
    torch.cuda.synchronize()
    bench.ar.snapshot()
    torch.cuda.synchronize()
    graph, rc, msg, ended = torch.cuda.CUDAGraph(), None, b"", None
    try:
        with torch.cuda.graph(graph, stream=S):
            rc = bench._call(S)
            msg = bench.last_error() if rc != rf._ffi.RF_OK else b""
    except RuntimeError as err:
        ended = err
    torch.cuda.synchronize()
    return graph, rc, msg, ended


# ---- 1. the capturable class -------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", CAPTURABLE_CASES)
def test_capturable_case_is_captured_and_replays(env, ctx, name):
    rf, co, torch = env
    lib, S = ctx.lib, ctx.S
    bench = _bench(env, ctx, name)
    case = bench.case
    assert not refuses(case.entries) and set(case.entries) <= set(CAPTURABLE)
    if name not in COLD:
        bench.idle_call(S)                                # first use: tables, per-stream slots, code objects
    routed = lib.rf_debug_jbf_two_wg_calls()
    graph, rc, msg, ended = _capture(env, ctx, bench)
    routed = lib.rf_debug_jbf_two_wg_calls() - routed
    head = "capture contract %-32s capturable  rc %d" % (name, -99 if rc is None else rc)
    if rc != rf._ffi.RF_OK or ended is not None:
        print("%s; the capture ended with: %s" % (head, ended))
    assert rc == rf._ffi.RF_OK, (name, rc, msg)
    assert ended is None, "%s returned RF_OK and left a capture that cannot be ended: %s" % (name, ended)
    ctx.graphs.append(graph)                              # alive to the end of the capture tests
    try:
        bench.ar.assert_only_changed(bench.regions("ws"))
    except AssertionError as err:
        raise AssertionError("%s ran work eagerly while its stream was being captured: %s" % (name, err))
    if case.two_wg is not None:
        assert routed == (1 if case.two_wg else 0), "the captured call did not take the route the plan names"

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
        torch.cuda.synchronize()                          # (replays of one stream's graphs never overlap)
        try:
            bench.ar.assert_only_changed(bench.regions("out") + bench.regions("ws"))
        except AssertionError as err:
            raise AssertionError("%s, replay on %s inputs: %s" % (name, inputs, err))
        return bench.matches()

    first = replay("true", None)
    on_decoys = replay("decoy", 0xFF)
    again = replay("true", 0x00)
    print("%s; replays: true inputs %s, decoys over a 0xFF workspace %s, true inputs over a 0x00 workspace %s"
          % (head, "match" if first is None else "DIFFER", "differ" if on_decoys is not None else "MATCH",
             "match" if again is None else "DIFFER"))
    assert first is None, "%s: the first replay is not the oracle's: %s" % (name, first)
    assert on_decoys is not None, ("%s: a replay on the decoys gave the true inputs' result: it does not read its "
                                   "buffers at replay time" % name)
    assert again is None, "%s: the replay after the decoys, over a zeroed workspace, is not the oracle's: %s" % (
        name, again)


# ---- 2. the refusing class ---------------------------------------------------------------------------------------

@pytest.mark.filterwarnings("ignore:The CUDA Graph is empty")      # (it is meant to be)
@pytest.mark.parametrize("name", REFUSING_CASES)
def test_refusing_case_is_refused_and_leaves_the_capture_alone(env, ctx, name):
    rf, co, torch = env
    lib, S = ctx.lib, ctx.S
    bench = _bench(env, ctx, name)
    case = bench.case
    named = [e for e in case.entries if e in REFUSING]
    assert named
    bench.idle_call(S)                                    # the refusal is no first-use effect
    graph, rc, msg, ended = _capture(env, ctx, bench)
    del graph                                             # (empty: never replayed)
    print("capture contract %-32s refusing    rc %d; the capture ended %s; %r"
          % (name, -99 if rc is None else rc, "cleanly" if ended is None else "with: %s" % ended, msg))
    assert rc == rf._ffi.RF_E_UNSUPPORTED, (name, rc, msg)
    assert any(e.encode() in msg for e in named) and b"captur" in msg, msg
    assert ended is None, "%s was refused and the capture is invalid all the same: %s" % (name, ended)
    try:
        bench.ar.assert_only_changed([])
    except AssertionError as err:
        raise AssertionError("%s was refused on a capturing stream after device work: %s" % (name, err))
    for r in [bench.regs[o] for o in bench.outs if o not in bench.decoy] + bench.regions("ws"):
        assert bool((bench.ar.bytes(r) == 0xA5).all()), (name, r)
    bench.eager(S, "%s on the stream of the refused capture" % name)


# ---- 3. rf_shutdown and rf_jbf_release_scratch ---------------------------------------------------------------------

@pytest.fixture(scope="module")
def no_graphs(env, ctx):
    """The header's rule for rf_shutdown: no captured graph of a library call is left."""
    del ctx.graphs[:]
    gc.collect()
    env[2].cuda.synchronize()


@pytest.mark.parametrize("name", sorted(CASES))
def test_entry_across_shutdown_and_release_scratch(env, ctx, no_graphs, name):
    rf, co, torch = env
    lib, S = ctx.lib, ctx.S
    bench = _bench(env, ctx, name)
    bench.eager(S, "%s before rf_shutdown" % name)
    torch.cuda.synchronize()
    assert lib.rf_shutdown() == rf._ffi.RF_OK
    bench.eager(S, "%s after rf_shutdown" % name)
    torch.cuda.synchronize()
    assert lib.rf_jbf_release_scratch() == rf._ffi.RF_OK
    bench.eager(S, "%s after rf_jbf_release_scratch" % name)
    print("lifecycle %-32s right before and after rf_shutdown and after rf_jbf_release_scratch" % name)


def test_entries_in_turn_across_two_shutdowns(env, ctx, no_graphs):
    rf, co, torch = env
    lib, S = ctx.lib, ctx.S
    benches = [(name, _bench(env, ctx, name)) for name in CROSSING]
    assert benches[0][1].case.two_wg
    for order in (benches, benches[::-1]):
        torch.cuda.synchronize()
        assert lib.rf_shutdown() == rf._ffi.RF_OK
        for name, bench in order:
            routed = lib.rf_debug_jbf_two_wg_calls()
            bench.eager(S, "%s, %s" % (name, "in turn" if order is benches else "in reverse"))
            if bench.case.two_wg:
                assert lib.rf_debug_jbf_two_wg_calls() - routed == 1, "the vote bytes were not rebuilt"
