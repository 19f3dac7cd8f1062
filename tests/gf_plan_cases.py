"""What the guided filter's host code plans and refuses, as plain data: the table behind
tests/test_gf_plan_pinned.py and tests/golden/make_gf_plan.py.  record(ffi) asks a loaded library for

  workspace     rf_gf_workspace_bytes over batch sizes, shapes, src channels and radii on either side of
                every route (0, the fused radii, 96 | 97, 128 | 129, the float route)
  ragged        rf_gf_ragged_workspace_bytes and rf_debug_gf_ragged_plan (return value and its six ints)
                for three lists, both guide kinds, with no switch and with each switch that changes the plan
  launch_chunk  rf_debug_gf_launch_chunk for the same shapes and for shapes whose chunk the launch rule lowers
  refusals      the return code and rf_last_error() text of every refusal the shared argument rules
                (rf_gf_common.hpp) produce, per entry: each rule broken alone, then pairs of rules, which
                show the order of the checks

Host arrays and invented pointers only: every call is a size or plan query, an empty batch, or refused
before a pointer is used, so nothing here needs or touches a device.  All sizes stay far below the 6 GiB
workspace cap of a process without a device, so the device-dependent cap never enters."""
import ctypes

import numpy as np

BATCHES = (1, 2, 7)
SHAPES = ((1, 1), (5, 17), (64, 64), (97, 130), (270, 480))
RADII = (0, 1, 45, 52, 96, 97, 128, 129, 300)
LISTS = {
    "one": [(5, 17)],
    "three": [(64, 64), (97, 130), (33, 700)],
    "mixed16": [(270, 480), (1, 1)] * 8,
}
RAGGED_RADII = (0, 1, 45, 128, 129)
SWITCHES = ({}, {"gf_two_kernel": 1}, {"gf_chained": 1}, {"gf_s1_legacy_strips": 1}, {"gf_s1_cap": 2})
# chunks the launch rule lowers (the shapes of tests/test_launch_limits_abi.py): asked, h, w, src_cn, float kernels
LOWERED = ((16383, 21888, 1, 3, 0), (65535, 3073, 1, 3, 1), (16383, 1, 65536, 3, 0), (5, (1 << 31) - 1, 1, 1, 0))

G, S, D, W = 1 << 40, 2 << 40, 3 << 40, 4 << 40      # invented device pointers, far apart; never used
GREY = 1                                              # RF_GF_GREY_AS_BGR
WIDE = 1 << 27


def _sizes(sizes):
    a = np.asarray(sizes, np.int32).reshape(-1, 2)
    return np.ascontiguousarray(a[:, 0]), np.ascontiguousarray(a[:, 1])


def _switch_name(sw):
    return ",".join("%s=%d" % kv for kv in sorted(sw.items())) or "none"


def record(ffi):
    lib = ffi.load_library()
    out = {}
    out["workspace"] = [[n, h, w, scn, r, lib.rf_gf_workspace_bytes(n, h, w, 3, scn, r)]
                        for n in BATCHES for (h, w) in SHAPES for scn in (1, 3) for r in RADII]
    ragged = []
    for sw in SWITCHES:
        with ffi.debug_options(**sw):
            for name, sizes in LISTS.items():
                hs, ws = _sizes(sizes)
                for grey in (0, 1):
                    for scn in (1, 3):
                        for r in RAGGED_RADII:
                            gcn, flags = (1, GREY) if grey else (3, 0)
                            nbytes = lib.rf_gf_ragged_workspace_bytes(len(sizes), hs.ctypes.data, ws.ctypes.data,
                                                                      gcn, scn, r, flags)
                            plan = (ctypes.c_int * 6)()
                            rc = lib.rf_debug_gf_ragged_plan(len(sizes), hs.ctypes.data, ws.ctypes.data, gcn, scn,
                                                             r, flags, plan, 6)
                            ragged.append([_switch_name(sw), name, grey, scn, r, nbytes, rc, list(plan)])
    out["ragged"] = ragged
    chunk = lib.rf_debug_gf_launch_chunk
    out["launch_chunk"] = ([[7, h, w, scn, f, chunk(7, h, w, scn, f)]
                            for (h, w) in SHAPES for scn in (1, 3) for f in (0, 1)] +
                           [list(c) + [chunk(*c)] for c in LOWERED])
    out["refusals"] = _refusals(ffi, lib)
    return out


# One rule broken alone, then pairs of rules, as changes to a call every entry would accept:
# guide G, src S, dst D, one 4 x 4 image, 3-channel guide, one src channel, radius 2, one pass, no flags.
BASE = dict(guide=G, src=S, dst=D, n=1, h=4, w=4, gcn=3, scn=1, r=2, it=1, flags=0, ws=W, opts={})
NONE = dict(guide=None, src=None, dst=None, ws=None)
RULE_CASES = (
    ("unknown flag", dict(flags=2)),
    ("grey flag, 3-channel guide", dict(flags=GREY, gcn=3)),
    ("grey flag, 2-channel guide", dict(flags=GREY, gcn=2)),
    ("1-channel guide, no flag", dict(gcn=1)),
    ("4-channel guide", dict(gcn=4)),
    ("2 src channels", dict(scn=2)),
    ("radius -1", dict(r=-1)),
    ("radius 4097", dict(r=4097)),
    ("width 2^27", dict(h=1, w=WIDE)),
    ("dst is guide", dict(guide=D)),
    ("dst overlaps src partially", dict(src=D + 1)),
    ("grey guide under gf_exact", dict(flags=GREY, gcn=1, opts={"gf_exact": 1})),
    ("grey guide under gf_guide_cache", dict(flags=GREY, gcn=1, opts={"gf_guide_cache": 1})),
    ("NULL guide", dict(guide=None)),
    ("n = -1", dict(n=-1)),
    ("iterations = 0", dict(it=0)),
    ("pair: unknown flag, n = -1", dict(flags=2, n=-1)),
    ("pair: grey flag with 3-channel guide, 2 src channels", dict(flags=GREY, gcn=3, scn=2)),
    ("pair: radius 5000, width 2^27", dict(r=5000, h=1, w=WIDE)),
    ("pair: 2 src channels, dst is guide", dict(scn=2, guide=D)),
    ("pair: dst is guide, grey guide under gf_exact", dict(flags=GREY, gcn=1, guide=D, opts={"gf_exact": 1})),
    ("pair: NULL guide, iterations = 0, radius 5000", dict(guide=None, it=0, r=5000)),
    ("empty batch, NULL pointers", dict(NONE, n=0)),
    ("empty batch, unknown flag", dict(NONE, n=0, flags=2)),
)


def _refusals(ffi, lib):
    rows = []
    plan = (ctypes.c_int * 6)()

    def note(entry, case, call, may_pass=False):
        lib.rf_debug_gf_launch_chunk(-1, 1, 1, 1, 0)          # a known message: shows where a call leaves none
        stale = lib.rf_last_error()
        rc = call()
        text = lib.rf_last_error()
        rows.append([entry, case, rc, "" if text == stale else text.decode()])
        # an entry that got past its argument rules would use the invented pointers: none may
        assert may_pass or rc < 0, (entry, case, rc)

    for case, change in RULE_CASES:
        a = dict(BASE, **change)
        empty_ok = a["n"] == 0 and a["flags"] in (0, GREY)
        hs, ws = _sizes([(a["h"], a["w"])] * max(a["n"], 1))
        lists = (a["n"], hs.ctypes.data, ws.ctypes.data, a["gcn"], a["scn"], a["r"])
        with ffi.debug_options(**a["opts"]):
            if a["flags"] == 0:     # (the entries without a flags argument)
                note("rf_gf_u8", case, lambda: lib.rf_gf_u8(
                    a["guide"], a["src"], a["dst"], a["n"], a["h"], a["w"], a["gcn"], a["scn"], a["r"], 1e-3,
                    a["it"], a["ws"], 1 << 30, None), empty_ok)
                if a["w"] != WIDE:  # (no width rule there: a wide image alone would get past the rules)
                    fsrc = D + 4 if a["src"] == D + 1 else a["src"]
                    note("rf_gf_f32", case, lambda: lib.rf_gf_f32(
                        a["guide"], fsrc, a["dst"], a["n"], a["h"], a["w"], a["gcn"], a["scn"], a["r"], 1e-3,
                        a["it"], a["ws"], 1 << 30, None), empty_ok)
            note("rf_gf_ex_u8", case, lambda: lib.rf_gf_ex_u8(
                a["guide"], a["src"], a["dst"], a["n"], a["h"], a["w"], a["gcn"], a["scn"], a["r"], 1e-3,
                a["it"], a["flags"], a["ws"], 1 << 30, None), empty_ok)
            note("rf_gf_ragged_u8", case, lambda: lib.rf_gf_ragged_u8(
                a["guide"], a["src"], a["dst"], *lists, 1e-3, a["it"], a["flags"], a["ws"], 1 << 30, None), empty_ok)
            # the two queries take no pointers and no pass count: the cases that change nothing else are left out
            if any(k not in ("guide", "src", "dst", "ws", "it") for k in change):
                note("rf_gf_ragged_workspace_bytes", case,
                     lambda: lib.rf_gf_ragged_workspace_bytes(*lists, a["flags"]), True)
                note("rf_debug_gf_ragged_plan", case,
                     lambda: lib.rf_debug_gf_ragged_plan(*lists, a["flags"], plan, 6), True)
    # the float entry's overlap rule counts 4-byte elements: 16 pixels of one channel are 64 bytes
    note("rf_gf_f32", "guide 32 bytes behind dst", lambda: lib.rf_gf_f32(
        D + 32, S, D, 1, 4, 4, 3, 1, 2, 1e-3, 1, W, 1 << 30, None))
    # lists: the width rule names the image; the list's own refusals stand between the shared rules
    wide = _sizes([(4, 4), (1, WIDE)])
    norows = _sizes([(4, 4), (0, 4)])
    for case, (hs, ws), r in (("list: width 2^27 of image 1", wide, 2),
                              ("list: radius 5000, width 2^27 of image 1", wide, 5000),
                              ("list: image 1 has no rows, radius 5000", norows, 5000)):
        lists = (2, hs.ctypes.data, ws.ctypes.data, 3, 1, r)
        note("rf_gf_ragged_u8", case,
             lambda: lib.rf_gf_ragged_u8(G, S, D, *lists, 1e-3, 1, 0, W, 1 << 30, None))
        note("rf_gf_ragged_workspace_bytes", case, lambda: lib.rf_gf_ragged_workspace_bytes(*lists, 0), True)
        note("rf_debug_gf_ragged_plan", case, lambda: lib.rf_debug_gf_ragged_plan(*lists, 0, plan, 6), True)
    return rows

