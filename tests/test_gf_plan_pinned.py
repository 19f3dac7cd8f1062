"""CPU suite: the guided filter's planning and argument rules, pinned to the values the library gave
before its source was split by role (tests/golden/gf_plan_parent.json, written by
tests/golden/make_gf_plan.py from a build of the commit the file names).  Workspace sizes, the ragged
route and its launch counts, the chunk the launch rule admits, and the return code and message of every
refusal of the shared argument rules, entry by entry: what a refactor of rf_gf.hip's host code can change
without any kernel or GPU test noticing.  Exact equality; the table is tests/gf_plan_cases.py."""
import json
import os

import pytest

from reflectance_filtering_amd import _ffi

from tests import gf_plan_cases


@pytest.fixture(scope="module")
def pinned(golden_dir):
    with open(os.path.join(golden_dir, "gf_plan_parent.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def recorded(built):
    return json.loads(json.dumps(gf_plan_cases.record(_ffi)))     # (tuples to lists, as the file holds them)


@pytest.mark.parametrize("section,rows", [("workspace", 270), ("ragged", 300), ("launch_chunk", 24),
                                          ("refusals", 0)])
def test_gf_plan_is_what_the_parent_planned(pinned, recorded, section, rows):
    want, got = pinned[section], recorded[section]
    assert len(want) == len(got) and len(got) >= max(rows, 1)
    wrong = [(w, g) for w, g in zip(want, got) if w != g]
    assert not wrong, "%d of %d rows differ, first (pinned, now): %r" % (len(wrong), len(want), wrong[0])


def test_gf_plan_table_reaches_every_route_and_rule(pinned):
    """The fixture is only worth its name if the table reaches what it claims to."""
    ragged = pinned["ragged"]
    assert {row[6] for row in ragged} == {0, 1}                     # both routes of the ragged entry
    assert any(row[0] != "none" and row[6] == 0 for row in ragged)  # a switch that turns the ragged route off
    by_key = {(n, h, w, scn, r): b for n, h, w, scn, r, b in pinned["workspace"]}
    # (the float route beyond radius 128, the kernel pair's row sums at radius 0, the chained form's at radius 1)
    assert by_key[(7, 270, 480, 3, 129)] > by_key[(7, 270, 480, 3, 1)] > by_key[(7, 270, 480, 3, 0)] > 0
    assert [c[-1] for c in pinned["launch_chunk"][-4:]] == [16352, 65217, 2730, 0]
    texts = {row[3] for row in pinned["refusals"]}
    for part in ("unknown flag bits 0x2", "takes a 1-channel guide (got 3 channels)", "takes a 1-channel guide (got 2)",
                 "guide must have 3 channels (got 1)", "src channels must be 1 or 3 (got 2)",
                 "radius 4097 outside 0..4096", "width 134217728 beyond 2^27 - 1",
                 "width 134217728 of image 1 beyond 2^27 - 1", "dst must not overlap guide",
                 "dst may equal src but not partially overlap it", "gf_guide_cache / gf_exact",
                 "NULL image pointer", "bad iterations=0", "bad size n=-1 h=4 w=4 iterations=1"):
        assert any(part in t for t in texts), part
    entries = {row[0] for row in pinned["refusals"]}
    assert entries == {"rf_gf_u8", "rf_gf_ex_u8", "rf_gf_ragged_u8", "rf_gf_f32", "rf_gf_ragged_workspace_bytes",
                       "rf_debug_gf_ragged_plan"}
    # an empty batch: fine with NULL pointers, refused with an unknown flag (the flags come first)
    empty = {(e, c): rc for e, c, rc, _ in pinned["refusals"] if c.startswith("empty batch")}
    assert empty[("rf_gf_ex_u8", "empty batch, NULL pointers")] == 0
    assert empty[("rf_gf_ex_u8", "empty batch, unknown flag")] == _ffi.RF_E_BADARG
    assert empty[("rf_gf_ragged_u8", "empty batch, unknown flag")] == _ffi.RF_E_BADARG
