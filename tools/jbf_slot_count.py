#!/usr/bin/env python3
"""Slots and instructions of the grey tap loop of the joint bilateral (jbf_tap_loop_grey4_la2), counted
without a device: what the trimmed end groups of a tap row take out of a wave's instruction stream.

A lane owns four horizontally adjacent outputs 0..3.  A tap row of half-width hw is walked from the even
column -hws (hws = hw rounded up to even) in whole groups of four columns; a column step does one SLOT of
work per output:

  front half   SAD, LUT address and LUT gather (AND / MSAD form: 2 VALU + 1 LDS; J1: the one v_sad_u32 is
               the address too, 1 VALU + 1 LDS), issued two steps before the column's back half
  back half    w = space * lut, wsum += w, w * src, sum += .  (4 VALU)

and, per step whatever the slots, one v_cvt_f32_ubyte3 (plus the v_and_b32 of the AND and J1 forms) and
half a ds_read2_b32.  Column c of the row (c = 0 is column -hws) lies in the disk of output o only where
|c - hws - o| <= hw; everywhere else the slot multiplies by a spatial weight of exactly 0.  The loop
leaves out the slots that are dead whatever the parity of hw:

  FIRST_BACK   live outputs (bit o = output o) of the columns 0..3 of a row's first group
  LAST_BACK    the same of its last group
  a row of one group (hw = 0) is both: SINGLE_BACK, the intersection
  *_FRONT      what the front halves of those columns are issued with (a superset of the back mask: a back
               half never runs for a slot whose front half did not)

`python tools/jbf_slot_count.py [radius ...]` prints the table the profile notes quote.
"""
import json
import math
import sys

FULL = 15
FIRST_BACK = (1, 3, 7, 15)
LAST_BACK = (15, 14, 12, 8)
SINGLE_BACK = tuple(a & b for a, b in zip(FIRST_BACK, LAST_BACK))     # (1, 2, 4, 8)
# fronts: columns 0 and 1 of a row are formed by the steps 2 and 3 of the row before's last group
FIRST_FRONT = (1, 3, 7, 15)
LAST_FRONT = (15, 15, 12, 8)
SINGLE_FRONT = (1, 3, 4, 8)

STAGES = ("parent", "a", "ab")
#          VALU per front slot, LDS per front slot, VALU per back slot, VALU per step, LDS per step
FORMS = {"and": (2, 1, 4, 2, 0.5), "msad": (2, 1, 4, 1, 0.5), "j1": (1, 1, 4, 2, 0.5)}


def half_widths(radius):
    """hw of the tap rows -radius .. radius: the largest j with i^2 + j^2 <= radius^2."""
    return [math.isqrt(radius * radius - i * i) for i in range(-radius, radius + 1)]


def row_groups(hw):
    hws = (hw + 1) & ~1
    return (hws + hw + 4 + 3) >> 2


def live_masks(hw):
    """Per column of the row (4 * groups of them): the outputs whose disk holds the column."""
    hws = (hw + 1) & ~1
    return [sum(1 << o for o in range(4) if abs(c - hws - o) <= hw) for c in range(4 * row_groups(hw))]


def issued_masks(hw, stage="ab"):
    """(front, back) masks per column of the row as the loop of `stage` issues them: "parent" every
    slot, "a" the last group trimmed, "ab" the first group and the one-group rows as well."""
    n = row_groups(hw)
    front, back = [FULL] * (4 * n), [FULL] * (4 * n)
    if stage == "parent":
        return front, back
    if stage == "a":
        front[-4:], back[-4:] = LAST_FRONT, LAST_BACK
        return front, back
    assert stage == "ab", stage
    if n == 1:
        return list(SINGLE_FRONT), list(SINGLE_BACK)
    front[:4], back[:4] = FIRST_FRONT, FIRST_BACK
    front[-4:], back[-4:] = LAST_FRONT, LAST_BACK
    return front, back


def _bits(m):
    return bin(m).count("1")


def count(radius, form="msad", stage="ab"):
    """Steps, slots and instructions of one wave's walk over the whole disk (the prologue before the first
    row and the row bookkeeping are not part of it)."""
    fv, fl, bv, sv, sl = FORMS[form]
    steps = slots = live = fronts = backs = 0
    for hw in half_widths(radius):
        lm = live_masks(hw)
        fm, bm = issued_masks(hw, stage)
        for l, f, b in zip(lm, fm, bm):
            assert l & b == l and b & f == b, (radius, hw, l, f, b)
        steps += len(lm)
        slots += 4 * len(lm)
        live += sum(map(_bits, lm))
        fronts += sum(map(_bits, fm))
        backs += sum(map(_bits, bm))
    return {"radius": radius, "form": form, "stage": stage, "steps": steps, "slots": slots,
            "live_slots": live, "front_slots": fronts, "back_slots": backs,
            "valu": fv * fronts + bv * backs + sv * steps, "lds": fl * fronts + sl * steps}


def reduction(radius, form="msad", stage="ab"):
    """The share of the parent loop's VALU and LDS instructions that `stage` leaves out."""
    p, c = count(radius, form, "parent"), count(radius, form, stage)
    return {"radius": radius, "form": form, "stage": stage,
            "valu_parent": p["valu"], "valu": c["valu"], "valu_drop": 1.0 - c["valu"] / p["valu"],
            "lds_parent": p["lds"], "lds": c["lds"], "lds_drop": 1.0 - c["lds"] / p["lds"],
            "dead_slots": p["slots"] - p["live_slots"], "back_slots_trimmed": p["slots"] - c["back_slots"],
            "front_slots_trimmed": p["slots"] - c["front_slots"]}


def main(argv):
    radii = [int(a) for a in argv] or [33, 42, 54]
    for radius in radii:
        for form in ("msad", "and", "j1"):
            for stage in ("a", "ab"):
                print(json.dumps(reduction(radius, form, stage)))


if __name__ == "__main__":
    main(sys.argv[1:])
