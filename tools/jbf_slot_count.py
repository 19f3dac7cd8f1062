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

Stage "abp" looks at the parity of hw as well.  A row of odd hw starts at column -(hw + 1): its first column
lies left of the disk of all four outputs, the padding column at its end right of it, and the live outputs
of its end groups are one less per column than the union over both parities:

  FIRST_BACK_ODD / LAST_BACK_ODD    [0, 1, 3, 7] and [14, 12, 8, 0]
  FIRST_FRONT_ODD / LAST_FRONT_ODD  the fronts those columns are issued with; a row's columns 0 and 1 are
               formed by the row before with [1, 3] whatever the parity of either row

The colour loop (jbf_tap_loop_rgb6) walks the same rows with its gathers ONE step ahead: only a row's column 0
is formed by the row before.  Its slots cost 2 VALU + 1 LDS (front) and 8 VALU (back: weight, weight sum and
three multiply-adds), a step 3 VALU (MSAD; 4 with the v_and_b32) and 2 LDS beside them; its end groups are
trimmed by the parity-independent masks (COLOUR_*, stage "ab" of count_colour).

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

# rows of odd half-width (at least two groups): column 0 and the last column are dead for every output
FIRST_BACK_ODD = (0, 1, 3, 7)
LAST_BACK_ODD = (14, 12, 8, 0)
FIRST_FRONT_ODD = (1, 3, 3, 7)
LAST_FRONT_ODD = (15, 15, 8, 0)

STAGES = ("parent", "a", "ab")
PARITY_STAGE = "abp"
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
    assert stage in ("ab", PARITY_STAGE), stage
    if n == 1:
        return list(SINGLE_FRONT), list(SINGLE_BACK)
    if stage == PARITY_STAGE and hw & 1:
        front[:4], back[:4] = FIRST_FRONT_ODD, FIRST_BACK_ODD
        front[-4:], back[-4:] = LAST_FRONT_ODD, LAST_BACK_ODD
        return front, back
    front[:4], back[:4] = FIRST_FRONT, FIRST_BACK
    front[-4:], back[-4:] = LAST_FRONT, LAST_BACK
    return front, back


# the colour loop: a column's front half is issued one step before its back half, so only column 0 of a row
# comes from the row before (with [1]); the masks do not look at the parity
COLOUR_STAGES = ("parent", "ab")
COLOUR_FIRST_BACK, COLOUR_FIRST_FRONT = FIRST_BACK, (1, 3, 7, 15)
COLOUR_LAST_BACK, COLOUR_LAST_FRONT = LAST_BACK, (15, 14, 12, 8)
COLOUR_SINGLE_BACK, COLOUR_SINGLE_FRONT = SINGLE_BACK, SINGLE_FRONT
COLOUR_FORMS = {"and": (2, 1, 8, 4, 2), "msad": (2, 1, 8, 3, 2)}


def colour_issued_masks(hw, stage="ab"):
    """(front, back) masks per column of the row as the colour loop of `stage` issues them."""
    n = row_groups(hw)
    front, back = [FULL] * (4 * n), [FULL] * (4 * n)
    if stage == "parent":
        return front, back
    assert stage == "ab", stage
    if n == 1:
        return list(COLOUR_SINGLE_FRONT), list(COLOUR_SINGLE_BACK)
    front[:4], back[:4] = COLOUR_FIRST_FRONT, COLOUR_FIRST_BACK
    front[-4:], back[-4:] = COLOUR_LAST_FRONT, COLOUR_LAST_BACK
    return front, back


def _bits(m):
    return bin(m).count("1")


def count(radius, form="msad", stage="ab"):
    """Steps, slots and instructions of one wave's walk over the whole disk (the prologue before the first
    row and the row bookkeeping are not part of it)."""
    return _count(radius, form, stage, FORMS[form], issued_masks)


def count_colour(radius, form="msad", stage="ab"):
    """The same for the colour loop."""
    return _count(radius, form, stage, COLOUR_FORMS[form], colour_issued_masks)


def _count(radius, form, stage, costs, masks):
    fv, fl, bv, sv, sl = costs
    steps = slots = live = fronts = backs = 0
    for hw in half_widths(radius):
        lm = live_masks(hw)
        fm, bm = masks(hw, stage)
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


def reduction(radius, form="msad", stage="ab", counter=count):
    """The share of the parent loop's VALU and LDS instructions that `stage` leaves out (counter =
    count_colour: of the colour loop's)."""
    p, c = counter(radius, form, "parent"), counter(radius, form, stage)
    return {"radius": radius, "form": form, "stage": stage,
            "loop": "colour" if counter is count_colour else "grey",
            "valu_parent": p["valu"], "valu": c["valu"], "valu_drop": 1.0 - c["valu"] / p["valu"],
            "lds_parent": p["lds"], "lds": c["lds"], "lds_drop": 1.0 - c["lds"] / p["lds"],
            "dead_slots": p["slots"] - p["live_slots"], "back_slots_trimmed": p["slots"] - c["back_slots"],
            "front_slots_trimmed": p["slots"] - c["front_slots"]}


def main(argv):
    radii = [int(a) for a in argv] or [33, 42, 54]
    for radius in radii:
        for form in ("msad", "and", "j1"):
            for stage in ("a", "ab", PARITY_STAGE):
                print(json.dumps(reduction(radius, form, stage)))
        for form in ("msad", "and"):
            print(json.dumps(reduction(radius, form, "ab", count_colour)))


if __name__ == "__main__":
    main(sys.argv[1:])
