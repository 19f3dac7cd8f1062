"""The end-group masks that look at the parity of a tap row's half-width (grey loop, stage "abp" of
tools/jbf_slot_count.py) and the parity-independent masks of the colour loop, without a device: for every
half-width the masks hold every live output, no back half runs without its front half, and nothing more
could be left out - over the rows of one parity the live outputs unite to exactly the masks of that parity.
"""
import importlib.util
import os

_spec = importlib.util.spec_from_file_location(
    "jbf_slot_count", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools",
                                   "jbf_slot_count.py"))
slots = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(slots)

HALF_WIDTHS = range(469)       # every half-width a radius up to 468 has


def test_every_half_width_occurs():
    assert sorted({hw for radius in range(1, 469) for hw in slots.half_widths(radius)}) == list(HALF_WIDTHS)


def test_odd_masks_are_the_even_ones_less_the_dead_column():
    assert slots.FIRST_BACK_ODD == (0, 1, 3, 7) and slots.LAST_BACK_ODD == (14, 12, 8, 0)
    # a row's columns 0 and 1 are formed by the row before with [1, 3], the last group's columns 0 and 1 by
    # the group before with every output
    assert slots.FIRST_FRONT_ODD == (1, 3, 3, 7) and slots.LAST_FRONT_ODD == (15, 15, 8, 0)
    assert slots.FIRST_FRONT_ODD[:2] == slots.FIRST_FRONT[:2] == slots.SINGLE_FRONT[:2]
    assert slots.PARITY_STAGE == "abp" and slots.STAGES == ("parent", "a", "ab")
    for odd, even in ((slots.FIRST_BACK_ODD, slots.FIRST_BACK), (slots.LAST_BACK_ODD, slots.LAST_BACK),
                      (slots.FIRST_FRONT_ODD, slots.FIRST_FRONT), (slots.LAST_FRONT_ODD, slots.LAST_FRONT)):
        assert all(o & e == o for o, e in zip(odd, even))


def test_parity_masks_hold_every_live_output_and_nothing_more():
    first = {0: [0] * 4, 1: [0] * 4}
    last = {0: [0] * 4, 1: [0] * 4}
    for hw in HALF_WIDTHS:
        live = slots.live_masks(hw)
        front, back = slots.issued_masks(hw, "abp")
        assert len(front) == len(back) == len(live) == 4 * slots.row_groups(hw)
        for l, f, b in zip(live, front, back):
            assert l & b == l, hw          # every live output is issued
            assert b & f == b, hw          # no back half without its front half
        if hw & 1:
            assert slots.row_groups(hw) >= 2, hw       # an odd row is never a row of one group
        if slots.row_groups(hw) >= 2:
            first[hw & 1] = [a | b for a, b in zip(first[hw & 1], live[:4])]
            last[hw & 1] = [a | b for a, b in zip(last[hw & 1], live[-4:])]
            # between the end groups every slot is issued
            assert set(front[4:-4]) | set(back[4:-4]) <= {slots.FULL}
        else:
            assert hw == 0 and (front, back) == (list(slots.SINGLE_FRONT), list(slots.SINGLE_BACK))
    assert tuple(first[1]) == slots.FIRST_BACK_ODD and tuple(last[1]) == slots.LAST_BACK_ODD
    assert tuple(first[0]) == slots.FIRST_BACK and tuple(last[0]) == slots.LAST_BACK


def test_odd_rows_issue_exactly_their_live_slots():
    """In a row of odd half-width - and in one of even half-width - the back halves issued are the live
    slots: what the parity-independent masks left over is gone."""
    for hw in HALF_WIDTHS:
        live = slots.live_masks(hw)
        _, back = slots.issued_masks(hw, "abp")
        assert back == live, hw


def test_the_last_group_forms_the_next_row_for_either_parity():
    """The fronts a row's columns 0 and 1 arrive with do not depend on the parity of the row that formed
    them, nor on that of the row itself: [1, 3] - and the first group of either parity (and the one-group
    row) runs a subset of them."""
    for hw in HALF_WIDTHS:
        front, back = slots.issued_masks(hw, "abp")
        assert tuple(front[:2]) == (1, 3), hw
        assert back[0] & 1 == back[0] and back[1] & 3 == back[1], hw


def test_radius_33_figures():
    c = slots.count(33, "msad", "abp")
    assert c["back_slots"] == c["live_slots"] == 13636
    assert c["front_slots"] == 13811
    assert c["valu"] == 85830 and c["lds"] == 15643
    ab = slots.count(33, "msad", "ab")
    assert (ab["valu"], ab["lds"]) == (86910, 15751)
    assert ab["back_slots"] - c["back_slots"] == 216 and ab["front_slots"] - c["front_slots"] == 108
    assert sum(hw & 1 for hw in slots.half_widths(33)) == 27 and len(slots.half_widths(33)) == 67
    r = slots.reduction(33, "msad", "abp")
    assert r["back_slots_trimmed"] == r["dead_slots"] == 1020
    for radius, valu, lds in ((33, 0.0124, 0.0069), (42, 0.0153, 0.0085), (54, 0.0097, 0.0053)):
        ab, abp = slots.count(radius, "msad", "ab"), slots.count(radius, "msad", "abp")
        assert abs(1 - abp["valu"] / ab["valu"] - valu) < 5e-5
        assert abs(1 - abp["lds"] / ab["lds"] - lds) < 5e-5
    for form in ("and", "j1"):
        assert slots.count(33, form, "abp")["valu"] < slots.count(33, form, "ab")["valu"]


def test_colour_masks_hold_every_live_output_and_nothing_more():
    assert slots.COLOUR_FIRST_BACK == slots.COLOUR_FIRST_FRONT == (1, 3, 7, 15)
    assert slots.COLOUR_LAST_BACK == slots.COLOUR_LAST_FRONT == (15, 14, 12, 8)
    assert slots.COLOUR_SINGLE_BACK == (1, 2, 4, 8) and slots.COLOUR_SINGLE_FRONT == (1, 3, 4, 8)
    first, last = [0] * 4, [0] * 4
    for hw in HALF_WIDTHS:
        live = slots.live_masks(hw)
        front, back = slots.colour_issued_masks(hw, "ab")
        assert len(front) == len(back) == len(live)
        for l, f, b in zip(live, front, back):
            assert l & b == l and b & f == b, hw
        # column 0 of a row is formed by the last step of the row before, with [1] whatever the rows
        assert front[0] == 1, hw
        if slots.row_groups(hw) >= 2:
            first = [a | b for a, b in zip(first, live[:4])]
            last = [a | b for a, b in zip(last, live[-4:])]
            assert set(front[4:-4]) | set(back[4:-4]) <= {slots.FULL}
        else:
            assert hw == 0 and live == list(slots.COLOUR_SINGLE_BACK)
        assert slots.colour_issued_masks(hw, "parent") == ([15] * len(live), [15] * len(live))
    assert tuple(first) == slots.COLOUR_FIRST_BACK and tuple(last) == slots.COLOUR_LAST_BACK


def test_colour_radius_33_figures():
    """A full step of the colour loop is 43 (MSAD) / 44 VALU and 6 LDS instructions; the masks take out 804
    back and 802 front slots of 14,656: 5.1 % of the VALU instructions."""
    p = slots.count_colour(33, "msad", "parent")
    assert (p["steps"], p["slots"], p["live_slots"]) == (3664, 14656, 13636)
    assert p["valu"] == 43 * 3664 and p["lds"] == 6 * 3664
    assert slots.count_colour(33, "and", "parent")["valu"] == 44 * 3664
    c = slots.count_colour(33, "msad", "ab")
    assert p["slots"] - c["back_slots"] == 804 and p["slots"] - c["front_slots"] == 802
    assert c["valu"] == p["valu"] - 8 * 804 - 2 * 802 and c["lds"] == p["lds"] - 802
    assert 0.050 < 1 - c["valu"] / p["valu"] < 0.052
    for radius in (1, 2, 3, 42, 54):
        p, c = slots.count_colour(radius, "and", "parent"), slots.count_colour(radius, "and", "ab")
        assert c["live_slots"] <= c["back_slots"] <= c["front_slots"] <= p["slots"]
        assert c["valu"] < p["valu"] and c["lds"] < p["lds"]
