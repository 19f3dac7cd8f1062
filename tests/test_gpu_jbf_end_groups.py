"""The trimmed end groups of the grey tap loop of the joint bilateral (jbf_tap_loop_grey4_la2: the first and
the last group of four column steps of every tap row leave out the slots - column x output - that lie
outside the output's disk whatever the parity of the row's half-width) against the ORACLE and against
loops that share none of the inline assembly, byte for byte.

Shapes and forms are those of tests/test_gpu_jbf_group_pairs.py (W x H = 75 x 70 and 70 x 141, two images
per call: one 64x64 tile plus every strip class, reflected borders; msad, and, mixed, j1).  Two sets of
inputs:

  flat      the joint is ONE non-grey colour without a zero byte (B, G, R = 90, 120, 150; one channel for j1;
            zeroed bytes in the first rows of a tile for mixed), so every colour weight is 1, and the src is
            seeded two-level noise in {0, 255}: an output is the spatially weighted share of bright taps,
            and a live slot skipped by mistake - one tap of one output class in one row - moves it across a
            rounding boundary in dozens of pixels (test_a_dropped_live_slot_shows, on a float64 model,
            without a device)
  natural   the seeded images of the existing file

  radius 1..12   every half-width parity, rows of one, two and three groups, a role change at every row
  radius 33, 42  the benchmark's (pitch 144); pitch 176
  radius 54      the slab kernel: slabs start on rows of either parity and role

The masks and the slot counts come from tools/jbf_slot_count.py, which needs no device either.
"""
import importlib.util
import os

import numpy as np
import pytest

from tests.test_gpu_fuzz import env  # noqa: F401  (a fixture)
from tests.test_gpu_jbf_group_pairs import (SHAPES, SIGMA_COLOR, _first_difference, _options, _sigma_space)
from tests.test_gpu_jbf_group_pairs import _images as _natural_images

RADII = tuple(range(1, 13)) + (33, 42, 54)
FORMS = ("msad", "and", "mixed", "j1")
KINDS = ("flat", "natural")
FLAT_BGR = (90, 120, 150)

_spec = importlib.util.spec_from_file_location(
    "jbf_slot_count", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools",
                                   "jbf_slot_count.py"))
slots = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(slots)

_inputs = {}
_references = {}


def _noise(h, w, seed):
    return (np.random.default_rng(seed).integers(0, 2, size=(h, w, 1)) * 255).astype(np.uint8)


def _images(kind, form, h, w):
    """(joint [2,h,w,jcn], src [2,h,w,scn]); "and" filters the images of "msad"."""
    if kind == "natural":
        return _natural_images(form, h, w)
    key = ("msad" if form == "and" else form, h, w)
    if key not in _inputs:
        seed = 7000 + 10 * h + w
        if key[0] == "j1":
            joint = np.full((2, h, w, 1), FLAT_BGR[1], np.uint8)
            src = np.stack([_noise(h, w, seed + k) for k in range(2)])
        else:
            joint = np.empty((2, h, w, 3), np.uint8)
            joint[:] = FLAT_BGR
            src = np.stack([np.repeat(_noise(h, w, seed + k), 3, axis=2) for k in range(2)])
            if key[0] == "mixed":
                # zero channels in rows 0..3 of the first tile only: that wave keeps the mask, the
                # other fifteen of the workgroup take the masked SAD
                rng = np.random.default_rng(seed)
                top = joint[:, 0:4, 0:64]
                top[rng.random(top.shape) < 0.2] = 0
        _inputs[key] = (np.ascontiguousarray(joint), np.ascontiguousarray(src))
    return _inputs[key]


def _reference(co, kind, form, h, w, radius, threads=0):
    """The oracle's outputs [2,h,w,scn], computed once per input set, form, size and radius."""
    key = (kind, "msad" if form == "and" else form, h, w, radius)
    if key not in _references or threads:
        joint, src = _images(kind, form, h, w)
        outs = []
        for j, s in zip(joint, src):
            j3 = np.repeat(j, 3, axis=2) if j.shape[2] == 1 else j    # grey_as_bgr
            outs.append(co.joint_bilateral_filter(j3, s, 2 * radius + 1, SIGMA_COLOR,
                                                  _sigma_space(radius), threads=threads).reshape(s.shape))
        if threads:
            return np.stack(outs)
        _references[key] = np.stack(outs)
    return _references[key]


def _run(rf, torch, kind, form, h, w, radius, flags=0, **opts):
    joint, src = _images(kind, form, h, w)
    tj, ts = torch.from_numpy(joint).cuda(), torch.from_numpy(src).cuda()
    with rf._ffi.debug_options(**_options(form, **opts)):
        out = rf.ops.joint_bilateral_u8(tj, ts, 2 * radius + 1, SIGMA_COLOR, _sigma_space(radius),
                                        flags=flags, grey_as_bgr=(form == "j1")).cpu().numpy()
    torch.cuda.synchronize()
    return out


# ---------------------------------------------------------------- without a device


@pytest.mark.parametrize("radius", RADII)
def test_reference_side_needs_no_device(built, radius):
    """The oracle on the flat inputs of this file, without a GPU: one thread (four above radius 7) and all
    give the same bytes, and the result is a filtered image (not the src, not a constant)."""
    from oracle import c_oracle as co
    for form in ("msad", "mixed", "j1"):
        for h, w in SHAPES:
            ref = _reference(co, "flat", form, h, w, radius)
            again = _reference(co, "flat", form, h, w, radius, threads=1 if radius <= 7 else 4)
            _, src = _images("flat", form, h, w)
            assert ref.shape == src.shape and ref.dtype == np.uint8
            assert np.array_equal(ref, again)
            assert not np.array_equal(ref, src) and ref.min() != ref.max()


def test_masks_hold_every_live_output():
    """For every row of every radius 1..468 the masks the loop issues - [1, 3, 7, 15] for the columns of
    the first group, [15, 14, 12, 8] for those of the last, their intersection in a row of one group -
    hold every output whose disk has the column, the front masks hold the back masks, and over all rows
    of two groups or more the live outputs unite to exactly these masks (nothing more could be left out
    without looking at the parity)."""
    assert slots.FIRST_BACK == (1, 3, 7, 15) and slots.LAST_BACK == (15, 14, 12, 8)
    assert slots.SINGLE_BACK == (1, 2, 4, 8)
    first, last = [0] * 4, [0] * 4
    # (a row's masks depend on its half-width alone: every half-width that occurs, once)
    seen = sorted({hw for radius in range(1, 469) for hw in slots.half_widths(radius)})
    assert seen == list(range(469))
    for hw in seen:
        live = slots.live_masks(hw)
        assert len(live) == 4 * slots.row_groups(hw)
        for stage in ("a", "ab"):
            front, back = slots.issued_masks(hw, stage)
            assert len(front) == len(back) == len(live)
            for l, f, b in zip(live, front, back):
                assert l & b == l, (hw, stage)
                assert b & f == b, (hw, stage)
        if len(live) >= 8:
            first = [a | b for a, b in zip(first, live[:4])]
            last = [a | b for a, b in zip(last, live[-4:])]
        else:
            assert hw == 0 and live == list(slots.SINGLE_BACK)
    assert tuple(first) == slots.FIRST_BACK and tuple(last) == slots.LAST_BACK


def test_slot_counts_at_the_benchmark_radius():
    """The row walk of the counting tool is the one bench.py's valu_roofline prices (3,664 steps per output
    quad at radius 33), a full step is 26 / 25 / 22 VALU and 4.5 LDS instructions, and the trimmed loop
    issues every live slot."""
    p = slots.count(33, "msad", "parent")
    assert (p["steps"], p["slots"], p["live_slots"]) == (3664, 14656, 13636)
    assert p["valu"] == 25 * 3664 and p["lds"] == 4.5 * 3664
    assert slots.count(33, "and", "parent")["valu"] == 26 * 3664
    assert slots.count(33, "j1", "parent")["valu"] == 22 * 3664
    for radius in (1, 2, 3, 33, 42, 54):
        a, ab = slots.count(radius, "msad", "a"), slots.count(radius, "msad", "ab")
        assert ab["live_slots"] <= ab["back_slots"] <= ab["front_slots"] <= a["front_slots"] <= a["slots"]
        assert ab["valu"] < a["valu"] < slots.count(radius, "msad", "parent")["valu"]


_model_sums = {}


def _model(radius, image):
    """Float64 model of the filter on a flat joint (every colour weight 1): padded src plane, weighted sum
    and weight sum per pixel, the disk's spatial weights."""
    key = (radius, image)
    if key not in _model_sums:
        h, w = SHAPES[0]
        src = _images("flat", "msad", h, w)[1][image, :, :, 0].astype(np.float64)
        pad = np.pad(src, radius, mode="reflect")
        coeff = -0.5 / _sigma_space(radius) ** 2
        num, den = np.zeros((h, w)), np.zeros((h, w))
        for i in range(-radius, radius + 1):
            hw = slots.half_widths(radius)[i + radius]
            for j in range(-hw, hw + 1):
                wgt = np.exp((i * i + j * j) * coeff)
                num += wgt * pad[radius + i:radius + i + h, radius + j:radius + j + w]
                den += wgt
        _model_sums[key] = (pad, num, den)
    return _model_sums[key]


def _bordering_slots(last):
    """(column u, output o) of the live slots of an end group that border a trimmed one: the diagonal and
    the live side next to it."""
    if last:
        return [(u, u) for u in range(4)] + [(u, u + 1) for u in range(3)]
    return [(u, u) for u in range(4)] + [(u, u - 1) for u in range(1, 4)]


@pytest.mark.parametrize("radius", (3, 12, 33))
def test_a_dropped_live_slot_shows(radius):
    """On the flat-joint inputs a model that leaves out ONE live slot next to a trimmed one - one tap of one
    output class in one row - differs from the full model in at least one byte: for each such slot of the
    first group and of the last group (the four on the diagonal, live in rows of even half-width, and the
    three beside them), in the row nearest the centre where the slot is live.  A loop that trimmed one slot
    too many would fail the comparisons below."""
    h, w = SHAPES[0]
    coeff = -0.5 / _sigma_space(radius) ** 2
    hws_of = slots.half_widths(radius)
    for last in (False, True):
        for u, o in _bordering_slots(last):
            rows = [i for i in sorted(range(-radius, radius + 1), key=abs)
                    if slots.row_groups(hws_of[i + radius]) >= 2
                    and slots.live_masks(hws_of[i + radius])[(-4 if last else 0) + u] >> o & 1]
            assert rows, (radius, last, u, o)
            i = rows[0]
            hw = hws_of[i + radius]
            c = 4 * (slots.row_groups(hw) - 1) + u if last else u
            j = c - ((hw + 1) & ~1) - o          # the tap's column offset from the output
            assert abs(j) <= hw
            flipped = 0
            for image in range(2):
                pad, num, den = _model(radius, image)
                wgt = np.exp((i * i + j * j) * coeff)
                tap = pad[radius + i:radius + i + h, radius + j:radius + j + w]
                full = np.rint(num / den)
                cut = np.rint((num - wgt * tap) / (den - wgt))
                flipped += int((full != cut)[:, o::4].sum())     # tiles start at multiples of 64
            assert flipped >= 1, (radius, "last" if last else "first", u, o, i, j)


# ---------------------------------------------------------------- on the device


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("radius", RADII)
def test_end_groups_match_the_oracle(env, radius, form):
    """Uniform entry, strips and 64x64 tiles only (jbf_tile64_only): every byte equals the oracle's."""
    rf, co, torch = env
    for kind in KINDS:
        for h, w in SHAPES:
            want = _reference(co, kind, form, h, w, radius)
            for only64 in (0, 1):
                got = _run(rf, torch, kind, form, h, w, radius, jbf_tile64_only=only64)
                assert _first_difference(got, want) is None, "%s %d x %d, jbf_tile64_only=%d: %s" % (
                    kind, w, h, only64, _first_difference(got, want))


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("radius", RADII)
def test_end_groups_equal_a_loop_without_the_asm(env, radius, form):
    """The same call through the compiler-scheduled tap loop (the tile kernel, radius <= 52) or the
    one-thread-per-pixel kernel (radius 54, where jbf_compiler_loop switches nothing): equal bytes (and
    the oracle's)."""
    rf, co, torch = env
    for kind in KINDS:
        for h, w in SHAPES:
            got = _run(rf, torch, kind, form, h, w, radius)
            if radius <= 52:
                other = _run(rf, torch, kind, form, h, w, radius, jbf_compiler_loop=1)
            else:
                other = _run(rf, torch, kind, form, h, w, radius, flags=rf._ffi.JBF_FORCE_GENERIC)
            assert _first_difference(got, other) is None, "%s %d x %d: %s" % (
                kind, w, h, _first_difference(got, other))
            want = _reference(co, kind, form, h, w, radius)
            assert _first_difference(other, want) is None, "%s %d x %d, the other loop against the oracle: %s" % (
                kind, w, h, _first_difference(other, want))


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("radius", RADII)
def test_ragged_entry_gives_the_bytes_of_the_uniform_entry(env, radius, form):
    """One ragged call over a list of the two sizes: per image the uniform entry's bytes."""
    rf, co, torch = env
    for kind in KINDS:
        joints, srcs, uniform = [], [], []
        for h, w in SHAPES:
            joint, src = _images(kind, form, h, w)
            joints.append(torch.from_numpy(np.ascontiguousarray(joint[0])).cuda())
            srcs.append(torch.from_numpy(np.ascontiguousarray(src[0])).cuda())
            uniform.append(_run(rf, torch, kind, form, h, w, radius)[0])
        with rf._ffi.debug_options(**_options(form)):
            _, views = rf.ops.joint_bilateral_ragged_u8(joints, srcs, 2 * radius + 1, SIGMA_COLOR,
                                                        _sigma_space(radius), grey_as_bgr=(form == "j1"))
            got = [v.cpu().numpy() for v in views]
        torch.cuda.synchronize()
        for i, (h, w) in enumerate(SHAPES):
            want = _reference(co, kind, form, h, w, radius)[0]
            assert np.array_equal(got[i].reshape(uniform[i].shape), uniform[i]), \
                "%s image %d (%d x %d): the ragged entry differs from the uniform one" % (kind, i, w, h)
            assert np.array_equal(uniform[i], want), "%s image %d (%d x %d) differs from the oracle" % (
                kind, i, w, h)
