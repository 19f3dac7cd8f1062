"""The end groups of the colour tap loop of the joint bilateral (jbf_tap_loop_rgb6: first group [1, 3, 7, 15],
last group [15, 14, 12, 8], a row of one group [1, 2, 4, 8]) and the parity-aware end groups of the grey loop
(jbf_tap_loop_grey4_la2: rows of odd half-width run [0, 1, 3, 7] and [14, 12, 8, 0]) against the ORACLE and
against loops that share none of the inline assembly, byte for byte.

Shapes are those of tests/test_gpu_jbf_group_pairs.py (W x H = 75 x 70 and 70 x 141, two images per call: one
64x64 tile plus every strip class, reflected borders).

Colour loop - a 3-channel src whose channels differ, forms msad, and, mixed:

  flat      the joint is ONE non-grey colour without a zero byte (zeroed bytes in the first rows of a tile for
            mixed), the src three INDEPENDENT planes of two-level noise in {0, 255}: a live slot skipped by
            mistake moves one channel across a rounding boundary in dozens of pixels, a swapped channel
            changes nearly every byte (test_a_dropped_live_slot_shows_in_colour, without a device)
  natural   seeded colour scenes

  radius 1..12   every half-width parity, rows of one, two and three groups
  radius 33      the one-pass colour tile (pitch 144)
  radius 42, 52  the colour route of two or more passes (pitch 176: radius 37..52)
  radius 54      the slab kernel's colour pass: slabs of 49 rows, the second one starts at tap row -5, a row of
                 odd half-width (53) in the middle of the disk

Grey loop - which files drive the parity forms:

  tests/test_gpu_jbf_end_groups.py    radius 1..12, 33, 42 in the tile kernels: every radius from 2 on has rows
                                      of both parities (radius 1: half-widths 0, 1, 0), so both forms of the
                                      first and of the last group run in both roles, all four forms of the SAD;
                                      radius 54 in the slab kernel: slabs of 106 rows, they start on the
                                      disk's top row and at tap row 52 - half-widths 0 and 14, both EVEN
  tests/test_gpu_jbf_group_pairs.py   radius 70: slabs of 83 rows, the second one starts at tap row 13, whose
                                      half-width 68 is even too
  here                                radius 56 on the flat inputs of test_gpu_jbf_end_groups.py: slabs of 106
                                      rows, the second one starts at tap row 50, half-width 25 - the one slab
                                      launch of the grey loop that starts on an ODD row
                                      (test_slab_launches_that_start_on_an_odd_row computes, without a device,
                                      where the slabs of all these radii start)
"""
import numpy as np
import pytest

from tests import synth
from tests.test_gpu_fuzz import env  # noqa: F401  (a fixture)
from tests.test_gpu_jbf_group_pairs import SHAPES, SIGMA_COLOR, _first_difference, _options, _sigma_space
from tests import test_gpu_jbf_end_groups as grey
from tests.test_gpu_jbf_end_groups import FLAT_BGR, _bordering_slots, slots

RADII = tuple(range(1, 13)) + (33, 42, 52, 54)
FORMS = ("msad", "and", "mixed")
KINDS = ("flat", "natural")
GREY_SLAB_RADIUS = 56

_inputs = {}
_references = {}


def _noise3(h, w, seed):
    """Three independent two-level planes."""
    return (np.random.default_rng(seed).integers(0, 2, size=(h, w, 3)) * 255).astype(np.uint8)


def _images(kind, form, h, w):
    """(joint [2,h,w,3], src [2,h,w,3], the channels of src differ); "and" filters the images of "msad"."""
    key = (kind, "msad" if form == "and" else form, h, w)
    if key not in _inputs:
        seed = 5000 + 10 * h + w
        if kind == "flat":
            joint = np.empty((2, h, w, 3), np.uint8)
            joint[:] = FLAT_BGR
            src = np.stack([_noise3(h, w, seed + k) for k in range(2)])
        else:
            joint = np.stack([np.maximum(synth.scene_u8(h, w, seed + k), 1) for k in range(2)])
            src = np.stack([synth.scene_u8(h, w, seed + 5 + k) for k in range(2)])
        if key[1] == "mixed":
            # zero channels in rows 0..3 of the first tile only: that wave keeps the mask, the other
            # fifteen of the workgroup take the masked SAD
            rng = np.random.default_rng(seed)
            top = joint[:, 0:4, 0:64]
            top[rng.random(top.shape) < 0.2] = 0
        _inputs[key] = (np.ascontiguousarray(joint), np.ascontiguousarray(src))
    return _inputs[key]


def _reference(co, kind, form, h, w, radius):
    """The oracle's outputs [2,h,w,3], computed once per input set, form, size and radius."""
    key = (kind, "msad" if form == "and" else form, h, w, radius)
    if key not in _references:
        joint, src = _images(kind, form, h, w)
        _references[key] = np.stack([
            co.joint_bilateral_filter(j, s, 2 * radius + 1, SIGMA_COLOR, _sigma_space(radius)).reshape(s.shape)
            for j, s in zip(joint, src)])
    return _references[key]


def _run(rf, torch, kind, form, h, w, radius, flags=0, **opts):
    joint, src = _images(kind, form, h, w)
    tj, ts = torch.from_numpy(joint).cuda(), torch.from_numpy(src).cuda()
    with rf._ffi.debug_options(**_options(form, **opts)):
        out = rf.ops.joint_bilateral_u8(tj, ts, 2 * radius + 1, SIGMA_COLOR, _sigma_space(radius),
                                        flags=flags).cpu().numpy()
    torch.cuda.synchronize()
    return out


# ---------------------------------------------------------------- without a device


def test_colour_inputs_are_colour():
    """No tile of these inputs is grey (a grey tile would take the grey loop), the flat joint has no zero byte
    and the mixed one has some, in the first rows of the first tile only."""
    for kind in KINDS:
        for h, w in SHAPES:
            for form in ("msad", "mixed"):
                joint, src = _images(kind, form, h, w)
                assert joint.shape == src.shape == (2, h, w, 3)
                for y0 in range(0, h, 64):
                    for x0 in range(0, w, 64):
                        t = src[:, y0:y0 + 64, x0:x0 + 64].astype(int)
                        assert (t[..., 0] != t[..., 1]).any() and (t[..., 1] != t[..., 2]).any()
                if form == "msad":
                    assert joint.min() >= 1
                else:
                    assert (joint[:, 0:4, 0:64] == 0).any() and joint[:, 4:].min() >= 1
    flat = _images("flat", "msad", *SHAPES[0])[1]
    assert set(np.unique(flat)) == {0, 255}
    # independent planes: every one of the eight channel patterns occurs
    assert len(np.unique(flat.reshape(-1, 3), axis=0)) == 8


def test_slab_launches_that_start_on_an_odd_row(built):
    """Where the slab kernel's launches start (tap row -radius + k * slab rows, jbf_slab_kernel): the colour
    pass at radius 54 and the grey pass at radius 56 each have a slab whose first row has an odd half-width
    and at least two groups - the loop enters it through the odd forms, the prologue's gathers of all four
    outputs behind it; the grey passes at radius 54 and 70, which the older files run, have none."""
    from reflectance_filtering_amd import _ffi
    sizes = [(h, w) for h, w in SHAPES]

    def odd_starts(radius, scn):
        plan = _ffi.jbf_ragged_slab_plan(sizes, 3, scn, 2 * radius + 1, SIGMA_COLOR, _sigma_space(radius))
        assert plan is not None and (scn == 1 or plan[4] > 0)      # (scn 3: one pass of the colour loop)
        slab = plan[5] if scn == 3 else plan[3]
        hws = [slots.half_widths(radius)[i + radius] for i in range(-radius, radius + 1, slab)]
        assert len(hws) >= 2 and hws[0] == 0
        return [hw for hw in hws[1:] if hw & 1 and slots.row_groups(hw) >= 2]

    assert odd_starts(54, 3) and odd_starts(GREY_SLAB_RADIUS, 1)
    assert not odd_starts(54, 1) and not odd_starts(70, 1)


_model_sums = {}


def _model(radius, image):
    """Float64 model of the filter on the flat joint (every colour weight 1), per channel: padded src,
    weighted sums and weight sum per pixel."""
    key = (radius, image)
    if key not in _model_sums:
        h, w = SHAPES[0]
        src = _images("flat", "msad", h, w)[1][image].astype(np.float64)
        pad = np.pad(src, ((radius, radius), (radius, radius), (0, 0)), mode="reflect")
        coeff = -0.5 / _sigma_space(radius) ** 2
        num, den = np.zeros((h, w, 3)), np.zeros((h, w, 1))
        for i in range(-radius, radius + 1):
            hw = slots.half_widths(radius)[i + radius]
            for j in range(-hw, hw + 1):
                wgt = np.exp((i * i + j * j) * coeff)
                num += wgt * pad[radius + i:radius + i + h, radius + j:radius + j + w]
                den += wgt
        _model_sums[key] = (pad, num, den)
    return _model_sums[key]


@pytest.mark.parametrize("radius", (3, 12, 33))
def test_a_dropped_live_slot_shows_in_colour(radius):
    """On the flat colour inputs a model that leaves out ONE live slot next to a trimmed one - one tap of one
    output class in one row, in all three channels - differs from the full model in at least one byte: for
    each such slot of the first and of the last group, in the row nearest the centre of EITHER parity of the
    half-width where the slot is live (in odd rows the slots next to the trimmed ones are those beside the
    diagonal).  A loop that trimmed one slot too many - the colour loop's masks or the grey loop's odd forms -
    would fail the comparisons below."""
    h, w = SHAPES[0]
    coeff = -0.5 / _sigma_space(radius) ** 2
    hws_of = slots.half_widths(radius)
    checked = {0: 0, 1: 0}
    for last in (False, True):
        for u, o in _bordering_slots(last):
            for parity in (0, 1):
                rows = [i for i in sorted(range(-radius, radius + 1), key=abs)
                        if hws_of[i + radius] & 1 == parity and slots.row_groups(hws_of[i + radius]) >= 2
                        and slots.live_masks(hws_of[i + radius])[(-4 if last else 0) + u] >> o & 1]
                if not rows:
                    # the diagonal is dead in every odd row: that is the parity trim
                    assert parity == 1 and u == o, (radius, last, u, o, parity)
                    continue
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
                checked[parity] += 1
    assert checked[0] == 14 and checked[1] == 6


# ---------------------------------------------------------------- on the device


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("radius", RADII)
def test_colour_end_groups_match_the_oracle(env, radius, form):
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
def test_colour_end_groups_equal_a_loop_without_the_asm(env, radius, form):
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
def test_colour_ragged_entry_gives_the_bytes_of_the_uniform_entry(env, radius, form):
    """One ragged call over a list of the two sizes: per image the uniform entry's bytes, the oracle's."""
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
                                                        _sigma_space(radius))
            got = [v.cpu().numpy() for v in views]
        torch.cuda.synchronize()
        for i, (h, w) in enumerate(SHAPES):
            want = _reference(co, kind, form, h, w, radius)[0]
            assert np.array_equal(got[i].reshape(uniform[i].shape), uniform[i]), \
                "%s image %d (%d x %d): the ragged entry differs from the uniform one" % (kind, i, w, h)
            assert np.array_equal(uniform[i], want), "%s image %d (%d x %d) differs from the oracle" % (
                kind, i, w, h)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_grey_slab_that_starts_on_an_odd_row(env, form):
    """The grey loop in the slab kernel at radius 56 on the flat inputs: the second slab starts on a row of odd
    half-width.  The oracle's bytes, the one-thread-per-pixel kernel's, through both entries."""
    rf, co, torch = env
    radius = GREY_SLAB_RADIUS
    joints, srcs, uniform = [], [], []
    for h, w in SHAPES:
        want = grey._reference(co, "flat", form, h, w, radius)
        got = grey._run(rf, torch, "flat", form, h, w, radius)
        other = grey._run(rf, torch, "flat", form, h, w, radius, flags=rf._ffi.JBF_FORCE_GENERIC)
        assert _first_difference(got, want) is None, "%d x %d: %s" % (w, h, _first_difference(got, want))
        assert _first_difference(other, want) is None, "%d x %d, the untiled kernel: %s" % (
            w, h, _first_difference(other, want))
        joint, src = grey._images("flat", form, h, w)
        joints.append(torch.from_numpy(np.ascontiguousarray(joint[0])).cuda())
        srcs.append(torch.from_numpy(np.ascontiguousarray(src[0])).cuda())
        uniform.append(got[0])
    with rf._ffi.debug_options(**_options(form)):
        _, views = rf.ops.joint_bilateral_ragged_u8(joints, srcs, 2 * radius + 1, SIGMA_COLOR,
                                                    _sigma_space(radius))
        ragged = [v.cpu().numpy() for v in views]
    torch.cuda.synchronize()
    for i, (h, w) in enumerate(SHAPES):
        assert np.array_equal(ragged[i].reshape(uniform[i].shape), uniform[i]), \
            "image %d (%d x %d): the ragged entry differs from the uniform one" % (i, w, h)
