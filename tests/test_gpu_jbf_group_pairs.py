"""The grey tap loop of the joint bilateral in its pair form (jbf_tap_loop_grey4_la2: two groups of four
column steps per loop iteration, the two weight windows in two SGPR octets that swap roles from group
to group, rows that start in either role) against the ORACLE, byte for byte.

Inputs are seeded tests/synth.py images, two per call, W x H = 75 x 70 and 70 x 141: one 64x64 tile plus
every strip class, reflected borders on all sides.  The places where the pair form can go wrong:

  radius 1, 2, 3       rows of 1, 2, 1 groups (lone groups, rows without a pair, a role change at every
                       row) and of 1, 2, 3 groups
  radius 7, 33         pitch 144; 33 is the benchmark's
  radius 42, 52        pitch 176
  radius 54, 70        the slab kernel: slabs start and end on rows of either parity, in either role
  every form           msad (3-channel joint, grey 3-channel src), and (the same under jbf_no_msad), mixed (a
                       joint with zero channels in the first rows of a tile only: both forms within one
                       workgroup), j1 (1-channel joint and src with grey_as_bgr)
  jbf_tile64_only      strips against 64x64 tiles
  ragged               the list entry on the two sizes: the bytes of the uniform entry per image
  other loop           the same call through code that shares none of the inline assembly: up to radius 52
                       the compiler-scheduled tap loop (jbf_compiler_loop, a switch of jbf_tile64_kernel only);
                       the slab kernel has no such switch, so radius 54 and 70 are cross-checked against
                       the one-thread-per-pixel kernel (RF_JBF_FORCE_GENERIC)

The reference side runs without a device (test_reference_side_needs_no_device): the oracle reproduces
itself on these inputs with one thread and with many.
"""
import numpy as np
import pytest

from tests import synth
from tests.test_gpu_fuzz import env  # noqa: F401  (a fixture)

SHAPES = ((70, 75), (141, 70))          # (h, w)
RADII = (1, 2, 3, 7, 33, 42, 52, 54, 70)
FORMS = ("msad", "and", "mixed", "j1")
SIGMA_COLOR = 25.0

_inputs = {}
_references = {}


def _sigma_space(radius):
    return max(radius / 1.5, 0.5)


def _images(form, h, w):
    """(joint [2,h,w,jcn], src [2,h,w,scn]) of one form and size; "and" filters the images of "msad"."""
    key = ("msad" if form == "and" else form, h, w)
    if key not in _inputs:
        seed = 9000 + 10 * h + w
        if key[0] == "j1":
            joint = np.stack([synth.reflectance_like_u8(h, w, seed + k)[:, :, :1] for k in range(2)])
            src = np.stack([synth.reflectance_like_u8(h, w, seed + 5 + k)[:, :, :1] for k in range(2)])
        else:
            joint = np.stack([np.maximum(synth.scene_u8(h, w, seed + k), 1) for k in range(2)])
            src = np.stack([synth.reflectance_like_u8(h, w, seed + 5 + k) for k in range(2)])
            if key[0] == "mixed":
                # zero channels in rows 0..3 of the first tile only: that wave keeps the mask, the
                # other fifteen of the workgroup take the masked SAD
                rng = np.random.default_rng(seed)
                top = joint[:, 0:4, 0:64]
                top[rng.random(top.shape) < 0.2] = 0
        _inputs[key] = (np.ascontiguousarray(joint), np.ascontiguousarray(src))
    return _inputs[key]


def _reference(co, form, h, w, radius, threads=0):
    """The oracle's outputs [2,h,w,scn] for one form, size and radius, computed once."""
    key = ("msad" if form == "and" else form, h, w, radius)
    if key not in _references or threads:
        joint, src = _images(form, h, w)
        outs = []
        for j, s in zip(joint, src):
            j3 = np.repeat(j, 3, axis=2) if j.shape[2] == 1 else j    # grey_as_bgr
            outs.append(co.joint_bilateral_filter(j3, s, 2 * radius + 1, SIGMA_COLOR,
                                                  _sigma_space(radius), threads=threads).reshape(s.shape))
        if threads:
            return np.stack(outs)
        _references[key] = np.stack(outs)
    return _references[key]


def _first_difference(got, want):
    bad = np.argwhere((got != want).reshape(got.shape[0], got.shape[1], got.shape[2], -1).any(axis=3))
    if bad.size == 0:
        return None
    n, y, x = bad[0]
    return "%d pixels differ, first (image %d, y %d, x %d) got %s want %s" % (
        len(bad), n, y, x, got[n, y, x], want[n, y, x])


def _options(form, **more):
    opts = dict(more)
    if form == "and":
        opts["jbf_no_msad"] = 1
    return opts


def _run(rf, torch, form, h, w, radius, flags=0, **opts):
    joint, src = _images(form, h, w)
    tj, ts = torch.from_numpy(joint).cuda(), torch.from_numpy(src).cuda()
    with rf._ffi.debug_options(**_options(form, **opts)):
        out = rf.ops.joint_bilateral_u8(tj, ts, 2 * radius + 1, SIGMA_COLOR, _sigma_space(radius),
                                        flags=flags, grey_as_bgr=(form == "j1")).cpu().numpy()
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("radius", RADII)
def test_reference_side_needs_no_device(built, radius):
    """The oracle on the inputs of this file, without a GPU: one thread (four above radius 7) and all
    give the same bytes,
    the result has the src's shape and is a filtered image (not the src, not a constant)."""
    from oracle import c_oracle as co
    for form in ("msad", "mixed", "j1"):
        for h, w in SHAPES:
            ref = _reference(co, form, h, w, radius)
            again = _reference(co, form, h, w, radius, threads=1 if radius <= 7 else 4)
            _, src = _images(form, h, w)
            assert ref.shape == src.shape and ref.dtype == np.uint8
            assert np.array_equal(ref, again)
            assert not np.array_equal(ref, src) and ref.min() != ref.max()


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("radius", RADII)
def test_pair_loop_matches_the_oracle(env, radius, form):
    """Uniform entry, strips and 64x64 tiles only: every byte equals the oracle's."""
    rf, co, torch = env
    for h, w in SHAPES:
        want = _reference(co, form, h, w, radius)
        for only64 in (0, 1):
            got = _run(rf, torch, form, h, w, radius, jbf_tile64_only=only64)
            assert _first_difference(got, want) is None, "%d x %d, jbf_tile64_only=%d: %s" % (
                w, h, only64, _first_difference(got, want))


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("radius", RADII)
def test_pair_loop_equals_a_loop_without_the_asm(env, radius, form):
    """The same call through the compiler-scheduled tap loop (the tile kernel, radius <= 52) or the
    one-thread-per-pixel kernel (radius 54 and 70, where jbf_compiler_loop switches nothing): equal
    bytes (and the oracle's)."""
    rf, co, torch = env
    for h, w in SHAPES:
        got = _run(rf, torch, form, h, w, radius)
        if radius <= 52:
            other = _run(rf, torch, form, h, w, radius, jbf_compiler_loop=1)
        else:
            other = _run(rf, torch, form, h, w, radius, flags=rf._ffi.JBF_FORCE_GENERIC)
        assert _first_difference(got, other) is None, "%d x %d: %s" % (w, h, _first_difference(got, other))
        want = _reference(co, form, h, w, radius)
        assert _first_difference(other, want) is None, "%d x %d, the other loop against the oracle: %s" % (
            w, h, _first_difference(other, want))


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("radius", RADII)
def test_ragged_entry_gives_the_bytes_of_the_uniform_entry(env, radius, form):
    """One ragged call over a list of the two sizes: per image the uniform entry's bytes."""
    rf, co, torch = env
    joints, srcs, uniform = [], [], []
    for h, w in SHAPES:
        joint, src = _images(form, h, w)
        joints.append(torch.from_numpy(np.ascontiguousarray(joint[0])).cuda())
        srcs.append(torch.from_numpy(np.ascontiguousarray(src[0])).cuda())
        uniform.append(_run(rf, torch, form, h, w, radius)[0])
    with rf._ffi.debug_options(**_options(form)):
        _, views = rf.ops.joint_bilateral_ragged_u8(joints, srcs, 2 * radius + 1, SIGMA_COLOR,
                                                    _sigma_space(radius), grey_as_bgr=(form == "j1"))
        got = [v.cpu().numpy() for v in views]
    torch.cuda.synchronize()
    for i, (h, w) in enumerate(SHAPES):
        want = _reference(co, form, h, w, radius)[0]
        assert np.array_equal(got[i].reshape(uniform[i].shape), uniform[i]), \
            "image %d (%d x %d): the ragged entry differs from the uniform one" % (i, w, h)
        assert np.array_equal(uniform[i], want), "image %d (%d x %d) differs from the oracle" % (i, w, h)
