"""GPU suite: the masked-SAD form of the joint bilateral tap loops (v_msad_u8 on the unmasked tap
texel, taken per wave where no centre pixel of the wave has a zero joint channel) against the form
with the mask, which every other wave keeps and the debug option "jbf_no_msad" forces on all.

Every case is held byte for byte to the ORACLE, once by default and once under jbf_no_msad, and the
two outputs must be equal.  Shapes are W x H = 96 x 80 at sigma_spatial 3 (radius 5) unless the
case says otherwise; a wave of the 64x64 tile kernel covers 4 tile rows of 64 columns.

  no zero channel      every wave takes the masked SAD; src bytes 0 and 255 ride in byte 3 of the texel
  zeros only at taps   v_msad_u8 masks by its REFERENCE operand: with tap and centre swapped a zero in
                       a tap channel would drop that channel's difference (only the oracle tells)
  zero at the centre   such a wave must have fallen back
  mixed waves          zero channels in rows 0..3 of a tile only: one wave falls back, fifteen do not
  all fallback         an all-black joint
  radius 33            W x H = 130 x 70, sigma_color 20, sigma_spatial 22, about 1 % zero channels
  radius 54            W x H = 80 x 72, sigma_spatial 36: the slab kernel
  ragged               two of the images above in one call
"""
import numpy as np
import pytest

from tests.test_gpu_fuzz import env  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

H, W = 80, 96
SC, SS = 30.0, 3.0


def _src(rng, h, w, scn):
    """Noise with the extremes forced in: bytes 0 and 255 in every row (colour: never a grey tile)."""
    s = rng.integers(0, 256, (h, w, scn)).astype(np.uint8)
    s[:, 0::5] = 0
    s[:, 1::5] = 255
    if scn == 3:
        s[:, 2::5, 1] = 17     # B != G: the tile is not grey, the colour loop runs
        s[:, 2::5, 0] = 200
    return s


def _joint_no_zero(rng, h, w):
    return rng.integers(1, 256, (h, w, 3)).astype(np.uint8)


def _joint_zero_taps(rng, h, w):
    """200 everywhere but a lattice of isolated pixels with one channel 0 (rows 4, 13, 22 ...: the
    waves of rows 0..3, 8..11, 16..19 ... have no such centre and see them as taps only)."""
    j = np.full((h, w, 3), 200, np.uint8)
    for k, (y, x) in enumerate((y, x) for y in range(4, h, 9) for x in range(5, w, 11)):
        j[y, x, k % 3] = 0
    return j


def _joint_zero_centres(rng, h, w):
    j = np.full((h, w, 3), 255, np.uint8)
    for k, (y, x) in enumerate((y, x) for y in range(2, h, 7) for x in range(3, w, 13)):
        j[y, x, k % 3] = 0
    return j


def _joint_mixed_waves(rng, h, w):
    j = _joint_no_zero(rng, h, w)
    top = j[0:4, 0:64]
    top[rng.random(top.shape) < 0.2] = 0
    return j


def _joint_black(rng, h, w):
    return np.zeros((h, w, 3), np.uint8)


def _joint_noise(rng, h, w):
    """Noise with about 1 % zero channels."""
    j = rng.integers(1, 256, (h, w, 3)).astype(np.uint8)
    j[rng.random(j.shape) < 0.01] = 0
    return j


JOINTS = {"no_zero": _joint_no_zero, "zero_taps": _joint_zero_taps, "zero_centres": _joint_zero_centres,
          "mixed_waves": _joint_mixed_waves, "black": _joint_black}


def _first_difference(got, want):
    bad = np.argwhere((got != want).any(axis=2))
    if bad.size == 0:
        return None
    y, x = bad[0]
    return "%d pixels differ, first (y %d, x %d) got %s want %s" % (len(bad), y, x, got[y, x], want[y, x])


def _both_forms(rf, torch, run):
    """run() by default and under jbf_no_msad: the two outputs as numpy arrays."""
    out = run()
    with rf._ffi.debug_options(jbf_no_msad=1):
        ref = run()
    torch.cuda.synchronize()
    return out, ref


def _check(rf, co, torch, joint, src, sc, ss, what):
    want = co.joint_bilateral_filter(joint, src, -1, sc, ss).reshape(src.shape)
    tj, ts = torch.from_numpy(joint[None]).cuda(), torch.from_numpy(src[None]).cuda()
    got, masked = _both_forms(rf, torch,
                              lambda: rf.ops.joint_bilateral_u8(tj, ts, -1, sc, ss)[0].cpu().numpy())
    assert _first_difference(masked, want) is None, \
        "%s, jbf_no_msad: %s" % (what, _first_difference(masked, want))
    assert _first_difference(got, want) is None, "%s, default: %s" % (what, _first_difference(got, want))
    assert np.array_equal(got, masked)
    return got


@pytest.mark.parametrize("scn", [1, 3])
@pytest.mark.parametrize("kind", sorted(JOINTS))
def test_small_radius_cases_match_the_oracle_in_both_forms(env, kind, scn):
    rf, co, torch = env
    rng = np.random.default_rng(7100 + 10 * sorted(JOINTS).index(kind) + scn)
    joint, src = JOINTS[kind](rng, H, W), _src(rng, H, W, scn)
    got = _check(rf, co, torch, joint, src, SC, SS, "%s scn %d" % (kind, scn))
    if kind == "zero_taps":
        # the outputs this case is about: a centre without a zero channel, a zero channel among its taps
        zero = (joint == 0).any(axis=2)
        near = np.zeros_like(zero)
        ys, xs = np.nonzero(zero)
        for y, x in zip(ys, xs):
            near[max(0, y - 5):y + 6, max(0, x - 5):x + 6] = True
        assert (near & ~zero).sum() > 1000 and got.shape == src.shape


@pytest.mark.parametrize("scn", [1, 3])
def test_radius_33_with_one_percent_zero_channels(env, scn):
    """The benchmark's parameters (row structure of radius 33, rows that start at even columns)."""
    rf, co, torch = env
    rng = np.random.default_rng(7200 + scn)
    joint, src = _joint_noise(rng, 70, 130), _src(rng, 70, 130, scn)
    _check(rf, co, torch, joint, src, 20.0, 22.0, "radius 33 scn %d" % scn)


@pytest.mark.parametrize("scn", [1, 3])
def test_radius_54_runs_the_slab_kernel_in_both_forms(env, scn):
    rf, co, torch = env
    rng = np.random.default_rng(7300 + scn)
    joint, src = _joint_noise(rng, 72, 80), _src(rng, 72, 80, scn)
    _check(rf, co, torch, joint, src, 20.0, 36.0, "radius 54 scn %d" % scn)


@pytest.mark.parametrize("ss", [3.0, 36.0])
def test_ragged_call_of_two_sizes(env, ss):
    """One ragged launch (tile kernel at radius 5, slab kernel at radius 54) over two of the images."""
    rf, co, torch = env
    rng = np.random.default_rng(7400 + int(ss))
    shapes = [(H, W), (70, 130)]
    joints = [_joint_mixed_waves(rng, *shapes[0]), _joint_noise(rng, *shapes[1])]
    srcs = [_src(rng, h, w, 1) for h, w in shapes]
    dev = (lambda images: [torch.from_numpy(np.ascontiguousarray(im)).cuda() for im in images])
    tj, ts = dev(joints), dev(srcs)

    def run():
        _, views = rf.ops.joint_bilateral_ragged_u8(tj, ts, -1, SC, ss)
        return [v.cpu().numpy() for v in views]
    got, masked = _both_forms(rf, torch, run)
    for i, (j, s) in enumerate(zip(joints, srcs)):
        want = co.joint_bilateral_filter(j, s, -1, SC, ss).reshape(s.shape)
        assert _first_difference(masked[i], want) is None, \
            "image %d, jbf_no_msad: %s" % (i, _first_difference(masked[i], want))
        assert _first_difference(got[i], want) is None, \
            "image %d, default: %s" % (i, _first_difference(got[i], want))
        assert np.array_equal(got[i], masked[i])
