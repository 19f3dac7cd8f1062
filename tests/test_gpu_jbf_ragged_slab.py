"""GPU suite: the ragged joint bilateral at radius 53..468 (rf_jbf_ragged_u8: every image's 64x64
tiles in ONE launch of the slab kernel).  Everything is held, byte for byte, to the ORACLE run on
each image alone; no tolerance anywhere.

The entry's fall-back - rf_jbf_u8 once per image - writes the same bytes, so every case first
asserts from the plan query (rf_debug_jbf_ragged_slab_plan, computed by the functions the launch
uses) that the call takes the ragged slab launch, at the pitch and with the tile count expected.

  a  radius 54: nine images from 1x1 to 100x150 in one call, all borders, channel pairs, grey_as_bgr
  b  radius 54: grey, colour and half-grey 3-channel images in one call (grey scan per tile)
  c  the per-channel route (no room for the colour plane) on a 20x24 colour image
  d  one case per pitch class: radius 70, 99, 132, 150, 373 (pitch 1008); 8 LUT replicas
  e  sixteen 64x64 and sixteen 65x1 images interleaved: neighbouring workgroups on different images
  f  equal sizes: the bytes of the uniform entry
  g  apply_filter_list at c20 s36
"""
import numpy as np
import pytest

from tests.test_gpu_fuzz import _image, env  # noqa: F401  (env is a fixture)
from tests.test_gpu_jbf_ragged import _check, _images, _ragged
from tests.test_gpu_points_fuzz import (B101, BCONST, BREFLECT, BREP, BWRAP, GREY_AS_BGR,
                                        _oracle_full)

pytestmark = pytest.mark.gpu


def _tiles64(shapes):
    return sum(-(-h // 64) * -(-w // 64) for h, w in shapes)


def _slab_plan(rf, shapes, jcn, scn, sc, ss, grey=False):
    return rf._ffi.jbf_ragged_slab_plan(shapes, jcn, scn, -1, sc, ss, GREY_AS_BGR if grey else 0)


def _assert_slab_launch(rf, shapes, jcn, scn, sc, ss, grey, pitch):
    """The call takes the ragged slab launch at this pitch over all 64x64 tiles; returns the plan."""
    plan = _slab_plan(rf, shapes, jcn, scn, sc, ss, grey)
    assert plan is not None, "the call falls back to one launch per image"
    assert plan[0] == pitch and plan[6] == _tiles64(shapes), plan
    assert rf._ffi.jbf_ragged_plan(shapes, jcn, scn, -1, sc, ss, GREY_AS_BGR if grey else 0) is None
    return plan


# ---- a. radius 54: mixed and degenerate shapes in one call ---------------------------------------------

A_SHAPES = [(1, 1), (3, 200), (5, 7), (64, 64), (65, 65), (40, 130), (130, 40), (100, 150), (70, 70)]
A_ROWS = [(1, 1, False), (1, 1, True), (3, 1, False), (1, 3, False), (1, 3, True), (3, 3, False)]


@pytest.mark.parametrize("border", [BCONST, BREP, BREFLECT, BWRAP, B101])
@pytest.mark.parametrize("jcn,scn,grey", A_ROWS)
def test_nine_images_at_radius_54_in_one_call_match_the_oracle(env, border, jcn, scn, grey):
    """Five of the nine images are smaller than the radius in one direction or both, so their disks
    fold several times at the border.  A wrong width, or a base that is off by one image, shows as
    wrong bytes; the sentinel bytes around dst show a store outside it."""
    rf, co, torch = env
    rng = np.random.default_rng(3000 + 10 * border + 3 * jcn + scn)
    joints, srcs = _images(rng, A_SHAPES, jcn), _images(rng, A_SHAPES, scn, 1)
    plan = _assert_slab_launch(rf, A_SHAPES, jcn, scn, 20.0, 36.0, grey, 208)
    assert plan[6] == 1 + 4 + 1 + 1 + 4 + 3 + 3 + 6 + 4
    assert plan[4] == (64 if scn == 3 else 0)                       # a colour tile takes one pass
    _check(rf, co, torch, joints, srcs, 20.0, 36.0, border=border, grey=grey, what="slab case a")


# ---- b. grey and colour tiles of 3-channel images in one call -----------------------------------------

def test_grey_colour_and_half_grey_images_in_one_call_match_the_oracle(env):
    """Every image is passed with three src channels.  The first has B = G = R throughout: each of
    its tiles is found grey by the scan and takes the grey loop.  The second differs in its
    channels: the one-pass colour loop.  The third, 40x200, is grey in columns 0..151 and coloured
    from column 152 on: its first tile scans the 208 columns -56..151 it will ever stage (a
    REFLECT_101 or REPLICATE border folds the negative ones into columns 0..56), finds them grey
    and takes the grey loop, the tile beside it scans columns 8..215 and takes the colour loop."""
    rf, co, torch = env
    rng = np.random.default_rng(3100)
    shapes = [(70, 90), (66, 70), (40, 200)]
    joints = _images(rng, shapes, 3)
    grey3 = np.repeat(_image(rng, 70, 90, 1, 0), 3, axis=2)
    colour = _image(rng, 66, 70, 3, 2)
    half = _image(rng, 40, 200, 3, 2)
    half[:, :152] = half[:, :152, :1]
    assert (half[:, :152, 0] == half[:, :152, 2]).all() and (half[:, 152:, 0] != half[:, 152:, 2]).any()
    plan = _assert_slab_launch(rf, shapes, 3, 3, 20.0, 36.0, False, 208)
    assert plan[4:6] == (64, 53)
    for border in (B101, BWRAP):
        _check(rf, co, torch, joints, [grey3, colour, half], 20.0, 36.0, border=border,
               what="slab case b")
    # (under WRAP the first tile's left halo is the image's coloured right edge: a colour tile too);
    # a single-channel joint beside the same three srcs
    joints1 = _images(rng, shapes, 1, 1)
    _assert_slab_launch(rf, shapes, 1, 3, 20.0, 36.0, True, 208)
    _check(rf, co, torch, joints1, [grey3, colour, half], 20.0, 36.0, border=BREP, grey=True,
           what="slab case b, grey_as_bgr")


# ---- c. no room for the colour plane: one grey pass per channel ------------------------------------------

# radius 373 = lrint(1.5 * 248.7); sigma_color 100 keeps all 768 LUT entries (test_jbf_ragged_slab_abi.py)
SS_373 = 248.7


def test_the_per_channel_route_matches_the_oracle(env):
    rf, co, torch = env
    rng = np.random.default_rng(3200)
    shapes = [(20, 24), (3, 5)]
    joints, srcs = _images(rng, shapes, 3, 2), _images(rng, shapes, 3, 2)
    plan = _assert_slab_launch(rf, shapes, 3, 3, 100.0, SS_373, False, 1008)
    assert plan[2] > 0 and plan[4] == 0, plan                       # crows_c == 0
    _check(rf, co, torch, joints, srcs, 100.0, SS_373, border=BREFLECT, what="slab case c")


# ---- d. one case per pitch class -------------------------------------------------------------------------

D_CASES = [
    # sc, ss, radius, pitch, replicas, shapes
    (20.0, 47.0, 70, 240, 16, [(70, 70), (9, 66), (65, 3)]),
    (20.0, 66.0, 99, 272, 16, [(70, 70), (9, 66), (65, 3)]),
    (20.0, 88.0, 132, 336, 16, [(66, 70), (5, 9)]),
    (20.0, 100.0, 150, 400, 16, [(24, 24), (5, 9)]),
    (100.0, 100.0, 150, 400, 8, [(24, 24), (5, 9)]),
    (20.0, SS_373, 373, 1008, 16, [(20, 24), (3, 5)]),
]


@pytest.mark.parametrize("jcn,scn,grey", [(1, 1, True), (3, 3, False)])
@pytest.mark.parametrize("sc,ss,radius,pitch,rep,shapes", D_CASES,
                         ids=["r%d_rep%d" % (c[2], c[4]) for c in D_CASES])
def test_every_pitch_class_matches_the_oracle(env, sc, ss, radius, pitch, rep, shapes, jcn, scn, grey):
    """Oracle work: 70 x 70 px x pi 99^2 taps = 1.5e8, 66 x 70 x pi 132^2 = 2.5e8,
    24 x 24 x pi 150^2 = 4e7, 20 x 24 x pi 373^2 = 2.1e8 - under 5e8 taps per case."""
    rf, co, torch = env
    assert int(np.rint(1.5 * ss)) == radius
    rng = np.random.default_rng(3300 + radius + jcn)
    joints, srcs = _images(rng, shapes, jcn, 1), _images(rng, shapes, scn, 2)
    plan = _assert_slab_launch(rf, shapes, jcn, scn, sc, ss, grey, pitch)
    assert plan[1] == rep, plan
    _check(rf, co, torch, joints, srcs, sc, ss, border=B101 if radius % 2 else BWRAP, grey=grey,
           what="slab case d")


# ---- e. neighbouring workgroups on different images ------------------------------------------------------

def test_interleaved_64x64_and_65x1_images_match_the_oracle(env):
    """48 tiles: six per XCD under the XCD remapping, more tiles than XCDs; every 64x64 tile lies
    between the two tiles of a 65x1 image and those of the next."""
    rf, co, torch = env
    rng = np.random.default_rng(3400)
    shapes = [(64, 64), (65, 1)] * 16
    joints, srcs = _images(rng, shapes, 1), _images(rng, shapes, 1, 1)
    plan = _assert_slab_launch(rf, shapes, 1, 1, 20.0, 36.0, True, 208)
    assert plan[6] == 16 * 1 + 16 * 2
    _check(rf, co, torch, joints, srcs, 20.0, 36.0, border=BREFLECT, grey=True, what="slab case e")


# ---- f. equal sizes ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ss,pitch", [(36.0, 208), (66.0, 272)])
@pytest.mark.parametrize("jcn,scn,grey", [(1, 1, True), (3, 3, False)])
def test_equal_sizes_give_the_bytes_of_the_uniform_entry(env, ss, pitch, jcn, scn, grey):
    rf, co, torch = env
    shapes = [(70, 66)] * 3
    rng = np.random.default_rng(3500 + jcn)
    joints, srcs = _images(rng, shapes, jcn), _images(rng, shapes, scn, 1)
    _assert_slab_launch(rf, shapes, jcn, scn, 20.0, ss, grey, pitch)
    ragged = _ragged(rf, torch, joints, srcs, 20.0, ss, grey=grey)
    uniform = rf.ops.joint_bilateral_u8(torch.from_numpy(np.stack(joints)).cuda(),
                                        torch.from_numpy(np.stack(srcs)).cuda(), -1, 20.0, ss,
                                        grey_as_bgr=grey).cpu().numpy()
    assert uniform.shape == (3, 70, 66, scn)
    assert np.array_equal(np.stack(ragged), uniform)


# ---- g. apply_filter_list --------------------------------------------------------------------------------------

def test_apply_filter_list_at_c20_s36_equals_apply_filter_and_the_oracle_applied_twice(env, monkeypatch):
    rf, co, torch = env
    from reflectance_filtering_amd import filter_reflectance as fr
    rng = np.random.default_rng(3600)
    shapes = [(43, 64), (64, 43), (66, 70)]
    joints, srcs = _images(rng, shapes, 3), _images(rng, shapes, 3, 1)
    _assert_slab_launch(rf, shapes, 3, 3, 20.0, 36.0, False, 208)
    calls = []
    real = rf.ops.joint_bilateral_ragged_u8
    monkeypatch.setattr(rf.ops, "joint_bilateral_ragged_u8",
                        lambda *a, **kw: (calls.append(len(kw["sizes"])), real(*a, **kw))[1])
    dev = (lambda images: [torch.from_numpy(im).cuda() for im in images])
    got = fr.apply_filter_list("bilateral", dev(srcs), dev(joints), 20.0, 36.0)
    assert calls == [3]                                              # the list is not cut by radius
    for g, j, s in zip(got, joints, srcs):
        one = fr.apply_filter("bilateral", s, j, 20.0, 36.0)
        assert np.array_equal(g.cpu().numpy(), np.asarray(one).reshape(s.shape))
        assert np.array_equal(g.cpu().numpy(), _oracle_full(co, j, s, 20.0, 36.0, -1, B101, 0, False))
    del calls[:]
    got = fr.apply_filter_list("bilateral", dev(srcs), dev(joints), 20.0, 36.0, iterations=2)
    assert calls == [3, 3]
    for g, j, s in zip(got, joints, srcs):
        once = _oracle_full(co, j, s, 20.0, 36.0, -1, B101, 0, False)
        assert np.array_equal(g.cpu().numpy(), _oracle_full(co, j, once, 20.0, 36.0, -1, B101, 0, False))
