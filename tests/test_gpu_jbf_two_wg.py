"""Grey tiles of the joint bilateral at two workgroups per CU (jbf_tile64x2_kernel: 81,920 B of LDS, 64 output
rows + a slab of the disk's tap rows resident, the tile re-staged slab by slab; a vote launch in front writes
one byte per tile, colour tiles go to a launch of jbf_tile64_kernel that filters flagged tiles only).  Every
case byte for byte against the ORACLE and against the same call under "jbf_no_two_wg" (the
one-workgroup-per-CU path); the plan query says that the first call is on the new route, and the library's
count of the calls that launched it (rf_debug_jbf_two_wg_calls) that it really was.

At sigma_color 20 the tile holds 78 rows: slabs of 15 tap rows.  Radius 1..7 is one slab (3..15 rows), 13 / 14
/ 15 straddle the step from two slabs to three (27 / 29 / 31 tap rows), 33 (the metric's) is five slabs and 36
(the last radius of pitch 144) is five as well.
"""
import ctypes

import numpy as np
import pytest

from tests import synth
from tests.test_gpu_fuzz import env  # noqa: F401  (a fixture)

SIGMA_COLOR = 20.0
RADII = (1, 2, 3, 7, 13, 14, 15, 33, 36)
FLAT_BGR = (90, 140, 200)

_cache = {}


def _sigma_space(radius):
    return max(1.0, radius / 1.5)


def _two_level(h, w, seed):
    """A grey map of two levels, as three equal channels."""
    g = (np.random.default_rng(seed).integers(0, 2, size=(h, w, 1)) * 255).astype(np.uint8)
    return np.ascontiguousarray(np.repeat(g, 3, axis=2))


def _flat(h, w):
    joint = np.empty((h, w, 3), np.uint8)
    joint[:] = FLAT_BGR
    return joint


def _oracle(co, key, joint, src, radius, grey_as_bgr=False):
    """The oracle's bytes for one image, computed once per key."""
    key = key + (radius, grey_as_bgr)
    if key not in _cache:
        j = np.ascontiguousarray(np.repeat(joint, 3, axis=2)) if grey_as_bgr else joint
        _cache[key] = co.joint_bilateral_filter(j, src, 2 * radius + 1, SIGMA_COLOR,
                                                _sigma_space(radius)).reshape(src.shape)
    return _cache[key]


def _call(rf, torch, joints, srcs, radius, two_wg, grey_as_bgr=False, **opts):
    tj, ts = torch.from_numpy(joints).cuda(), torch.from_numpy(srcs).cuda()
    lib = rf._ffi.load_library()
    before = lib.rf_debug_jbf_two_wg_calls()
    with rf._ffi.debug_options(jbf_no_two_wg=0 if two_wg else 1, **opts):
        out = rf.ops.joint_bilateral_u8(tj, ts, 2 * radius + 1, SIGMA_COLOR, _sigma_space(radius),
                                        grey_as_bgr=grey_as_bgr).cpu().numpy()
    torch.cuda.synchronize()
    # the plan query sees neither the device's LDS probes nor the flag buffer: the library counts the calls
    # that really launched jbf_tile64x2_kernel
    assert lib.rf_debug_jbf_two_wg_calls() - before == (1 if two_wg else 0), \
        "the call did not take the route it was meant to"
    return out


def _on_route(rf, joints, srcs, radius, grey_as_bgr=False, **opts):
    n, h, w, jcn = joints.shape
    with rf._ffi.debug_options(**opts):
        return rf._ffi.jbf_two_wg_plan(n, h, w, jcn, srcs.shape[3], 2 * radius + 1, SIGMA_COLOR,
                                       _sigma_space(radius), rf._ffi.JBF_GREY_AS_BGR if grey_as_bgr else 0)


def _first_difference(got, want):
    bad = np.argwhere(got != want)
    if bad.size == 0:
        return None
    i = tuple(int(v) for v in bad[0])
    return "%d bytes differ, the first at %r: %d against %d" % (len(bad), i, got[i], want[i])


def _check(env, key, joints, srcs, radius, grey_as_bgr=False, **opts):
    """joints [n,h,w,jcn], srcs [n,h,w,scn]: new route == old path == oracle."""
    rf, co, torch = env
    assert _on_route(rf, joints, srcs, radius, grey_as_bgr, **opts) is not None
    new = _call(rf, torch, joints, srcs, radius, True, grey_as_bgr, **opts)
    old = _call(rf, torch, joints, srcs, radius, False, grey_as_bgr, **opts)
    for i in range(joints.shape[0]):
        want = _oracle(co, key + (i,), joints[i], srcs[i], radius, grey_as_bgr)
        assert _first_difference(new[i], want) is None, "image %d against the oracle: %s" % (
            i, _first_difference(new[i], want))
        assert _first_difference(old[i], want) is None, "image %d, jbf_no_two_wg, against the oracle: %s" % (
            i, _first_difference(old[i], want))
    return new


# ---------------------------------------------------------------- 1. ring and slab edges

@pytest.mark.gpu
@pytest.mark.parametrize("radius", RADII)
def test_slab_edges_on_a_cut_image(env, radius):
    """70 x 72 (rows x columns): tiles cut on both axes, rows reflected at the top and at the bottom inside one
    tile.  A flat joint with a two-level src - one skipped or doubled tap row flips many bytes - and a seeded
    scene as joint; as the planner cuts it (two tiles + a strip) and in 64x64 tiles only (four tiles)."""
    h, w = 70, 72
    src = _two_level(h, w, 11)[None]
    for name, joint in (("flat", _flat(h, w)), ("scene", synth.scene_u8(h, w, seed=12))):
        for only64 in (0, 1):
            _check(env, ("cut", name), np.ascontiguousarray(joint[None]), src, radius, jbf_tile64_only=only64)


# ---------------------------------------------------------------- 2. three tile rows

@pytest.mark.gpu
def test_three_tile_rows_at_the_metric_radius(env):
    """130 x 64, radius 33: five slabs per tile, three rows of tiles under jbf_tile64_only (two and a strip
    without), the middle one with no border in reach of its first slabs."""
    h, w = 130, 64
    src = _two_level(h, w, 21)[None]
    for name, joint in (("flat", _flat(h, w)), ("scene", synth.scene_u8(h, w, seed=22))):
        for only64 in (0, 1):
            _check(env, ("rows3", name), np.ascontiguousarray(joint[None]), src, 33, jbf_tile64_only=only64)


# ---------------------------------------------------------------- 3. both SAD forms and J1

@pytest.mark.gpu
@pytest.mark.parametrize("radius", (7, 33))
def test_sad_forms_and_single_channel_joint(env, radius):
    rf, co, torch = env
    h, w = 70, 72
    grey_src = synth.reflectance_like_u8(h, w, seed=31)
    if grey_src.ndim == 2:
        grey_src = grey_src[:, :, None]
    src1 = np.ascontiguousarray(grey_src[:, :, :1])
    src3 = np.ascontiguousarray(np.repeat(src1, 3, axis=2))
    # zero channels in rows 0..3 of the first tile only: that wave keeps the mask, the other fifteen of the
    # workgroup take the masked SAD
    joint = np.maximum(synth.scene_u8(h, w, seed=32), 1)
    top = joint[0:4, 0:64]
    top[np.random.default_rng(33).random(top.shape) < 0.2] = 0
    assert (joint[0:4, 0:64] == 0).any() and joint[4:].min() >= 1
    _check(env, ("mixed",), np.ascontiguousarray(joint[None]), src3[None], radius)
    _check(env, ("mixed1",), np.ascontiguousarray(joint[None]), src1[None], radius)
    # every wave with the mask
    _check(env, ("mixed",), np.ascontiguousarray(joint[None]), src3[None], radius, jbf_no_msad=1)
    # a 1-channel joint counted as three equal channels (J1 known up front), 1- and 3-channel src
    j1 = np.ascontiguousarray(synth.scene_u8(h, w, seed=34)[:, :, :1])
    _check(env, ("j1", 1), j1[None], src1[None], radius, grey_as_bgr=True)
    _check(env, ("j1", 3), j1[None], src3[None], radius, grey_as_bgr=True)
    # ... and counted once
    _check(env, ("j1once",), j1[None], src1[None], radius)
    # a grey 3-channel joint (J1 found by the vote)
    j3 = np.ascontiguousarray(np.repeat(j1, 3, axis=2))
    _check(env, ("j3grey",), j3[None], src3[None], radius)


# ---------------------------------------------------------------- 4. mixed batch

def _mixed_batch():
    h, w = 64, 128
    joints = np.stack([synth.scene_u8(h, w, seed=40 + k) for k in range(3)])
    g = np.stack([_two_level(h, w, 45 + k) for k in range(3)])
    srcs = g.copy()
    srcs[1, 63, 127] = (10, 200, 90)          # one coloured pixel in the last row of image 1's second tile
    srcs[2] = synth.scene_u8(h, w, seed=49)   # image 2 is colour all over
    return np.ascontiguousarray(joints), np.ascontiguousarray(srcs)


@pytest.mark.gpu
def test_mixed_batch_of_grey_and_colour_tiles(env):
    """Three images of 64 x 128 (two tiles each), radius 33 (a tile stages 36 columns of halo: the coloured pixel
    at column 127 is in reach of its own tile only).  Image 0: both tiles grey.  Image 1: the first tile grey,
    the second flagged.  Image 2: both flagged.  Nothing is written twice and nothing is missed - every byte is
    the oracle's; the same call again, and then a call with the images in another order on the same stream:
    no stale flag."""
    rf, co, torch = env
    joints, srcs = _mixed_batch()
    t = srcs[1, :, 64:].astype(int)
    assert (t[..., 0] != t[..., 1]).sum() == 1 and np.array_equal(srcs[1, :, :64, 0], srcs[1, :, :64, 1])
    first = _check(env, ("mixed_batch",), joints, srcs, 33)
    again = _call(rf, torch, joints, srcs, 33, True)
    assert np.array_equal(first, again)
    order = [2, 0, 1]
    swapped = _call(rf, torch, np.ascontiguousarray(joints[order]), np.ascontiguousarray(srcs[order]), 33, True)
    assert np.array_equal(swapped, first[order])
    back = _call(rf, torch, joints, srcs, 33, True)
    assert np.array_equal(back, first)


@pytest.mark.gpu
def test_untouched_bytes_around_the_output(env):
    """The route writes the image's bytes and nothing else: guard bytes before and after dst keep their value
    (mixed batch: both launches)."""
    rf, co, torch = env
    joints, srcs = _mixed_batch()
    tj, ts = torch.from_numpy(joints).cuda(), torch.from_numpy(srcs).cuda()
    guard = 4096
    buf = torch.full((srcs.size + 2 * guard,), 0xA5, dtype=torch.uint8, device="cuda")
    out = buf[guard:guard + srcs.size].view(srcs.shape)
    rf.ops.joint_bilateral_u8(tj, ts, 67, SIGMA_COLOR, _sigma_space(33), out=out)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:guard] == 0xA5).all() and (host[-guard:] == 0xA5).all()
    want = np.stack([_oracle(co, ("mixed_batch", i), joints[i], srcs[i], 33) for i in range(3)])
    assert np.array_equal(host[guard:-guard].reshape(srcs.shape), want)


# ---------------------------------------------------------------- 5. refusals

@pytest.mark.gpu
def test_refusals_are_those_of_the_old_path(env):
    """dst overlapping an input, unknown flag bits, bad sizes and channels, an empty batch: the same return
    codes on the route and under jbf_no_two_wg."""
    rf, co, torch = env
    lib = rf._ffi.load_library()
    h, w = 64, 128
    j = torch.zeros((1, h, w, 3), dtype=torch.uint8, device="cuda")
    s = torch.zeros((1, h, w, 3), dtype=torch.uint8, device="cuda")
    o = torch.zeros((1, h, w, 3), dtype=torch.uint8, device="cuda")
    stream = rf._ffi.current_stream_ptr(torch)

    def rc(joint, src, dst, n=1, hh=h, ww=w, jcn=3, scn=3, flags=0, border=rf._ffi.BORDER_DEFAULT):
        return lib.rf_jbf_u8(joint, src, dst, n, hh, ww, jcn, scn, -1, 20.0, 22.0, border, flags, stream)

    cases = [
        ((j.data_ptr(), s.data_ptr(), o.data_ptr()), {}, rf._ffi.RF_OK),
        ((j.data_ptr(), s.data_ptr(), s.data_ptr()), {}, rf._ffi.RF_E_BADARG),
        ((j.data_ptr(), s.data_ptr(), j.data_ptr()), {}, rf._ffi.RF_E_BADARG),
        ((j.data_ptr(), s.data_ptr(), s.data_ptr() + 3 * h * w - 1), {}, rf._ffi.RF_E_BADARG),
        ((j.data_ptr(), s.data_ptr(), o.data_ptr()), {"flags": 0x100}, rf._ffi.RF_E_BADARG),
        ((j.data_ptr(), s.data_ptr(), o.data_ptr()), {"hh": 0}, rf._ffi.RF_E_BADARG),
        ((j.data_ptr(), s.data_ptr(), None), {}, rf._ffi.RF_E_BADARG),
        ((None, None, None), {"n": 0}, rf._ffi.RF_OK),
    ]
    for no_two_wg in (0, 1):
        with rf._ffi.debug_options(jbf_no_two_wg=no_two_wg):
            for ptrs, kw, want in cases:
                assert rc(*[ctypes.c_void_p(p) for p in ptrs], **kw) == want, (no_two_wg, kw)
            assert rc(ctypes.c_void_p(j.data_ptr()), ctypes.c_void_p(s.data_ptr()),
                      ctypes.c_void_p(o.data_ptr()), jcn=2) < 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 6. graph capture

@pytest.mark.gpu
def test_captured_call_replays_with_equal_bytes(env):
    """One call on the route captured into a graph (after a call on the capture's stream: the flag buffer is
    enlarged outside a capture only) and replayed twice, the second time on other inputs: the bytes of the
    eager calls."""
    rf, co, torch = env
    joints, srcs = _mixed_batch()
    eager = _call(rf, torch, joints, srcs, 33, True)
    order = [1, 2, 0]
    tj, ts = torch.from_numpy(joints).cuda(), torch.from_numpy(srcs).cuda()
    out = torch.zeros_like(ts)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        rf.ops.joint_bilateral_u8(tj, ts, 67, SIGMA_COLOR, _sigma_space(33), out=out)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    out.zero_()
    graph = torch.cuda.CUDAGraph()
    lib = rf._ffi.load_library()
    before = lib.rf_debug_jbf_two_wg_calls()
    with torch.cuda.graph(graph, stream=side):
        rf.ops.joint_bilateral_u8(tj, ts, 67, SIGMA_COLOR, _sigma_space(33), out=out)
    assert lib.rf_debug_jbf_two_wg_calls() - before == 1, "the captured call is not on the route"
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), eager)
    tj.copy_(torch.from_numpy(np.ascontiguousarray(joints[order])).cuda())
    ts.copy_(torch.from_numpy(np.ascontiguousarray(srcs[order])).cuda())
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), eager[order])
    del graph
