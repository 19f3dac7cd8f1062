"""The grey map of the joint bilateral's two-workgroups-per-CU route (jbf_grey_map_kernel: the route's one byte
per 64x64 tile from one pass over the images) and the tap loop that waves wholly below the image skip.

A tile's byte speaks of its REGION - rows tile_y0 - radius .. tile_y0 + 63 + radius and columns tile_x0 - r4 ..
tile_x0 - r4 + 143 (r4 = the radius rounded up to 4), each through the border rule: bit 0 = the src is not grey
somewhere in it, bit 1 = the joint is grey everywhere in it.  _rule() states that in numpy; the bytes of the map,
of the scan that every tile made of its own region before the map ("jbf_vote_scan") and of the rule must be
equal, tile for tile.  Output bytes are held to the ORACLE and to the one-workgroup-per-CU path
("jbf_no_two_wg").  sigma_color 20, radius 33 (r4 = 36, the metric's) and 7 (r4 = 8).
"""
import ctypes

import numpy as np
import pytest

from tests import arena, synth
from tests.test_gpu_fuzz import env  # noqa: F401  (a fixture)

SIGMA_COLOR = 20.0
RADII = (33, 7)
COLOURED = (10, 200, 90)

_cache = {}


def _sigma_space(radius):
    return max(1.0, radius / 1.5)


def _two_level(h, w, seed):
    """A grey map of two levels, as three equal channels."""
    g = (np.random.default_rng(seed).integers(0, 2, size=(h, w, 1)) * 200 + 30).astype(np.uint8)
    return np.ascontiguousarray(np.repeat(g, 3, axis=2))


def _grey_scene(h, w, seed):
    """A scene's first channel, as three equal channels."""
    g = synth.scene_u8(h, w, seed=seed)[:, :, :1]
    return np.ascontiguousarray(np.repeat(g, 3, axis=2))


def _reflect_101(p, n):
    """cv::borderInterpolate(p, n, BORDER_REFLECT_101), the border of every call here."""
    if n == 1:
        return 0
    while not 0 <= p < n:
        p = -p if p < 0 else 2 * n - 2 - p
    return p


def _grid(rf, joints, srcs, radius, **opts):
    """(tiles_x, tiles_y) of the main area's 64x64 tiles from the plan query, None off the route."""
    n, h, w, jcn = joints.shape
    assert srcs.shape[3] == 3     # (a 3-channel src has no column strip: the tiles span the whole width)
    with rf._ffi.debug_options(**opts):
        plan = rf._ffi.jbf_two_wg_plan(n, h, w, jcn, 3, 2 * radius + 1, SIGMA_COLOR, _sigma_space(radius))
    if plan is None:
        return None
    tiles_x = -(-w // 64)
    assert plan[1] % (n * tiles_x) == 0
    return tiles_x, plan[1] // (n * tiles_x)


def _rule(joints, srcs, radius, grid):
    """The tile bytes [n, tiles_y, tiles_x] the region rule gives."""
    tiles_x, tiles_y = grid
    n, h, w, _ = srcs.shape
    r4 = (radius + 3) & ~3

    def coloured(a):
        if a.shape[3] == 1:
            return np.zeros(a.shape[:3], bool)
        return (a[..., 0] != a[..., 1]) | (a[..., 1] != a[..., 2])

    cs, cj = coloured(srcs), coloured(joints)
    out = np.zeros((n, tiles_y, tiles_x), np.uint8)
    for ty in range(tiles_y):
        rows = sorted({_reflect_101(p, h) for p in range(64 * ty - radius, 64 * ty + 64 + radius)})
        for tx in range(tiles_x):
            cols = sorted({_reflect_101(p, w) for p in range(64 * tx - r4, 64 * tx - r4 + 144)})
            region = np.ix_(range(n), rows, cols)
            out[:, ty, tx] = cs[region].any(axis=(1, 2)) * 1 + (~cj[region].any(axis=(1, 2))) * 2
    return out


def _run(rf, torch, tj, ts, radius, out=None, on_route=True, grey_as_bgr=False, **opts):
    """One call on device tensors; asserts that it took (or did not take) the route."""
    lib = rf._ffi.load_library()
    before = lib.rf_debug_jbf_two_wg_calls()
    with rf._ffi.debug_options(**opts):
        out = rf.ops.joint_bilateral_u8(tj, ts, 2 * radius + 1, SIGMA_COLOR, _sigma_space(radius), out=out,
                                        grey_as_bgr=grey_as_bgr)
    assert lib.rf_debug_jbf_two_wg_calls() - before == (1 if on_route else 0), \
        "the call did not take the route it was meant to"
    return out


def _bytes(rf, torch, n, grid):
    tiles_x, tiles_y = grid
    flat = rf._ffi.jbf_tile_flags(rf._ffi.current_stream_ptr(torch), n * tiles_x * tiles_y)
    return flat.reshape(n, tiles_y, tiles_x)


def _oracle(co, key, joints, srcs, radius, grey_as_bgr=False):
    """The oracle's bytes for a batch, computed once per key."""
    key = key + (radius, grey_as_bgr)
    if key not in _cache:
        out = []
        for j, s in zip(joints, srcs):
            j3 = np.ascontiguousarray(np.repeat(j, 3, axis=2)) if grey_as_bgr else j
            out.append(co.joint_bilateral_filter(j3, s, 2 * radius + 1, SIGMA_COLOR,
                                                 _sigma_space(radius)).reshape(s.shape))
        _cache[key] = np.stack(out)
        _cache[key].setflags(write=False)
    return _cache[key]


def _first_difference(got, want):
    bad = np.argwhere(got != want)
    if bad.size == 0:
        return None
    i = tuple(int(v) for v in bad[0])
    return "%d bytes differ, the first at %r: %d against %d" % (len(bad), i, got[i], want[i])


def _three_ways(env, key, joints, srcs, radius):
    """Flag bytes: map == scan == rule.  Output: map route == scan route == jbf_no_two_wg == oracle.
    Returns (bytes, output) of the default call."""
    rf, co, torch = env
    grid = _grid(rf, joints, srcs, radius)
    assert grid is not None
    n = srcs.shape[0]
    tj, ts = torch.from_numpy(joints).cuda(), torch.from_numpy(srcs).cuda()
    want_bytes = _rule(joints, srcs, radius, grid)
    new = _run(rf, torch, tj, ts, radius).cpu().numpy()
    got = _bytes(rf, torch, n, grid)
    assert np.array_equal(got, want_bytes), "map against the rule:\n%r\n%r" % (got, want_bytes)
    scan_out = _run(rf, torch, tj, ts, radius, jbf_vote_scan=1).cpu().numpy()
    scan = _bytes(rf, torch, n, grid)
    assert np.array_equal(scan, want_bytes), "scan against the rule:\n%r\n%r" % (scan, want_bytes)
    old = _run(rf, torch, tj, ts, radius, on_route=False, jbf_no_two_wg=1).cpu().numpy()
    want = _oracle(co, key, joints, srcs, radius)
    for name, arr in (("the route", new), ("jbf_vote_scan", scan_out), ("jbf_no_two_wg", old)):
        assert _first_difference(arr, want) is None, "%s against the oracle: %s" % (
            name, _first_difference(arr, want))
    return got, new


# ---------------------------------------------------------------- 1. flag bytes: rule, scan and map agree

def _corner_positions(h, w, radius):
    """For every tile of the h x w image: the four corners of its region, one step inside and one step outside,
    clamped to the image; the image's corners; a pixel of row 0 and of row h - 1."""
    r4 = (radius + 3) & ~3
    pos = set()
    for ty in range(-(-h // 64)):
        ys = (64 * ty - radius, 64 * ty - radius - 1, 64 * ty + 63 + radius, 64 * ty + 64 + radius)
        for tx in range(-(-w // 64)):
            xs = (64 * tx - r4, 64 * tx - r4 - 1, 64 * tx - r4 + 143, 64 * tx - r4 + 144)
            pos |= {(min(max(y, 0), h - 1), min(max(x, 0), w - 1)) for y in ys for x in xs}
    pos |= {(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, w // 2 + 5), (h - 1, w // 2 + 5)}
    return sorted(pos)


@pytest.mark.gpu
def test_one_coloured_pixel_at_every_region_corner(env):
    """192 x 192 (3 x 3 tiles), radius 33, all grey but for ONE pixel with B != G, once in the src and once in the
    joint, at every region corner (inside and outside), the image's corners and its first and last row: the
    bytes of the map, of the scan and of the rule are equal for every tile."""
    rf, co, torch = env
    h = w = 192
    radius = 33
    src = _two_level(h, w, 101)[None]
    joint = _grey_scene(h, w, 102)[None]
    grid = _grid(rf, joint, src, radius)
    assert grid == (3, 3)
    positions = _corner_positions(h, w, radius)
    assert 100 <= len(positions) <= 160, len(positions)     # (x 2 buffers x 2 launches: a few hundred calls)
    tj, ts = torch.from_numpy(joint).cuda(), torch.from_numpy(src).cuda()
    out = torch.empty_like(ts)
    pixel = torch.tensor(COLOURED, dtype=torch.uint8, device="cuda")
    seen = set()
    for which, host, dev in (("src", src, ts), ("joint", joint, tj)):
        for y, x in positions:
            keep = dev[0, y, x].clone()
            dev[0, y, x] = pixel
            changed = host.copy()
            changed[0, y, x] = COLOURED
            want = _rule(changed if which == "joint" else joint, changed if which == "src" else src, radius, grid)
            _run(rf, torch, tj, ts, radius, out=out)
            got = _bytes(rf, torch, 1, grid)
            _run(rf, torch, tj, ts, radius, out=out, jbf_vote_scan=1)
            scan = _bytes(rf, torch, 1, grid)
            dev[0, y, x] = keep
            assert np.array_equal(got, want), "%s pixel at (%d, %d): map\n%r\nrule\n%r" % (which, y, x, got, want)
            assert np.array_equal(scan, want), "%s pixel at (%d, %d): scan\n%r\nrule\n%r" % (which, y, x, scan, want)
            seen.add(want.tobytes())
    # the positions tell regions apart: many different byte patterns, the pixel in one tile's region only among them
    assert len(seen) >= 20


# ---------------------------------------------------------------- 2. cut image

def _cut_batch(w=200):
    """Three images of 150 x w, grey src and grey joint, a coloured pixel in other places per image (image 1: none);
    and the same srcs with a scene as joint."""
    h = 150
    srcs = np.stack([_two_level(h, w, 110 + k) for k in range(3)])
    greys = np.stack([_grey_scene(h, w, 120 + k) for k in range(3)])
    scenes = np.stack([synth.scene_u8(h, w, seed=130 + k) for k in range(3)])
    srcs[0, 130, w - 1] = COLOURED       # below row 128 (a strip's row, or the third row of tiles), in the halo above
    srcs[2, 10, 70] = COLOURED
    greys[0, 64, 64] = COLOURED
    greys[2, 100, w - 1] = COLOURED
    return np.ascontiguousarray(greys), np.ascontiguousarray(scenes), np.ascontiguousarray(srcs)


@pytest.mark.gpu
@pytest.mark.parametrize("radius", RADII)
def test_cut_image_batch_of_three(env, radius):
    """150 x 200: tiles cut in x, the last 22 rows a strip or a tile row as the plan says - the tiles of the main
    area are what is compared.  n = 3 with other pixels per image: the bytes are per image."""
    greys, scenes, srcs = _cut_batch()
    got, _ = _three_ways(env, ("cut", "grey"), greys, srcs, radius)
    assert (got[1] == 2).all() and (got[0] != 2).any() and (got[2] != 2).any()
    assert not np.array_equal(got[0], got[2])
    got, _ = _three_ways(env, ("cut", "scene"), scenes, srcs, radius)
    assert (got[1] == 0).all() and (got[0] & 1).any() and (got[2] & 1).any()


# ---------------------------------------------------------------- 3. no stale flags

@pytest.mark.gpu
@pytest.mark.parametrize("coloured_first", (True, False))
def test_no_stale_flags_between_calls(env, coloured_first):
    """One stream, two calls of one shape: a batch with coloured tiles and an all-grey batch, in both orders.  The
    grey call's bytes say grey everywhere and both outputs are the oracle's (a map that ORs into bytes it does
    not set first fails here)."""
    rf, co, torch = env
    radius = 33
    greys, scenes, srcs = _cut_batch()
    plain_src = np.stack([_two_level(150, 200, 110 + k) for k in range(3)])
    plain_joint = np.stack([_grey_scene(150, 200, 120 + k) for k in range(3)])
    grid = _grid(rf, greys, srcs, radius)
    batches = [("scene", scenes, srcs), ("plain", plain_joint, plain_src)]
    for name, joints, s in batches if coloured_first else batches[::-1]:
        out = _run(rf, torch, torch.from_numpy(joints).cuda(), torch.from_numpy(s).cuda(), radius).cpu().numpy()
        got = _bytes(rf, torch, 3, grid)
        assert np.array_equal(got, _rule(joints, s, radius, grid)), name
        if name == "plain":
            assert (got == 2).all()
        want = _oracle(co, ("cut", name), joints, s, radius)
        assert _first_difference(out, want) is None, "%s: %s" % (name, _first_difference(out, want))


# ---------------------------------------------------------------- 4. odd placement

def _guarded_call(env, joints, srcs, radius, residue, flags=0):
    """rf_jbf_u8 on buffers placed at `residue` (mod 256) inside a guarded arena: (dst bytes, two-per-CU calls
    the call made); nothing outside dst may change."""
    rf, co, torch = env
    lib = rf._ffi.load_library()
    n, h, w, jcn = joints.shape
    scn = srcs.shape[3]
    ar = arena.Arena(torch, "cuda", arena.arena_bytes([joints.nbytes, srcs.nbytes, srcs.nbytes]), 0xA5)
    rj = ar.place(joints.nbytes, residue, name="joint")
    rs = ar.place(srcs.nbytes, residue, name="src")
    rd = ar.place(srcs.nbytes, residue, name="dst")
    ar.write(rj, joints)
    ar.write(rs, srcs)
    ar.snapshot()
    before = lib.rf_debug_jbf_two_wg_calls()
    rc = lib.rf_jbf_u8(ctypes.c_void_p(ar.ptr(rj)), ctypes.c_void_p(ar.ptr(rs)), ctypes.c_void_p(ar.ptr(rd)),
                       n, h, w, jcn, scn, 2 * radius + 1, SIGMA_COLOR, _sigma_space(radius),
                       rf._ffi.BORDER_DEFAULT, flags, rf._ffi.current_stream_ptr(torch))
    rf._ffi.check(rc, "rf_jbf_u8")
    torch.cuda.synchronize()
    ar.assert_only_changed([rd])
    return ar.bytes(rd).cpu().numpy().reshape(srcs.shape), lib.rf_debug_jbf_two_wg_calls() - before


@pytest.mark.gpu
@pytest.mark.parametrize("radius", RADII)
def test_odd_placement_and_width(env, radius):
    """The cut batch at w = 197 (no multiple of 4: every row ends in a lane with one pixel) with every buffer at
    byte 1 and at byte 255 from a 256-byte boundary: the flag bytes and the output of the aligned call, and
    nothing changes outside dst."""
    rf, co, torch = env
    greys, scenes, srcs = _cut_batch(197)
    srcs[1, 149, 196] = COLOURED     # (the row end's lone pixel, last row of an image)
    for name, joints in (("grey", greys), ("scene", scenes)):
        want_bytes, want = _three_ways(env, ("odd", name), joints, srcs, radius)
        grid = _grid(rf, joints, srcs, radius)
        for residue in (1, 255):
            out, calls = _guarded_call(env, joints, srcs, radius, residue)
            assert calls == 1
            assert np.array_equal(_bytes(rf, torch, 3, grid), want_bytes), (name, residue)
            assert _first_difference(out, want) is None, "%s at %d: %s" % (name, residue,
                                                                            _first_difference(out, want))


# ---------------------------------------------------------------- 5. dead waves

# 64 + k rows at w = 128: the second row of tiles has k live rows.  At k <= 32 the plan gives those rows to one
# strip workgroup (fewer than two tiles), so by default the heights below with k > 32 run - checked with
# rf_debug_jbf_two_wg_plan for radius 33 and 7, 3- and 1-channel buffers alike - and every height under
# "jbf_tile64_only".  k = 56: waves 14 and 15 of a tile wholly dead; 57: wave 14 has one live row; 60: wave 15
# alone is dead; 63: none; 1 (64x64 tiles only): fifteen dead waves and one live row.
DEAD_K = (1, 3, 4, 5, 56, 57, 60, 63)
DEAD_K_IN_MAIN = (56, 57, 60, 63)


def _dead_inputs(h, form):
    w = 128
    if form == "grey3":
        return (np.ascontiguousarray(synth.scene_u8(h, w, seed=140)[None]), _two_level(h, w, 141)[None], False)
    j1 = np.ascontiguousarray(synth.scene_u8(h, w, seed=142)[None, :, :, :1])
    return j1, np.ascontiguousarray(_two_level(h, w, 143)[None, :, :, :1]), True


@pytest.mark.gpu
@pytest.mark.parametrize("form", ("grey3", "grey1_as_bgr"))
@pytest.mark.parametrize("radius", RADII)
def test_dead_waves_skip_the_tap_loop(env, radius, form):
    """Grey src and RGB joint (and the 1-channel form, which takes the route without tile bytes): output == the
    same call with the skip off == jbf_no_two_wg == oracle, and nothing changes outside dst."""
    rf, co, torch = env
    ran = 0
    for only64 in (0, 1):
        for k in DEAD_K:
            h = 64 + k
            joints, srcs, as_bgr = _dead_inputs(h, form)
            flags = rf._ffi.JBF_GREY_AS_BGR if as_bgr else 0
            with rf._ffi.debug_options(jbf_tile64_only=only64):
                plan = rf._ffi.jbf_two_wg_plan(1, h, 128, joints.shape[3], srcs.shape[3], 2 * radius + 1,
                                               SIGMA_COLOR, _sigma_space(radius), flags)
            in_main = plan is not None and plan[1] == 4
            assert in_main == (only64 == 1 or k in DEAD_K_IN_MAIN), (k, only64, plan)
            if not in_main:
                continue
            ran += 1 - only64
            want = _oracle(co, ("dead", form, h), joints, srcs, radius, as_bgr)
            tj, ts = torch.from_numpy(joints).cuda(), torch.from_numpy(srcs).cuda()
            with rf._ffi.debug_options(jbf_tile64_only=only64):
                out, calls = _guarded_call(env, joints, srcs, radius, 0, flags)
                assert calls == 1
                full = _run(rf, torch, tj, ts, radius, grey_as_bgr=as_bgr, jbf_no_dead_skip=1).cpu().numpy()
                old = _run(rf, torch, tj, ts, radius, on_route=False, grey_as_bgr=as_bgr,
                           jbf_no_two_wg=1).cpu().numpy()
            for name, arr in (("the route", out), ("jbf_no_dead_skip", full), ("jbf_no_two_wg", old)):
                assert _first_difference(arr, want) is None, "%d rows, jbf_tile64_only=%d, %s: %s" % (
                    h, only64, name, _first_difference(arr, want))
    assert ran >= 4, "fewer than four heights put their second row of tiles into the main area"


# ---------------------------------------------------------------- 6. capture

def _mixed_batch(seed):
    """Three images of 64 x 128 (two tiles each): grey, one coloured pixel, colour all over."""
    h, w = 64, 128
    joints = np.stack([synth.scene_u8(h, w, seed=seed + k) for k in range(3)])
    srcs = np.stack([_two_level(h, w, seed + 5 + k) for k in range(3)])
    srcs[1, 63, 127] = COLOURED
    srcs[2] = synth.scene_u8(h, w, seed=seed + 9)
    return np.ascontiguousarray(joints), np.ascontiguousarray(srcs)


@pytest.mark.gpu
def test_captured_call_follows_new_contents(env):
    """A call with mixed tiles captured into a graph after a warm call on that stream (the graph holds the
    clearing launch and the map); the inputs' contents then change so that other tiles are coloured: every
    replay gives the oracle's bytes for the contents it ran on."""
    rf, co, torch = env
    radius = 33
    joints, srcs = _mixed_batch(150)
    order = [2, 0, 1]
    joints2, srcs2 = np.ascontiguousarray(joints[order]), np.ascontiguousarray(srcs[order])
    grid = _grid(rf, joints, srcs, radius)
    assert not np.array_equal(_rule(joints, srcs, radius, grid), _rule(joints2, srcs2, radius, grid))
    tj, ts = torch.from_numpy(joints).cuda(), torch.from_numpy(srcs).cuda()
    out = torch.zeros_like(ts)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _run(rf, torch, tj, ts, radius, out=out)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    out.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        _run(rf, torch, tj, ts, radius, out=out)
    for j, s, key in ((joints, srcs, "first"), (joints2, srcs2, "second"), (joints, srcs, "first")):
        tj.copy_(torch.from_numpy(j).cuda())
        ts.copy_(torch.from_numpy(s).cuda())
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        want = _oracle(co, ("capture", key), j, s, radius)
        assert _first_difference(out.cpu().numpy(), want) is None, "%s contents: %s" % (
            key, _first_difference(out.cpu().numpy(), want))
    del graph


# ---------------------------------------------------------------- 7. the switch

@pytest.mark.gpu
@pytest.mark.parametrize("radius", RADII)
def test_vote_scan_switch_keeps_the_bytes(env, radius):
    rf, co, torch = env
    greys, scenes, srcs = _cut_batch()
    tj, ts = torch.from_numpy(scenes).cuda(), torch.from_numpy(srcs).cuda()
    new = _run(rf, torch, tj, ts, radius).cpu().numpy()
    scan = _run(rf, torch, tj, ts, radius, jbf_vote_scan=1).cpu().numpy()
    assert _first_difference(scan, new) is None, _first_difference(scan, new)
