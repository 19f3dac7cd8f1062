"""GPU suite: the buffer contract of every entry of the C ABI (include/reflectance_filtering.h).

Every buffer of a call - inputs, outputs, workspace - is a region of one guarded arena
(tests/arena.py).  Each case runs under five (layout, fill) pairs:

    L0  every base = 0 (mod 256)                                                 arena filled with 0xA5
    L1  uint8 buffers at the odd residues 1, 3, 5, ... 15 in turn, other element
        types at elem x 1 or elem x 3, the workspace at 16                       0x00, and again 0xFF
    L2  every uint8 buffer at 2, the others as L1                                0xFF
    L3  every uint8 buffer at 255, the others as L1                              0x00

The workspace holds exactly the bytes of the entry's size query and starts out as the arena's fill
(0xA5 bytes, zeros, or 0xFF: NaN as a float, -1 as a counter).  Asserted per case: RF_OK; no byte
outside the outputs and the workspace changes (guards, inputs, the bytes behind the workspace); the
L0 outputs equal the oracle under the entry's existing contract; every other layout's outputs are
bit-identical to L0's.

Shapes: S1 = 2 x 67 x 131 (w % 4 = 3, h % 64 = 3: 64x64 tiles with right and bottom strips; an image
is 26,331 or 8,777 bytes, both odd, so the second image of a batch is at an odd address even in L0),
S2 = 3 x 5 x 7 (smaller than every tile and window; 105 bytes), S3 = 1 x 1 x 1.
"""
import ctypes
import itertools
import zlib

import numpy as np
import pytest

from tests import arena as A
from tests import png_synth as ps
from tests import synth
from tests.test_gpu_fuzz import env  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

PAIRS = (("L0", 0xA5), ("L1", 0x00), ("L1", 0xFF), ("L2", 0xFF), ("L3", 0x00))
S1, S2, S3 = (2, 67, 131), (3, 5, 7), (1, 1, 1)
MIXED = ((67, 131), (5, 7), (5, 7), (67, 131), (5, 7))     # the ragged entries' list


class Buf(object):
    """One buffer of a call.  role: "in", "out" or "ws"; data: host array written before the call
    (None: the arena's fill); fixed: the residue this buffer takes in every layout but L0."""

    def __init__(self, name, role, nbytes=None, data=None, elem=None, fixed=None):
        if data is not None:
            data = np.ascontiguousarray(data)
            nbytes = data.nbytes if nbytes is None else nbytes
            elem = data.dtype.itemsize if elem is None else elem
        self.name, self.role, self.nbytes, self.data = name, role, int(nbytes), data
        self.elem, self.fixed = int(elem or 1), fixed


def _residues(bufs, layout):
    odd, alt = itertools.cycle(range(1, 16, 2)), itertools.cycle((1, 3))
    out = []
    for b in bufs:
        if layout == "L0":
            out.append(0)
        elif b.role == "ws":
            out.append(16)
        elif b.fixed is not None:
            out.append(b.fixed)
        elif b.elem == 1:
            out.append({"L1": next(odd), "L2": 2, "L3": 255}[layout])
        else:
            out.append(b.elem * next(alt))
    return out


class Case(object):
    """bufs: the call's buffers; call(lib, p, stream) -> return code, p[name] the device address;
    outputs: {name: (dtype, shape)} compared across layouts (a callable (raw bytes by name) -> dict of
    arrays where only part of an output is specified); check(outs): the L0 outputs against the oracle;
    around: a context manager factory held during the call (debug switches)."""

    def __init__(self, bufs, call, outputs, check, around=None, after=None):
        self.bufs, self.call, self.outputs, self.check = bufs, call, outputs, check
        self.around, self.after = around, after


def _run(env, case, layout, fill):
    rf, co, torch = env
    lib = rf._ffi.load_library()
    ar = A.Arena(torch, "cuda", A.arena_bytes([b.nbytes for b in case.bufs]), fill)
    regs = {}
    for b, res in zip(case.bufs, _residues(case.bufs, layout)):
        regs[b.name] = ar.place(b.nbytes, res, b.elem, name=b.name)
        assert ar.ptr(regs[b.name]) % A.ALIGN == res
        if b.data is not None:
            ar.write(regs[b.name], b.data)
    torch.cuda.synchronize()
    ar.snapshot()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptrs = dict((name, ar.ptr(r)) for name, r in regs.items())
    if case.around is not None:
        with case.around():
            rc = case.call(lib, ptrs, stream)
    else:
        rc = case.call(lib, ptrs, stream)
    torch.cuda.synchronize()
    assert rc == rf._ffi.RF_OK, (layout, fill, rc, lib.rf_last_error())
    try:
        ar.assert_only_changed([regs[b.name] for b in case.bufs if b.role in ("out", "ws")])
    except AssertionError as err:
        raise AssertionError("layout %s, fill 0x%02X: %s" % (layout, fill, err))
    raw = dict((b.name, ar.bytes(regs[b.name]).cpu().numpy().copy()) for b in case.bufs if b.role == "out")
    if callable(case.outputs):
        return case.outputs(raw)
    return dict((name, raw[name][:int(np.prod(shape)) * np.dtype(dt).itemsize].view(dt).reshape(shape))
                for name, (dt, shape) in case.outputs.items())


def _contract(env, case):
    base = None
    for layout, fill in PAIRS:
        outs = _run(env, case, layout, fill)
        if case.after is not None:
            case.after()
        if base is None:
            case.check(outs)
            base = outs
            continue
        for name in base:
            a, b = base[name], outs[name]
            assert a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), \
                "%s differs from L0's under layout %s, fill 0x%02X (%d bytes)" % (
                    name, layout, fill, int(np.count_nonzero(a.view(np.uint8) != b.view(np.uint8))))


# ---- inputs, made once ---------------------------------------------------------------------------------

_cache = {}


def _images(shape, kind):
    """uint8 [n,h,w,c]: "colour" (3 channels), "grey3" (3 equal channels), "grey1", "joint1"."""
    key = (shape, kind)
    if key not in _cache:
        n, h, w = shape
        if kind == "colour":
            imgs = [synth.scene_u8(h, w, 900 + i) for i in range(n)]
        elif kind == "grey3":
            imgs = [synth.reflectance_like_u8(h, w, 910 + i) for i in range(n)]
        elif kind == "grey1":
            imgs = [synth.reflectance_like_u8(h, w, 910 + i)[:, :, :1] for i in range(n)]
        else:
            imgs = [synth.scene_u8(h, w, 920 + i)[:, :, 1:2] for i in range(n)]
        _cache[key] = np.ascontiguousarray(np.stack(imgs))
    return _cache[key]


def _floats(shape, c, seed, scale=1.0):
    key = (shape, c, seed, scale)
    if key not in _cache:
        n, h, w = shape
        imgs = np.stack([synth.scene_u8(h, w, seed + i)[:, :, :c] for i in range(n)])
        _cache[key] = np.ascontiguousarray(imgs.astype(np.float32) / np.float32(255) * np.float32(scale))
    return _cache[key]


def _packed(kind, sizes=MIXED):
    """The images of `sizes` packed one after another, [total pixels, c]."""
    key = ("packed", kind, sizes)
    if key not in _cache:
        parts = [_images((1, h, w), kind)[0].reshape(h * w, -1) for h, w in sizes]
        _cache[key] = np.ascontiguousarray(np.concatenate(parts))
    return _cache[key]


def _split(packed, sizes=MIXED):
    out, at = [], 0
    for h, w in sizes:
        out.append(packed[at:at + h * w].reshape(h, w, -1))
        at += h * w
    return out


def _i32(values):
    return np.ascontiguousarray(values, dtype=np.int32)


# ---- rf_jbf_u8 -------------------------------------------------------------------------------------------

JBF_PAIRS = {   # name: (joint kind, src kind, flags)
    "colour_colour": ("colour", "colour", 0), "colour_grey3": ("colour", "grey3", 0),
    "colour_grey1": ("colour", "grey1", 0), "joint1_grey1": ("joint1", "grey1", 0),
    "joint1_as_bgr": ("joint1", "grey1", 4),
}
JBF_ROUTES = {  # name: (d, sigma_space, extra flags): radius 33 (two workgroups per CU for grey tiles),
                # 42 (the 37..52 tile kernel), 54 (slabs), 33 untiled, 1 (two workgroups per CU again)
    "s22": (-1, 22.0, 0), "s28": (-1, 28.0, 0), "s36": (-1, 36.0, 0), "generic": (-1, 22.0, 2), "d3": (3, 22.0, 0),
}


def _jbf_oracle(co, joint, src, d, sc, ss, flags):
    """Per image; RF_JBF_GREY_AS_BGR: the filter on the joint replicated to three channels."""
    out = []
    for j, s in zip(joint, src):
        if flags & 4:
            want = co.joint_bilateral_filter(np.repeat(j, 3, 2), np.repeat(s, 3, 2) if s.shape[2] == 1 else s,
                                             d, sc, ss)
            out.append(want[:, :, :s.shape[2]])
        else:
            out.append(co.joint_bilateral_filter(j, s, d, sc, ss).reshape(s.shape))
    return np.stack(out)


@pytest.mark.parametrize("shape", [S1, S2], ids=["S1", "S2"])
@pytest.mark.parametrize("route", sorted(JBF_ROUTES))
@pytest.mark.parametrize("pair", sorted(JBF_PAIRS))
def test_jbf_u8(env, pair, route, shape):
    rf, co, torch = env
    lib = rf._ffi.load_library()
    jkind, skind, flags = JBF_PAIRS[pair]
    d, ss, extra = JBF_ROUTES[route]
    flags |= extra
    joint, src = _images(shape, jkind), _images(shape, skind)
    n, h, w = shape
    jcn, scn, sc = joint.shape[3], src.shape[3], 20.0
    on_route = rf._ffi.jbf_two_wg_plan(n, h, w, jcn, scn, d, sc, ss, flags) is not None
    if route == "s22" and shape == S1 and pair in ("colour_grey3", "colour_grey1"):
        assert on_route, "the plan no longer puts this case on the two-workgroups-per-CU route"
    if route in ("s28", "s36", "generic"):
        assert not on_route
    count = [lib.rf_debug_jbf_two_wg_calls()]

    def call(lib, p, stream):
        return lib.rf_jbf_u8(p["joint"], p["src"], p["dst"], n, h, w, jcn, scn, d, sc, ss, 4, flags, stream)

    def after():
        now = lib.rf_debug_jbf_two_wg_calls()
        assert now - count[0] == (1 if on_route else 0), "the call did not take the route the plan names"
        count[0] = now

    def check(outs):
        want = _jbf_oracle(co, joint, src, d, sc, ss, flags)
        assert np.array_equal(outs["dst"], want), np.argwhere(outs["dst"] != want)[:4]

    _contract(env, Case([Buf("joint", "in", data=joint), Buf("src", "in", data=src),
                         Buf("dst", "out", nbytes=src.nbytes)],
                        call, {"dst": (np.uint8, src.shape)}, check, after=after))


# ---- rf_gf_u8, rf_gf_ex_u8 ---------------------------------------------------------------------------------

def _gf_oracle(co, guide, src, radius, eps, iterations, grey_guide=False):
    out = []
    for g, s in zip(guide, src):
        g3 = np.repeat(g, 3, 2) if grey_guide else g
        cur = s
        for _ in range(iterations):
            cur = co.guided_filter(g3, cur, radius, eps).reshape(s.shape)
        out.append(cur)
    return np.stack(out)


def _gf_case(env, shape, skind, radius, iterations, two_kernel=False, ws_images=None, in_place=False,
             grey_guide=False):
    rf, co, torch = env
    lib = rf._ffi.load_library()
    n, h, w = shape
    guide = _images(shape, "joint1" if grey_guide else "colour")
    src = _images(shape, skind)
    gcn, scn, eps = guide.shape[3], src.shape[3], 3.0
    need = lib.rf_gf_workspace_bytes(n if ws_images is None else ws_images, h, w, 3, scn, radius)
    assert need > 0
    if ws_images is not None and ws_images < n:
        assert need < lib.rf_gf_workspace_bytes(n, h, w, 3, scn, radius)

    def call(lib, p, stream):
        dst = p["src"] if in_place else p["dst"]
        if grey_guide:
            return lib.rf_gf_ex_u8(p["guide"], p["src"], dst, n, h, w, gcn, scn, radius, eps, iterations,
                                   rf._ffi.GF_GREY_AS_BGR, p["ws"], need, stream)
        return lib.rf_gf_u8(p["guide"], p["src"], dst, n, h, w, gcn, scn, radius, eps, iterations, p["ws"],
                            need, stream)

    out_name = "src" if in_place else "dst"

    def check(outs):
        want = _gf_oracle(co, guide, src, radius, eps, iterations, grey_guide)
        assert np.array_equal(outs[out_name], want), np.argwhere(outs[out_name] != want)[:4]

    bufs = [Buf("guide", "in", data=guide), Buf("src", "out" if in_place else "in", data=src)]
    if not in_place:
        bufs.append(Buf("dst", "out", nbytes=src.nbytes))
    bufs.append(Buf("ws", "ws", nbytes=need, elem=16))
    around = (lambda: rf._ffi.debug_options(gf_two_kernel=1)) if two_kernel else None
    _contract(env, Case(bufs, call, {out_name: (np.uint8, src.shape)}, check, around=around))


GF_ROUTES = {"r9": (9, False), "r45": (45, False), "r45_two_kernel": (45, True), "r129_float": (129, False)}


@pytest.mark.parametrize("shape", [S1, S2], ids=["S1", "S2"])
@pytest.mark.parametrize("iterations", [1, 2])
@pytest.mark.parametrize("skind", ["colour", "grey3", "grey1"])
@pytest.mark.parametrize("route", sorted(GF_ROUTES))
def test_gf_u8(env, route, skind, iterations, shape):
    radius, two_kernel = GF_ROUTES[route]
    _gf_case(env, shape, skind, radius, iterations, two_kernel=two_kernel)


@pytest.mark.parametrize("ws_images", [1, 3], ids=["chunked", "full"])
@pytest.mark.parametrize("radius", [45, 129])
def test_gf_u8_three_images_on_a_one_image_and_on_the_full_workspace(env, radius, ws_images):
    _gf_case(env, (3, 67, 131), "colour", radius, 2, ws_images=ws_images)


def test_gf_u8_in_place(env):
    _gf_case(env, S1, "colour", 9, 2, in_place=True)


@pytest.mark.parametrize("radius,skind", [(9, "grey1"), (45, "grey3"), (45, "colour")])
def test_gf_ex_u8_grey_guide(env, radius, skind):
    _gf_case(env, S1, skind, radius, 1, grey_guide=True)


# ---- the CNN -------------------------------------------------------------------------------------------

def _cnn_check(co, rf, bgr, outs):
    """The tolerance of tests/test_gpu_parity.py::test_cnn_matches_oracle_and_golden."""
    wts = rf.weights.load_weights()
    for i, img in enumerate(bgr):
        want_r, want_r8 = co.cnn_reflectance(img, wts)
        if "r" in outs:
            assert np.abs(outs["r"][i] - want_r).max() <= 2e-7
        if "r8" in outs:
            d8 = np.abs(outs["r8"][i].astype(int) - want_r8.astype(int))
            assert d8.max() <= 1 and np.mean(d8 != 0) < 1e-4


@pytest.mark.parametrize("shape", [S1, S2, S3], ids=["S1", "S2", "S3"])
@pytest.mark.parametrize("want", ["both", "float", "u8"])
@pytest.mark.parametrize("entry", ["u8", "f32_nchw_rgb", "f32_nhwc_bgr"])
def test_cnn_reflectance(env, entry, want, shape):
    rf, co, torch = env
    n, h, w = shape
    bgr = _images(shape, "colour")
    lut = rf.image_utils.srgb_byte_lut().astype(np.float32)
    wts = np.ascontiguousarray(rf.weights.load_weights(), dtype=np.float32).ravel()
    assert wts.size == rf._ffi.CNN_NPARAMS and lut.size == 256
    bufs = [Buf("weights", "in", data=wts)]
    if entry == "u8":
        bufs += [Buf("x", "in", data=bgr), Buf("lut", "in", data=lut)]
    elif entry == "f32_nhwc_bgr":
        bufs.append(Buf("x", "in", data=lut[bgr]))
    else:
        bufs.append(Buf("x", "in", data=np.ascontiguousarray(lut[bgr][..., ::-1].transpose(0, 3, 1, 2))))
    outputs = {}
    if want != "u8":
        bufs.append(Buf("r", "out", nbytes=4 * n * h * w, elem=4))
        outputs["r"] = (np.float32, (n, h, w))
    if want != "float":
        bufs.append(Buf("r8", "out", nbytes=n * h * w))
        outputs["r8"] = (np.uint8, (n, h, w))

    def call(lib, p, stream):
        if entry == "u8":
            return lib.rf_cnn_reflectance_u8(p["x"], p.get("r"), p.get("r8"), n, h, w, p["weights"], p["lut"], stream)
        layout = rf._ffi.CNN_NCHW_RGB if entry == "f32_nchw_rgb" else rf._ffi.CNN_NHWC_BGR
        return lib.rf_cnn_reflectance_f32(p["x"], p.get("r"), p.get("r8"), n, h, w, layout, p["weights"], stream)

    _contract(env, Case(bufs, call, outputs, lambda outs: _cnn_check(co, rf, bgr, outs)))


# ---- colourise -----------------------------------------------------------------------------------------

def _r_map(count, seed):
    return np.random.default_rng(seed).uniform(0.05, 1.0, count).astype(np.float32)


@pytest.mark.parametrize("shape", [S1, S3], ids=["S1", "S3"])
@pytest.mark.parametrize("want", ["both", "reflectance", "shading"])
def test_colorize_srgb_u8(env, want, shape):
    from oracle import colorize_numpy as oc
    rf, co, torch = env
    lib = rf._ffi.load_library()
    iu = rf.image_utils
    n, h, w = shape
    bgr = _images(shape, "colour")
    r = _r_map(n * h * w, 930).reshape(n, h, w)
    need = lib.rf_colorize_workspace_bytes(n)
    bufs = [Buf("bgr", "in", data=bgr), Buf("r", "in", data=r),
            Buf("steps", "in", data=np.ascontiguousarray(iu.srgb_write_steps(), dtype=np.float64))]
    outputs = {}
    if want != "shading":
        bufs.append(Buf("refl", "out", nbytes=3 * n * h * w))
        outputs["refl"] = (np.uint8, (n, h, w, 3))
    if want != "reflectance":
        bufs.append(Buf("shad", "out", nbytes=n * h * w))
        outputs["shad"] = (np.uint8, (n, h, w))
    bufs.append(Buf("ws", "ws", nbytes=need, elem=16))

    def call(lib, p, stream):
        return lib.rf_colorize_srgb_u8(p["bgr"], p["r"], p.get("refl"), p.get("shad"), n, h, w,
                                       iu.percentile_rank(3 * h * w), iu.percentile_rank(h * w), p["steps"],
                                       p["ws"], need, stream)

    def check(outs):
        for i in range(n):
            want_refl, want_shad = oc.colorize_srgb_u8(bgr[i], r[i])
            if "refl" in outs:
                assert np.array_equal(outs["refl"][i], want_refl), i
            if "shad" in outs:
                assert np.array_equal(outs["shad"][i], want_shad), i

    _contract(env, Case(bufs, call, outputs, check))


# ---- the float filters ---------------------------------------------------------------------------------

@pytest.mark.parametrize("cn", [3, 1], ids=["colour", "one_channel"])
def test_jbf_f32(env, cn):
    rf, co, torch = env
    lib = rf._ffi.load_library()
    n, h, w = S1
    joint, src = _floats(S1, cn, 940), _floats(S1, cn, 950)
    d, sc, ss = -1, 0.1, 4.0
    need = lib.rf_jbf_f32_workspace_bytes(n, cn)
    assert need > 0

    def call(lib, p, stream):
        return lib.rf_jbf_f32(p["joint"], p["src"], p["dst"], n, h, w, cn, cn, d, sc, ss, 4, p["ws"], need, stream)

    def check(outs):
        for i in range(n):
            want = co.joint_bilateral_filter_f32(joint[i], src[i], d, sc, ss).reshape(src[i].shape)
            assert np.array_equal(outs["dst"][i], want), i

    _contract(env, Case([Buf("joint", "in", data=joint), Buf("src", "in", data=src),
                         Buf("dst", "out", nbytes=src.nbytes, elem=4), Buf("ws", "ws", nbytes=need, elem=16)],
                        call, {"dst": (np.float32, src.shape)}, check))


@pytest.mark.parametrize("radius", [9, 150])
@pytest.mark.parametrize("cn", [3, 1], ids=["colour", "one_channel"])
def test_gf_f32(env, cn, radius):
    rf, co, torch = env
    lib = rf._ffi.load_library()
    n, h, w = S1
    guide, src = _floats(S1, 3, 960), _floats(S1, cn, 970)
    eps = 1e-3
    need = lib.rf_gf_f32_workspace_bytes(n, h, w, 3, cn, radius)
    assert need > 0

    def call(lib, p, stream):
        return lib.rf_gf_f32(p["guide"], p["src"], p["dst"], n, h, w, 3, cn, radius, eps, 1, p["ws"], need, stream)

    def check(outs):
        for i in range(n):
            want = co.guided_filter_f32(guide[i], src[i], radius, eps).reshape(src[i].shape)
            assert np.array_equal(outs["dst"][i], want, equal_nan=True), i

    _contract(env, Case([Buf("guide", "in", data=guide), Buf("src", "in", data=src),
                         Buf("dst", "out", nbytes=src.nbytes, elem=4), Buf("ws", "ws", nbytes=need, elem=16)],
                        call, {"dst": (np.float32, src.shape)}, check))


# ---- the point sweep -----------------------------------------------------------------------------------

POINT_PARAMS = ((20.0, 22.0), (15.0, 4.0))      # (sigma_color, sigma_space): radius 33 and 6


def _points(sizes, per_image, seed):
    rng = np.random.default_rng(seed)
    pts = np.concatenate([np.stack([rng.integers(0, w, per_image), rng.integers(0, h, per_image)], axis=1)
                          for h, w in sizes])
    pts[0], pts[per_image - 1] = (sizes[0][1] - 1, sizes[0][0] - 1), (0, 0)      # the corners too
    return _i32(pts), _i32(np.arange(len(sizes) + 1) * per_image)


def _points_want(co, joints, srcs, pts, offs):
    want = []
    for sc, ss in POINT_PARAMS:
        rows = []
        for i, (j, s) in enumerate(zip(joints, srcs)):
            full = co.joint_bilateral_filter(j, s, -1, sc, ss).reshape(s.shape)
            own = pts[offs[i]:offs[i + 1]]
            rows.append(full[own[:, 1], own[:, 0]])
        want.append(np.concatenate(rows))
    return np.stack(want)


@pytest.mark.parametrize("ragged", [False, True], ids=["rf_jbf_points_u8", "rf_jbf_points_ragged_u8"])
def test_jbf_points(env, ragged):
    rf, co, torch = env
    lib = rf._ffi.load_library()
    if ragged:
        sizes = MIXED
        joint, src = _packed("colour"), _packed("grey3")
        joints, srcs = _split(joint), _split(src)
        per = 60
    else:
        n, h, w = S1
        sizes = ((h, w),) * n
        joint, src = _images(S1, "colour"), _images(S1, "grey3")
        joints, srcs = list(joint), list(src)
        per = 150
    n = len(sizes)
    pts, offs = _points(sizes, per, 980)
    total = pts.shape[0]
    assert total == 300
    sc = np.array([p[0] for p in POINT_PARAMS], np.float64)
    ss = np.array([p[1] for p in POINT_PARAMS], np.float64)
    hs, wd = _i32([s[0] for s in sizes]), _i32([s[1] for s in sizes])
    if ragged:
        need = lib.rf_jbf_points_ragged_workspace_bytes(n, len(POINT_PARAMS), ss.ctypes.data, -1, 3, 0)
    else:
        need = lib.rf_jbf_points_workspace_bytes(len(POINT_PARAMS), ss.ctypes.data, -1, 3, 0)
    assert need > 0
    shape = (len(POINT_PARAMS), total, 3)

    def call(lib, p, stream):
        if ragged:
            return lib.rf_jbf_points_ragged_u8(p["joint"], p["src"], n, hs.ctypes.data, wd.ctypes.data, 3, 3,
                                               p["points"], p["offsets"], total, len(POINT_PARAMS), sc.ctypes.data,
                                               ss.ctypes.data, -1, 4, 0, p["out"], p["ws"], need, stream)
        return lib.rf_jbf_points_u8(p["joint"], p["src"], n, sizes[0][0], sizes[0][1], 3, 3, p["points"],
                                    p["offsets"], total, len(POINT_PARAMS), sc.ctypes.data, ss.ctypes.data, -1, 4,
                                    0, p["out"], p["ws"], need, stream)

    def check(outs):
        want = _points_want(co, joints, srcs, pts, offs)
        assert np.array_equal(outs["out"], want), np.argwhere(outs["out"] != want)[:4]

    _contract(env, Case([Buf("joint", "in", data=joint), Buf("src", "in", data=src),
                         Buf("points", "in", data=pts, fixed=4), Buf("offsets", "in", data=offs),
                         Buf("out", "out", nbytes=int(np.prod(shape))), Buf("ws", "ws", nbytes=need, elem=16)],
                        call, {"out": (np.uint8, shape)}, check))


# ---- WHDR ----------------------------------------------------------------------------------------------

def _comparisons(n, h, w, per_image, seed):
    """Per image [k,6] float64 rows (x1, y1, x2, y2, darker, weight) in pixel coordinates."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        comp = np.zeros((per_image, 6))
        comp[:, 0], comp[:, 2] = rng.integers(0, w, per_image), rng.integers(0, w, per_image)
        comp[:, 1], comp[:, 3] = rng.integers(0, h, per_image), rng.integers(0, h, per_image)
        comp[:, 4] = rng.integers(0, 3, per_image)
        comp[:, 5] = rng.random(per_image)
        out.append(comp)
    return out


@pytest.mark.parametrize("c", [3, 1])
def test_whdr_f32(env, c):
    rf, co, torch = env
    n, h, w = S1
    refl = np.ascontiguousarray(_floats(S1, c, 990).transpose(0, 3, 1, 2))        # planar [n][c][h][w]
    comps = _comparisons(n, h, w, 130, 991)
    allc = np.concatenate(comps)
    pts, wts = _i32(allc[:, :5]), np.ascontiguousarray(allc[:, 5])
    offs = _i32(np.arange(n + 1) * 130)

    def call(lib, p, stream):
        return lib.rf_whdr_f32(p["refl"], n, c, h, w, p["points"], p["weights"], p["offsets"], 0.1, p["out"], stream)

    def check(outs):
        want = np.array([rf.whdr.whdr(refl[i], comps[i], 0.1) for i in range(n)], dtype=np.float64)
        assert np.array_equal(outs["out"], want), (outs["out"], want)

    _contract(env, Case([Buf("refl", "in", data=refl), Buf("points", "in", data=pts), Buf("weights", "in", data=wts),
                         Buf("offsets", "in", data=offs), Buf("out", "out", nbytes=8 * n, elem=8, fixed=8)],
                        call, {"out": (np.float64, (n,))}, check))


@pytest.mark.parametrize("c", [3, 1])
def test_whdr_points_u8(env, c):
    """Two sets of whole images taken as point lists (pixel y * w + x of image i behind i * h * w)."""
    rf, co, torch = env
    n, h, w = S1
    sets = np.stack([_images(S1, "colour")[..., :c], _images(S1, "grey3")[..., :c]])     # [2][n][h][w][c]
    samples = np.ascontiguousarray(sets.reshape(2, n * h * w, c))
    comps = _comparisons(n, h, w, 130, 992)
    allc = np.concatenate(comps).astype(np.int64)
    idx = _i32(np.stack([allc[:, 1] * w + allc[:, 0], allc[:, 3] * w + allc[:, 2], allc[:, 4]], axis=1))
    wts = np.ascontiguousarray(np.concatenate(comps)[:, 5])
    poffs, coffs = _i32(np.arange(n + 1) * h * w), _i32(np.arange(n + 1) * 130)

    def call(lib, p, stream):
        return lib.rf_whdr_points_u8(p["samples"], 2, n * h * w, c, n, p["point_offsets"], p["comps"], p["weights"],
                                     p["comp_offsets"], 0.1, p["out"], stream)

    def check(outs):
        for s in range(2):
            for i in range(n):
                planar = np.ascontiguousarray(sets[s, i].transpose(2, 0, 1)).astype(np.float32) / np.float32(255)
                assert outs["out"][s, i] == np.float64(rf.whdr.whdr(planar, comps[i], 0.1)), (s, i)

    _contract(env, Case([Buf("samples", "in", data=samples), Buf("point_offsets", "in", data=poffs),
                         Buf("comps", "in", data=idx), Buf("weights", "in", data=wts),
                         Buf("comp_offsets", "in", data=coffs), Buf("out", "out", nbytes=8 * 2 * n, elem=8, fixed=8)],
                        call, {"out": (np.float64, (2, n))}, check))


# ---- the ragged entries: one mixed list each -------------------------------------------------------------

def _sizes_arrays():
    return _i32([s[0] for s in MIXED]), _i32([s[1] for s in MIXED])


def test_jbf_ragged_u8(env):
    rf, co, torch = env
    lib = rf._ffi.load_library()
    joint, src = _packed("colour"), _packed("grey3")
    hs, wd = _sizes_arrays()
    n, d, sc, ss = len(MIXED), -1, 20.0, 22.0
    need = lib.rf_jbf_ragged_workspace_bytes(n, hs.ctypes.data, wd.ctypes.data, 3, 3, d, ss, 0)
    assert need > 0 and rf._ffi.jbf_ragged_plan(MIXED, 3, 3, d, sc, ss) is not None

    def call(lib, p, stream):
        return lib.rf_jbf_ragged_u8(p["joint"], p["src"], p["dst"], n, hs.ctypes.data, wd.ctypes.data, 3, 3, d, sc,
                                    ss, 4, 0, p["ws"], need, stream)

    def check(outs):
        for i, (j, s, got) in enumerate(zip(_split(joint), _split(src), _split(outs["dst"]))):
            assert np.array_equal(got, co.joint_bilateral_filter(j, s, d, sc, ss)), i

    _contract(env, Case([Buf("joint", "in", data=joint), Buf("src", "in", data=src),
                         Buf("dst", "out", nbytes=src.nbytes), Buf("ws", "ws", nbytes=need, elem=16)],
                        call, {"dst": (np.uint8, src.shape)}, check))


def test_gf_ragged_u8(env):
    rf, co, torch = env
    lib = rf._ffi.load_library()
    guide, src = _packed("colour"), _packed("grey1")
    hs, wd = _sizes_arrays()
    n, radius, eps, iterations = len(MIXED), 9, 3.0, 2
    need = lib.rf_gf_ragged_workspace_bytes(n, hs.ctypes.data, wd.ctypes.data, 3, 1, radius, 0)
    assert need > 0 and rf._ffi.gf_ragged_plan(MIXED, 3, 1, radius) is not None

    def call(lib, p, stream):
        return lib.rf_gf_ragged_u8(p["guide"], p["src"], p["dst"], n, hs.ctypes.data, wd.ctypes.data, 3, 1, radius,
                                   eps, iterations, 0, p["ws"], need, stream)

    def check(outs):
        for i, (g, s, got) in enumerate(zip(_split(guide), _split(src), _split(outs["dst"]))):
            assert np.array_equal(got, _gf_oracle(co, [g], [s], radius, eps, iterations)[0]), i

    _contract(env, Case([Buf("guide", "in", data=guide), Buf("src", "in", data=src),
                         Buf("dst", "out", nbytes=src.nbytes), Buf("ws", "ws", nbytes=need, elem=16)],
                        call, {"dst": (np.uint8, src.shape)}, check))


@pytest.mark.parametrize("entry", ["rf_colorize_ragged_srgb_u8", "rf_colorize_ragged_r8_srgb_u8"])
def test_colorize_ragged(env, entry):
    from oracle import colorize_numpy as oc
    rf, co, torch = env
    lib = rf._ffi.load_library()
    iu = rf.image_utils
    bgr = _packed("colour")
    npx = bgr.shape[0]
    hs, wd = _sizes_arrays()
    n = len(MIXED)
    if entry.endswith("r8_srgb_u8"):
        r_in = np.random.default_rng(931).integers(13, 256, npx).astype(np.uint8)
        r = r_in.astype(np.float32) / np.float32(255)
    else:
        r_in = r = _r_map(npx, 932)
    k_refl = np.array([iu.percentile_rank(3 * h * w) for h, w in MIXED], np.uint64)
    k_shad = np.array([iu.percentile_rank(h * w) for h, w in MIXED], np.uint64)
    need = lib.rf_colorize_ragged_workspace_bytes(n, hs.ctypes.data, wd.ctypes.data)
    assert need > 0

    def call(lib, p, stream):
        return getattr(lib, entry)(p["bgr"], p["r"], p["refl"], p["shad"], n, hs.ctypes.data, wd.ctypes.data,
                                   k_refl.ctypes.data, k_shad.ctypes.data, p["steps"], p["ws"], need, stream)

    def check(outs):
        at = 0
        for i, (h, w) in enumerate(MIXED):
            want_refl, want_shad = oc.colorize_srgb_u8(bgr[at:at + h * w].reshape(h, w, 3),
                                                       r[at:at + h * w].reshape(h, w))
            assert np.array_equal(outs["refl"][at:at + h * w].reshape(h, w, 3), want_refl), i
            assert np.array_equal(outs["shad"][at:at + h * w].reshape(h, w), want_shad), i
            at += h * w

    _contract(env, Case([Buf("bgr", "in", data=bgr), Buf("r", "in", data=r_in),
                         Buf("steps", "in", data=np.ascontiguousarray(iu.srgb_write_steps(), dtype=np.float64)),
                         Buf("refl", "out", nbytes=3 * npx), Buf("shad", "out", nbytes=npx),
                         Buf("ws", "ws", nbytes=need, elem=16)],
                        call, {"refl": (np.uint8, (npx, 3)), "shad": (np.uint8, (npx,))}, check))


def test_png_deflate_ragged_u8(env):
    """The streams' used bytes and the offsets are the outputs; each stream inflates to the Up-filtered
    rows of its image (RGB order)."""
    rf, co, torch = env
    lib = rf._ffi.load_library()
    images = _packed("colour")
    hs, wd = _sizes_arrays()
    n = len(MIXED)
    args = (n, hs.ctypes.data, wd.ctypes.data, 3, 0)
    bound, need = lib.rf_png_stream_bound(*args), lib.rf_png_workspace_bytes(*args)
    assert bound > 0 and need > 0

    def call(lib, p, stream):
        return lib.rf_png_deflate_ragged_u8(p["images"], n, hs.ctypes.data, wd.ctypes.data, 3, 0, p["streams"], bound,
                                            p["offsets"], p["ws"], need, stream)

    def outputs(raw):
        offs = raw["offsets"][:8 * (n + 1)].view(np.uint64).copy()
        assert offs[0] == 0 and np.all(np.diff(offs.astype(np.int64)) > 0) and offs[-1] <= bound
        return {"offsets": offs, "streams": raw["streams"][:int(offs[-1])].copy()}

    def check(outs):
        offs = outs["offsets"]
        for i, img in enumerate(_split(images)):
            h, w = img.shape[:2]
            rows = np.frombuffer(zlib.decompress(outs["streams"][int(offs[i]):int(offs[i + 1])].tobytes()),
                                 np.uint8).reshape(h, 1 + 3 * w)
            assert (rows[:, 0] == 2).all()
            rgb = np.cumsum(rows[:, 1:].astype(np.int64), axis=0).astype(np.uint8).reshape(h, w, 3)
            assert np.array_equal(rgb[:, :, ::-1], img), i

    _contract(env, Case([Buf("images", "in", data=images), Buf("streams", "out", nbytes=bound),
                         Buf("offsets", "out", nbytes=8 * (n + 1), elem=8), Buf("ws", "ws", nbytes=need, elem=16)],
                        call, outputs, check))


def test_png_unfilter_ragged_u8(env):
    """raw is reconstructed in place, so it is an output; its bytes are not compared across layouts."""
    rf, co, torch = env
    lib = rf._ffi.load_library()
    iu = rf.image_utils
    rng = np.random.default_rng(995)
    formats = ((8, 2), (16, 6), (8, 3), (8, 0), (16, 0))
    datas, want = [], []
    for (h, w), (depth, ctype) in zip(MIXED, formats):
        rows = ps.samples(rng, h, w, depth, ctype, palette_len=200)
        palette = rng.integers(0, 256, (200, 3)).astype(np.uint8) if ctype == 3 else None
        datas.append(ps.write_png(rows, w, depth, ctype, ps.filters_for("random", h, rng), palette))
        want.append(iu._png_decode(datas[-1]))
    parsed = [iu.png_parse(d) for d in datas]
    assert all(p is not None for p in parsed)
    n = len(parsed)
    hs, wd = _sizes_arrays()
    fm = _i32([(p[2] << 8) | p[3] for p in parsed])
    offs = np.zeros(n + 1, np.uint64)
    offs[1:] = np.cumsum([len(p[5]) for p in parsed])
    raw = np.frombuffer(b"".join(p[5] for p in parsed), np.uint8)
    pal = np.zeros((n, 768), np.uint8)
    for i, p in enumerate(parsed):
        if p[4] is not None:
            pal[i, :np.asarray(p[4]).size] = np.asarray(p[4]).reshape(-1)
    npx = sum(h * w for h, w in MIXED)
    need = lib.rf_png_unfilter_workspace_bytes(n, hs.ctypes.data, wd.ctypes.data, fm.ctypes.data)
    assert need > 0

    def call(lib, p, stream):
        return lib.rf_png_unfilter_ragged_u8(p["raw"], offs.ctypes.data, n, hs.ctypes.data, wd.ctypes.data,
                                             fm.ctypes.data, p["palettes"], p["images"], p["flags"], p["ws"], need,
                                             stream)

    def check(outs):
        for i, (got, exp) in enumerate(zip(_split(outs["images"]), want)):
            assert np.array_equal(got, exp), i
        grey = [int((e[..., 0] == e[..., 1]).all() and (e[..., 1] == e[..., 2]).all()) for e in want]
        assert outs["flags"].tolist() == grey

    _contract(env, Case([Buf("raw", "out", data=raw), Buf("palettes", "in", data=pal),
                         Buf("images", "out", nbytes=3 * npx), Buf("flags", "out", nbytes=n),
                         Buf("ws", "ws", nbytes=need, elem=16)],
                        call, {"images": (np.uint8, (npx, 3)), "flags": (np.uint8, (n,))}, check))


# ---- the harness bites on the device -----------------------------------------------------------------------

def test_a_device_write_one_byte_past_an_output_is_reported(env):
    rf, co, torch = env
    ar = A.Arena(torch, "cuda", A.arena_bytes([105, 105]), 0xA5)
    src = ar.place(105, 1, name="src")
    dst = ar.place(105, 3, name="dst")
    ar.snapshot()
    view = ar.view(dst, (5, 7, 3), torch.uint8)
    view[:] = 7
    ar.assert_only_changed([dst])
    past = torch.tensor([dst.end], device="cuda")
    ar.buf[past] = 0                                  # an indexed write just past the output view
    torch.cuda.synchronize()
    with pytest.raises(AssertionError, match=r"1 byte\(s\) changed after dst .*first at offset 0 relative to its end"):
        ar.assert_only_changed([dst])
    ar.buf[torch.tensor([src.offset + 4], device="cuda")] = 1
    with pytest.raises(AssertionError, match=r"1 byte\(s\) changed inside src .*first at offset 4 relative"):
        ar.assert_only_changed([dst, A.Region("the byte behind dst", dst.end, 1)])
