"""The per-entry cases of the C ABI (include/reflectance_filtering.h), built once and run by three modules:
tests/test_gpu_buffer_contract.py places a case's buffers at odd addresses inside a guarded arena,
tests/test_gpu_stream_contract.py runs it on a busy side stream, tests/test_gpu_capture_contract.py
captures it into a graph (or sees it refused) and runs it across rf_shutdown().

A Case holds the buffers of one call with their host data, the call itself and the oracle check of its
outputs.  An input that holds pixel values, float values or weights also carries a `decoy`: another valid
input of the same kind and size whose result differs from the true one (complemented bytes, the same
floats in another order - a float decoy keeps the value range of the true image, since rf_jbf_f32 sizes
its table by that range -, the weights scaled by 0.5, another PNG stream of the same format and filter
bytes).  Index-like inputs (INDEX_LIKE) have none: whatever a call reads of them is always valid.

Shapes: S1 = 2 x 67 x 131 (w % 4 = 3, h % 64 = 3: 64x64 tiles with right and bottom strips; an image
is 26,331 or 8,777 bytes, both odd), S2 = 3 x 5 x 7 (smaller than every tile and window; 105 bytes),
S3 = 1 x 1 x 1, MIXED the ragged entries' list.

tests/size_cases.py runs the same cases over buffers that pass 2^31 and 2^32 bytes: for that a builder
takes `first` (the images behind the usual ones: another period of the same kind), the ragged ones
`sizes`, and a Case carries `sized(k)`: the same call over k periods, a period being the case's own
images (n of them for a uniform entry, the whole list for a ragged one), with the workspace it needs.
Buffers named in PER_CALL do not grow with the periods.

tests/train_cases.py builds the cases of librf_train_hip.so in the same format.
"""
import zlib

import numpy as np

from tests import png_synth as ps
from tests import synth

S1, S2, S3 = (2, 67, 131), (3, 5, 7), (1, 1, 1)
MIXED = ((67, 131), (5, 7), (5, 7), (67, 131), (5, 7))     # the ragged entries' list
INDEX_LIKE = ("points", "offsets", "point_offsets", "comps", "comp_offsets", "inc_offsets", "inc")
PER_CALL = ("weights", "lut", "steps", "packed", "ws")      # one per call, however many images it has


class Buf(object):
    """One buffer of a call.  role: "in", "out" or "ws"; data: host array written before the call
    (None: the arena's fill); fixed: the residue this buffer takes in every layout but L0; decoy: a
    host array of data's size and type (module docstring)."""

    def __init__(self, name, role, nbytes=None, data=None, elem=None, fixed=None, decoy=None):
        if data is not None:
            data = np.ascontiguousarray(data)
            nbytes = data.nbytes if nbytes is None else nbytes
            elem = data.dtype.itemsize if elem is None else elem
        if decoy is not None:
            decoy = np.ascontiguousarray(decoy)
            assert decoy.dtype == data.dtype and decoy.nbytes == data.nbytes, name
        self.name, self.role, self.nbytes, self.data = name, role, int(nbytes), data
        self.elem, self.fixed, self.decoy = int(elem or 1), fixed, decoy


class Case(object):
    """bufs: the call's buffers; call(lib, p, stream) -> return code, p[name] the device address;
    outputs: {name: (dtype, shape)} compared across layouts (a callable (raw bytes by name) -> dict of
    arrays where only part of an output is specified); check(outs): the L0 outputs against the oracle;
    around: a context manager factory held during the call (debug switches); entries: the header's
    entries the call goes through; sync: their header text says the call synchronises its stream;
    two_wg: the call takes rf_jbf_u8's two-workgroups-per-CU route (None: not such a call);
    sized(k) -> (call, workspace bytes): the call over k periods of this case's images (module docstring)."""

    def __init__(self, bufs, call, outputs, check, around=None, after=None, entries=(), sync=False,
                 two_wg=None, sized=None):
        self.bufs, self.call, self.outputs, self.check = bufs, call, outputs, check
        self.sized = sized
        self.around, self.after = around, after
        self.entries, self.sync, self.two_wg = tuple(entries), bool(sync), two_wg


def typed_outputs(case, raw):
    """The outputs of a case, typed and shaped, from the raw bytes of its "out" buffers by name."""
    if callable(case.outputs):
        return case.outputs(raw)
    return dict((name, raw[name][:int(np.prod(shape)) * np.dtype(dt).itemsize].view(dt).reshape(shape))
                for name, (dt, shape) in case.outputs.items())


def _once(fn):
    """fn() computed at the first call and kept (an oracle result shared by every run of a case)."""
    box = []

    def get():
        if not box:
            box.append(fn())
        return box[0]
    return get


def _inv(a):
    return np.ascontiguousarray(255 - np.asarray(a, dtype=np.uint8))


# ---- inputs, made once ---------------------------------------------------------------------------------

_cache = {}


def _images(shape, kind, first=0):
    """uint8 [n,h,w,c]: "colour" (3 channels), "grey3" (3 equal channels), "grey1", "joint1"; image i
    is number first + i of its kind."""
    key = (shape, kind, first)
    if key not in _cache:
        n, h, w = shape
        if kind == "colour":
            imgs = [synth.scene_u8(h, w, 900 + first + i) for i in range(n)]
        elif kind == "grey3":
            imgs = [synth.reflectance_like_u8(h, w, 910 + first + i) for i in range(n)]
        elif kind == "grey1":
            imgs = [synth.reflectance_like_u8(h, w, 910 + first + i)[:, :, :1] for i in range(n)]
        else:
            imgs = [synth.scene_u8(h, w, 920 + first + i)[:, :, 1:2] for i in range(n)]
        _cache[key] = np.ascontiguousarray(np.stack(imgs))
    return _cache[key]


def _floats(shape, c, seed, scale=1.0):
    key = (shape, c, seed, scale)
    if key not in _cache:
        n, h, w = shape
        imgs = np.stack([synth.scene_u8(h, w, seed + i)[:, :, :c] for i in range(n)])
        _cache[key] = np.ascontiguousarray(imgs.astype(np.float32) / np.float32(255) * np.float32(scale))
    return _cache[key]


def _packed(kind, sizes=MIXED, first=0):
    """The images of `sizes` packed one after another, [total pixels, c]."""
    key = ("packed", kind, sizes, first)
    if key not in _cache:
        parts = [_images((1, h, w), kind, first)[0].reshape(h * w, -1) for h, w in sizes]
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
                # 42 (the 37..52 tile kernel), 54 (slabs), 33 untiled, 1 (two workgroups per CU again), 1 untiled
    "s22": (-1, 22.0, 0), "s28": (-1, 28.0, 0), "s36": (-1, 36.0, 0), "generic": (-1, 22.0, 2), "d3": (3, 22.0, 0),
    "generic_d3": (3, 22.0, 2),
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


def jbf_u8(env, pair, route, shape, sigma_color=20.0, images=None, first=0):
    """images: (joint, src) uint8 [n,h,w,c] in place of the synthetic ones of `pair` (its flags stay)."""
    rf, co, torch = env
    lib = rf._ffi.load_library()
    jkind, skind, flags = JBF_PAIRS[pair]
    d, ss, extra = JBF_ROUTES[route]
    flags |= extra
    joint, src = images if images is not None else (_images(shape, jkind, first), _images(shape, skind, first))
    n, h, w = shape
    assert joint.shape[:3] == shape and src.shape[:3] == shape
    jcn, scn, sc = joint.shape[3], src.shape[3], sigma_color
    on_route = rf._ffi.jbf_two_wg_plan(n, h, w, jcn, scn, d, sc, ss, flags) is not None
    if route == "s22" and shape == S1 and pair in ("colour_grey3", "colour_grey1"):
        assert on_route, "the plan no longer puts this case on the two-workgroups-per-CU route"
    if route in ("s28", "s36", "generic", "generic_d3"):
        assert not on_route
    count = [lib.rf_debug_jbf_two_wg_calls()]

    def sized(k):
        assert (rf._ffi.jbf_two_wg_plan(k * n, h, w, jcn, scn, d, sc, ss, flags) is not None) == on_route

        def call(lib, p, stream):
            return lib.rf_jbf_u8(p["joint"], p["src"], p["dst"], k * n, h, w, jcn, scn, d, sc, ss, 4, flags, stream)
        return call, 0
    call = sized(1)[0]

    def after():
        now = lib.rf_debug_jbf_two_wg_calls()
        assert now - count[0] == (1 if on_route else 0), "the call did not take the route the plan names"
        count[0] = now

    oracle = _once(lambda: _jbf_oracle(co, joint, src, d, sc, ss, flags))

    def check(outs):
        want = oracle()
        assert np.array_equal(outs["dst"], want), np.argwhere(outs["dst"] != want)[:4]

    return Case([Buf("joint", "in", data=joint, decoy=_inv(joint)), Buf("src", "in", data=src, decoy=_inv(src)),
                 Buf("dst", "out", nbytes=src.nbytes)],
                call, {"dst": (np.uint8, src.shape)}, check, after=after, entries=("rf_jbf_u8",),
                two_wg=on_route, sized=sized)


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


def gf_u8(env, shape, skind, radius, iterations, two_kernel=False, ws_images=None, in_place=False,
          grey_guide=False, options=None, first=0):
    """options: debug switches held during the call ({"gf_force_two_streams": 1}, ...); ws_images: the
    workspace is sized for that many images, whatever n is."""
    rf, co, torch = env
    lib = rf._ffi.load_library()
    n, h, w = shape
    guide = _images(shape, "joint1" if grey_guide else "colour", first)
    src = _images(shape, skind, first)
    gcn, scn, eps = guide.shape[3], src.shape[3], 3.0
    need = lib.rf_gf_workspace_bytes(n if ws_images is None else ws_images, h, w, 3, scn, radius)
    assert need > 0
    if ws_images is not None and ws_images < n:
        assert need < lib.rf_gf_workspace_bytes(n, h, w, 3, scn, radius)

    def sized(k):
        ws = need if ws_images is not None else lib.rf_gf_workspace_bytes(k * n, h, w, 3, scn, radius)

        def call(lib, p, stream):
            dst = p["src"] if in_place else p["dst"]
            if grey_guide:
                return lib.rf_gf_ex_u8(p["guide"], p["src"], dst, k * n, h, w, gcn, scn, radius, eps, iterations,
                                       rf._ffi.GF_GREY_AS_BGR, p["ws"], ws, stream)
            return lib.rf_gf_u8(p["guide"], p["src"], dst, k * n, h, w, gcn, scn, radius, eps, iterations, p["ws"],
                                ws, stream)
        return call, ws
    call = sized(1)[0]

    out_name = "src" if in_place else "dst"
    oracle = _once(lambda: _gf_oracle(co, guide, src, radius, eps, iterations, grey_guide))

    def check(outs):
        want = oracle()
        assert np.array_equal(outs[out_name], want), np.argwhere(outs[out_name] != want)[:4]

    bufs = [Buf("guide", "in", data=guide, decoy=_inv(guide)),
            Buf("src", "out" if in_place else "in", data=src, decoy=_inv(src))]
    if not in_place:
        bufs.append(Buf("dst", "out", nbytes=src.nbytes))
    bufs.append(Buf("ws", "ws", nbytes=need, elem=16))
    opts = dict(options or {})
    if two_kernel:
        opts["gf_two_kernel"] = 1
    around = (lambda: rf._ffi.debug_options(**opts)) if opts else None
    return Case(bufs, call, {out_name: (np.uint8, src.shape)}, check, around=around,
                entries=("rf_gf_ex_u8" if grey_guide else "rf_gf_u8",), sized=sized)


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


def cnn_reflectance(env, entry, want, shape, packed=False, first=0):
    """packed: the weights go through rf_cnn_pack_weights into a caller-owned buffer and the forward pass
    is the packed twin of `entry`, both on the call's stream."""
    rf, co, torch = env
    n, h, w = shape
    bgr = _images(shape, "colour", first)
    lut = rf.image_utils.srgb_byte_lut().astype(np.float32)
    wts = np.ascontiguousarray(rf.weights.load_weights(), dtype=np.float32).ravel()
    assert wts.size == rf._ffi.CNN_NPARAMS and lut.size == 256
    half = np.float32(0.5)
    bufs = [Buf("weights", "in", data=wts, decoy=wts * half)]
    if entry == "u8":
        bufs += [Buf("x", "in", data=bgr, decoy=_inv(bgr)), Buf("lut", "in", data=lut, decoy=lut * half)]
    elif entry == "f32_nhwc_bgr":
        bufs.append(Buf("x", "in", data=lut[bgr], decoy=lut[bgr][:, ::-1, ::-1, :]))
    else:
        x = np.ascontiguousarray(lut[bgr][..., ::-1].transpose(0, 3, 1, 2))
        bufs.append(Buf("x", "in", data=x, decoy=x[:, :, ::-1, ::-1]))
    if packed:
        bufs.append(Buf("packed", "ws", nbytes=4 * rf._ffi.CNN_NPACKED, elem=4))
    outputs = {}
    if want != "u8":
        bufs.append(Buf("r", "out", nbytes=4 * n * h * w, elem=4))
        outputs["r"] = (np.float32, (n, h, w))
    if want != "float":
        bufs.append(Buf("r8", "out", nbytes=n * h * w))
        outputs["r8"] = (np.uint8, (n, h, w))
    layout = rf._ffi.CNN_NCHW_RGB if entry == "f32_nchw_rgb" else rf._ffi.CNN_NHWC_BGR

    def sized(k):
        m = k * n

        def call(lib, p, stream):
            if packed:
                rc = lib.rf_cnn_pack_weights(p["weights"], p["packed"], stream)
                if rc != rf._ffi.RF_OK:
                    return rc
                if entry == "u8":
                    return lib.rf_cnn_reflectance_packed_u8(p["x"], p.get("r"), p.get("r8"), m, h, w, p["packed"],
                                                            p["lut"], stream)
                return lib.rf_cnn_reflectance_packed_f32(p["x"], p.get("r"), p.get("r8"), m, h, w, layout,
                                                         p["packed"], stream)
            if entry == "u8":
                return lib.rf_cnn_reflectance_u8(p["x"], p.get("r"), p.get("r8"), m, h, w, p["weights"], p["lut"],
                                                 stream)
            return lib.rf_cnn_reflectance_f32(p["x"], p.get("r"), p.get("r8"), m, h, w, layout, p["weights"], stream)
        return call, 0
    call = sized(1)[0]

    forward = "rf_cnn_reflectance_%s%s" % ("packed_" if packed else "", "u8" if entry == "u8" else "f32")
    return Case(bufs, call, outputs, lambda outs: _cnn_check(co, rf, bgr, outs),
                entries=(("rf_cnn_pack_weights",) if packed else ()) + (forward,), sized=sized)


# ---- colourise -----------------------------------------------------------------------------------------

def _r_map(count, seed):
    return np.random.default_rng(seed).uniform(0.05, 1.0, count).astype(np.float32)


def _r_decoy(r):
    """Another valid reflectance map: 1.05 - r lies in [0.05, 1] like r."""
    return (np.float32(1.05) - r).astype(np.float32)


def _steps(iu):
    steps = np.ascontiguousarray(iu.srgb_write_steps(), dtype=np.float64)
    return Buf("steps", "in", data=steps, decoy=steps * 0.5)


def colorize_srgb_u8(env, want, shape, first=0):
    from oracle import colorize_numpy as oc
    rf, co, torch = env
    lib = rf._ffi.load_library()
    iu = rf.image_utils
    n, h, w = shape
    bgr = _images(shape, "colour", first)
    r = _r_map(n * h * w, 930 + 7 * first).reshape(n, h, w)
    need = lib.rf_colorize_workspace_bytes(n)
    bufs = [Buf("bgr", "in", data=bgr, decoy=_inv(bgr)), Buf("r", "in", data=r, decoy=_r_decoy(r)), _steps(iu)]
    outputs = {}
    if want != "shading":
        bufs.append(Buf("refl", "out", nbytes=3 * n * h * w))
        outputs["refl"] = (np.uint8, (n, h, w, 3))
    if want != "reflectance":
        bufs.append(Buf("shad", "out", nbytes=n * h * w))
        outputs["shad"] = (np.uint8, (n, h, w))
    bufs.append(Buf("ws", "ws", nbytes=need, elem=16))

    def sized(k):
        ws = lib.rf_colorize_workspace_bytes(k * n)

        def call(lib, p, stream):
            return lib.rf_colorize_srgb_u8(p["bgr"], p["r"], p.get("refl"), p.get("shad"), k * n, h, w,
                                           iu.percentile_rank(3 * h * w), iu.percentile_rank(h * w), p["steps"],
                                           p["ws"], ws, stream)
        return call, ws
    call = sized(1)[0]

    oracle = _once(lambda: [oc.colorize_srgb_u8(bgr[i], r[i]) for i in range(n)])

    def check(outs):
        for i in range(n):
            want_refl, want_shad = oracle()[i]
            if "refl" in outs:
                assert np.array_equal(outs["refl"][i], want_refl), i
            if "shad" in outs:
                assert np.array_equal(outs["shad"][i], want_shad), i

    return Case(bufs, call, outputs, check, entries=("rf_colorize_srgb_u8",), sized=sized)


# ---- the float filters ---------------------------------------------------------------------------------

def _flipped(x):
    """[n,h,w,c] floats: every image upside down and mirrored - the same values, hence the same range."""
    return np.ascontiguousarray(x[:, ::-1, ::-1, :])


def jbf_f32(env, cn, d=-1, sigma_color=0.1, sigma_space=4.0, shape=S1, first=0):
    rf, co, torch = env
    lib = rf._ffi.load_library()
    n, h, w = shape
    joint, src = _floats(shape, cn, 940 + first), _floats(shape, cn, 950 + first)
    sc, ss = sigma_color, sigma_space
    need = lib.rf_jbf_f32_workspace_bytes(n, cn)
    assert need > 0

    def sized(k):
        ws = lib.rf_jbf_f32_workspace_bytes(k * n, cn)

        def call(lib, p, stream):
            return lib.rf_jbf_f32(p["joint"], p["src"], p["dst"], k * n, h, w, cn, cn, d, sc, ss, 4, p["ws"], ws,
                                  stream)
        return call, ws
    call = sized(1)[0]

    oracle = _once(lambda: [co.joint_bilateral_filter_f32(joint[i], src[i], d, sc, ss).reshape(src[i].shape)
                            for i in range(n)])

    def check(outs):
        for i in range(n):
            assert np.array_equal(outs["dst"][i], oracle()[i]), i

    return Case([Buf("joint", "in", data=joint, decoy=_flipped(joint)), Buf("src", "in", data=src, decoy=_flipped(src)),
                 Buf("dst", "out", nbytes=src.nbytes, elem=4), Buf("ws", "ws", nbytes=need, elem=16)],
                call, {"dst": (np.float32, src.shape)}, check, entries=("rf_jbf_f32",), sync=True, sized=sized)


def gf_f32(env, cn, radius, shape=S1, first=0):
    rf, co, torch = env
    lib = rf._ffi.load_library()
    n, h, w = shape
    guide, src = _floats(shape, 3, 960 + first), _floats(shape, cn, 970 + first)
    eps = 1e-3
    need = lib.rf_gf_f32_workspace_bytes(n, h, w, 3, cn, radius)
    assert need > 0

    def sized(k):
        """(the workspace of 64 images at most: a longer batch runs in chunks)"""
        ws = lib.rf_gf_f32_workspace_bytes(min(k * n, 64), h, w, 3, cn, radius)

        def call(lib, p, stream):
            return lib.rf_gf_f32(p["guide"], p["src"], p["dst"], k * n, h, w, 3, cn, radius, eps, 1, p["ws"], ws,
                                 stream)
        return call, ws
    call = sized(1)[0]

    oracle = _once(lambda: [co.guided_filter_f32(guide[i], src[i], radius, eps).reshape(src[i].shape)
                            for i in range(n)])

    def check(outs):
        for i in range(n):
            assert np.array_equal(outs["dst"][i], oracle()[i], equal_nan=True), i

    return Case([Buf("guide", "in", data=guide, decoy=_flipped(guide)), Buf("src", "in", data=src, decoy=_flipped(src)),
                 Buf("dst", "out", nbytes=src.nbytes, elem=4), Buf("ws", "ws", nbytes=need, elem=16)],
                call, {"dst": (np.float32, src.shape)}, check, entries=("rf_gf_f32",), sized=sized)


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


def points_call(lib, ragged, sizes, jcn, scn, total):
    """(call, workspace bytes) of the point entry - ragged or uniform - over the images `sizes` ((h, w) each,
    all alike for the uniform entry) with `total` points and POINT_PARAMS."""
    n = len(sizes)
    sc = np.array([p[0] for p in POINT_PARAMS], np.float64)
    ss = np.array([p[1] for p in POINT_PARAMS], np.float64)
    hs, wd = _sizes_arrays(sizes)
    if ragged:
        need = lib.rf_jbf_points_ragged_workspace_bytes(n, len(POINT_PARAMS), ss.ctypes.data, -1, jcn, 0)
    else:
        assert len(set(sizes)) == 1
        need = lib.rf_jbf_points_workspace_bytes(len(POINT_PARAMS), ss.ctypes.data, -1, jcn, 0)
    assert need > 0

    def call(lib, p, stream):
        if ragged:
            return lib.rf_jbf_points_ragged_u8(p["joint"], p["src"], n, hs.ctypes.data, wd.ctypes.data, jcn, scn,
                                               p["points"], p["offsets"], total, len(POINT_PARAMS), sc.ctypes.data,
                                               ss.ctypes.data, -1, 4, 0, p["out"], p["ws"], need, stream)
        return lib.rf_jbf_points_u8(p["joint"], p["src"], n, sizes[0][0], sizes[0][1], jcn, scn, p["points"],
                                    p["offsets"], total, len(POINT_PARAMS), sc.ctypes.data, ss.ctypes.data, -1, 4,
                                    0, p["out"], p["ws"], need, stream)
    return call, need


def jbf_points(env, ragged, sizes=None, jkind="colour", skind="grey3", first=0):
    """sizes: the images ((h, w) each; MIXED for the ragged entry, S1's for the uniform one)."""
    rf, co, torch = env
    lib = rf._ffi.load_library()
    if ragged:
        sizes = MIXED if sizes is None else sizes
        joint, src = _packed(jkind, sizes, first), _packed(skind, sizes, first)
        joints, srcs = _split(joint, sizes), _split(src, sizes)
        per = 60
    else:
        sizes = ((S1[1], S1[2]),) * S1[0] if sizes is None else sizes
        shape = (len(sizes),) + tuple(sizes[0])
        joint, src = _images(shape, jkind, first), _images(shape, skind, first)
        joints, srcs = list(joint), list(src)
        per = 150
    jcn, scn = joints[0].shape[2], srcs[0].shape[2]
    pts, offs = _points(sizes, per, 980 + 7 * first)
    total = pts.shape[0]
    assert total == per * len(sizes)
    call, need = points_call(lib, ragged, sizes, jcn, scn, total)
    shape = (len(POINT_PARAMS), total, scn)

    oracle = _once(lambda: _points_want(co, joints, srcs, pts, offs))

    def check(outs):
        want = oracle()
        assert np.array_equal(outs["out"], want), np.argwhere(outs["out"] != want)[:4]

    return Case([Buf("joint", "in", data=joint, decoy=_inv(joint)), Buf("src", "in", data=src, decoy=_inv(src)),
                 Buf("points", "in", data=pts, fixed=4), Buf("offsets", "in", data=offs),
                 Buf("out", "out", nbytes=int(np.prod(shape))), Buf("ws", "ws", nbytes=need, elem=16)],
                call, {"out": (np.uint8, shape)}, check,
                entries=("rf_jbf_points_ragged_u8" if ragged else "rf_jbf_points_u8",), sync=True)


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


def whdr_f32(env, c, shape=S1, first=0):
    rf, co, torch = env
    n, h, w = shape
    refl = np.ascontiguousarray(_floats(shape, c, 990 + first).transpose(0, 3, 1, 2))        # planar [n][c][h][w]
    comps = _comparisons(n, h, w, 130, 991 + 7 * first)
    allc = np.concatenate(comps)
    pts, wts = _i32(allc[:, :5]), np.ascontiguousarray(allc[:, 5])
    offs = _i32(np.arange(n + 1) * 130)

    def call(lib, p, stream):
        return lib.rf_whdr_f32(p["refl"], n, c, h, w, p["points"], p["weights"], p["offsets"], 0.1, p["out"], stream)

    def check(outs):
        want = np.array([rf.whdr.whdr(refl[i], comps[i], 0.1) for i in range(n)], dtype=np.float64)
        assert np.array_equal(outs["out"], want), (outs["out"], want)

    return Case([Buf("refl", "in", data=refl, decoy=refl[:, :, ::-1, ::-1]), Buf("points", "in", data=pts),
                 Buf("weights", "in", data=wts, decoy=wts[::-1]),
                 Buf("offsets", "in", data=offs), Buf("out", "out", nbytes=8 * n, elem=8, fixed=8)],
                call, {"out": (np.float64, (n,))}, check, entries=("rf_whdr_f32",))


def whdr_points_u8(env, c, shape=S1, first=0):
    """Two sets of whole images taken as point lists (pixel y * w + x of image i behind i * h * w)."""
    rf, co, torch = env
    n, h, w = shape
    sets = np.stack([_images(shape, "colour", first)[..., :c], _images(shape, "grey3", first)[..., :c]])  # [2][n][h][w][c]
    samples = np.ascontiguousarray(sets.reshape(2, n * h * w, c))
    comps = _comparisons(n, h, w, 130, 992 + 7 * first)
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

    # the decoy samples are the true ones back to front (complemented bytes would keep most decisions:
    # the ratio test is close to symmetric in light and dark)
    return Case([Buf("samples", "in", data=samples, decoy=samples[:, ::-1, :]), Buf("point_offsets", "in", data=poffs),
                 Buf("comps", "in", data=idx), Buf("weights", "in", data=wts, decoy=wts[::-1]),
                 Buf("comp_offsets", "in", data=coffs), Buf("out", "out", nbytes=8 * 2 * n, elem=8, fixed=8)],
                call, {"out": (np.float64, (2, n))}, check, entries=("rf_whdr_points_u8",))


# ---- the ragged entries: one mixed list each -------------------------------------------------------------

def _sizes_arrays(sizes=MIXED):
    return _i32([s[0] for s in sizes]), _i32([s[1] for s in sizes])


def jbf_ragged_u8(env, sigma_space=22.0, sizes=MIXED, skind="grey3", first=0, flags=0):
    """sigma_space 22: radius 33, the tile classes; 36: radius 54, the slab launch; flags
    RF_JBF_FORCE_GENERIC: the fallback route, rf_jbf_u8 once per image."""
    rf, co, torch = env
    lib = rf._ffi.load_library()
    joint, src = _packed("colour", sizes, first), _packed(skind, sizes, first)
    scn = src.shape[1]
    hs, wd = _sizes_arrays(sizes)
    n, d, sc, ss = len(sizes), -1, 20.0, sigma_space
    need = lib.rf_jbf_ragged_workspace_bytes(n, hs.ctypes.data, wd.ctypes.data, 3, scn, d, ss, flags)
    assert need > 0
    tiled = rf._ffi.jbf_ragged_plan(sizes, 3, scn, d, sc, ss, flags)
    slabs = rf._ffi.jbf_ragged_slab_plan(sizes, 3, scn, d, sc, ss, flags)
    if flags & rf._ffi.JBF_FORCE_GENERIC:
        assert tiled is None and slabs is None, "the plan no longer puts this list on the fallback route"
    elif int(np.rint(ss * 1.5)) <= 52:
        assert tiled is not None
    else:
        assert slabs is not None

    def sized(k):
        hk, wk = np.tile(hs, k), np.tile(wd, k)
        ws = lib.rf_jbf_ragged_workspace_bytes(k * n, hk.ctypes.data, wk.ctypes.data, 3, scn, d, ss, flags)
        assert ws > 0

        def call(lib, p, stream):
            return lib.rf_jbf_ragged_u8(p["joint"], p["src"], p["dst"], k * n, hk.ctypes.data, wk.ctypes.data, 3, scn,
                                        d, sc, ss, 4, flags, p["ws"], ws, stream)
        return call, ws
    call = sized(1)[0]

    oracle = _once(lambda: [co.joint_bilateral_filter(j, s, d, sc, ss).reshape(s.shape)
                            for j, s in zip(_split(joint, sizes), _split(src, sizes))])

    def check(outs):
        for i, got in enumerate(_split(outs["dst"], sizes)):
            assert np.array_equal(got, oracle()[i]), i

    return Case([Buf("joint", "in", data=joint, decoy=_inv(joint)), Buf("src", "in", data=src, decoy=_inv(src)),
                 Buf("dst", "out", nbytes=src.nbytes), Buf("ws", "ws", nbytes=need, elem=16)],
                call, {"dst": (np.uint8, src.shape)}, check, entries=("rf_jbf_ragged_u8",), sync=True, sized=sized)


def gf_ragged_u8(env, sizes=MIXED, grey_guide=False, first=0, skind="grey1", radius=9):
    """grey_guide: a one-channel guide under RF_GF_GREY_AS_BGR; skind "grey3" (a 3-channel src) or radius
    0: the fallback route, rf_gf_ex_u8 once per image."""
    rf, co, torch = env
    lib = rf._ffi.load_library()
    guide, src = _packed("joint1" if grey_guide else "colour", sizes, first), _packed(skind, sizes, first)
    gcn, scn, flags = guide.shape[1], src.shape[1], (rf._ffi.GF_GREY_AS_BGR if grey_guide else 0)
    hs, wd = _sizes_arrays(sizes)
    n, eps, iterations = len(sizes), 3.0, 2
    need = lib.rf_gf_ragged_workspace_bytes(n, hs.ctypes.data, wd.ctypes.data, gcn, scn, radius, flags)
    assert need > 0
    if not grey_guide:
        on_route = rf._ffi.gf_ragged_plan(sizes, 3, scn, radius) is not None
        assert on_route == (scn == 1 and 1 <= radius <= 128), "the plan names another route for this list"

    def sized(k):
        hk, wk = np.tile(hs, k), np.tile(wd, k)
        ws = lib.rf_gf_ragged_workspace_bytes(k * n, hk.ctypes.data, wk.ctypes.data, gcn, scn, radius, flags)
        assert ws > 0

        def call(lib, p, stream):
            return lib.rf_gf_ragged_u8(p["guide"], p["src"], p["dst"], k * n, hk.ctypes.data, wk.ctypes.data, gcn, scn,
                                       radius, eps, iterations, flags, p["ws"], ws, stream)
        return call, ws
    call = sized(1)[0]

    oracle = _once(lambda: [_gf_oracle(co, [g], [s], radius, eps, iterations, grey_guide)[0]
                            for g, s in zip(_split(guide, sizes), _split(src, sizes))])

    def check(outs):
        for i, got in enumerate(_split(outs["dst"], sizes)):
            assert np.array_equal(got, oracle()[i]), i

    return Case([Buf("guide", "in", data=guide, decoy=_inv(guide)), Buf("src", "in", data=src, decoy=_inv(src)),
                 Buf("dst", "out", nbytes=src.nbytes), Buf("ws", "ws", nbytes=need, elem=16)],
                call, {"dst": (np.uint8, src.shape)}, check, entries=("rf_gf_ragged_u8",), sync=True, sized=sized)


def colorize_ragged(env, entry, sizes=MIXED, first=0):
    from oracle import colorize_numpy as oc
    rf, co, torch = env
    lib = rf._ffi.load_library()
    iu = rf.image_utils
    bgr = _packed("colour", sizes, first)
    npx = bgr.shape[0]
    hs, wd = _sizes_arrays(sizes)
    n = len(sizes)
    if entry.endswith("r8_srgb_u8"):
        r_in = np.random.default_rng(931 + 7 * first).integers(13, 256, npx).astype(np.uint8)
        r = r_in.astype(np.float32) / np.float32(255)
        r_decoy = (268 - r_in.astype(np.int64)).astype(np.uint8)          # 13..255 again
    else:
        r_in = r = _r_map(npx, 932 + 7 * first)
        r_decoy = _r_decoy(r_in)
    k_refl = np.array([iu.percentile_rank(3 * h * w) for h, w in sizes], np.uint64)
    k_shad = np.array([iu.percentile_rank(h * w) for h, w in sizes], np.uint64)
    need = lib.rf_colorize_ragged_workspace_bytes(n, hs.ctypes.data, wd.ctypes.data)
    assert need > 0

    def sized(k):
        hk, wk, kr, ks = np.tile(hs, k), np.tile(wd, k), np.tile(k_refl, k), np.tile(k_shad, k)
        ws = lib.rf_colorize_ragged_workspace_bytes(k * n, hk.ctypes.data, wk.ctypes.data)
        assert ws > 0

        def call(lib, p, stream):
            return getattr(lib, entry)(p["bgr"], p["r"], p["refl"], p["shad"], k * n, hk.ctypes.data, wk.ctypes.data,
                                       kr.ctypes.data, ks.ctypes.data, p["steps"], p["ws"], ws, stream)
        return call, ws
    call = sized(1)[0]

    def want_all():
        out, at = [], 0
        for h, w in sizes:
            out.append(oc.colorize_srgb_u8(bgr[at:at + h * w].reshape(h, w, 3), r[at:at + h * w].reshape(h, w)))
            at += h * w
        return out
    oracle = _once(want_all)

    def check(outs):
        at = 0
        for i, (h, w) in enumerate(sizes):
            want_refl, want_shad = oracle()[i]
            assert np.array_equal(outs["refl"][at:at + h * w].reshape(h, w, 3), want_refl), i
            assert np.array_equal(outs["shad"][at:at + h * w].reshape(h, w), want_shad), i
            at += h * w

    return Case([Buf("bgr", "in", data=bgr, decoy=_inv(bgr)), Buf("r", "in", data=r_in, decoy=r_decoy), _steps(iu),
                 Buf("refl", "out", nbytes=3 * npx), Buf("shad", "out", nbytes=npx),
                 Buf("ws", "ws", nbytes=need, elem=16)],
                call, {"refl": (np.uint8, (npx, 3)), "shad": (np.uint8, (npx,))}, check, entries=(entry,), sync=True,
                sized=sized)


def png_deflate_ragged_u8(env):
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

    return Case([Buf("images", "in", data=images, decoy=_inv(images)), Buf("streams", "out", nbytes=bound),
                 Buf("offsets", "out", nbytes=8 * (n + 1), elem=8), Buf("ws", "ws", nbytes=need, elem=16)],
                call, outputs, check, entries=("rf_png_deflate_ragged_u8",), sync=True)


def png_unfilter_ragged_u8(env, first=0):
    """raw is reconstructed in place, so it is an output; its bytes are not compared across layouts."""
    rf, co, torch = env
    lib = rf._ffi.load_library()
    iu = rf.image_utils
    rng = np.random.default_rng(995 + 7 * first)
    other = np.random.default_rng(996 + 7 * first)          # the decoy streams: other samples behind the same filter bytes
    formats = ((8, 2), (16, 6), (8, 3), (8, 0), (16, 0))
    datas, want, decoys = [], [], []
    for (h, w), (depth, ctype) in zip(MIXED, formats):
        rows = ps.samples(rng, h, w, depth, ctype, palette_len=200)
        palette = rng.integers(0, 256, (200, 3)).astype(np.uint8) if ctype == 3 else None
        filters = ps.filters_for("random", h, rng)
        datas.append(ps.write_png(rows, w, depth, ctype, list(filters), palette))
        want.append(iu._png_decode(datas[-1]))
        decoys.append(ps.write_png(ps.samples(other, h, w, depth, ctype, palette_len=200), w, depth, ctype,
                                   list(filters), palette))
    parsed = [iu.png_parse(d) for d in datas]
    assert all(p is not None for p in parsed)
    n = len(parsed)
    hs, wd = _sizes_arrays()
    fm = _i32([(p[2] << 8) | p[3] for p in parsed])
    offs = np.zeros(n + 1, np.uint64)
    offs[1:] = np.cumsum([len(p[5]) for p in parsed])
    raw = np.frombuffer(b"".join(p[5] for p in parsed), np.uint8)
    raw_decoy = np.frombuffer(b"".join(iu.png_parse(d)[5] for d in decoys), np.uint8)
    assert raw_decoy.size == raw.size and not np.array_equal(raw_decoy, raw)
    at = 0
    for (h, w), p in zip(MIXED, parsed):         # ... row by row the same filter byte
        pitch = len(p[5]) // h
        assert np.array_equal(raw[at:at + len(p[5]):pitch], raw_decoy[at:at + len(p[5]):pitch])
        at += len(p[5])
    pal = np.zeros((n, 768), np.uint8)
    for i, p in enumerate(parsed):
        if p[4] is not None:
            pal[i, :np.asarray(p[4]).size] = np.asarray(p[4]).reshape(-1)
    npx = sum(h * w for h, w in MIXED)
    need = lib.rf_png_unfilter_workspace_bytes(n, hs.ctypes.data, wd.ctypes.data, fm.ctypes.data)
    assert need > 0

    def sized(k):
        hk, wk, fk = np.tile(hs, k), np.tile(wd, k), np.tile(fm, k)
        ok = np.concatenate([offs[:-1] + np.uint64(i) * offs[-1] for i in range(k)] + [offs[-1:] * np.uint64(k)])
        ws = lib.rf_png_unfilter_workspace_bytes(k * n, hk.ctypes.data, wk.ctypes.data, fk.ctypes.data)
        assert ws > 0 and ok.dtype == np.uint64 and ok.size == k * n + 1

        def call(lib, p, stream):
            return lib.rf_png_unfilter_ragged_u8(p["raw"], ok.ctypes.data, k * n, hk.ctypes.data, wk.ctypes.data,
                                                 fk.ctypes.data, p["palettes"], p["images"], p["flags"], p["ws"], ws,
                                                 stream)
        return call, ws
    call = sized(1)[0]

    def check(outs):
        for i, (got, exp) in enumerate(zip(_split(outs["images"]), want)):
            assert np.array_equal(got, exp), i
        grey = [int((e[..., 0] == e[..., 1]).all() and (e[..., 1] == e[..., 2]).all()) for e in want]
        assert outs["flags"].tolist() == grey

    return Case([Buf("raw", "out", data=raw, decoy=raw_decoy), Buf("palettes", "in", data=pal, decoy=_inv(pal)),
                 Buf("images", "out", nbytes=3 * npx), Buf("flags", "out", nbytes=n),
                 Buf("ws", "ws", nbytes=need, elem=16)],
                call, {"images": (np.uint8, (npx, 3)), "flags": (np.uint8, (n,))}, check,
                entries=("rf_png_unfilter_ragged_u8",), sync=True, sized=sized)
