"""ctypes binding of librf_hip.so -- the only way the Python host code reaches the GPU.

The C ABI is declared in include/reflectance_filtering.h.  PyTorch is used purely as the
device-buffer container (allocation, H2D/D2H copies, the current HIP stream); no torch op
computes anything on the path.  There is NO CPU fallback: if the library is missing, cannot
be loaded, or no GPU is visible, every entry point raises.
"""
import ctypes
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
# The one library this package loads.  (A/B timing of two builds: tools/gf_c5_exp.py --lib PATH sets
# this attribute before the first call - announced on stderr, version checked; no environment
# variable redirects the shipped loader.)
LIB_PATH = os.path.join(_HERE, "librf_hip.so")

RF_OK, RF_E_BADARG, RF_E_UNSUPPORTED, RF_E_WORKSPACE, RF_E_HIP = 0, -1, -2, -3, -4
BORDER_CONSTANT, BORDER_REPLICATE, BORDER_REFLECT, BORDER_WRAP, BORDER_REFLECT_101 = range(5)
BORDER_DEFAULT = BORDER_REFLECT_101
JBF_TRUE_DIVISION = 1
JBF_FORCE_GENERIC = 2
JBF_GREY_AS_BGR = 4
GF_GREY_AS_BGR = 1          # rf_gf_ex_u8: a 1-channel guide stands for three equal channels
PNG_GREY_AS_RGB = 1         # rf_png_deflate_ragged_u8: a 1-channel image is written as three equal samples
PNG_FLAG_GREY, PNG_FLAG_BAD_FILTER = 1, 2   # image_flags of rf_png_unfilter_ragged_u8
CNN_NPARAMS = 4513
CNN_NPACKED = 4673          # RF_CNN_NPACKED: floats of rf_cnn_pack_weights' output
CNN_NCHW_RGB, CNN_NHWC_BGR = 0, 1           # layouts of rf_cnn_reflectance_f32 / _packed_f32
CNN_LAYOUTS = {"nchw_rgb": CNN_NCHW_RGB, "nhwc_bgr": CNN_NHWC_BGR}

EXPORTS = ("rf_version", "rf_last_error", "rf_shutdown", "rf_jbf_u8", "rf_gf_workspace_bytes",
           "rf_gf_u8", "rf_gf_ex_u8", "rf_cnn_reflectance_u8", "rf_cnn_pack_weights",
           "rf_cnn_reflectance_packed_u8", "rf_colorize_workspace_bytes",
           "rf_colorize_srgb_u8", "rf_whdr_f32", "rf_jbf_f32_workspace_bytes", "rf_jbf_f32",
           "rf_gf_f32_workspace_bytes", "rf_gf_f32", "rf_jbf_points_workspace_bytes",
           "rf_jbf_points_u8", "rf_jbf_points_ragged_workspace_bytes", "rf_jbf_points_ragged_u8",
           "rf_whdr_points_u8", "rf_jbf_ragged_workspace_bytes", "rf_jbf_ragged_u8",
           "rf_colorize_ragged_workspace_bytes", "rf_colorize_ragged_srgb_u8",
           "rf_gf_ragged_workspace_bytes", "rf_gf_ragged_u8", "rf_png_stream_bound",
           "rf_png_workspace_bytes", "rf_png_deflate_ragged_u8",
           "rf_png_unfilter_workspace_bytes", "rf_png_unfilter_ragged_u8",
           "rf_colorize_ragged_r8_srgb_u8", "rf_cnn_reflectance_f32",
           "rf_cnn_reflectance_packed_f32", "rf_jbf_release_scratch")

# include/reflectance_filtering_debug.h: test / benchmark switches, not part of the boundary
DEBUG_EXPORTS = ("rf_debug_option", "rf_debug_clock_probe", "rf_debug_build_info",
                 "rf_debug_jbf_points_plan", "rf_debug_jbf_ragged_plan",
                 "rf_debug_jbf_ragged_slab_plan", "rf_debug_jbf_two_wg_plan",
                 "rf_debug_jbf_two_wg_calls", "rf_debug_jbf_tile_flags",
                 "rf_debug_colorize_ragged_plan",
                 "rf_debug_gf_ragged_plan", "rf_debug_gf_launch_chunk", "rf_debug_png_plan")
# switches that leave work out (wrong results, timing experiments only); all others keep the bytes
RESULT_CHANGING_OPTIONS = ("jbf_stage_only", "gf_exp_skip")

_lib = None
_lock = threading.Lock()


class RFError(RuntimeError):
    """A librf_hip.so entry point returned a negative code."""


def load_library():
    """dlopen librf_hip.so and declare the prototypes.  Raises if it was not built."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        # torch bundles its own libamdhip64 / libhsa-runtime64.  The device pointers and the
        # stream we are handed belong to THAT runtime instance, so it has to be in the process
        # before librf_hip.so resolves its libamdhip64.so.7 dependency (same SONAME -> shared).
        import torch  # noqa: F401
        if not os.path.exists(LIB_PATH):
            raise RFError("%s not found: build it with `python -c 'import __graft_entry__ as g; "
                          "g.build()'` or `make -C reflectance_filtering_amd/csrc` "
                          "(there is no CPU fallback)" % LIB_PATH)
        lib = ctypes.CDLL(LIB_PATH)
        vp, ci, cd, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_size_t
        lib.rf_version.argtypes = []
        lib.rf_version.restype = ci
        lib.rf_last_error.argtypes = []
        lib.rf_last_error.restype = ctypes.c_char_p
        lib.rf_shutdown.argtypes = []
        lib.rf_shutdown.restype = ci
        lib.rf_jbf_release_scratch.argtypes = []
        lib.rf_jbf_release_scratch.restype = ci
        lib.rf_jbf_u8.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, ci, cd, cd, ci, ci, vp]
        lib.rf_jbf_u8.restype = ci
        lib.rf_gf_workspace_bytes.argtypes = [ci, ci, ci, ci, ci, ci]
        lib.rf_gf_workspace_bytes.restype = sz
        lib.rf_gf_u8.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, ci, cd, ci, vp, sz, vp]
        lib.rf_gf_u8.restype = ci
        lib.rf_gf_ex_u8.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, ci, cd, ci, ci, vp, sz, vp]
        lib.rf_gf_ex_u8.restype = ci
        lib.rf_gf_ragged_workspace_bytes.argtypes = [ci, vp, vp, ci, ci, ci, ci]
        lib.rf_gf_ragged_workspace_bytes.restype = sz
        lib.rf_gf_ragged_u8.argtypes = [vp, vp, vp, ci, vp, vp, ci, ci, ci, cd, ci, ci, vp, sz, vp]
        lib.rf_gf_ragged_u8.restype = ci
        lib.rf_cnn_reflectance_u8.argtypes = [vp, vp, vp, ci, ci, ci, vp, vp, vp]
        lib.rf_cnn_reflectance_u8.restype = ci
        lib.rf_cnn_pack_weights.argtypes = [vp, vp, vp]
        lib.rf_cnn_pack_weights.restype = ci
        lib.rf_cnn_reflectance_packed_u8.argtypes = [vp, vp, vp, ci, ci, ci, vp, vp, vp]
        lib.rf_cnn_reflectance_packed_u8.restype = ci
        lib.rf_cnn_reflectance_f32.argtypes = [vp, vp, vp, ci, ci, ci, ci, vp, vp]
        lib.rf_cnn_reflectance_f32.restype = ci
        lib.rf_cnn_reflectance_packed_f32.argtypes = [vp, vp, vp, ci, ci, ci, ci, vp, vp]
        lib.rf_cnn_reflectance_packed_f32.restype = ci
        u64 = ctypes.c_ulonglong
        lib.rf_colorize_workspace_bytes.argtypes = [ci]
        lib.rf_colorize_workspace_bytes.restype = sz
        lib.rf_colorize_srgb_u8.argtypes = [vp, vp, vp, vp, ci, ci, ci, u64, u64, vp, vp, sz, vp]
        lib.rf_colorize_srgb_u8.restype = ci
        lib.rf_colorize_ragged_workspace_bytes.argtypes = [ci, vp, vp]
        lib.rf_colorize_ragged_workspace_bytes.restype = sz
        lib.rf_colorize_ragged_srgb_u8.argtypes = [vp, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, sz, vp]
        lib.rf_colorize_ragged_srgb_u8.restype = ci
        lib.rf_colorize_ragged_r8_srgb_u8.argtypes = [vp, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, sz, vp]
        lib.rf_colorize_ragged_r8_srgb_u8.restype = ci
        lib.rf_jbf_f32_workspace_bytes.argtypes = [ci, ci]
        lib.rf_jbf_f32_workspace_bytes.restype = sz
        lib.rf_jbf_f32.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, ci, cd, cd, ci, vp, sz, vp]
        lib.rf_jbf_f32.restype = ci
        lib.rf_gf_f32_workspace_bytes.argtypes = [ci, ci, ci, ci, ci, ci]
        lib.rf_gf_f32_workspace_bytes.restype = sz
        lib.rf_gf_f32.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, ci, cd, ci, vp, sz, vp]
        lib.rf_gf_f32.restype = ci
        lib.rf_whdr_f32.argtypes = [vp, ci, ci, ci, ci, vp, vp, vp, cd, vp, vp]
        lib.rf_whdr_f32.restype = ci
        lib.rf_jbf_points_workspace_bytes.argtypes = [ci, vp, ci, ci, ci]
        lib.rf_jbf_points_workspace_bytes.restype = sz
        lib.rf_jbf_points_u8.argtypes = [vp, vp, ci, ci, ci, ci, ci, vp, vp, ci, ci, vp, vp, ci, ci,
                                         ci, vp, vp, sz, vp]
        lib.rf_jbf_points_u8.restype = ci
        lib.rf_jbf_points_ragged_workspace_bytes.argtypes = [ci, ci, vp, ci, ci, ci]
        lib.rf_jbf_points_ragged_workspace_bytes.restype = sz
        lib.rf_jbf_points_ragged_u8.argtypes = [vp, vp, ci, vp, vp, ci, ci, vp, vp, ci, ci, vp, vp, ci,
                                                ci, ci, vp, vp, sz, vp]
        lib.rf_jbf_points_ragged_u8.restype = ci
        lib.rf_jbf_ragged_workspace_bytes.argtypes = [ci, vp, vp, ci, ci, ci, cd, ci]
        lib.rf_jbf_ragged_workspace_bytes.restype = sz
        lib.rf_jbf_ragged_u8.argtypes = [vp, vp, vp, ci, vp, vp, ci, ci, ci, cd, cd, ci, ci, vp, sz,
                                         vp]
        lib.rf_jbf_ragged_u8.restype = ci
        lib.rf_whdr_points_u8.argtypes = [vp, ci, ctypes.c_longlong, ci, ci, vp, vp, vp, vp, cd, vp,
                                          vp]
        lib.rf_whdr_points_u8.restype = ci
        lib.rf_png_stream_bound.argtypes = [ci, vp, vp, ci, ci]
        lib.rf_png_stream_bound.restype = sz
        lib.rf_png_workspace_bytes.argtypes = [ci, vp, vp, ci, ci]
        lib.rf_png_workspace_bytes.restype = sz
        lib.rf_png_deflate_ragged_u8.argtypes = [vp, ci, vp, vp, ci, ci, vp, sz, vp, vp, sz, vp]
        lib.rf_png_deflate_ragged_u8.restype = ci
        lib.rf_png_unfilter_workspace_bytes.argtypes = [ci, vp, vp, vp]
        lib.rf_png_unfilter_workspace_bytes.restype = sz
        lib.rf_png_unfilter_ragged_u8.argtypes = [vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, sz, vp]
        lib.rf_png_unfilter_ragged_u8.restype = ci
        lib.rf_debug_png_plan.argtypes = [ci, vp, vp, ci, ci, vp, ci]
        lib.rf_debug_png_plan.restype = ci
        lib.rf_debug_option.argtypes = [ctypes.c_char_p, ci]
        lib.rf_debug_option.restype = ci
        lib.rf_debug_clock_probe.argtypes = [vp, ci, vp]
        lib.rf_debug_clock_probe.restype = ci
        lib.rf_debug_build_info.argtypes = []
        lib.rf_debug_build_info.restype = ctypes.c_char_p
        lib.rf_debug_jbf_points_plan.argtypes = [ci, vp, ci, ci, ci, ci, vp, ci]
        lib.rf_debug_jbf_points_plan.restype = ci
        lib.rf_debug_jbf_ragged_plan.argtypes = [ci, vp, vp, ci, ci, ci, cd, cd, ci, vp, ci]
        lib.rf_debug_jbf_ragged_plan.restype = ci
        lib.rf_debug_jbf_ragged_slab_plan.argtypes = [ci, vp, vp, ci, ci, ci, cd, cd, ci, vp, ci]
        lib.rf_debug_jbf_ragged_slab_plan.restype = ci
        lib.rf_debug_jbf_two_wg_plan.argtypes = [ci, ci, ci, ci, ci, ci, cd, cd, ci, vp]
        lib.rf_debug_jbf_two_wg_plan.restype = ci
        lib.rf_debug_jbf_two_wg_calls.argtypes = []
        lib.rf_debug_jbf_two_wg_calls.restype = ci
        lib.rf_debug_jbf_tile_flags.argtypes = [vp, vp, ci]
        lib.rf_debug_jbf_tile_flags.restype = ci
        lib.rf_debug_colorize_ragged_plan.argtypes = [ci, vp, vp, vp, ci]
        lib.rf_debug_colorize_ragged_plan.restype = ci
        lib.rf_debug_gf_ragged_plan.argtypes = [ci, vp, vp, ci, ci, ci, ci, vp, ci]
        lib.rf_debug_gf_ragged_plan.restype = ci
        lib.rf_debug_gf_launch_chunk.argtypes = [ci, ci, ci, ci, ci]
        lib.rf_debug_gf_launch_chunk.restype = ci
        # RF_DEBUG_OPTIONS="name=value,...": preset the test / benchmark switches of
        # include/reflectance_filtering_debug.h for a whole process (timing experiments only).
        # Every preset is announced on stderr - loudly for the switches that change results.
        import sys
        for item in filter(None, os.environ.get("RF_DEBUG_OPTIONS", "").split(",")):
            name, _, value = item.partition("=")
            name = name.strip()
            try:
                number = int(value or 1)
            except ValueError:
                raise RFError("RF_DEBUG_OPTIONS: %r is not an integer (option %r)" % (value, name))
            if lib.rf_debug_option(name.encode(), number) < 0:
                raise RFError("RF_DEBUG_OPTIONS: unknown debug option %r" % name)
            if name in RESULT_CHANGING_OPTIONS and number:
                sys.stderr.write("reflectance_filtering_amd: WARNING: RF_DEBUG_OPTIONS sets %s=%d, a "
                                 "TIMING-ONLY switch - results of this process are WRONG\n"
                                 % (name, number))
            else:
                sys.stderr.write("reflectance_filtering_amd: RF_DEBUG_OPTIONS sets %s=%d\n"
                                 % (name, number))
        _lib = lib
        return lib


class debug_options:
    """Context manager around rf_debug_option (include/reflectance_filtering_debug.h):
    ``with debug_options(gf_two_kernel=1): ...`` selects the alternative kernels that tests and
    timing tools compare with the default ones, and restores the previous values on exit."""

    def __init__(self, **opts):
        self.opts = opts
        self.prev = {}

    def __enter__(self):
        lib = load_library()
        for name, value in self.opts.items():
            old = lib.rf_debug_option(name.encode(), int(value))
            if old < 0:
                raise ValueError("unknown debug option %r" % name)
            self.prev[name] = old
        return self

    def __exit__(self, *exc):
        lib = load_library()
        for name, old in self.prev.items():
            lib.rf_debug_option(name.encode(), old)
        return False


def check(rc, what):
    if rc == RF_OK:
        return
    msg = load_library().rf_last_error().decode("utf-8", "replace")
    if rc in (RF_E_BADARG, RF_E_UNSUPPORTED):
        raise ValueError("%s: %s" % (what, msg))
    raise RFError("%s failed (%d): %s" % (what, rc, msg))


def jbf_points_plan(sigma_space, d, joint_cn, flags, total_points):
    """The launch plan of rf_jbf_points_u8 for these arguments (rf_debug_jbf_points_plan, host
    only): one (radius, nsets, ppw, waves) tuple per chunk, in launch order."""
    import numpy as np
    lib = load_library()
    ss = np.ascontiguousarray(sigma_space, dtype=np.float64).ravel()
    args = (ss.shape[0], ss.ctypes.data, int(d), int(joint_cn), int(flags), int(total_points))
    nchunks = lib.rf_debug_jbf_points_plan(*(args + (None, 0)))
    if nchunks < 0:
        check(nchunks, "rf_debug_jbf_points_plan")
    out = np.zeros((max(nchunks, 1), 4), dtype=np.int32)
    if lib.rf_debug_jbf_points_plan(*(args + (out.ctypes.data, nchunks))) != nchunks:
        raise RFError("rf_debug_jbf_points_plan: the chunk count changed between two calls")
    return [tuple(int(v) for v in row) for row in out[:nchunks]]


def jbf_ragged_plan(sizes, joint_cn, src_cn, d, sigma_color, sigma_space, flags=0):
    """The launches of rf_jbf_ragged_u8 for images of these sizes ([n,2] (h, w))
    (rf_debug_jbf_ragged_plan, host only): one (tile rows, tile cols, pitch, tiles) tuple per
    launch, or None where the entry falls back to one rf_jbf_u8 call per image."""
    import numpy as np
    lib = load_library()
    sizes = np.asarray(sizes, dtype=np.int64).reshape(-1, 2)
    hs = np.ascontiguousarray(sizes[:, 0], dtype=np.int32)
    ws = np.ascontiguousarray(sizes[:, 1], dtype=np.int32)
    out = np.zeros((4, 4), dtype=np.int32)
    rc = lib.rf_debug_jbf_ragged_plan(sizes.shape[0], hs.ctypes.data, ws.ctypes.data, int(joint_cn),
                                      int(src_cn), int(d), float(sigma_color), float(sigma_space),
                                      int(flags), out.ctypes.data, 4)
    if rc == -1:
        # -1 is the fall-back and RF_E_BADARG alike: a workspace size of 0 (for n > 0) says refused
        if sizes.shape[0] == 0 or lib.rf_jbf_ragged_workspace_bytes(
                sizes.shape[0], hs.ctypes.data, ws.ctypes.data, int(joint_cn), int(src_cn), int(d),
                float(sigma_space), int(flags)) > 0:
            return None
        lib.rf_debug_jbf_ragged_plan(sizes.shape[0], hs.ctypes.data, ws.ctypes.data, int(joint_cn),
                                     int(src_cn), int(d), float(sigma_color), float(sigma_space),
                                     int(flags), out.ctypes.data, 4)     # (its message again)
    if rc < 0:
        check(rc, "rf_debug_jbf_ragged_plan")
    return [tuple(int(v) for v in row) for row in out[:rc]]


def jbf_ragged_slab_plan(sizes, joint_cn, src_cn, d, sigma_color, sigma_space, flags=0):
    """The slab launch of rf_jbf_ragged_u8 (radius 53..468) for images of these sizes ([n,2] (h, w))
    (rf_debug_jbf_ragged_slab_plan, host only): the tuple (pitch, LUT replicas, crows_g, slab_g,
    crows_c, slab_c, tiles), or None where the entry does not run that launch (the tile classes of
    jbf_ragged_plan, or one rf_jbf_u8 call per image)."""
    import numpy as np
    lib = load_library()
    sizes = np.asarray(sizes, dtype=np.int64).reshape(-1, 2)
    hs = np.ascontiguousarray(sizes[:, 0], dtype=np.int32)
    ws = np.ascontiguousarray(sizes[:, 1], dtype=np.int32)
    out = np.zeros(7, dtype=np.int32)
    args = (sizes.shape[0], hs.ctypes.data, ws.ctypes.data, int(joint_cn), int(src_cn), int(d),
            float(sigma_color), float(sigma_space), int(flags), out.ctypes.data, 1)
    rc = lib.rf_debug_jbf_ragged_slab_plan(*args)
    if rc == -1:
        # -1 is "not this launch" and RF_E_BADARG alike: a workspace size of 0 (for n > 0) says refused
        if sizes.shape[0] == 0 or lib.rf_jbf_ragged_workspace_bytes(*(args[:6] + (args[7], args[8]))) > 0:
            return None
        lib.rf_debug_jbf_ragged_slab_plan(*args)                         # (its message again)
    if rc < 0:
        check(rc, "rf_debug_jbf_ragged_slab_plan")
    return tuple(int(v) for v in out)


def jbf_two_wg_plan(n, h, w, joint_cn, src_cn, d, sigma_color, sigma_space, flags=0):
    """The route of rf_jbf_u8's grey tiles for n images of h x w (rf_debug_jbf_two_wg_plan, host
    only): (tile rows resident in the LDS, tiles of the launch, bytes of the tile-flag buffer) on the
    two-workgroups-per-CU route, None off it."""
    import numpy as np
    lib = load_library()
    out = np.zeros(4, dtype=np.int32)
    rc = lib.rf_debug_jbf_two_wg_plan(int(n), int(h), int(w), int(joint_cn), int(src_cn), int(d),
                                      float(sigma_color), float(sigma_space), int(flags),
                                      out.ctypes.data)
    if rc < 0:
        check(rc, "rf_debug_jbf_two_wg_plan")
    return tuple(int(v) for v in out[1:]) if rc == 1 else None


def jbf_tile_flags(stream, tiles):
    """The first `tiles` tile bytes of the two-per-CU route as the last rf_jbf_u8 call on `stream` (a
    pointer, as current_stream_ptr gives it) left them (rf_debug_jbf_tile_flags: synchronises the
    stream): a uint8 array, bit 0 = the tile's src is not grey, bit 1 = its joint is."""
    import numpy as np
    lib = load_library()
    out = np.zeros(int(tiles), dtype=np.uint8)
    rc = lib.rf_debug_jbf_tile_flags(stream, out.ctypes.data, int(tiles))
    if rc < 0:
        check(rc, "rf_debug_jbf_tile_flags")
    if rc != int(tiles):
        raise RFError("rf_debug_jbf_tile_flags: %d bytes where %d tiles were asked for" % (rc, tiles))
    return out


def colorize_ragged_plan(sizes):
    """The launch plan of rf_colorize_ragged_srgb_u8 for images of these sizes ([n,2] (h, w))
    (rf_debug_colorize_ragged_plan, host only): (chunk_px, workgroups, [first workgroup of each
    image])."""
    import numpy as np
    lib = load_library()
    sizes = np.asarray(sizes, dtype=np.int64).reshape(-1, 2)
    n = sizes.shape[0]
    hs = np.ascontiguousarray(sizes[:, 0], dtype=np.int32)
    ws = np.ascontiguousarray(sizes[:, 1], dtype=np.int32)
    out = np.zeros(n + 2, dtype=np.int32)
    rc = lib.rf_debug_colorize_ragged_plan(n, hs.ctypes.data, ws.ctypes.data, out.ctypes.data, n + 2)
    if rc < 0:
        check(rc, "rf_debug_colorize_ragged_plan")
    return int(out[0]), int(out[1]), [int(v) for v in out[2:]]


def gf_ragged_plan(sizes, guide_cn, src_cn, radius, flags=0):
    """The route of rf_gf_ragged_u8 for images of these sizes ([n,2] (h, w)) (rf_debug_gf_ragged_plan,
    host only): None where the entry calls rf_gf_ex_u8 once per image, else the dict {launches (per
    pass), stage1, rowstate, colwalk (the three grids), hl, out_w (the stage-1 strip)}."""
    import numpy as np
    lib = load_library()
    sizes = np.asarray(sizes, dtype=np.int64).reshape(-1, 2)
    hs = np.ascontiguousarray(sizes[:, 0], dtype=np.int32)
    ws = np.ascontiguousarray(sizes[:, 1], dtype=np.int32)
    out = np.zeros(6, dtype=np.int32)
    rc = lib.rf_debug_gf_ragged_plan(sizes.shape[0], hs.ctypes.data, ws.ctypes.data, int(guide_cn),
                                     int(src_cn), int(radius), int(flags), out.ctypes.data, 6)
    if rc < 0:
        check(rc, "rf_debug_gf_ragged_plan")
    if rc == 0:
        return None
    return dict(zip(("launches", "stage1", "rowstate", "colwalk", "hl", "out_w"),
                    (int(v) for v in out)))


def png_plan(sizes, cn_in=1, flags=0):
    """The plan of rf_png_deflate_ragged_u8 for images of these sizes ([n,2] (h, w)) (rf_debug_png_plan,
    host only): (chunk length in raw bytes, chunks of all images, [chunks of each image])."""
    import numpy as np
    lib = load_library()
    sizes = np.asarray(sizes, dtype=np.int64).reshape(-1, 2)
    n = sizes.shape[0]
    hs = np.ascontiguousarray(sizes[:, 0], dtype=np.int32)
    ws = np.ascontiguousarray(sizes[:, 1], dtype=np.int32)
    out = np.zeros(n + 2, dtype=np.int32)
    rc = lib.rf_debug_png_plan(n, hs.ctypes.data, ws.ctypes.data, int(cn_in), int(flags),
                               out.ctypes.data, n + 2)
    if rc < 0:
        check(rc, "rf_debug_png_plan")
    return int(out[0]), int(out[1]), [int(v) for v in out[2:]]


def require_gpu():
    """torch with a visible HIP device, or a loud failure (never a silent CPU path)."""
    import torch
    if not torch.cuda.is_available():
        raise RFError("no HIP device visible: reflectance_filtering_amd runs on MI355X only "
                      "and has no CPU fallback")
    return torch


def current_stream_ptr(torch):
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
