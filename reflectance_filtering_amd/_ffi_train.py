"""ctypes binding of librf_train_hip.so (include/reflectance_filtering_train.h): the WHDR hinge loss at
judgement points and the CNN's backward pass.  The library is loaded on first use; like _ffi there
is NO CPU fallback: a missing library or a missing GPU raises.
"""
import ctypes
import os
import threading

from ._ffi import RFError, RF_OK, RF_E_BADARG, RF_E_UNSUPPORTED, current_stream_ptr, require_gpu  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "librf_train_hip.so")
TRAIN_VERSION = 100
CNN_NPARAMS = 4513

EXPORTS = ("rf_train_version", "rf_train_last_error", "rf_train_whdr_hinge_points_f32",
           "rf_train_cnn_points_workspace_bytes", "rf_train_cnn_points_plan",
           "rf_train_cnn_points_backward_f32")

_lib = None
_lock = threading.Lock()


def load_library():
    """dlopen librf_train_hip.so and declare the prototypes.  Raises if it was not built."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        import torch  # noqa: F401  (its HIP runtime has to be in the process first: see _ffi)
        if not os.path.exists(LIB_PATH):
            raise RFError("%s not found: build it with `python -c 'import __graft_entry__ as g; "
                          "g.build()'` or `make -C reflectance_filtering_amd/csrc` "
                          "(there is no CPU fallback)" % LIB_PATH)
        lib = ctypes.CDLL(LIB_PATH)
        vp, ci, cd, sz, ll = (ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_size_t,
                              ctypes.c_longlong)
        lib.rf_train_version.argtypes = []
        lib.rf_train_version.restype = ci
        lib.rf_train_last_error.argtypes = []
        lib.rf_train_last_error.restype = ctypes.c_char_p
        lib.rf_train_whdr_hinge_points_f32.argtypes = [vp, vp, vp, vp, vp, vp, vp, ci, cd, cd, vp, vp,
                                                       vp]
        lib.rf_train_whdr_hinge_points_f32.restype = ci
        lib.rf_train_cnn_points_workspace_bytes.argtypes = [ll]
        lib.rf_train_cnn_points_workspace_bytes.restype = sz
        lib.rf_train_cnn_points_plan.argtypes = [ll, vp]
        lib.rf_train_cnn_points_plan.restype = ci
        lib.rf_train_cnn_points_backward_f32.argtypes = [vp, vp, vp, ll, vp, vp, sz, vp]
        lib.rf_train_cnn_points_backward_f32.restype = ci
        if lib.rf_train_version() != TRAIN_VERSION:
            raise RFError("%s is version %d, this package binds version %d: build it again"
                          % (LIB_PATH, lib.rf_train_version(), TRAIN_VERSION))
        _lib = lib
        return lib


def check(rc, what):
    if rc == RF_OK:
        return
    msg = load_library().rf_train_last_error().decode("utf-8", "replace")
    if rc in (RF_E_BADARG, RF_E_UNSUPPORTED):
        raise ValueError("%s: %s" % (what, msg))
    raise RFError("%s failed (%d): %s" % (what, rc, msg))


def cnn_points_plan(npoints):
    """(points per workgroup pass, workgroups, partial-gradient rows) of
    rf_train_cnn_points_backward_f32 for this many points (host only)."""
    out = (ctypes.c_int * 3)()
    check(load_library().rf_train_cnn_points_plan(int(npoints), out), "rf_train_cnn_points_plan")
    return int(out[0]), int(out[1]), int(out[2])


def cnn_points_workspace_bytes(npoints):
    return int(load_library().rf_train_cnn_points_workspace_bytes(int(npoints)))
