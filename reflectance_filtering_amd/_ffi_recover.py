"""ctypes binding of librf_recover_hip.so (include/reflectance_filtering_recover.h): the recover
layer, the boundary losses and the hinge scatter of the rRel* training modes.  The library is
loaded on first use; like _ffi there is NO CPU fallback: a missing library or a missing GPU raises.
"""
import ctypes
import os
import threading

from ._ffi import RFError, RF_OK, RF_E_BADARG, RF_E_UNSUPPORTED, current_stream_ptr, require_gpu  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "librf_recover_hip.so")
RECOVER_VERSION = 100
NORMS = {"Mean": 0, "Max": 1, "Y": 2, "Norm": 3}
PENALTIES = {"L1": 1, "L2": 2}

EXPORTS = ("rf_recover_version", "rf_recover_last_error", "rf_recover_forward_f32",
           "rf_recover_boundary_workspace_bytes", "rf_recover_boundary_plan",
           "rf_recover_boundary_backward_f32", "rf_recover_hinge_scatter_f32")

_lib = None
_lock = threading.Lock()


def load_library():
    """dlopen librf_recover_hip.so and declare the prototypes.  Raises if it was not built."""
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
        vp, ci, sz, ll, fl = (ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_longlong,
                              ctypes.c_float)
        lib.rf_recover_version.argtypes = []
        lib.rf_recover_version.restype = ci
        lib.rf_recover_last_error.argtypes = []
        lib.rf_recover_last_error.restype = ctypes.c_char_p
        lib.rf_recover_forward_f32.argtypes = [vp, vp, ll, vp, ll, ci, vp, vp, vp, vp]
        lib.rf_recover_forward_f32.restype = ci
        lib.rf_recover_boundary_workspace_bytes.argtypes = [ll]
        lib.rf_recover_boundary_workspace_bytes.restype = sz
        lib.rf_recover_boundary_plan.argtypes = [ll, ctypes.POINTER(ci)]
        lib.rf_recover_boundary_plan.restype = ci
        lib.rf_recover_boundary_backward_f32.argtypes = [vp, vp, ll, ci, ci, fl, fl, vp, vp, vp, sz, vp]
        lib.rf_recover_boundary_backward_f32.restype = ci
        lib.rf_recover_hinge_scatter_f32.argtypes = [vp, vp, vp, vp, ll, ll, ci, fl, vp, vp]
        lib.rf_recover_hinge_scatter_f32.restype = ci
        if lib.rf_recover_version() != RECOVER_VERSION:
            raise RFError("%s is version %d, this package binds version %d: build it again"
                          % (LIB_PATH, lib.rf_recover_version(), RECOVER_VERSION))
        _lib = lib
        return lib


def check(rc, what):
    if rc == RF_OK:
        return
    msg = load_library().rf_recover_last_error().decode("utf-8", "replace")
    if rc in (RF_E_BADARG, RF_E_UNSUPPORTED):
        raise ValueError("%s: %s" % (what, msg))
    raise RFError("%s failed (%d): %s" % (what, rc, msg))


def boundary_plan(npixels):
    """(pixels per workgroup pass, workgroups, partial rows) of rf_recover_boundary_backward_f32 for
    this many pixels (host only)."""
    out = (ctypes.c_int * 3)()
    check(load_library().rf_recover_boundary_plan(int(npixels), out), "rf_recover_boundary_plan")
    return int(out[0]), int(out[1]), int(out[2])


def boundary_workspace_bytes(npixels):
    return int(load_library().rf_recover_boundary_workspace_bytes(int(npixels)))
