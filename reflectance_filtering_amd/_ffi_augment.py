"""ctypes binding of librf_augment_hip.so (include/reflectance_filtering_augment.h): the transitive
hull of judgement graphs.  The library is loaded on first use; like _ffi there is NO CPU fallback:
a missing library or a missing GPU raises.
"""
import ctypes
import os
import threading

from ._ffi import RFError, RF_OK, RF_E_BADARG, RF_E_UNSUPPORTED, current_stream_ptr, require_gpu  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "librf_augment_hip.so")
AUGMENT_VERSION = 100
MAX_NODES = 2560

EXPORTS = ("rf_augment_version", "rf_augment_last_error", "rf_augment_hull_workspace_bytes",
           "rf_augment_hull_f64")

_lib = None
_lock = threading.Lock()


def load_library():
    """dlopen librf_augment_hip.so and declare the prototypes.  Raises if it was not built."""
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
        vp, ci, sz, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_longlong
        lib.rf_augment_version.argtypes = []
        lib.rf_augment_version.restype = ci
        lib.rf_augment_last_error.argtypes = []
        lib.rf_augment_last_error.restype = ctypes.c_char_p
        lib.rf_augment_hull_workspace_bytes.argtypes = [ll]
        lib.rf_augment_hull_workspace_bytes.restype = sz
        lib.rf_augment_hull_f64.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, ll, ll, ll, ll,
                                            vp, vp, vp, vp, sz, vp]
        lib.rf_augment_hull_f64.restype = ci
        if lib.rf_augment_version() != AUGMENT_VERSION:
            raise RFError("%s is version %d, this package binds version %d: build it again"
                          % (LIB_PATH, lib.rf_augment_version(), AUGMENT_VERSION))
        _lib = lib
        return lib


def check(rc, what):
    if rc == RF_OK:
        return
    msg = load_library().rf_augment_last_error().decode("utf-8", "replace")
    if rc in (RF_E_BADARG, RF_E_UNSUPPORTED):
        raise ValueError("%s: %s" % (what, msg))
    raise RFError("%s failed (%d): %s" % (what, rc, msg))


def hull_workspace_bytes(total_matrix):
    return int(load_library().rf_augment_hull_workspace_bytes(int(total_matrix)))
