"""rf_gf_ex_u8 (guided filter with flags; RF_GF_GREY_AS_BGR: a 1-channel guide standing for three
equal channels) at the C ABI: declared, exported, and every refusal made before any HIP call - so
all of this runs without a GPU (host buffers are never dereferenced on the refusal paths)."""
import ctypes
import os
import re
import subprocess

import pytest

from reflectance_filtering_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(name):
    with open(os.path.join(ROOT, "include", "reflectance_filtering.h")) as fh:
        text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    return re.search(r"\b%s\s*\(" % name, text) is not None


def test_rf_gf_ex_u8_is_declared_and_exported(built):
    assert _declared("rf_gf_ex_u8")
    assert "rf_gf_ex_u8" in _ffi.EXPORTS
    with open(os.path.join(ROOT, "include", "reflectance_filtering.h")) as fh:
        assert re.search(r"#define RF_GF_GREY_AS_BGR 1\b", fh.read())
    assert _ffi.GF_GREY_AS_BGR == 1
    out = subprocess.check_output(["nm", "-D", "--defined-only", _ffi.LIB_PATH]).decode()
    assert re.search(r"\bT rf_gf_ex_u8\b", out)
    assert _ffi.load_library().rf_gf_ex_u8 is not None


@pytest.fixture
def bufs(built):
    keep = [ctypes.create_string_buffer(64 * 64 * 3) for _ in range(4)]
    return keep, [ctypes.cast(b, ctypes.c_void_p) for b in keep]


def _ex(lib, p, q, o, ws, gcn, scn, flags, radius=2, iterations=1, n=1, h=4, w=4, wsb=1 << 20):
    return lib.rf_gf_ex_u8(p, q, o, n, h, w, gcn, scn, radius, 3.0, iterations, flags, ws, wsb, None)


def test_grey_flag_refusals(bufs):
    lib = _ffi.load_library()
    _, (p, q, o, ws) = bufs
    G = _ffi.GF_GREY_AS_BGR
    # the flag with a 3-channel guide is a caller error
    assert _ex(lib, p, q, o, ws, 3, 3, G) == _ffi.RF_E_BADARG
    assert b"1-channel" in lib.rf_last_error()
    assert _ex(lib, p, q, o, ws, 3, 1, G) == _ffi.RF_E_BADARG
    # unknown flag bits, with or without the grey flag, whatever the guide
    for flags in (2, 4, 0x100, 0x80000000 - 1, G | 2, -1):
        for gcn in (1, 3):
            assert _ex(lib, p, q, o, ws, gcn, 1, flags) == _ffi.RF_E_BADARG, (flags, gcn)
    assert b"flag" in lib.rf_last_error()
    # a 1-channel guide without the flag: unsupported, as rf_gf_u8 says
    assert _ex(lib, p, q, o, ws, 1, 3, 0) == _ffi.RF_E_UNSUPPORTED
    assert lib.rf_gf_u8(p, q, o, 1, 4, 4, 1, 3, 2, 3.0, 1, ws, 1 << 20, None) == _ffi.RF_E_UNSUPPORTED
    # other guide channel counts stay unsupported with the flag; src must be 1 or 3 channels
    assert _ex(lib, p, q, o, ws, 2, 1, G) == _ffi.RF_E_UNSUPPORTED
    assert _ex(lib, p, q, o, ws, 4, 3, G) == _ffi.RF_E_UNSUPPORTED
    assert _ex(lib, p, q, o, ws, 1, 2, G) == _ffi.RF_E_UNSUPPORTED
    assert _ex(lib, p, q, o, ws, 1, 4, G) == _ffi.RF_E_UNSUPPORTED
    # the rest of rf_gf_u8's checks hold for the grey form too
    assert _ex(lib, None, q, o, ws, 1, 1, G) == _ffi.RF_E_BADARG
    assert _ex(lib, p, q, o, None, 1, 1, G) == _ffi.RF_E_BADARG
    assert _ex(lib, p, q, o, ws, 1, 1, G, iterations=0) == _ffi.RF_E_BADARG
    assert _ex(lib, p, q, o, ws, 1, 1, G, h=0) == _ffi.RF_E_BADARG
    assert _ex(lib, p, q, o, ws, 1, 1, G, radius=5000) == _ffi.RF_E_UNSUPPORTED
    assert _ex(lib, p, q, o, ws, 1, 1, G, radius=-1) == _ffi.RF_E_UNSUPPORTED
    assert _ex(lib, p, q, o, ws, 1, 3, G, h=64, w=64, radius=2, wsb=16) == _ffi.RF_E_WORKSPACE
    assert _ex(lib, p, q, o, ws, 1, 3, G, h=64, w=64, radius=500, wsb=1 << 16) == _ffi.RF_E_WORKSPACE
    # an empty batch is fine
    assert _ex(lib, None, None, None, None, 1, 1, G, n=0) == _ffi.RF_OK


def test_grey_flag_overlap_is_checked_on_one_byte_per_pixel(bufs):
    lib = _ffi.load_library()
    big = ctypes.create_string_buffer(256)
    base = ctypes.cast(big, ctypes.c_void_p).value
    _, (_, _, _, ws) = bufs
    G = _ffi.GF_GREY_AS_BGR
    # 4x4 grey guide = 16 bytes at base, src at base + 64: dst partially over src is refused ...
    assert lib.rf_gf_ex_u8(base, base + 64, base + 70, 1, 4, 4, 1, 1, 2, 3.0, 1, G, ws, 1 << 20,
                           None) == _ffi.RF_E_BADARG
    assert b"overlap" in lib.rf_last_error()
    # ... and so is dst over the guide's 16 bytes
    assert lib.rf_gf_ex_u8(base, base + 64, base + 8, 1, 4, 4, 1, 1, 2, 3.0, 1, G, ws, 1 << 20,
                           None) == _ffi.RF_E_BADARG
    assert b"guide" in lib.rf_last_error()


def test_grey_flag_refused_under_switches_without_a_grey_form(bufs):
    lib = _ffi.load_library()
    _, (p, q, o, ws) = bufs
    for name in ("gf_guide_cache", "gf_exact"):
        with _ffi.debug_options(**{name: 1}):
            assert _ex(lib, p, q, o, ws, 1, 1, _ffi.GF_GREY_AS_BGR) == _ffi.RF_E_UNSUPPORTED, name
            assert name.encode() in lib.rf_last_error()


@pytest.mark.parametrize("args", [
    # (guide, src, dst offsets or None, n, h, w, guide_cn, src_cn, radius, iterations, ws bytes)
    ("p", "q", "o", 1, 4, 4, 1, 3, 2, 1, 1 << 20),      # 1-channel guide
    ("p", "q", "o", 1, 4, 4, 2, 3, 2, 1, 1 << 20),      # 2-channel guide
    ("p", "q", "o", 1, 4, 4, 3, 2, 2, 1, 1 << 20),      # 2-channel src
    ("p", "q", "o", 1, 4, 4, 3, 3, 2, 0, 1 << 20),      # no iteration
    ("p", "q", "o", 1, 4, 4, 3, 3, 5000, 1, 1 << 20),   # radius beyond 4096
    ("p", "q", "o", 1, 4, 4, 3, 3, -3, 1, 1 << 20),     # negative radius
    ("p", "q", "o", 1, 0, 4, 3, 3, 2, 1, 1 << 20),      # empty image
    ("p", "q", "o", -1, 4, 4, 3, 3, 2, 1, 1 << 20),     # negative batch
    (None, "q", "o", 1, 4, 4, 3, 3, 2, 1, 1 << 20),     # NULL guide
    ("p", "q", None, 1, 4, 4, 3, 3, 2, 1, 1 << 20),     # NULL dst
    ("p", "q", "o", 1, 64, 64, 3, 3, 2, 1, 16),         # workspace too small
    ("p", "q", "o", 1, 64, 64, 3, 3, 500, 1, 1 << 16),  # ... for the float route
])
def test_flags_zero_refuses_what_rf_gf_u8_refuses(bufs, args):
    lib = _ffi.load_library()
    _, (p, q, o, ws) = bufs
    ptr = {"p": p, "q": q, "o": o, None: None}
    g, s, d, n, h, w, gcn, scn, radius, its, wsb = args
    a = lib.rf_gf_u8(ptr[g], ptr[s], ptr[d], n, h, w, gcn, scn, radius, 3.0, its, ws, wsb, None)
    b = lib.rf_gf_ex_u8(ptr[g], ptr[s], ptr[d], n, h, w, gcn, scn, radius, 3.0, its, 0, ws, wsb, None)
    assert a == b and a < 0, (a, b)


def test_flags_zero_overlap_refusals_match(bufs):
    lib = _ffi.load_library()
    big = ctypes.create_string_buffer(256)
    base = ctypes.cast(big, ctypes.c_void_p).value
    _, (_, _, _, ws) = bufs
    for g, s, d in ((0, 64, 80), (0, 128, 40), (0, 128, 0)):
        a = lib.rf_gf_u8(base + g, base + s, base + d, 1, 4, 4, 3, 3, 2, 1.0, 1, ws, 1 << 20, None)
        b = lib.rf_gf_ex_u8(base + g, base + s, base + d, 1, 4, 4, 3, 3, 2, 1.0, 1, 0, ws, 1 << 20,
                            None)
        assert a == b == _ffi.RF_E_BADARG, (g, s, d, a, b)


def test_workspace_size_does_not_depend_on_the_guide(built):
    lib = _ffi.load_library()
    for args in ((1, 100, 200, 3, 1), (4, 1080, 1920, 3, 3), (2, 64, 64, 3, 1)):
        for radius in (0, 9, 52, 128, 129, 500):
            n, h, w, _, scn = args
            assert lib.rf_gf_workspace_bytes(n, h, w, 1, scn, radius) == \
                lib.rf_gf_workspace_bytes(n, h, w, 3, scn, radius)
