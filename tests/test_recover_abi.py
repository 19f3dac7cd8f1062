"""The C ABI of librf_recover_hip.so without a device: header, binding and dynamic symbols agree, the code
object is gfx950 only, the library is separate from the other three, every refusal is decided on the host (on
invented pointers), and the plan and workspace queries answer."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "reflectance_filtering_recover.h")


def header_functions():
    with open(HEADER) as fh:
        text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    return set(re.findall(r"\b(rf_recover_\w+)\s*\(", text))


def test_header_exports_and_symbols(built):
    from reflectance_filtering_amd import _ffi, _ffi_augment, _ffi_recover, _ffi_train
    assert header_functions() == set(_ffi_recover.EXPORTS)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _ffi_recover.LIB_PATH]).decode()
    syms = {line.split()[-1] for line in out.splitlines()
            if len(line.split()) == 3 and line.split()[1] == "T" and line.split()[-1].startswith("rf_")}
    assert syms == set(_ffi_recover.EXPORTS)
    others = set(_ffi.EXPORTS) | set(_ffi.DEBUG_EXPORTS) | set(_ffi_train.EXPORTS) | set(_ffi_augment.EXPORTS)
    assert not set(_ffi_recover.EXPORTS) & others
    for path in (_ffi.LIB_PATH, _ffi_train.LIB_PATH, _ffi_augment.LIB_PATH):
        other = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        assert "rf_recover_" not in other and "rfr" not in other, path
    assert "rf_train_" not in out and "rf_augment_" not in out and "rft" not in out and "rfa" not in out
    with open(_ffi_recover.LIB_PATH, "rb") as fh:
        blob = fh.read()
    assert set(re.findall(rb"amdgcn-amd-amdhsa--(gfx[0-9a-f]+)", blob)) == {b"gfx950"}
    with open(HEADER) as fh:
        text = fh.read()
    assert int(re.search(r"#define RF_RECOVER_VERSION (\d+)", text).group(1)) == _ffi_recover.RECOVER_VERSION
    for name, code in _ffi_recover.NORMS.items():
        assert int(re.search(r"#define RF_RECOVER_NORM_%s (\d+)" % name.upper(), text).group(1)) == code
    for name, code in _ffi_recover.PENALTIES.items():
        assert int(re.search(r"#define RF_RECOVER_PENALTY_%s (\d+)" % name, text).group(1)) == code
    # the contract sentences of the train header are kept
    flat = " ".join(text.split()).replace(" * ", " ")
    for sentence in ("DEVICE pointers only", "keeps NO state", "no allocation", "synchronises nothing",
                     "safe to capture", "decided on the host before any device work", "rf_recover_last_error()",
                     "RF_OK 0, RF_E_BADARG -1, RF_E_UNSUPPORTED -2, RF_E_HIP -4", "MUST be pairwise distinct",
                     "NOT checked on the device"):
        assert sentence in flat, sentence


@pytest.fixture()
def lib(built):
    from reflectance_filtering_amd import _ffi_recover
    return _ffi_recover.load_library()


P = ctypes.c_void_p(0x1000)          # invented: every refusal comes before any device work
NAN, INF = float("nan"), float("inf")


def test_version_and_forward_refusals(lib):
    assert lib.rf_recover_version() == 100
    err = (lambda: lib.rf_recover_last_error().decode())
    fwd = lib.rf_recover_forward_f32
    ok = [P, P, 100, P, 10, 0, P, P, P, None]
    for zero in ((2, 0), (4, 0)):                   # P == 0 or K == 0: RF_OK whatever the pointers
        args = [None, None, 100, None, 10, 9, None, None, None, None]
        args[zero[0]] = zero[1]
        assert fwd(*args) == 0
    for i in (0, 1):
        args = list(ok)
        args[i] = None
        assert fwd(*args) == -1 and "NULL pointer" in err(), i
    for i in (2, 4):
        args = list(ok)
        args[i] = -1
        assert fwd(*args) == -1 and "bad size" in err(), i
        args[i] = 1 << 31
        assert fwd(*args) == -2 and "too many pixels" in err(), i
    for norm in (-1, 4):
        args = list(ok)
        args[5] = norm
        assert fwd(*args) == -1 and "unknown norm" in err()
    args = list(ok)
    args[3], args[4] = None, 101                    # the identity list is as long as there are pixels
    assert fwd(*args) == -1 and "without a pixel list" in err()


def test_boundary_refusals(lib):
    err = (lambda: lib.rf_recover_last_error().decode())
    call = lib.rf_recover_boundary_backward_f32
    need = lib.rf_recover_boundary_workspace_bytes(1000)
    ok = [P, P, 1000, 0, 1, 0.1, 0.1, P, P, P, need, None]
    assert call(None, None, 0, 9, 9, NAN, NAN, None, None, None, 0, None) == 0      # P == 0, no loss_out
    for i in (0, 1, 7, 8):
        args = list(ok)
        args[i] = None
        assert call(*args) == -1 and "NULL pointer" in err(), i
    args = list(ok)
    args[2] = -1
    assert call(*args) == -1 and "bad size" in err()
    args[2] = 1 << 31
    assert call(*args) == -2 and "too many pixels" in err()
    for norm in (-1, 4):
        args = list(ok)
        args[3] = norm
        assert call(*args) == -1 and "unknown norm" in err()
    for penalty in (0, 3):
        args = list(ok)
        args[4] = penalty
        assert call(*args) == -1 and "unknown penalty" in err()
    for i in (5, 6):
        for value in (NAN, INF, -INF):
            args = list(ok)
            args[i] = value
            assert call(*args) == -1 and "finite" in err(), (i, value)
    for ws, size in ((None, need), (P, need - 1), (ctypes.c_void_p(0x1008), need), (P, 0)):
        args = list(ok)
        args[9], args[10] = ws, size
        assert call(*args) == -1 and "16-byte aligned" in err()


def test_scatter_refusals(lib):
    err = (lambda: lib.rf_recover_last_error().decode())
    call = lib.rf_recover_hinge_scatter_f32
    ok = [P, P, P, P, 10, 100, 0, 1.0, P, None]
    assert call(None, None, None, None, 0, 100, 9, NAN, None, None) == 0
    assert call(None, None, None, None, 10, 0, 9, NAN, None, None) == 0
    for i in (0, 1, 2, 3, 8):
        args = list(ok)
        args[i] = None
        assert call(*args) == -1 and "NULL pointer" in err(), i
    for i in (4, 5):
        args = list(ok)
        args[i] = -1
        assert call(*args) == -1 and "bad size" in err(), i
        args[i] = 1 << 31
        assert call(*args) == -2 and "too many pixels" in err(), i
    for norm in (-1, 4):
        args = list(ok)
        args[6] = norm
        assert call(*args) == -1 and "unknown norm" in err()
    for value in (NAN, INF):
        args = list(ok)
        args[7] = value
        assert call(*args) == -1 and "finite" in err()


def test_plan_and_workspace_queries(lib):
    from reflectance_filtering_amd import _ffi_recover
    per, most, rows = _ffi_recover.boundary_plan(2 ** 31 - 1)
    assert per == 256 and most == rows and most >= 256
    last = 0
    for npixels in (1, 255, 256, 257, 65, per * most - 1, per * most, per * most + 1, 357914007, 2 ** 31 - 1):
        plan = _ffi_recover.boundary_plan(npixels)
        passes = (npixels + per - 1) // per
        assert plan == (per, min(passes, most), min(passes, most)), npixels
        size = _ffi_recover.boundary_workspace_bytes(npixels)
        assert size >= 16 * plan[2] and size % 16 == 0 and (size >= last or npixels == 65)
        last = size
    assert _ffi_recover.boundary_workspace_bytes(0) == 0
    assert _ffi_recover.boundary_workspace_bytes(-1) == 0
    assert _ffi_recover.boundary_workspace_bytes(2 ** 31) == 0
    assert lib.rf_recover_boundary_plan(5, None) == -1
    with pytest.raises(ValueError, match="bad size"):
        _ffi_recover.boundary_plan(-1)
    with pytest.raises(ValueError, match="too many pixels"):
        _ffi_recover.boundary_plan(2 ** 31)


def test_refusals_under_the_host_sanitizers(tmp_path):
    """tests/recover_refusals_main.cpp: a program of its own (no Python, no preloaded runtime) built from the
    library's three sources with AddressSanitizer and UBSan on the HOST code, driving every refusal; it never
    reaches the device."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "reflectance_filtering_amd", "csrc", "recover")
    exe = str(tmp_path / "recover_refusals")
    cmd = [hipcc, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-gpu-rdc",
           "-I" + os.path.join(ROOT, "include"), "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-omit-frame-pointer"]
    cmd += [os.path.join(src, name) for name in ("rf_recover_api.hip", "rf_recover_points.hip",
                                                 "rf_recover_boundary.hip")]
    cmd += ["-x", "hip", os.path.join(ROOT, "tests", "recover_refusals_main.cpp"), "-o", exe]
    subprocess.check_call(cmd)
    symbols = subprocess.check_output(["nm", exe]).decode()
    assert "__asan_init" in symbols and "__ubsan_handle" in symbols
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert run.returncode == 0 and run.stdout.decode().strip().endswith("0 failures"), run.stdout.decode()
