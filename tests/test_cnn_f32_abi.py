"""rf_cnn_reflectance_f32 / rf_cnn_reflectance_packed_f32 (the network on float32 linear images, i.e.
any Caffe blob) at the C ABI and in the Python routing above it: declared, exported, every refusal made
before any device work (made-up pointers are never dereferenced on those paths), and ReflectanceNet /
get_reflectance_batch choosing the byte or the float entry - with `ops` stubbed, so all of this runs
without a GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from reflectance_filtering_amd import _ffi
from reflectance_filtering_amd import decompose_with_trained_CNN as dc
from reflectance_filtering_amd import image_utils as iu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rf_cnn_reflectance_f32", "rf_cnn_reflectance_packed_f32")


def _header():
    with open(os.path.join(ROOT, "include", "reflectance_filtering.h")) as fh:
        return fh.read()


def test_symbols_and_prototypes(built):
    text = _header()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"#define RF_CNN_NCHW_RGB 0\b", text) and re.search(r"#define RF_CNN_NHWC_BGR 1\b", text)
    assert (_ffi.CNN_NCHW_RGB, _ffi.CNN_NHWC_BGR) == (0, 1)
    assert _ffi.CNN_LAYOUTS == {"nchw_rgb": 0, "nhwc_bgr": 1}
    lib = _ffi.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _ffi.LIB_PATH]).decode()
    vp, ci = ctypes.c_void_p, ctypes.c_int
    for name in ENTRIES:
        assert re.search(r"\bint %s\s*\(const float \*x, float \*r_out, uint8_t \*r_u8_out" % name, code)
        assert name in _ffi.EXPORTS
        assert re.search(r"\bT %s\b" % name, out), name
        fn = getattr(lib, name)
        assert fn.argtypes == [vp, vp, vp, ci, ci, ci, ci, vp, vp] and fn.restype is ci


@pytest.fixture
def ptrs(built):
    """x (room for 4x4x3 floats and more), two outputs and weights: host memory that no refusal reads."""
    keep = [ctypes.create_string_buffer(1024) for _ in range(4)]
    return keep, [ctypes.cast(b, ctypes.c_void_p) for b in keep]


@pytest.mark.parametrize("name", ENTRIES)
def test_refusals_are_decided_before_any_device_work(ptrs, name):
    lib = _ffi.load_library()
    fn = getattr(lib, name)
    _, (x, r, r8, wts) = ptrs
    E = _ffi.RF_E_BADARG
    for layout in (_ffi.CNN_NCHW_RGB, _ffi.CNN_NHWC_BGR):
        assert fn(None, r, r8, 1, 4, 4, layout, wts, None) == E          # NULL x
        assert b"NULL" in lib.rf_last_error() and name.encode() in lib.rf_last_error()
        assert fn(x, r, r8, 1, 4, 4, layout, None, None) == E            # NULL weights
        assert fn(x, None, None, 1, 4, 4, layout, wts, None) == E        # both outputs NULL
        assert fn(x, r, r8, -1, 4, 4, layout, wts, None) == E
        assert fn(x, r, r8, 1, 0, 4, layout, wts, None) == E
        assert fn(x, r, r8, 1, 4, 0, layout, wts, None) == E
        assert b"size" in lib.rf_last_error()
        # an empty batch is fine whatever the pointers are
        assert fn(None, None, None, 0, 4, 4, layout, None, None) == _ffi.RF_OK
    for layout in (2, -1):
        assert fn(x, r, r8, 1, 4, 4, layout, wts, None) == E
        assert b"layout" in lib.rf_last_error()
    assert fn(None, None, None, 0, 4, 4, 2, None, None) == _ffi.RF_OK


@pytest.mark.parametrize("name", ENTRIES)
def test_outputs_inside_the_input_are_refused(ptrs, name):
    """4x4 pixels: x is 192 bytes; a lane reads pixel i + half long after others wrote theirs."""
    lib = _ffi.load_library()
    fn = getattr(lib, name)
    _, (_, r, r8, wts) = ptrs
    big = ctypes.create_string_buffer(1024)
    base = ctypes.cast(big, ctypes.c_void_p).value
    for layout in (_ffi.CNN_NCHW_RGB, _ffi.CNN_NHWC_BGR):
        for off in (0, 64, 188):                                  # r_out inside x (its last float too)
            assert fn(base, base + off, r8, 1, 4, 4, layout, wts, None) == _ffi.RF_E_BADARG, off
            assert b"r_out" in lib.rf_last_error() and b"overlap" in lib.rf_last_error()
            assert fn(base, base + off, None, 1, 4, 4, layout, wts, None) == _ffi.RF_E_BADARG
        for off in (0, 100, 191):                                 # r_u8_out inside x
            assert fn(base, r, base + off, 1, 4, 4, layout, wts, None) == _ffi.RF_E_BADARG, off
            assert b"r_u8_out" in lib.rf_last_error() and b"overlap" in lib.rf_last_error()
            assert fn(base, None, base + off, 1, 4, 4, layout, wts, None) == _ffi.RF_E_BADARG
        # an output that ENDS inside x: 16 floats starting 32 bytes before it
        assert fn(base + 64, base + 32, r8, 1, 4, 4, layout, wts, None) == _ffi.RF_E_BADARG
        assert fn(base + 64, r, base + 56, 1, 4, 4, layout, wts, None) == _ffi.RF_E_BADARG


# ---------------------------------------------------------------------------- Python routing
class _FakeTensor(object):
    """What forward() needs of a device tensor: made from numpy, moved, brought back."""

    def __init__(self, array):
        self.array = array

    def cuda(self):
        return self

    def cpu(self):
        return self

    def numpy(self):
        return self.array


class _FakeTorch(object):
    @staticmethod
    def from_numpy(array):
        return _FakeTensor(array)


class _Recorder(object):
    """ops with the two forward passes recorded instead of run."""

    def __init__(self):
        self.calls = []

    def _result(self, shape, want_float, want_u8):
        n, h, w = shape
        return (_FakeTensor(np.full((n, h, w), 0.25, np.float32)) if want_float else None,
                _FakeTensor(np.full((n, h, w), 63, np.uint8)) if want_u8 else None)

    def cnn_reflectance_u8(self, bgr, weights=None, want_float=True, want_u8=True):
        self.calls.append(("u8", bgr, {"weights": weights}))
        n, h, w, _ = bgr.array.shape if isinstance(bgr, _FakeTensor) else bgr.shape
        return self._result((n, h, w), want_float, want_u8)

    def cnn_reflectance_f32(self, x, layout="nchw_rgb", weights=None, want_float=True, want_u8=True):
        self.calls.append(("f32", x, {"weights": weights, "layout": layout}))
        shape = x.array.shape if isinstance(x, _FakeTensor) else tuple(x.shape)
        n, h, w = (shape[0], shape[2], shape[3]) if layout == "nchw_rgb" else shape[:3]
        return self._result((n, h, w), want_float, want_u8)


@pytest.fixture
def stubbed(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(dc, "ops", rec)
    monkeypatch.setattr(dc._ffi, "require_gpu", lambda: _FakeTorch)
    return rec


def _byte_blob(n, h, w, seed):
    bgr = np.random.RandomState(seed).randint(0, 256, (n, h, w, 3)).astype(np.uint8)
    blob = iu.srgb_byte_lut()[bgr[..., ::-1]].transpose(0, 3, 1, 2)
    return bgr, np.ascontiguousarray(blob)


def test_forward_routes_byte_level_blobs_to_the_u8_entry(stubbed):
    net = dc.ReflectanceNet()
    bgr, blob = _byte_blob(1, 4, 5, 1)
    net.blobs["images"].reshape(1, 3, 4, 5)
    net.blobs["images"].data[...] = blob
    out = net.forward()
    assert [c[0] for c in stubbed.calls] == ["u8"]
    sent = stubbed.calls[0][1].array
    assert sent.dtype == np.uint8 and np.array_equal(sent, bgr)
    assert stubbed.calls[0][2]["weights"] is net.weights
    assert out["reflectance_intensity"].shape == (1, 1, 4, 5)


def test_forward_routes_other_blobs_to_the_float_entry(stubbed):
    net = dc.ReflectanceNet()
    _, blob = _byte_blob(1, 4, 5, 2)
    blob[0, 0, 0, 0] = 0.123456                   # not an sRGB byte level
    net.blobs["images"].reshape(1, 3, 4, 5)
    net.blobs["images"].data[...] = blob
    with pytest.raises(ValueError):               # _blob_to_bytes keeps its refusal ...
        net._blob_to_bytes()
    out = net.forward()                           # ... and forward() runs the floats, as Caffe does
    assert [c[0] for c in stubbed.calls] == ["f32"]
    kind, sent, kw = stubbed.calls[0]
    assert kw["layout"] == "nchw_rgb" and kw["weights"] is net.weights
    assert sent.array.dtype == np.float32 and sent.array.shape == (1, 3, 4, 5)
    assert sent.array.flags["C_CONTIGUOUS"] and np.array_equal(sent.array, blob)
    assert out["reflectance_intensity"].shape == (1, 1, 4, 5)
    assert out["reflectance_intensity"] is net.blobs["reflectance_intensity"].data


def test_forward_takes_batches_and_keeps_its_shape_error(stubbed):
    net = dc.ReflectanceNet()
    net.blobs["images"].reshape(2, 3, 4, 5)
    net.blobs["images"].data[...] = np.random.RandomState(3).rand(2, 3, 4, 5)
    out = net.forward()
    assert [c[0] for c in stubbed.calls] == ["f32"]
    assert out["reflectance_intensity"].shape == (2, 1, 4, 5)
    assert out["reflectance_intensity"].dtype == np.float32
    _, blob = _byte_blob(2, 4, 5, 4)              # N > 1 on the byte route too
    net.blobs["images"].data[...] = blob
    assert net.forward()["reflectance_intensity"].shape == (2, 1, 4, 5)
    assert [c[0] for c in stubbed.calls] == ["f32", "u8"]
    net.blobs["images"].reshape(1, 4, 4, 4)
    with pytest.raises(ValueError) as e:
        net.forward()
    assert "[N,3,H,W]" in str(e.value)
    assert len(stubbed.calls) == 2


def test_get_reflectance_batch_routes_by_dtype(stubbed):
    import torch
    u8 = torch.zeros((2, 4, 5, 3), dtype=torch.uint8)
    f32 = torch.zeros((2, 4, 5, 3), dtype=torch.float32)
    dc.get_reflectance_batch(u8)
    dc.get_reflectance_batch(f32, weights="w")
    assert [c[0] for c in stubbed.calls] == ["u8", "f32"]
    assert stubbed.calls[0][1] is u8 and stubbed.calls[1][1] is f32
    assert stubbed.calls[1][2] == {"weights": "w", "layout": "nhwc_bgr"}
    for bad in (f32.double(), f32.half(), u8.to(torch.int32), np.zeros((1, 4, 5, 3), np.uint8)):
        with pytest.raises(ValueError) as e:
            dc.get_reflectance_batch(bad)
        assert "uint8" in str(e.value) and "float32" in str(e.value)
    assert len(stubbed.calls) == 2


def test_ops_f32_checks_its_arguments_before_the_library(built, monkeypatch):
    """Layout names and tensor checks of ops.cnn_reflectance_f32 need no device."""
    import torch
    from reflectance_filtering_amd import ops
    monkeypatch.setattr(ops._ffi, "require_gpu", lambda: torch)
    x = torch.zeros((1, 3, 4, 5), dtype=torch.float32)
    with pytest.raises(ValueError):
        ops.cnn_reflectance_f32(x, layout="nchw")
    with pytest.raises(ValueError):                 # not on the device
        ops.cnn_reflectance_f32(x)
