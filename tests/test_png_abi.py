"""CPU suite: the device-side PNG encoder without a device - the stream bound and the chunk plan of
rf_png_deflate_ragged_u8 against hand-computed values, every refusal before any device work, the
host-side container around any zlib stream, the batch pipeline's two payload kinds and the parser's
default.  No compute calls."""
import ctypes
import os
import zlib

import numpy as np
import pytest

from reflectance_filtering_amd import _ffi, batch, ops
from reflectance_filtering_amd import image_utils as iu

C = 32768                                            # the library's chunk length in raw bytes
RECORD = 40                                          # first, slot0 (u64), rawlen, rowlen, w, chunk0, nchunks, pad (u32)
SLOT = (C + 9 + 15) & ~15                            # bytes between the slots of an image's chunks


def _ints(values):
    a = np.ascontiguousarray(values, dtype=np.int32)
    return a, a.ctypes.data


def _align256(b):
    return (b + 255) & ~255


def test_plan_and_bound_of_hand_computed_lists(built):
    lib = _ffi.load_library()
    # one pixel: grey 1 * (1 + 1) = 2 raw bytes, colour 1 * (1 + 3) = 4; one chunk each
    assert _ffi.png_plan([(1, 1)]) == (C, 1, [1])
    hs, p_h = _ints([1])
    ws, p_w = _ints([1])
    assert lib.rf_png_stream_bound(1, p_h, p_w, 1, 0) == 2 + (2 + 9) + 2 + 4
    assert lib.rf_png_stream_bound(1, p_h, p_w, 3, 0) == 2 + (4 + 9) + 2 + 4
    assert lib.rf_png_stream_bound(1, p_h, p_w, 1, _ffi.PNG_GREY_AS_RGB) == 2 + (4 + 9) + 2 + 4
    # 341 x 512: grey 341 * 513 = 174933 raw bytes = 5 chunks of 32768 and one of 11093;
    # colour 341 * 1537 = 524117 = 15 chunks and one of 32597.  1080 x 1920 colour:
    # 1080 * 5761 = 6221880 = 189 chunks and one of 28728.  (1, 32767): 32768 raw bytes, one chunk;
    # (1, 32768): 32769, two
    sizes = [(341, 512), (1080, 1920), (1, 32767), (1, 32768)]
    assert _ffi.png_plan(sizes, 1) == (C, 6 + 64 + 1 + 2, [6, 64, 1, 2])
    assert 1080 * 1921 == 63 * C + 10296
    assert _ffi.png_plan(sizes, 3) == (C, 16 + 190 + 3 + 4, [16, 190, 3, 4])
    assert _ffi.png_plan(sizes, 1, _ffi.PNG_GREY_AS_RGB) == _ffi.png_plan(sizes, 3)
    hs, p_h = _ints([s[0] for s in sizes])
    ws, p_w = _ints([s[1] for s in sizes])
    raw_grey = 174933 + 1080 * 1921 + 32768 + 32769
    assert lib.rf_png_stream_bound(4, p_h, p_w, 1, 0) == raw_grey + 9 * 73 + 8 * 4
    raw_bgr = 524117 + 6221880 + (1 + 3 * 32767) + (1 + 3 * 32768)
    assert lib.rf_png_stream_bound(4, p_h, p_w, 3, 0) == raw_bgr + 9 * 213 + 8 * 4
    # the empty list: a valid call, nothing to size
    assert _ffi.png_plan(np.zeros((0, 2), np.int64)) == (C, 0, [])
    assert lib.rf_png_stream_bound(0, None, None, 1, 0) == 0
    assert lib.rf_png_workspace_bytes(0, None, None, 1, 0) == 0
    assert lib.rf_png_deflate_ragged_u8(None, 0, None, None, 1, 0, None, 0, None, None, 0, None) == _ffi.RF_OK
    # the plan query writes what fits `cap` ints and returns n
    out = np.full(5, -7, dtype=np.int32)
    assert lib.rf_debug_png_plan(4, p_h, p_w, 1, 0, out.ctypes.data, 3) == 4
    assert out.tolist() == [C, 73, 6, -7, -7]
    assert lib.rf_debug_png_plan(4, p_h, p_w, 1, 0, None, 0) == 4
    assert lib.rf_debug_png_plan(4, p_h, p_w, 1, 0, None, 1) == _ffi.RF_E_BADARG
    assert lib.rf_debug_png_plan(4, p_h, p_w, 1, 0, out.ctypes.data, -1) == _ffi.RF_E_BADARG


def test_workspace_is_the_tables_plus_one_slot_per_chunk(built):
    lib = _ffi.load_library()
    # 3 images of 2, 32769 and 70000 raw bytes (grey): 1 + 2 + 3 = 6 chunks; the slots of an image are
    # SLOT bytes apart and its last one holds its bytes + 9, rounded up to 16
    hs, p_h = _ints([1, 1, 7])
    ws, p_w = _ints([1, 32768, 9999])
    assert _ffi.png_plan([(1, 1), (1, 32768), (7, 9999)]) == (C, 6, [1, 2, 3])
    up16 = lambda b: (b + 15) & ~15
    slots = up16(2 + 9) + (SLOT + up16(1 + 9)) + (2 * SLOT + up16(70000 - 2 * C + 9))
    want = (_align256(RECORD * 3) + 2 * _align256(4 * 6) + _align256(8 * 6) + 2 * _align256(4 * 3)
            + _align256(slots))
    assert lib.rf_png_workspace_bytes(3, p_h, p_w, 1, 0) == want
    # a size query that cannot answer
    bad, p_bad = _ints([1, 0, 7])
    assert lib.rf_png_workspace_bytes(3, p_bad, p_w, 1, 0) == 0
    assert lib.rf_png_stream_bound(3, p_bad, p_w, 1, 0) == 0
    assert lib.rf_png_workspace_bytes(-1, p_h, p_w, 1, 0) == 0
    assert lib.rf_png_workspace_bytes(3, None, p_w, 1, 0) == 0
    assert lib.rf_png_stream_bound(3, p_h, None, 1, 0) == 0
    assert lib.rf_png_stream_bound(3, p_h, p_w, 2, 0) == 0
    assert lib.rf_png_stream_bound(3, p_h, p_w, 3, _ffi.PNG_GREY_AS_RGB) == 0


def test_refusals_need_no_gpu(built):
    lib = _ffi.load_library()
    buf = ctypes.create_string_buffer(1 << 16)
    base = (ctypes.addressof(buf) + 255) & ~255
    images, streams, offsets, wsp = (base + 8192 * i for i in range(4))
    hs, p_h = _ints([8, 3, 5])
    wd, p_w = _ints([8, 7, 2])
    bound = lib.rf_png_stream_bound(3, p_h, p_w, 1, 0)
    assert bound == (72 + 24 + 15) + 3 * (9 + 8)
    need = lib.rf_png_workspace_bytes(3, p_h, p_w, 1, 0)
    assert need > 0

    def call(images=images, n=3, ph=p_h, pw=p_w, cn=1, flags=0, streams=streams, cap=bound,
             offsets=offsets, ws=wsp, ws_bytes=need - 1):
        # a call that passes every argument rule ends at the workspace that is one byte short
        return lib.rf_png_deflate_ragged_u8(images, n, ph, pw, cn, flags, streams, cap, offsets, ws,
                                            ws_bytes, None)

    def refused(code, word, **kw):
        assert call(**kw) == code, kw
        msg = lib.rf_last_error()
        assert b"rf_png_deflate_ragged_u8" in msg and word in msg, (kw, msg)

    refused(_ffi.RF_E_WORKSPACE, b"workspace")
    refused(_ffi.RF_E_WORKSPACE, b"workspace", ws_bytes=0)
    refused(_ffi.RF_E_WORKSPACE, b"workspace", cn=3, cap=4096, ws_bytes=16)
    refused(_ffi.RF_E_WORKSPACE, b"workspace", flags=_ffi.PNG_GREY_AS_RGB, cap=4096, ws_bytes=16)
    for kw in ({"images": None}, {"ph": None}, {"pw": None}, {"streams": None}, {"offsets": None},
               {"ws": None}):
        refused(_ffi.RF_E_BADARG, b"NULL", **kw)
    # an empty list is valid whatever the pointers are
    assert call(n=0, images=None, ph=None, pw=None, streams=None, offsets=None, ws=None) == _ffi.RF_OK
    refused(_ffi.RF_E_BADARG, b"n=-1", n=-1)
    for bad_h, bad_w, word in (([8, 0, 5], [8, 7, 2], b"size of image 1"),
                               ([8, 3, 5], [8, 7, 0], b"size of image 2"),
                               ([-8, 3, 5], [8, 7, 2], b"size of image 0"),
                               ([8, 3, 5], [8, -7, 2], b"size of image 1")):
        a, p_a = _ints(bad_h)
        b, p_b = _ints(bad_w)
        refused(_ffi.RF_E_BADARG, word, ph=p_a, pw=p_b)
    for cn in (0, 2, 4):
        refused(_ffi.RF_E_UNSUPPORTED, b"cn_in", cn=cn)
    refused(_ffi.RF_E_BADARG, b"flag", flags=2)
    refused(_ffi.RF_E_BADARG, b"flag", flags=0x1000 | _ffi.PNG_GREY_AS_RGB)
    refused(_ffi.RF_E_BADARG, b"RF_PNG_GREY_AS_RGB", cn=3, flags=_ffi.PNG_GREY_AS_RGB)
    # an image whose own bound reaches 2^31 = 2147483648: 46000 rows of 1 + 46675 bytes are 2147096000
    # raw bytes in 65525 chunks, bound 2147096000 + 9 * 65525 + 8 = 2147685733: refused; 45990 such rows
    # are 2146629240 bytes in 65510 chunks, bound 2147218838: pass
    a, p_a = _ints([8, 46000, 5])
    b, p_b = _ints([8, 46675, 2])
    refused(_ffi.RF_E_UNSUPPORTED, b"image 1", ph=p_a, pw=p_b, cap=1 << 40)
    a, p_a = _ints([8, 45990, 5])
    refused(_ffi.RF_E_WORKSPACE, b"workspace", ph=p_a, pw=p_b, cap=1 << 40)
    assert 45990 * 46676 + 9 * 65510 + 8 == 2147218838 < 2 ** 31 <= 46000 * 46676 + 9 * 65525 + 8
    # ... each image on its own: two such images in one list pass as well
    a, p_a = _ints([45990, 45990, 5])
    b, p_b = _ints([46675, 46675, 2])
    refused(_ffi.RF_E_WORKSPACE, b"workspace", ph=p_a, pw=p_b, cap=1 << 40)
    refused(_ffi.RF_E_BADARG, b"capacity", cap=bound - 1)
    refused(_ffi.RF_E_BADARG, b"capacity", cap=0)
    refused(_ffi.RF_E_BADARG, b"aligned", ws=wsp + 8, ws_bytes=need)
    refused(_ffi.RF_E_BADARG, b"aligned", offsets=offsets + 4, ws_bytes=need)
    # overlap is judged by range: 64 + 21 + 10 = 95 pixels of input, `bound` bytes of streams
    refused(_ffi.RF_E_BADARG, b"overlap", streams=images + 94, ws_bytes=need)
    refused(_ffi.RF_E_BADARG, b"overlap", streams=images - bound + 1, ws_bytes=need)
    refused(_ffi.RF_E_BADARG, b"overlap", streams=images, ws_bytes=need)


def test_the_container_decodes_with_any_zlib_stream(built, tmp_path):
    rng = np.random.default_rng(61)
    for shape, ctype in (((5, 7), 0), ((6, 4, 3), 2), ((1, 1), 0)):
        img = rng.integers(0, 256, shape).astype(np.uint8)
        rows = img if img.ndim == 2 else img[:, :, ::-1].reshape(shape[0], -1)
        raw = b"".join(b"\x00" + bytes(r.tobytes()) for r in rows)         # filter type 0: None
        png = iu.png_container(zlib.compress(raw, 6), shape[0], shape[1], ctype)
        want = img if img.ndim == 3 else np.repeat(img[:, :, None], 3, axis=2)
        assert np.array_equal(iu._png_decode(png), want)
        path = str(tmp_path / "x.png")
        with open(path, "wb") as fh:
            fh.write(png)
        assert np.array_equal(iu.imread(path), want)
        # around the host encoder's own stream it is the host encoder's file
        host = iu._png_encode(img)
        idat = host[8 + 25 + 8:-12 - 4]
        assert iu.png_container(idat, shape[0], shape[1], ctype) == host
    with pytest.raises(ValueError):
        iu.png_container(b"", 4, 4, 3)
    with pytest.raises(ValueError):
        iu.png_container(b"", 0, 4, 0)


def test_pipeline_writes_bytes_as_they_are_and_arrays_through_imwrite(built, tmp_path):
    rng = np.random.default_rng(62)
    arrays = [rng.integers(0, 256, (5, 6, 3)).astype(np.uint8) for _ in range(5)]
    blobs = [b"not a picture %d" % i for i in range(5)]

    def compute(loaded):
        jobs = []
        for i in loaded:
            jobs.append((str(tmp_path / ("a%d.png" % i)), arrays[i]))
            jobs.append((str(tmp_path / ("b%d.png" % i)), blobs[i]))
        return jobs

    written = batch.pipeline(range(5), lambda i: i, compute, step=2)
    assert [os.path.basename(f) for f in written] == [n % i for i in range(5) for n in ("a%d.png", "b%d.png")]
    for i in range(5):
        with open(str(tmp_path / ("b%d.png" % i)), "rb") as fh:
            assert fh.read() == blobs[i]
        with open(str(tmp_path / ("a%d.png" % i)), "rb") as fh:
            assert fh.read() == iu._png_encode(arrays[i])
    with pytest.raises(Exception) as err:
        batch.pipeline([0], lambda i: i, lambda loaded: [(str(tmp_path / "none" / "x.png"), b"x")])
    assert "Not able to write" in str(err.value)


def test_the_parser_defaults_to_the_host_encoder(built):
    parser = batch.build_parser()
    f = parser.parse_args(["filter", "--inputs", "x", "--path_out", "o", "--sigma_color", "1",
                           "--sigma_spatial", "2", "--filter_type", "guided"])
    d = parser.parse_args(["decompose", "--inputs", "x", "--path_out", "o"])
    assert f.png_encoder == "host" and d.png_encoder == "host"
    d = parser.parse_args(["decompose", "--inputs", "x", "--path_out", "o", "--png_encoder", "device"])
    assert d.png_encoder == "device"
    with pytest.raises(SystemExit):
        parser.parse_args(["decompose", "--inputs", "x", "--path_out", "o", "--png_encoder", "gpu"])
    import inspect
    assert inspect.signature(batch.filter_files).parameters["png_encoder"].default == "host"
    assert inspect.signature(batch.decompose_files).parameters["png_encoder"].default == "host"
    with pytest.raises(ValueError):
        batch.decompose_files([], "o", png_encoder="gpu")


def test_the_operator_raises_without_a_gpu(built, monkeypatch):
    """No CPU fallback: like the other operators, the encoder raises where no device is visible."""
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(_ffi.RFError):
        ops.png_encode_ragged_u8([torch.zeros((4, 5, 3), dtype=torch.uint8)])
    with pytest.raises(_ffi.RFError):
        ops.png_encode_ragged_u8([])
