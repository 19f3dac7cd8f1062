"""CPU suite: the hybrid PNG decoder without a device - image_utils.png_parse on files of three
writers and on everything it has to decline, the workspace query of rf_png_unfilter_ragged_u8
against a hand-computed value, every refusal of the entry before any device work with its message,
and the batch tools' `png_decoder` option.  No compute calls."""
import ctypes
import inspect
import io
import struct
import zlib

import numpy as np
import pytest

from reflectance_filtering_amd import _ffi, batch, ops
from reflectance_filtering_amd import image_utils as iu
from tests import png_synth as ps
from tests import synth


def _ints(values):
    a = np.ascontiguousarray(values, dtype=np.int32)
    return a, a.ctypes.data


def _fmt(depth, ctype):
    return (depth << 8) | ctype


def _align256(b):
    return (b + 255) & ~255


def _pillow(array, mode=None):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(array, mode).save(buf, format="PNG")
    return buf.getvalue()


# ---- png_parse -------------------------------------------------------------------------------------

def test_parse_reads_the_built_in_and_the_pillow_writer():
    scene = synth.scene_u8(48, 70, 6001)
    grey = synth.reflectance_like_u8(48, 70, 6002)[:, :, 0]
    for data, want in ((iu._png_encode(scene), (48, 70, 8, 2)), (iu._png_encode(grey), (48, 70, 8, 0))):
        h, w, depth, ctype, palette, raw = iu.png_parse(data)
        assert (h, w, depth, ctype) == want and palette is None
        assert raw == zlib.decompress(ps.idat_of(data))
    pytest.importorskip("PIL")
    for data, want in ((_pillow(np.ascontiguousarray(scene[:, :, ::-1])), (48, 70, 8, 2)),
                       (_pillow(grey), (48, 70, 8, 0)),
                       (_pillow(grey.astype(np.uint16) * 257), (48, 70, 16, 0))):
        h, w, depth, ctype, palette, raw = iu.png_parse(data)
        assert (h, w, depth, ctype) == want and palette is None
        assert raw == zlib.decompress(ps.idat_of(data))
        assert len(raw) == h * (1 + w * ps.bpp_of(depth, ctype))


@pytest.mark.parametrize("depth,ctype", ps.FORMATS)
def test_parse_reads_every_format_with_split_idat_and_ancillary_chunks(depth, ctype):
    rng = np.random.default_rng(6100 + depth + ctype)
    h, w = 9, 13
    rows = ps.samples(rng, h, w, depth, ctype, palette_len=37)
    palette = rng.integers(0, 256, (37, 3)).astype(np.uint8) if ctype == 3 else None
    filters = ps.filters_for("random", h, rng)
    for chunks, anc in ((1, False), (3, True), (7, True)):
        data = ps.write_png(rows, w, depth, ctype, filters, palette, idat_chunks=chunks, ancillary=anc)
        got = iu.png_parse(data)
        assert got is not None
        assert got[:4] == (h, w, depth, ctype)
        assert got[5] == ps.filter_rows(rows, ps.bpp_of(depth, ctype), filters)
        assert got[5] == zlib.decompress(ps.idat_of(data))
        if ctype == 3:
            assert np.array_equal(got[4], palette)
        else:
            assert got[4] is None
        assert iu.png_parse(bytearray(data))[5] == got[5]       # any buffer of bytes
        # ... and the built-in reader agrees on what the file holds
        assert iu._png_decode(data) is not None


def test_parse_declines_what_the_device_route_does_not_take():
    rng = np.random.default_rng(6200)
    h, w = 6, 10
    rows = ps.samples(rng, h, w, 8, 2)
    good = ps.write_png(rows, w, 8, 2, [4] * h, ancillary=True, idat_chunks=2)
    assert iu.png_parse(good) is not None
    # the interlace flag
    assert iu.png_parse(ps.write_png(rows, w, 8, 2, [0] * h, interlace=1)) is None
    # sub-byte depths, grey and palette
    for depth in (1, 2, 4):
        packed = rng.integers(0, 256, (h, (w * depth + 7) // 8)).astype(np.uint8)
        assert iu.png_parse(ps.write_png(packed, w, depth, 0, [0] * h)) is None
        pal = rng.integers(0, 256, (1 << depth, 3)).astype(np.uint8)
        assert iu.png_parse(ps.write_png(packed, w, depth, 3, [0] * h, palette=pal)) is None
    # an unknown colour type, a 16-bit palette, a palette file without PLTE
    assert iu.png_parse(ps.write_png(rows[:, :w], w, 8, 5, [0] * h)) is None
    assert iu.png_parse(ps.write_png(rows[:, :2 * w], w, 16, 3, [0] * h,
                                     palette=np.zeros((4, 3), np.uint8))) is None
    assert iu.png_parse(ps.write_png(rows[:, :w], w, 8, 3, [0] * h)) is None
    # truncated: inside the IDAT, before IEND, inside the header
    for cut in (len(good) - 12, len(good) - 20, len(good) - 1, 40, 20, 8, 3, 0):
        assert iu.png_parse(good[:cut]) is None, cut
    # one flipped CRC byte in every chunk the parser uses; an ancillary chunk's CRC is not its business
    pos, seen = 8, []
    while pos < len(good):
        (length,) = struct.unpack(">I", good[pos:pos + 4])
        tag = good[pos + 4:pos + 8]
        crc_at = pos + 8 + length
        bad = bytearray(good)
        bad[crc_at + 3] ^= 0x01
        if tag in (b"IHDR", b"IDAT", b"IEND"):
            assert iu.png_parse(bytes(bad)) is None, tag
        else:
            assert iu.png_parse(bytes(bad)) is not None, tag
        seen.append(tag)
        pos = crc_at + 4
    assert seen.count(b"IDAT") == 2 and b"gAMA" in seen
    palfile = ps.write_png(rows[:, :w] % 5, w, 8, 3, [1] * h, palette=np.zeros((5, 3), np.uint8))
    assert iu.png_parse(palfile) is not None
    at = palfile.index(b"PLTE")
    bad = bytearray(palfile)
    bad[at + 4 + 15 + 2] ^= 0x80
    assert iu.png_parse(bytes(bad)) is None
    # the inflated stream itself: its length, its filter bytes

    def with_raw(raw, hh=h):
        return (ps.SIG + ps.chunk(b"IHDR", struct.pack(">IIBBBBB", w, hh, 8, 2, 0, 0, 0))
                + ps.chunk(b"IDAT", zlib.compress(raw)) + ps.chunk(b"IEND", b""))

    raw = ps.filter_rows(rows, 3, [2] * h)
    assert iu.png_parse(with_raw(raw))[5] == raw
    assert iu.png_parse(with_raw(raw[:-1])) is None               # raw one byte short
    assert iu.png_parse(with_raw(raw + b"\x00")) is None          # ... and one too long
    five = bytearray(raw)
    five[(h - 1) * (1 + 3 * w)] = 5                               # a filter byte 5 on the last row
    assert iu.png_parse(with_raw(bytes(five))) is None
    five = bytearray(raw)
    five[0] = 255
    assert iu.png_parse(with_raw(bytes(five))) is None
    # not a PNG at all, and an empty picture
    for data in (b"", b"GIF89a" + bytes(40), b"\xff\xd8\xff\xe0" + bytes(64), good[1:], bytes(64)):
        assert iu.png_parse(data) is None
    assert iu.png_parse(ps.SIG + ps.chunk(b"IHDR", struct.pack(">IIBBBBB", 0, 4, 8, 0, 0, 0, 0))
                        + ps.chunk(b"IDAT", zlib.compress(b"\x00" * 4)) + ps.chunk(b"IEND", b"")) is None


# ---- the entry without a device --------------------------------------------------------------------

def test_workspace_is_the_table_and_the_flag_words(built):
    lib = _ffi.load_library()
    # 48 bytes of table and 4 bytes of flags per image, each part rounded up to 256
    for n in (1, 5, 6, 64, 65):
        hs, p_h = _ints([3 + i for i in range(n)])
        ws, p_w = _ints([7 + i for i in range(n)])
        fm, p_f = _ints([_fmt(*ps.FORMATS[i % 9]) for i in range(n)])
        assert lib.rf_png_unfilter_workspace_bytes(n, p_h, p_w, p_f) == _align256(48 * n) + _align256(4 * n)
    assert lib.rf_png_unfilter_workspace_bytes(6, p_h, p_w, p_f) == 512 + 256
    assert lib.rf_png_unfilter_workspace_bytes(0, None, None, None) == 0
    assert lib.rf_png_unfilter_workspace_bytes(-1, p_h, p_w, p_f) == 0
    assert lib.rf_png_unfilter_workspace_bytes(3, None, p_w, p_f) == 0
    assert lib.rf_png_unfilter_workspace_bytes(3, p_h, p_w, None) == 0
    bad, p_bad = _ints([3, 0, 4])
    assert lib.rf_png_unfilter_workspace_bytes(3, p_bad, p_w, p_f) == 0
    bad, p_bad = _ints([_fmt(8, 0), _fmt(4, 0), _fmt(8, 2)])
    assert lib.rf_png_unfilter_workspace_bytes(3, p_h, p_w, p_bad) == 0
    assert lib.rf_png_unfilter_ragged_u8(None, None, 0, None, None, None, None, None, None, None, 0,
                                         None) == _ffi.RF_OK


def test_refusals_need_no_gpu(built):
    lib = _ffi.load_library()
    buf = ctypes.create_string_buffer(1 << 16)
    base = (ctypes.addressof(buf) + 255) & ~255
    raw, images, flags, wsp, pal = (base + 8192 * i for i in range(5))
    hs, p_h = _ints([8, 3, 5])
    wd, p_w = _ints([8, 7, 2])
    fm, p_f = _ints([_fmt(8, 0), _fmt(16, 6), _fmt(8, 2)])
    lens = [8 * (1 + 8), 3 * (1 + 7 * 8), 5 * (1 + 2 * 3)]
    assert lens == [72, 171, 35]
    offs = np.array([16, 16 + 72, 16 + 72 + 171, 16 + 72 + 171 + 35], dtype=np.uint64)
    need = lib.rf_png_unfilter_workspace_bytes(3, p_h, p_w, p_f)
    assert need == 512

    def call(raw=raw, po=offs.ctypes.data, n=3, ph=p_h, pw=p_w, pf=p_f, pal=None, images=images,
             flags=flags, ws=wsp, ws_bytes=need - 1):
        # a call that passes every argument rule ends at the workspace that is one byte short
        return lib.rf_png_unfilter_ragged_u8(raw, po, n, ph, pw, pf, pal, images, flags, ws, ws_bytes, None)

    def refused(code, word, **kw):
        assert call(**kw) == code, kw
        msg = lib.rf_last_error()
        assert b"rf_png_unfilter_ragged_u8" in msg and word in msg, (kw, msg)

    refused(_ffi.RF_E_WORKSPACE, b"workspace")
    refused(_ffi.RF_E_WORKSPACE, b"workspace", ws_bytes=0)
    for kw in ({"raw": None}, {"po": None}, {"ph": None}, {"pw": None}, {"pf": None}, {"images": None},
               {"flags": None}, {"ws": None}):
        refused(_ffi.RF_E_BADARG, b"NULL", **kw)
    # an empty list is valid whatever the pointers are
    assert call(n=0, raw=None, po=None, ph=None, pw=None, pf=None, images=None, flags=None,
                ws=None) == _ffi.RF_OK
    refused(_ffi.RF_E_BADARG, b"n=-1", n=-1)
    for bad_h, bad_w, word in (([8, 0, 5], [8, 7, 2], b"size of image 1"),
                               ([8, 3, 5], [8, 7, 0], b"size of image 2"),
                               ([-8, 3, 5], [8, 7, 2], b"size of image 0"),
                               ([8, 3, 5], [8, -7, 2], b"size of image 1")):
        a, p_a = _ints(bad_h)
        b, p_b = _ints(bad_w)
        refused(_ffi.RF_E_BADARG, word, ph=p_a, pw=p_b)
    # formats: sub-byte depths, a 16-bit palette, colour types that do not exist, garbage
    for bad in (_fmt(1, 0), _fmt(2, 0), _fmt(4, 3), _fmt(16, 3), _fmt(8, 1), _fmt(8, 5), _fmt(8, 7),
                _fmt(32, 0), 0, -1, _fmt(8, 2) | (1 << 20)):
        a, p_a = _ints([_fmt(8, 0), _fmt(16, 6), bad])
        refused(_ffi.RF_E_UNSUPPORTED, b"of image 2", pf=p_a)
    # a palette image needs the palettes
    a, p_a = _ints([_fmt(8, 3), _fmt(16, 6), _fmt(8, 2)])
    refused(_ffi.RF_E_BADARG, b"NULL", pf=p_a)
    refused(_ffi.RF_E_WORKSPACE, b"workspace", pf=p_a, pal=pal)
    # the raw length of every image is h * (1 + w * bpp)
    for i in range(3):
        for d in (-1, 1):
            o = offs.copy()
            o[i + 1:] += np.uint64(d) if d > 0 else np.uint64(0)
            o[i + 1:] -= np.uint64(1) if d < 0 else np.uint64(0)
            if i < 2:
                o[i + 2:] = o[i + 1] + (offs[i + 2:] - offs[i + 1])       # only image i is wrong
            refused(_ffi.RF_E_BADARG, b"raw length of image %d" % i, po=o.ctypes.data)
    # an image whose raw stream reaches 2^31 = 2147483648 bytes: 32768 rows of 1 + 65535 bytes are exactly
    # 2^31 (refused), 32767 such rows pass; grey, so the pixel count stays below
    a, p_a = _ints([8, 3, 32768])
    b, p_b = _ints([8, 7, 65535])
    g, p_g = _ints([_fmt(8, 0), _fmt(16, 6), _fmt(8, 0)])
    o = np.array([0, 72, 243, 243 + 32768 * 65536], dtype=np.uint64)
    refused(_ffi.RF_E_UNSUPPORTED, b"image 2", ph=p_a, pw=p_b, pf=p_g, po=o.ctypes.data)
    a, p_a = _ints([8, 3, 32767])
    o = np.array([0, 72, 243, 243 + 32767 * 65536], dtype=np.uint64)
    refused(_ffi.RF_E_WORKSPACE, b"workspace", ph=p_a, pw=p_b, pf=p_g, po=o.ctypes.data)
    # ... and the pixel count: 46341^2 = 2147488281 >= 2^31 pixels of one byte
    a, p_a = _ints([8, 3, 46341])
    b, p_b = _ints([8, 7, 46341])
    o = np.array([0, 72, 243, 243 + 46341 * 46342], dtype=np.uint64)
    refused(_ffi.RF_E_UNSUPPORTED, b"image 2", ph=p_a, pw=p_b, pf=p_g, po=o.ctypes.data)
    refused(_ffi.RF_E_BADARG, b"aligned", ws=wsp + 8, ws_bytes=need)
    # overlap is judged by range: 64 + 21 + 10 = 95 pixels of 3 bytes, 278 bytes of raw from raw + 16 on
    refused(_ffi.RF_E_BADARG, b"overlap", images=raw + 16 + 277, ws_bytes=need)
    refused(_ffi.RF_E_BADARG, b"overlap", images=raw + 16 - 285 + 1, ws_bytes=need)
    refused(_ffi.RF_E_BADARG, b"overlap", images=raw + 16, ws_bytes=need)


# ---- the batch tools' option -----------------------------------------------------------------------

def test_the_parser_defaults_to_the_host_decoder(built):
    parser = batch.build_parser()
    f = parser.parse_args(["filter", "--inputs", "x", "--path_out", "o", "--sigma_color", "1",
                           "--sigma_spatial", "2", "--filter_type", "guided"])
    d = parser.parse_args(["decompose", "--inputs", "x", "--path_out", "o"])
    assert f.png_decoder == "host" and d.png_decoder == "host"
    d = parser.parse_args(["decompose", "--inputs", "x", "--path_out", "o", "--png_decoder", "device"])
    assert d.png_decoder == "device" and d.png_encoder == "host"
    f = parser.parse_args(["filter", "--inputs", "x", "--path_out", "o", "--sigma_color", "1",
                           "--sigma_spatial", "2", "--filter_type", "guided", "--png_decoder", "device"])
    assert f.png_decoder == "device"
    with pytest.raises(SystemExit):
        parser.parse_args(["decompose", "--inputs", "x", "--path_out", "o", "--png_decoder", "gpu"])
    assert inspect.signature(batch.filter_files).parameters["png_decoder"].default == "host"
    assert inspect.signature(batch.decompose_files).parameters["png_decoder"].default == "host"
    with pytest.raises(ValueError):
        batch.decompose_files([], "o", png_decoder="gpu")
    with pytest.raises(ValueError):
        batch.filter_files("guided", [], None, 7.0, 52.0, "o", png_decoder="gpu")


def test_the_io_thread_falls_back_to_imread(tmp_path):
    """What `load` hands over for the device decoder: the parsed file where the parser takes it, the
    decoded array for an interlaced file or another extension, imread's error for a broken one."""
    rng = np.random.default_rng(6300)
    rows = ps.samples(rng, 5, 6, 8, 2)
    good = str(tmp_path / "good.png")
    with open(good, "wb") as fh:
        fh.write(ps.write_png(rows, 6, 8, 2, [4] * 5))
    got = batch._read_for_device(good)
    assert isinstance(got, tuple) and got[:4] == (5, 6, 8, 2)
    pytest.importorskip("PIL")
    from PIL import Image
    img = rng.integers(0, 256, (5, 6, 3)).astype(np.uint8)
    laced = str(tmp_path / "laced.png")
    bmp = str(tmp_path / "plain.bmp")
    # Pillow writes no interlaced files: Adam7 of a 1x1 image is its one pixel, so set the flag by hand
    one = ps.write_png(img[:1, :1].reshape(1, 3), 1, 8, 2, [0], interlace=1)
    with open(laced, "wb") as fh:
        fh.write(one)
    Image.fromarray(img).save(bmp)
    for name, want in ((laced, img[:1, :1, ::-1]), (bmp, img[:, :, ::-1])):
        got = batch._read_for_device(name)
        assert isinstance(got, np.ndarray) and np.array_equal(got, want)
    broken = str(tmp_path / "broken.png")
    with open(broken, "wb") as fh:
        fh.write(open(good, "rb").read()[:50])
    with pytest.raises(Exception) as err:
        batch._read_for_device(broken)
    assert "not readable" in str(err.value)
    with pytest.raises(Exception) as err:
        batch._read_for_device(str(tmp_path / "absent.png"))
    assert "not readable" in str(err.value)


def test_the_operator_raises_without_a_gpu(built, monkeypatch):
    """No CPU fallback: like the other operators, the decoder raises where no device is visible."""
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    parsed = iu.png_parse(iu._png_encode(np.zeros((4, 5, 3), np.uint8)))
    assert parsed is not None
    with pytest.raises(_ffi.RFError):
        ops.png_decode_ragged_u8([parsed])
    with pytest.raises(_ffi.RFError):
        ops.png_decode_ragged_u8([])
