"""GPU suite: the device half of the PNG decoder (rf_png_unfilter_ragged_u8,
ops.png_decode_ragged_u8) and the batch tools with png_decoder="device".

Expected pixels are always image_utils.imread of the same bytes written to a file, and
image_utils._png_decode of them; equality is exact.

  filters       each of the five filter types on all rows and a seeded random type per row, for every
                supported format (bytes per pixel 1, 2, 3, 4, 6, 8), at 1x1, 1x70, 70x1, 65x3 (two
                blocks of rows, rows shorter than the skew) and 130x70 (three blocks, rows longer
                than the skew) - and one tall image whose blocks go twice round the workgroup's waves
  writers       Pillow's and the built-in encoder's files of two synthetic pictures
  one list      mixed formats and sizes in one call: guard bytes, order, a second run
  grey flag     colour type 0, RGB with equal channels, one sample changed in the last pixel, a grey
                palette
  bad filter    a filter byte 5 handed to the entry directly: the image's bad bit, exact neighbours
  capture       refused on a capturing stream, nothing enqueued
  batch tools   filter_files / decompose_files with png_decoder="device" against the default run
"""
import ctypes
import io
import os
import struct
import zlib

import numpy as np
import pytest

from tests import png_synth as ps
from tests import synth
from tests.test_gpu_fuzz import env  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 4096, 0xA5
SHAPES = ((1, 1), (1, 70), (70, 1), (65, 3), (130, 70))
MODES = (0, 1, 2, 3, 4, "random")


def _expected(data, path):
    """The pixels of a file: imread's, which the built-in reader has to agree with."""
    from reflectance_filtering_amd import image_utils as iu
    with open(path, "wb") as fh:
        fh.write(data)
    want = iu.imread(path)
    assert np.array_equal(iu._png_decode(data), want)
    return want


def _file(rng, h, w, depth, ctype, mode, **kw):
    rows = ps.samples(rng, h, w, depth, ctype, palette_len=200)
    palette = rng.integers(0, 256, (200, 3)).astype(np.uint8) if ctype == 3 else None
    return ps.write_png(rows, w, depth, ctype, ps.filters_for(mode, h, rng), palette, **kw)


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """Every (format, shape, filter mode) file with its expected pixels, made once."""
    d = tmp_path_factory.mktemp("png_decode")
    rng = np.random.default_rng(6500)
    files = {}
    for depth, ctype in ps.FORMATS:
        for h, w in SHAPES:
            for mode in MODES:
                data = _file(rng, h, w, depth, ctype, mode, idat_chunks=1 + (h + w) % 3)
                files[(depth, ctype, h, w, mode)] = (data, _expected(data, str(d / "x.png")))
    return files


def _decode(rf, datas):
    from reflectance_filtering_amd import image_utils as iu
    parsed = [iu.png_parse(d) for d in datas]
    assert all(p is not None for p in parsed)
    images, grey = rf.ops.png_decode_ragged_u8(parsed)
    return [t.cpu().numpy() for t in images], grey


@pytest.mark.parametrize("depth,ctype", ps.FORMATS)
def test_every_filter_type_at_every_shape(env, corpus, depth, ctype):
    rf, co, torch = env
    keys = [(depth, ctype, h, w, mode) for h, w in SHAPES for mode in MODES]
    got, grey = _decode(rf, [corpus[k][0] for k in keys])
    for k, g in zip(keys, got):
        want = corpus[k][1]
        assert g.shape == want.shape and g.dtype == np.uint8, k
        assert np.array_equal(g, want), (k, np.argwhere(g != want)[:4])
    for k, g in zip(keys, grey):
        want = corpus[k][1]
        assert g == bool((want[..., 0] == want[..., 1]).all() and (want[..., 1] == want[..., 2]).all()), k


def test_blocks_twice_round_the_waves(env, tmp_path):
    """1100 rows are 18 blocks of 63 for a workgroup of 16 waves: the first two waves take a second
    block.  1100 x 1300 has more groups per block than 16 times the waves' lag (a wave goes from one
    block straight to its next), the narrow ones fewer.  (The wide one against imread alone: the
    built-in reader walks it byte by byte.)"""
    rf, co, torch = env
    from reflectance_filtering_amd import image_utils as iu
    rng = np.random.default_rng(6600)
    datas = [_file(rng, 1100, 5, 8, 0, "random"), _file(rng, 1100, 1300, 8, 0, "random"),
             _file(rng, 1100, 9, 16, 6, 4)]
    got, _ = _decode(rf, datas)
    for i, (g, data) in enumerate(zip(got, datas)):
        if i == 1:
            with open(str(tmp_path / "wide.png"), "wb") as fh:
                fh.write(data)
            want = iu.imread(str(tmp_path / "wide.png"))
        else:
            want = _expected(data, str(tmp_path / "x.png"))
        assert np.array_equal(g, want), (i, np.argwhere(g != want)[:4])


def test_files_of_pillow_and_of_the_built_in_encoder(env, tmp_path):
    rf, co, torch = env
    from PIL import Image
    from reflectance_filtering_amd import image_utils as iu
    scene = synth.scene_u8(48, 70, 6701)
    grey = synth.reflectance_like_u8(48, 70, 6702)
    datas = [iu._png_encode(scene), iu._png_encode(grey[:, :, 0]), iu._png_encode(grey)]
    for arr in (np.ascontiguousarray(scene[:, :, ::-1]), grey[:, :, 0],
                np.ascontiguousarray(grey), grey[:, :, 0].astype(np.uint16) * 256 + 3):
        buf = io.BytesIO()
        Image.fromarray(arr).save(buf, format="PNG")
        datas.append(buf.getvalue())
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(scene[:, :, ::-1])).quantize(64).save(buf, format="PNG")
    datas.append(buf.getvalue())
    got, flags = _decode(rf, datas)
    for i, (g, data) in enumerate(zip(got, datas)):
        assert np.array_equal(g, _expected(data, str(tmp_path / "x.png"))), i
    assert np.array_equal(got[0], scene) and np.array_equal(got[3], scene)
    assert np.array_equal(got[1], grey) and np.array_equal(got[4], grey)
    assert flags == [False, True, True, False, True, True, True, False]


def _raw_call(rf, torch, parsed, guard=GUARD):
    """The entry itself on a list of (h, w, depth, ctype, palette, raw): returns (call(stream pointer) ->
    return code, images buffer with its guards, flags buffer with its guards, the arrays kept alive)."""
    lib = rf._ffi.load_library()
    n = len(parsed)
    hs = np.array([p[0] for p in parsed], np.int32)
    wd = np.array([p[1] for p in parsed], np.int32)
    fm = np.array([(p[2] << 8) | p[3] for p in parsed], np.int32)
    offs = np.zeros(n + 1, np.uint64)
    offs[1:] = np.cumsum([len(p[5]) for p in parsed])
    raw = torch.from_numpy(np.frombuffer(b"".join(p[5] for p in parsed), np.uint8).copy()).cuda()
    pal = np.zeros((n, 768), np.uint8)
    for i, p in enumerate(parsed):
        if p[4] is not None:
            pal[i, :p[4].size] = np.asarray(p[4]).reshape(-1)
    pal = torch.from_numpy(pal).cuda()
    npx = int((hs.astype(np.int64) * wd).sum())
    images = torch.full((guard + 3 * npx + guard,), SENTINEL, dtype=torch.uint8, device="cuda")
    flags = torch.full((guard + n + guard,), SENTINEL, dtype=torch.uint8, device="cuda")
    need = lib.rf_png_unfilter_workspace_bytes(n, hs.ctypes.data, wd.ctypes.data, fm.ctypes.data)
    ws = torch.zeros(max(need, 1), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    keep = (raw, pal, ws, hs, wd, fm, offs)

    def call(stream):
        return lib.rf_png_unfilter_ragged_u8(raw.data_ptr(), offs.ctypes.data, n, hs.ctypes.data,
                                             wd.ctypes.data, fm.ctypes.data, pal.data_ptr(),
                                             images.data_ptr() + guard, flags.data_ptr() + guard,
                                             ws.data_ptr(), need, ctypes.c_void_p(stream))

    return call, images, flags, keep


def _split(images, parsed, guard=GUARD):
    data = images.cpu().numpy()
    assert (data[:guard] == SENTINEL).all() and (data[-guard:] == SENTINEL).all()
    out, at = [], guard
    for p in parsed:
        out.append(data[at:at + 3 * p[0] * p[1]].reshape(p[0], p[1], 3))
        at += 3 * p[0] * p[1]
    assert at == data.size - guard
    return out


def test_one_list_of_mixed_formats_guards_order_and_a_second_run(env, corpus):
    rf, co, torch = env
    from reflectance_filtering_amd import image_utils as iu
    keys = [(8, 2, 130, 70, "random"), (16, 0, 1, 1, 3), (8, 3, 65, 3, 4), (16, 6, 130, 70, 4),
            (8, 0, 70, 1, 2), (8, 4, 1, 70, 1), (16, 2, 65, 3, "random"), (8, 6, 130, 70, 3),
            (16, 4, 1, 70, 0), (8, 0, 130, 70, 4)]
    parsed = [iu.png_parse(corpus[k][0]) for k in keys]
    current = torch.cuda.current_stream().cuda_stream

    def run(order):
        call, images, flags, keep = _raw_call(rf, torch, [parsed[i] for i in order])
        assert call(current) == rf._ffi.RF_OK
        torch.cuda.synchronize()
        fl = flags.cpu().numpy()
        assert (fl[:GUARD] == SENTINEL).all() and (fl[-GUARD:] == SENTINEL).all()
        return _split(images, [parsed[i] for i in order]), fl[GUARD:-GUARD]

    order = list(range(len(keys)))
    first, fl = run(order)
    for k, g, f in zip(keys, first, fl):
        want = corpus[k][1]
        assert np.array_equal(g, want), k
        assert f == (1 if k[1] in (0, 4) else 0), k
    again, fl2 = run(order)
    assert all(np.array_equal(a, b) for a, b in zip(first, again)) and np.array_equal(fl, fl2)
    rng = np.random.default_rng(6800)
    for other in (order[::-1], [int(v) for v in rng.permutation(len(keys))]):
        got, fl3 = run(other)
        for i, g, f in zip(other, got, fl3):
            assert np.array_equal(g, first[i]) and f == fl[i], keys[i]


def test_grey_flag(env):
    rf, co, torch = env
    rng = np.random.default_rng(6900)
    h, w = 70, 65            # 4550 pixels: two workgroups of the unpack kernel
    g = rng.integers(0, 256, (h, w)).astype(np.uint8)
    rgb = np.repeat(g[:, :, None], 3, axis=2).reshape(h, 3 * w)
    one_off = rgb.copy()
    one_off[-1, -1] ^= 1     # one sample of the last pixel of the last row
    first_off = rgb.copy()
    first_off[0, 1] ^= 128
    grey_pal = np.repeat(rng.integers(0, 256, (256, 1)), 3, axis=1).astype(np.uint8)
    colour_pal = grey_pal.copy()
    colour_pal[g[-1, -1], 2] ^= 1
    rgba = np.concatenate([np.repeat(g[:, :, None], 3, axis=2), rng.integers(0, 256, (h, w, 1))],
                          axis=2).astype(np.uint8).reshape(h, 4 * w)
    f = ps.filters_for("random", h, rng)
    datas = [ps.write_png(g, w, 8, 0, f), ps.write_png(rgb, w, 8, 2, f), ps.write_png(one_off, w, 8, 2, f),
             ps.write_png(g, w, 8, 3, f, palette=grey_pal), ps.write_png(g, w, 8, 3, f, palette=colour_pal),
             ps.write_png(first_off, w, 8, 2, f), ps.write_png(rgba, w, 8, 6, f)]
    got, flags = _decode(rf, datas)
    assert flags == [True, True, False, True, False, False, True]
    assert np.array_equal(got[1], got[0]) and not np.array_equal(got[2], got[0])
    assert (got[2] != got[0]).sum() == 1 and got[2][-1, -1, 0] != got[0][-1, -1, 0]   # B is the last sample
    assert np.array_equal(got[3], grey_pal[g][:, :, ::-1])
    assert np.array_equal(got[6], got[0])


def test_a_filter_byte_five_sets_the_bad_bit_and_nothing_else(env, corpus):
    """Input validation, not a fault: png_parse keeps such a file away from the device; handed to the
    entry directly, the image is flagged, its neighbours decode exactly and the call returns normally.
    The operator raises and names the image."""
    rf, co, torch = env
    from reflectance_filtering_amd import image_utils as iu
    keys = [(8, 2, 130, 70, 4), (8, 0, 65, 3, "random"), (16, 2, 130, 70, 3)]
    parsed = [iu.png_parse(corpus[k][0]) for k in keys]
    h, w = 65, 3
    raw = bytearray(parsed[1][5])
    raw[64 * (1 + w)] = 5                  # the one row of the second block
    bad = parsed[1][:5] + (bytes(raw),)
    call, images, flags, keep = _raw_call(rf, torch, [parsed[0], bad, parsed[2]])
    assert call(torch.cuda.current_stream().cuda_stream) == rf._ffi.RF_OK
    torch.cuda.synchronize()
    got = _split(images, parsed)
    assert np.array_equal(got[0], corpus[keys[0]][1]) and np.array_equal(got[2], corpus[keys[2]][1])
    assert np.array_equal(got[1][:64], corpus[keys[1]][1][:64])          # the rows before it
    assert np.array_equal(got[1][64, :, 0], np.frombuffer(bytes(raw), np.uint8)[64 * 4 + 1:65 * 4])
    assert flags.cpu().numpy()[GUARD:-GUARD].tolist() == [0, 3, 0]       # grey, and the bad bit
    with pytest.raises(rf._ffi.RFError) as err:
        rf.ops.png_decode_ragged_u8([parsed[0], bad, parsed[2]])
    assert "image 1" in str(err.value)


def test_the_entry_is_refused_on_a_capturing_stream(env, corpus):
    rf, co, torch = env
    from reflectance_filtering_amd import image_utils as iu
    lib = rf._ffi.load_library()
    keys = [(8, 2, 65, 3, 4), (8, 0, 1, 70, 1)]
    parsed = [iu.png_parse(corpus[k][0]) for k in keys]
    call, images, flags, keep = _raw_call(rf, torch, parsed)
    before = keep[0].clone()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        rc = call(side.cuda_stream)
    assert rc == rf._ffi.RF_E_UNSUPPORTED and b"captured" in lib.rf_last_error()
    torch.cuda.synchronize()
    assert (images == SENTINEL).all() and (flags == SENTINEL).all() and not keep[2].any()
    assert torch.equal(keep[0], before)                                  # nothing was enqueued
    assert call(side.cuda_stream) == rf._ffi.RF_OK
    torch.cuda.synchronize()
    for k, g in zip(keys, _split(images, parsed)):
        assert np.array_equal(g, corpus[k][1])


# ---- the batch tools ---------------------------------------------------------------------------------

def _same_files(dir_a, dir_b):
    names = sorted(os.listdir(dir_a))
    assert names == sorted(os.listdir(dir_b)) and names
    for name in names:
        with open(os.path.join(dir_a, name), "rb") as fa, open(os.path.join(dir_b, name), "rb") as fb:
            assert fa.read() == fb.read(), name
    return names


def _save(path, data):
    with open(path, "wb") as fh:
        fh.write(data)
    return path


def _pillow_png(arr):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, format="PNG")
    return buf.getvalue()


def _interlaced(arr):
    """An Adam7 file of arr (RGB), written with the pass geometry of the PNG specification."""
    h, w = arr.shape[:2]
    raw = b""
    for y0, x0, dy, dx in ((0, 0, 8, 8), (0, 4, 8, 8), (4, 0, 8, 4), (0, 2, 4, 4), (2, 0, 4, 2), (0, 1, 2, 2),
                           (1, 0, 2, 1)):
        sub = arr[y0::dy, x0::dx]
        if sub.shape[0] and sub.shape[1]:
            raw += ps.filter_rows(sub.reshape(sub.shape[0], -1), 3, [1] * sub.shape[0])
    return (ps.SIG + ps.chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 1))
            + ps.chunk(b"IDAT", zlib.compress(raw)) + ps.chunk(b"IEND", b""))


def test_filter_files_with_the_device_decoder(env, tmp_path):
    rf, co, torch = env
    from reflectance_filtering_amd import batch
    from reflectance_filtering_amd import image_utils as iu
    shapes = [(43, 64), (64, 43), (48, 64), (64, 43), (43, 64), (48, 64), (70, 50)]
    src, pho, out_dev, out_host = (tmp_path / d for d in ("in", "photos", "device", "host"))
    for d in (src, pho, out_dev, out_host):
        d.mkdir()
    rng = np.random.default_rng(7000)
    inputs = []
    for i, (h, w) in enumerate(shapes):
        grey = synth.reflectance_like_u8(h, w, 7010 + i)[:, :, 0]
        photo = np.ascontiguousarray(synth.scene_u8(h, w, 7030 + i)[:, :, ::-1])     # RGB
        if i % 3 == 0:      # the built-in encoder, a Pillow photo
            data, gdata = iu._png_encode(grey), _pillow_png(photo)
        elif i % 3 == 1:    # Pillow (grey as RGB), a 16-bit photo with every filter type
            data = _pillow_png(np.repeat(grey[:, :, None], 3, axis=2))
            wide = np.stack([photo, rng.integers(0, 256, photo.shape).astype(np.uint8)], axis=3)
            gdata = ps.write_png(wide.reshape(h, -1), w, 16, 2, ps.filters_for("random", h, rng), idat_chunks=3)
        else:               # 16-bit grey, an interlaced photo: the fallback
            data = _pillow_png(grey.astype(np.uint16) * 256 + 77)
            gdata = _interlaced(photo)
            assert iu.png_parse(gdata) is None
        inputs.append(_save(str(src / ("%03d-r.png" % i)), data))
        _save(str(pho / ("%03d.png" % i)), gdata)
    runs = (("bilateral", str(pho / "{base}.png"), 20.0, 3.0, 1),     # colour guidance, ragged
            ("bilateral", None, 20.0, 3.0, 2),                         # the input guides itself
            ("guided", str(pho / "{base}.png"), 7.0, 52.0, 1),         # grey sources, ragged
            ("guided", None, 7.0, 52.0, 1))
    for k, (ftype, gui, sc, ss, it) in enumerate(runs):
        a, b = out_host / str(k), out_dev / str(k)
        a.mkdir()
        b.mkdir()
        host = batch.filter_files(ftype, inputs, gui, sc, ss, str(a), iterations=it, rank=0, world=1)
        dev = batch.filter_files(ftype, inputs, gui, sc, ss, str(b), iterations=it, rank=0, world=1,
                                 png_decoder="device")
        assert [os.path.basename(f) for f in dev] == [os.path.basename(f) for f in host]
        assert len(_same_files(str(a), str(b))) == len(shapes)
    # one shape: the batch route, colour sources (the photos filter themselves) and both codecs on the device
    uniform = [str(pho / ("%03d.png" % i)) for i in (0, 4)] + [inputs[0], inputs[4]]
    for ftype, sc, ss in (("bilateral", 20.0, 3.0), ("guided", 7.0, 52.0)):
        a, b = out_host / ("u" + ftype), out_dev / ("u" + ftype)
        a.mkdir()
        b.mkdir()
        batch.filter_files(ftype, uniform, None, sc, ss, str(a), rank=0, world=1, png_encoder="device")
        batch.filter_files(ftype, uniform, None, sc, ss, str(b), rank=0, world=1, png_encoder="device",
                           png_decoder="device")
        _same_files(str(a), str(b))
    with pytest.raises(ValueError):
        batch.filter_files("guided", inputs, None, 7.0, 52.0, str(out_dev), png_decoder="gpu")


def test_decompose_files_with_the_device_decoder(env, tmp_path):
    rf, co, torch = env
    from reflectance_filtering_amd import batch
    from reflectance_filtering_amd import image_utils as iu
    shapes = [(43, 64), (64, 43), (48, 64), (64, 43), (43, 64)]
    src, out_dev, out_host = (tmp_path / d for d in ("in", "device", "host"))
    for d in (src, out_dev, out_host):
        d.mkdir()
    rng = np.random.default_rng(7100)
    inputs = []
    for i, (h, w) in enumerate(shapes):
        photo = synth.scene_u8(h, w, 7110 + i)
        rgb = np.ascontiguousarray(photo[:, :, ::-1])
        if i == 0:
            data = iu._png_encode(photo)
        elif i == 1:
            data = _pillow_png(rgb)
        elif i == 2:
            data = ps.write_png(np.concatenate([rgb, rgb[:, :, :1]], axis=2).reshape(h, -1), w, 8, 6,
                                ps.filters_for("random", h, rng), ancillary=True, idat_chunks=2)
        elif i == 3:
            data = _interlaced(rgb)
        else:
            data = _pillow_png(rgb)
        inputs.append(_save(str(src / ("%03d.png" % i)), data))
    host = batch.decompose_files(inputs, str(out_host), rank=0, world=1)
    dev = batch.decompose_files(inputs, str(out_dev), rank=0, world=1, png_decoder="device")
    assert [os.path.basename(f) for f in dev] == [os.path.basename(f) for f in host]
    assert len(_same_files(str(out_dev), str(out_host))) == 3 * len(shapes)
    # a step of one shape: the batch call
    a, b = out_host / "u", out_dev / "u"
    a.mkdir()
    b.mkdir()
    batch.decompose_files([inputs[1], inputs[3]], str(a), rank=0, world=1)
    batch.decompose_files([inputs[1], inputs[3]], str(b), rank=0, world=1, png_decoder="device")
    assert len(_same_files(str(a), str(b))) == 6
