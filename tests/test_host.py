"""CPU suite, part 2: the host-side mirror of the reference's Python API against golden
vectors captured from the reference itself (tests/golden/make_golden.py)."""
import json
import os
import types

import numpy as np
import pytest

import reflectance_filtering_amd as rf
from reflectance_filtering_amd import decompose_with_trained_CNN as dc
from reflectance_filtering_amd import filter_reflectance as fr
from reflectance_filtering_amd import image_utils as iu

G = os.path.join(os.path.dirname(__file__), "golden")


def test_colour_curves_bitwise():
    g = np.load(os.path.join(G, "colour_tables.npz"))
    assert np.array_equal(iu.srgb_to_rgb(g["levels"]), g["srgb_to_rgb_levels"])
    assert np.array_equal(iu.rgb_to_srgb(g["levels"]), g["rgb_to_srgb_levels"])
    assert np.array_equal(iu.srgb_to_rgb(g["extra"]), g["srgb_to_rgb_extra"])
    assert np.array_equal(iu.rgb_to_srgb(g["extra"]), g["rgb_to_srgb_extra"])
    f32 = iu.srgb_to_rgb(g["levels"].astype(np.float32))
    assert f32.dtype == np.float32 and np.array_equal(f32, g["srgb_to_rgb_levels_f32"])
    assert abs(float(iu.rgb_to_srgb(np.array([1.0]))[0]) - 0.9676) < 1e-4  # the kept quirk
    assert np.array_equal(iu.srgb_byte_lut(), g["srgb_to_rgb_levels"].astype(np.float32))


def test_normalize_colorize_bitwise():
    g = np.load(os.path.join(G, "normalize_colorize.npz"))
    assert np.array_equal(iu.normalize(g["img_small"]), g["normalize_small"])
    assert np.array_equal(iu.normalize(g["img_big"]), g["normalize_big"])
    n32 = iu.normalize(g["img_big_f32"])
    assert n32.dtype == np.float32 and np.array_equal(n32, g["normalize_big_f32"])
    keep = g["img_big"].copy()
    iu.normalize(keep)
    assert np.array_equal(keep, g["img_big"]), "normalize must not modify its argument"
    refl, shad = iu.colorize(g["inten16"], g["bgr16"])
    assert np.array_equal(refl, g["colorize_reflectance"])
    assert np.array_equal(shad, g["colorize_shading"])


def test_imwrite_conversion_and_roundtrip(tmp_path):
    g = np.load(os.path.join(G, "normalize_colorize.npz"))
    cases = (("small_lin", g["img_small"], False), ("small_srgb", g["img_small"], True),
             ("big_lin", g["img_big"], False), ("big_srgb", g["img_big"], True),
             ("big32_lin", g["img_big_f32"], False),
             ("refl_srgb", g["colorize_reflectance"], True),
             ("shad_srgb", g["colorize_shading"], True), ("u8_passthrough", g["bgr16"], False),
             ("inten_lin", g["inten16"], False))
    for tag, arr, srgb in cases:
        path = str(tmp_path / (tag + ".png"))
        iu.imwrite(path, arr, sRGB=srgb)
        want = g["imwrite_" + tag]
        back = iu.imread(path)                      # always uint8 HxWx3 BGR, gray replicated
        assert back.dtype == np.uint8 and back.shape == want.shape[:2] + (3,)
        want3 = want if want.ndim == 3 else np.repeat(want[:, :, None], 3, axis=2)
        assert np.array_equal(back, want3), tag


def test_imread_imwrite_errors(tmp_path):
    with pytest.raises(Exception) as e:
        iu.imread(str(tmp_path / "missing.png"))
    assert str(e.value) == "Input image not readable: {}".format(tmp_path / "missing.png")
    bad = str(tmp_path / "no_such_dir" / "x.png")
    with pytest.raises(Exception) as e:
        iu.imwrite(bad, np.zeros((2, 2), np.uint8))
    assert str(e.value) == "Not able to write {}, does the folder exist?".format(bad)


def test_builtin_png_codec_roundtrip(tmp_path):
    rng = np.random.default_rng(0)
    bgr = rng.integers(0, 256, (13, 17, 3), dtype=np.uint8)
    gray = rng.integers(0, 256, (13, 17), dtype=np.uint8)
    assert np.array_equal(iu._png_decode(iu._png_encode(bgr)), bgr)
    assert np.array_equal(iu._png_decode(iu._png_encode(gray)), np.repeat(gray[:, :, None], 3, 2))
    if iu._PILImage is not None:  # Pillow's adaptive filters through the built-in decoder
        p = str(tmp_path / "pil.png")
        iu._PILImage.fromarray(bgr[:, :, ::-1].copy()).save(p)
        with open(p, "rb") as fh:
            assert np.array_equal(iu._png_decode(fh.read()), bgr)


def test_caffe_blob_helpers():
    g = np.load(os.path.join(G, "caffe_blob.npz"))
    blob = dc.imgCV2_to_caffeBlob(g["bgr8"])
    assert blob.dtype == np.float64 and np.array_equal(blob, g["blob8"])
    assert np.array_equal(dc.imgCV2_to_caffeBlob(g["ramp"]), g["blob_ramp"])
    ok = dc.caffeBlob_to_imgGrayLinear(np.arange(12, dtype=np.float32).reshape(1, 1, 3, 4))
    assert np.array_equal(ok, g["gray_ok"])
    for shp, msg in zip(((2, 1, 3, 4), (1, 3, 3, 4)), g["shape_errors"]):
        with pytest.raises(ValueError) as e:
            dc.caffeBlob_to_imgGrayLinear(np.zeros(shp, np.float32))
        assert str(e.value) == str(msg)


def _pb_varint(v):
    out = bytearray()
    while True:
        b = v & 0x7F
        v >>= 7
        out.append(b | (0x80 if v else 0))
        if not v:
            return bytes(out)


def _pb_field(field, wtype, payload):
    key = _pb_varint(field << 3 | wtype)
    if wtype == 2:
        return key + _pb_varint(len(payload)) + payload
    return key + payload


def _pb_blob(arr, packed=True):
    """BlobProto: shape = 7 {dim = 1, packed}, data = 5 (packed float, or repeated fixed32)."""
    dims = b"".join(_pb_varint(d) for d in arr.shape)
    body = _pb_field(7, 2, _pb_field(1, 2, dims))
    flat = np.ascontiguousarray(arr, dtype="<f4").reshape(-1)
    if packed:
        body += _pb_field(5, 2, flat.tobytes())
    else:
        body += b"".join(_pb_field(5, 5, flat[i:i + 1].tobytes()) for i in range(flat.size))
    return body


def _caffemodel_bytes(flat):
    """A NetParameter (layer = 100; name = 1, blobs = 7) holding `flat` in the decoder's layout,
    with a blob-less input layer and an unrelated field in front, as Caffe writes them."""
    msg = _pb_field(1, 2, b"ReflectanceNet")
    msg += _pb_field(100, 2, _pb_field(1, 2, b"data") + _pb_field(2, 2, b"Input"))
    pos = 0
    for i, name in enumerate(rf.weights.CONV_LAYERS):
        wshape, bshape = rf.weights._EXPECTED_SHAPES[name]
        nw, nb = int(np.prod(wshape)), int(np.prod(bshape))
        wgt = flat[pos:pos + nw].reshape(wshape)
        bias = flat[pos + nw:pos + nw + nb].reshape(bshape)
        pos += nw + nb
        layer = _pb_field(1, 2, name.encode()) + _pb_field(2, 2, b"Convolution")
        layer += _pb_field(7, 2, _pb_blob(wgt, packed=i != 1)) + _pb_field(7, 2, _pb_blob(bias))
        msg += _pb_field(100, 2, layer)
    assert pos == flat.size
    return msg


def test_caffemodel_decoder_and_shipped_weights(tmp_path):
    g = np.load(os.path.join(G, "cnn_forward.npz"))
    shipped = rf.weights.load_weights()
    assert shipped.dtype == np.float32 and np.array_equal(shipped, g["weights"])
    # the decoder on a NetParameter encoded here from the shipped weights (packed and unpacked
    # float data, a layer without blobs, fields it must skip)
    model = tmp_path / "learned_weights.caffemodel"
    model.write_bytes(_caffemodel_bytes(shipped))
    assert np.array_equal(rf.weights.load_weights(str(model)), shipped)
    layers = rf.weights.read_caffemodel(str(model))
    assert set(layers) == set(rf.weights.CONV_LAYERS)
    assert layers["conv1"][0].shape == (32, 32, 1, 1) and layers["fuse_skip_layers"][1].shape == (1,)


def test_reflectance_net_blob_to_bytes_roundtrip():
    g = np.load(os.path.join(G, "cnn_forward.npz"))
    net = dc.ReflectanceNet()
    net.blobs["images"].reshape(1, 3, 32, 32)
    net.blobs["images"].data[...] = dc.imgCV2_to_caffeBlob(g["bgr32"])
    assert np.array_equal(net.blobs["images"].data, g["blob32"])
    assert np.array_equal(net._blob_to_bytes()[0], g["bgr32"])
    net.blobs["images"].data[0, 0, 0, 0] = 0.123456  # not an sRGB byte level
    with pytest.raises(ValueError):
        net._blob_to_bytes()


class _Recorder(object):
    def __init__(self):
        self.calls = []

    def jointBilateralFilter(self, *a, **k):
        self.calls.append(("jbf", a, k))
        return np.full_like(a[1], 7)

    def guidedFilter(self, *a, **k):
        self.calls.append(("gf", a, k))
        return np.full_like(k["src"], 9)


def test_apply_filter_plumbing_matches_reference(monkeypatch):
    with open(os.path.join(G, "cli_plumbing.json")) as fh:
        gold = json.load(fh)
    rec = _Recorder()
    monkeypatch.setattr(fr, "ximgproc", rec)
    a = np.full((4, 5, 3), 0x11, np.uint8)
    b = np.full((4, 5, 3), 0x22, np.uint8)
    out = fr.apply_filter("bilateral", a, b, 20, 22)
    kind, args, kwargs = rec.calls[-1]
    gcall = gold["apply_filter_bilateral"]["calls"][0]
    assert kind == "jbf" and args[0] is b and args[1] is a      # (joint, image) positional
    assert kwargs == gcall[2] == {"d": -1, "sigmaColor": 20, "sigmaSpace": 22}
    assert int(out[0, 0, 0]) == gold["apply_filter_bilateral"]["result_fill"]
    out = fr.apply_filter("guided", a, b, 3.0, 45.9)
    kind, args, kwargs = rec.calls[-1]
    gcall = gold["apply_filter_guided"]["calls"][0]
    assert kind == "gf" and args == () and kwargs["guide"] is b and kwargs["src"] is a
    assert kwargs["radius"] == gcall[2]["radius"] == 45 and kwargs["eps"] == gcall[2]["eps"] == 3.0
    for key, args in (("sigma_color_zero", ("bilateral", a, b, 0, 22)),
                      ("sigma_spatial_negative", ("guided", a, b, 3, -1)),
                      ("bad_type", ("median", a, b, 3, 3))):
        with pytest.raises(ValueError) as e:
            fr.apply_filter(*args)
        assert [type(e.value).__name__, str(e.value)] == gold["apply_filter_errors"][key]


def test_read_filter_write_names_and_errors(monkeypatch, tmp_path):
    with open(os.path.join(G, "cli_plumbing.json")) as fh:
        gold = json.load(fh)
    monkeypatch.setattr(fr, "ximgproc", _Recorder())
    img = np.full((4, 5, 3), 0x11, np.uint8)
    src = str(tmp_path / "photo.final.png")
    gui = str(tmp_path / "guide.png")
    iu.imwrite(src, img)
    iu.imwrite(gui, img)
    out_dir = tmp_path / "dir"
    out_dir.mkdir()
    for tag, (ftype, sc, ss) in {"int_like": ("bilateral", 20.0, 22.0),
                                 "fractional": ("guided", 3.5, 45.25),
                                 "python_int": ("guided", 7, 52)}.items():
        res = fr.read_filter_write(ftype, src, gui, sc, ss, str(out_dir))
        want = os.path.basename(gold["read_filter_write"][tag]["written"][0])
        assert os.path.exists(str(out_dir / want)), want
        assert np.array_equal(iu.imread(str(out_dir / want)), res)
    with pytest.raises(Exception) as e:
        fr.read_filter_write("guided", str(tmp_path / "missing.png"), gui, 3.0, 45.0, str(out_dir))
    assert str(e.value).startswith("Input image not readable: ")
    with pytest.raises(Exception) as e:
        fr.read_filter_write("guided", src, gui, 3.0, 45.0, str(tmp_path / "nonexistent"))
    assert "does the folder exist?" in str(e.value)
    assert "photo.final_guided_c3.0s45.0.png" in str(e.value)


def test_cli_without_arguments_prints_help_and_hints(capsys):
    assert fr.main([]) == 0
    out = capsys.readouterr().out
    assert "--filter_type=bilateral --sigma_color=20 --sigma_spatial=22" in out
    assert "--filter_type=guided --sigma_color=7 --sigma_spatial=52" in out
    assert "--filter_type=guided --sigma_color=3 --sigma_spatial=45" in out
    for flag in ("--filename_in", "--guidance_in", "--path_out", "--sigma_color",
                 "--sigma_spatial", "--filter_type"):
        assert flag in out
    assert dc.main([]) == 0
    assert "--filename_in" in capsys.readouterr().out


def test_decompose_image_outputs_match_reference(monkeypatch, tmp_path):
    """decompose_image with the network output injected: file names and all three PNGs must
    equal what the reference wrote (captured with the same injected output)."""
    d = np.load(os.path.join(G, "decompose_outputs.npz"))
    src = str(tmp_path / "scene.01.png")
    iu.imwrite(src, d["scene"])

    class FakeNet(dc.ReflectanceNet):
        def forward(self):
            self.blobs["reflectance_intensity"].data = d["r"][np.newaxis, np.newaxis]

    monkeypatch.setattr(dc, "ReflectanceNet", FakeNet)
    r = dc.decompose_image(src, str(tmp_path))
    assert np.array_equal(r, d["r"])
    for name, key in (("scene.01-r.png", "r_png"), ("scene.01-r_colorized.png", "r_colorized_png"),
                      ("scene.01-s_colorized.png", "s_colorized_png")):
        got = iu.imread(str(tmp_path / name))
        want = d[key] if d[key].ndim == 3 else np.repeat(d[key][:, :, None], 3, axis=2)
        assert np.array_equal(got, want), name


def test_batch_front_end_host_logic(tmp_path):
    from reflectance_filtering_amd import batch
    for name in ("b-r.png", "a-r.png", "c.png"):
        iu.imwrite(str(tmp_path / name), np.zeros((3, 4), np.uint8))
    files = batch.expand_inputs([str(tmp_path / "*-r.png"), str(tmp_path / "c.png"),
                                 str(tmp_path / "a-r.png"), str(tmp_path / "missing.png")])
    assert [os.path.basename(f) for f in files] == ["a-r.png", "b-r.png", "c.png"]
    assert batch.guidance_for("/x/y/118495-r.png", None) == "/x/y/118495-r.png"
    assert batch.guidance_for("/x/y/118495-r.png", "/p/{base}{ext}") == "/p/118495.png"
    assert batch.guidance_for("/x/y/img.png", "{dir}/flat/{stem}_flat{ext}") == "/x/y/flat/img_flat.png"
    items = list("abcdefg")
    parts = [batch.my_slice(items, r, 3) for r in range(3)]
    assert sum(parts, []) == items and [len(p) for p in parts] == [3, 2, 2]
    shapes = {"a": (4, 4, 3), "b": (4, 4, 3), "c": (5, 4, 3), "d": (5, 4, 3), "e": (5, 4, 3),
              "f": (4, 4, 3), "g": (4, 4, 3)}
    groups = batch.group_by_shape(items, lambda k: shapes[k], max_bytes=2 * 5 * 4 * 3)
    assert groups == [["a", "b"], ["c", "d"], ["e"], ["f", "g"]]
    assert batch.main([]) == 0


def test_no_oracle_in_product():
    """The product package must never import or load the oracle (no CPU fallback)."""
    pkg = os.path.dirname(rf.__file__)
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".cpp", ".h")):
                with open(os.path.join(root, f)) as fh:
                    text = fh.read()
                assert "oracle" not in text.replace("no oracle", ""), os.path.join(root, f)


def test_imread_16bit_png_keeps_the_high_byte_whatever_the_values(tmp_path):
    """cv2.imread(IMREAD_COLOR) reduces 16-bit samples to 8 bits by bit depth: a DARK 16-bit
    image (all values <= 255) must decode to zeros, not to its low bytes."""
    import struct
    import zlib
    from reflectance_filtering_amd import image_utils as iu

    def png16(values):
        h, w = values.shape
        raw = b"".join(b"\x00" + values[r].astype(">u2").tobytes() for r in range(h))

        def chunk(tag, body):
            return (struct.pack(">I", len(body)) + tag + body
                    + struct.pack(">I", zlib.crc32(tag + body) & 0xFFFFFFFF))
        return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 16, 0, 0, 0, 0))
                + chunk(b"IDAT", zlib.compress(raw)) + chunk(b"IEND", b""))

    dark = np.arange(12, dtype=np.uint16).reshape(3, 4) * 20          # max 220 < 256
    bright = dark * 256 + 7
    for vals in (dark, bright):
        f = tmp_path / "x.png"
        f.write_bytes(png16(vals))
        got = iu.imread(str(f))
        assert got.shape == (3, 4, 3) and got.dtype == np.uint8
        assert np.array_equal(got[:, :, 0], (vals >> 8).astype(np.uint8))


def test_batch_pipeline_orders_overlaps_and_propagates_errors(tmp_path):
    """batch.pipeline: results are written in input order whatever the step size, every file is
    loaded exactly once, and an exception of a stage surfaces in the caller."""
    import threading
    from reflectance_filtering_amd import batch, image_utils as iu
    items = list(range(11))
    seen, lock = [], threading.Lock()

    def load(i):
        with lock:
            seen.append(i)
        return i, np.full((4, 5, 3), i, np.uint8)

    def compute(loaded):
        return [(str(tmp_path / ("o%02d.png" % i)), arr + 1) for i, arr in loaded]

    for step in (1, 4, 64):
        seen.clear()
        names = batch.pipeline(items, load, compute, step=step)
        assert names == [str(tmp_path / ("o%02d.png" % i)) for i in items]
        assert sorted(seen) == items
        for i, name in zip(items, names):
            assert int(iu.imread(name)[0, 0, 0]) == i + 1
    assert batch.pipeline([], load, compute) == []

    def bad(loaded):
        raise RuntimeError("device stage failed")
    with pytest.raises(RuntimeError, match="device stage failed"):
        batch.pipeline(items, load, bad, step=3)
    with pytest.raises(ZeroDivisionError):
        batch.pipeline(items, lambda i: 1 // 0, compute, step=3)


def test_ximgproc_refuses_the_float_same_buffer_shortcut():
    """OpenCV sends jointBilateralFilter(a, a) to cv::bilateralFilter; for 8-bit images that is
    mirrored, for float32 it would be another operator (not implemented): refused before any GPU
    work, with a message that says what to do."""
    from reflectance_filtering_amd import ximgproc
    a = np.zeros((8, 8, 3), np.float32)
    with pytest.raises(ValueError, match="bilateralFilter"):
        ximgproc.jointBilateralFilter(a, a, -1, 0.1, 2.0)
    with pytest.raises(ValueError, match="bilateralFilter"):
        ximgproc.jointBilateralFilter(None, a, -1, 0.1, 2.0)
