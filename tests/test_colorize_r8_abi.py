"""CPU suite: the colourise of an 8-bit reflectance map (rf_colorize_ragged_r8_srgb_u8) - the export
and its binding, every refusal of the ragged entry before any device work, the fixture against the
numpy oracle, and the host side of `batch.py decompose_filter` (parser, output names).  No compute
calls."""
import ctypes
import os

import numpy as np
import pytest

from reflectance_filtering_amd import _ffi

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SELSTATE = 3 * 8 + 256 * 4                          # prefix, k, maxkey, hist[256]
TAGS = ("ramp", "photo", "dark", "nan")


def _ints(values):
    a = np.ascontiguousarray(values, dtype=np.int32)
    return a, a.ctypes.data


def _u64(values):
    a = np.ascontiguousarray(values, dtype=np.uint64)
    return a, a.ctypes.data


def test_the_export_is_present_and_bound(built):
    lib = _ffi.load_library()
    assert "rf_colorize_ragged_r8_srgb_u8" in _ffi.EXPORTS
    fn = lib.rf_colorize_ragged_r8_srgb_u8
    assert fn.restype is ctypes.c_int
    assert list(fn.argtypes) == list(lib.rf_colorize_ragged_srgb_u8.argtypes)
    assert len(fn.argtypes) == 13 and fn.argtypes[11] is ctypes.c_size_t


def test_every_refusal_of_the_ragged_entry_holds_and_needs_no_gpu(built):
    lib = _ffi.load_library()
    buf = ctypes.create_string_buffer(1 << 16)
    base = (ctypes.addressof(buf) + 255) & ~255
    bgr, r8, ro, so, steps, wsp = (base + 4096 * i for i in range(6))
    hs, p_h = _ints([8, 3, 5])
    wd, p_w = _ints([8, 7, 2])                                 # 64, 21 and 10 pixels
    kr, p_kr = _u64([191, 62, 29])                             # the last rank inside each image
    ks, p_ks = _u64([63, 20, 9])
    need = lib.rf_colorize_ragged_workspace_bytes(3, p_h, p_w)
    assert need == 256 + 6 * SELSTATE

    def call(bgr=bgr, r8=r8, ro=ro, so=so, n=3, ph=p_h, pw=p_w, pkr=p_kr, pks=p_ks, steps=steps,
             ws=wsp, ws_bytes=need - 1):
        # a call that passes every argument rule ends at the workspace that is one byte short
        return lib.rf_colorize_ragged_r8_srgb_u8(bgr, r8, ro, so, n, ph, pw, pkr, pks, steps, ws,
                                                 ws_bytes, None)

    def refused(code, word, **kw):
        assert call(**kw) == code, kw
        msg = lib.rf_last_error()
        assert b"rf_colorize_ragged_r8_srgb_u8" in msg and word in msg, (kw, msg)

    refused(_ffi.RF_E_WORKSPACE, b"workspace")
    refused(_ffi.RF_E_WORKSPACE, b"workspace", ws_bytes=0)
    refused(_ffi.RF_E_WORKSPACE, b"workspace", ro=None)           # one output is enough
    refused(_ffi.RF_E_WORKSPACE, b"workspace", so=None)
    for kw in ({"bgr": None}, {"r8": None}, {"steps": None}, {"ws": None}, {"ph": None}, {"pw": None},
               {"pkr": None}, {"pks": None}, {"ro": None, "so": None}):
        refused(_ffi.RF_E_BADARG, b"NULL", **kw)
    # an empty list is valid whatever the pointers are
    assert call(n=0, bgr=None, r8=None, ro=None, so=None, ph=None, pw=None, ws=None) == _ffi.RF_OK
    refused(_ffi.RF_E_BADARG, b"n=-1", n=-1)
    for bad_h, bad_w, which in (([8, 0, 5], [8, 7, 2], 1), ([8, 3, 5], [8, 7, 0], 2),
                                ([8, -3, 5], [8, 7, 2], 1), ([-8, 3, 5], [8, -7, 2], 0)):
        a, p_a = _ints(bad_h)
        b, p_b = _ints(bad_w)
        refused(_ffi.RF_E_BADARG, b"size of image %d" % which, ph=p_a, pw=p_b)
    # a rank outside its image, on the image in the middle: 3 * 21 = 63 values, 21 pixels
    a, p_a = _u64([191, 63, 29])
    refused(_ffi.RF_E_BADARG, b"rank outside image 1", pkr=p_a)
    a, p_a = _u64([63, 21, 9])
    refused(_ffi.RF_E_BADARG, b"rank outside image 1", pks=p_a)
    a, p_a = _u64([191, 62, 30])
    refused(_ffi.RF_E_BADARG, b"rank outside image 2", pkr=p_a)
    # 3 * 37838^2 = 4295142732 >= 2^32
    z, p_z = _u64([0, 0, 0])
    a, p_a = _ints([8, 37838, 5])
    b, p_b = _ints([8, 37838, 2])
    refused(_ffi.RF_E_UNSUPPORTED, b"image 1", ph=p_a, pw=p_b, pkr=p_z, pks=p_z)
    # more workgroups than one grid takes (see tests/test_colorize_ragged_abi.py)
    a, p_a = _ints([30000] * 4)
    b, p_b = _ints([40000] * 4)
    z4, p_z4 = _u64([0] * 4)
    with _ffi.debug_options(colorize_chunk_px=256):
        refused(_ffi.RF_E_UNSUPPORTED, b"workgroups", n=4, ph=p_a, pw=p_b, pkr=p_z4, pks=p_z4)
    refused(_ffi.RF_E_BADARG, b"aligned", ws=wsp + 8, ws_bytes=need)


def test_the_fixture_equals_the_oracle(built):
    """tests/golden/colorize_r8_write.npz holds the reference's bytes (make_colorize_r8.py); the numpy
    oracle on float32(byte) / float32(255) gives the same, and the fixture covers what it must."""
    from oracle import colorize_numpy as oc
    d = np.load(os.path.join(G, "colorize_r8_write.npz"))
    seen = set()
    for tag in TAGS:
        img, r8 = d[tag + "_image"], d[tag + "_r8"]
        assert img.dtype == np.uint8 and r8.dtype == np.uint8 and img.shape == r8.shape + (3,)
        r = r8.astype(np.float32) / np.float32(255)
        with np.errstate(all="ignore"):
            refl, shad = oc.colorize_srgb_u8(img, r)
        assert np.array_equal(refl, d[tag + "_refl_png"]), tag
        assert np.array_equal(shad, d[tag + "_shading_png"]), tag
        seen.update(np.unique(r8).tolist())
    assert seen == set(range(256))

    def floats(tag):
        img, r = d[tag + "_image"], d[tag + "_r8"].astype(np.float32) / np.float32(255)
        with np.errstate(all="ignore"):
            sh = img.astype(np.float64).sum(axis=2) / 3.0 / r.astype(np.float64)
            return sh, img.astype(np.float64) / np.maximum(sh, 1e-3)[:, :, None]

    sh, refl = floats("dark")                               # both branches: written as they are
    assert sh.max() <= 1 and refl.max() <= 1
    sh, refl = floats("photo")
    assert sh.max() > 1 and refl.max() > 1 and np.isfinite(sh).all()
    sh, refl = floats("ramp")                               # byte 0 under a lit pixel: shading +inf
    zero = d["ramp_r8"] == 0
    assert zero.sum() == 1 and d["ramp_image"][zero].min() > 0 and np.isposinf(sh[zero]).all()
    assert not np.isnan(sh).any() and not np.isnan(refl).any()
    sh, refl = floats("nan")                                # byte 0 under a black pixel: 0/0
    zero = d["nan_r8"] == 0
    assert zero.sum() == 1 and not d["nan_image"][zero].any()
    assert np.isnan(sh[zero]).all() and np.isnan(refl[zero]).all()
    for x in (sh, refl):                                    # below byte 256 of the unnormalised write
        x = x[~np.isnan(x)]
        assert np.isfinite(x).all()
        assert not (np.trunc((np.power(1.055 * x, 1.0 / 2.4) - 0.055) * 255) >= 256).any()


def test_the_python_forms_raise_without_a_gpu(built, monkeypatch):
    import torch
    import reflectance_filtering_amd as rf
    import decompose_with_trained_CNN as shim
    assert shim.decompose_filter_list is rf.decompose_filter_list
    assert shim.decompose_filter_packed is rf.decompose_with_trained_CNN.decompose_filter_packed
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    img = torch.zeros((4, 5, 3), dtype=torch.uint8)
    with pytest.raises(_ffi.RFError):
        rf.ops.colorize_ragged_r8_srgb_u8([img], [torch.zeros((4, 5), dtype=torch.uint8)])
    with pytest.raises(_ffi.RFError):
        rf.decompose_filter_list([img])
    with pytest.raises(ValueError):                         # the parameters are checked first
        rf.decompose_filter_packed([img], sigma_color=0)
    with pytest.raises(ValueError):
        rf.decompose_filter_packed([img], iterations=0)


def test_the_parser_accepts_decompose_filter_and_keeps_the_others():
    from reflectance_filtering_amd import batch
    parser = batch.build_parser()
    args = parser.parse_args(["decompose_filter", "--inputs", "a.png", "b.png", "--path_out", "out"])
    assert args.command == "decompose_filter" and args.inputs == ["a.png", "b.png"]
    assert (args.filter_type, args.sigma_color, args.sigma_spatial) == ("bilateral", 20.0, 22.0)
    assert (args.guidance, args.iterations, args.png_encoder, args.png_decoder) == (None, 1, "host", "host")
    args = parser.parse_args(["decompose_filter", "--inputs", "a.png", "--path_out", "out",
                              "--filter_type", "guided", "--sigma_color", "7", "--sigma_spatial", "52",
                              "--guidance", "image", "--iterations", "3", "--png_encoder", "device",
                              "--png_decoder", "device"])
    assert (args.filter_type, args.sigma_color, args.sigma_spatial) == ("guided", 7.0, 52.0)
    assert (args.guidance, args.iterations, args.png_encoder, args.png_decoder) == ("image", 3, "device",
                                                                                   "device")
    args = parser.parse_args(["decompose_filter", "--inputs", "a.png", "--path_out", "out", "--guidance",
                              "flat/{stem}.png"])
    assert args.guidance == "flat/{stem}.png"
    with pytest.raises(SystemExit):
        parser.parse_args(["decompose_filter", "--inputs", "a.png"])
    args = parser.parse_args(["filter", "--inputs", "x-r.png", "--path_out", "out", "--sigma_color", "20",
                              "--sigma_spatial", "22", "--filter_type", "bilateral"])
    assert args.command == "filter" and args.iterations == 1 and args.png_decoder == "host"
    args = parser.parse_args(["decompose", "--inputs", "x.png", "--path_out", "out"])
    assert args.command == "decompose" and args.png_encoder == "host"


def test_the_six_output_names():
    from reflectance_filtering_amd import batch
    from reflectance_filtering_amd import filter_reflectance as fr
    names = batch.decompose_filter_names("photos/x.png", "out", "bilateral", 20.0, 22.0)
    assert names == (os.path.join("out", "x-r.png"), os.path.join("out", "x-r_colorized.png"),
                     os.path.join("out", "x-s_colorized.png"),
                     os.path.join("out", "x-r_bilateral_c20.0s22.0.png"),
                     os.path.join("out", "x-r_bilateral_c20.0s22.0-r_colorized.png"),
                     os.path.join("out", "x-r_bilateral_c20.0s22.0-s_colorized.png"))
    assert names[3] == fr.output_filename(names[0], "out", "bilateral", 20.0, 22.0)
    names = batch.decompose_filter_names("/a/b/scene.01.jpg", "/o", "guided", 7.5, 52.0, iterations=2)
    assert names[:3] == ("/o/scene.01-r.png", "/o/scene.01-r_colorized.png", "/o/scene.01-s_colorized.png")
    assert names[3] == "/o/scene.01-r_guided_c7.5s52.0_guided_c7.5s52.0.png"
    assert names[3] == fr.output_filename(fr.output_filename(names[0], "/o", "guided", 7.5, 52.0), "/o",
                                          "guided", 7.5, 52.0)
    assert names[4:] == ("/o/scene.01-r_guided_c7.5s52.0_guided_c7.5s52.0-r_colorized.png",
                         "/o/scene.01-r_guided_c7.5s52.0_guided_c7.5s52.0-s_colorized.png")
    # the parameters are formatted as the command line hands them over
    assert batch.decompose_filter_names("x.png", "o", "bilateral", 20, 22)[3] == os.path.join(
        "o", "x-r_bilateral_c20s22.png")
