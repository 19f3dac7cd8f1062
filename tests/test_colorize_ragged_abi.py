"""CPU suite: the ragged colourise (rf_colorize_ragged_srgb_u8: photos of different sizes packed one
after another, one chunk length per call) - the launch plan against hand-computed plans, the
workspace size, every refusal before any device work, and the Python forms without a GPU.  No
compute calls."""
import ctypes

import numpy as np
import pytest

from reflectance_filtering_amd import _ffi, ops

IIW = ((341, 512), (512, 341), (384, 512))          # 174592, 174592 and 196608 pixels
SELSTATE = 3 * 8 + 256 * 4                          # prefix, k, maxkey, hist[256]
RECORD = 40                                         # first, npx, k_refl, k_shading (u64), wg0, pad (u32)


def _ints(values):
    a = np.ascontiguousarray(values, dtype=np.int32)
    return a, a.ctypes.data


def _u64(values):
    a = np.ascontiguousarray(values, dtype=np.uint64)
    return a, a.ctypes.data


def _align256(b):
    return (b + 255) & ~255


def _running(sizes, chunk):
    counts = [-(-h * w // chunk) for h, w in sizes]
    return [sum(counts[:i]) for i in range(len(counts))], sum(counts)


def test_plan_of_one_pixel(built):
    # 1 pixel: chunks of 2048 make 1 workgroup < 1024, so 256 * max(1, ceil(1 / 262144)) = 256
    assert _ffi.colorize_ragged_plan([(1, 1)]) == (256, 1, [0])


def test_plan_of_an_iiw_step_in_both_regimes(built):
    # 16 photos, 11 of 174592 pixels (86 chunks of 2048: 85.25) and 5 of 196608 (96): 2903552 pixels,
    # m = 1, 11 * 86 + 5 * 96 = 1426 workgroups >= 1024: chunks of 2048
    step = [IIW[i % 3] for i in range(16)]
    chunk, wgs, first = _ffi.colorize_ragged_plan(step)
    assert (chunk, wgs) == (2048, 1426)
    assert first[:4] == [0, 86, 172, 268] and first == _running(step, 2048)[0]
    # its first 8 photos, 6 of 174592 and 2 of 196608: 1440768 pixels, 6 * 86 + 2 * 96 = 708 < 1024, so
    # 256 * ceil(1440768 / 262144) = 256 * 6 = 1536: 6 * 114 + 2 * 128 = 940 workgroups
    half = step[:8]
    chunk, wgs, first = _ffi.colorize_ragged_plan(half)
    assert (chunk, wgs) == (1536, 940)
    assert first[:4] == [0, 114, 228, 356] and first == _running(half, 1536)[0]


def test_plan_of_a_list_beyond_65536_chunks_of_2048(built):
    # 40000 x 1080x1920 = 82944000000 pixels: m = ceil(82944000000 / 134217728) = 618 (617.98),
    # chunks of 2048 * 618 = 1265664 pixels, 2 per image (2073600 pixels): sizes only, nothing allocated
    n = 40000
    chunk, wgs, first = _ffi.colorize_ragged_plan([(1080, 1920)] * n)
    assert (chunk, wgs) == (1265664, 80000) and wgs <= 65536 + n
    assert first == list(range(0, 2 * n, 2))


def test_the_debug_option_replaces_the_rule(built):
    sizes = [(15, 17), (16, 16), (1, 257), (16, 32), (769, 1), (64, 48)]      # 255 256 257 512 769 3072
    with _ffi.debug_options(colorize_chunk_px=256):
        assert _ffi.colorize_ragged_plan(sizes) == (256, 22, [0, 1, 2, 4, 6, 10])
    with _ffi.debug_options(colorize_chunk_px=4096):
        assert _ffi.colorize_ragged_plan(sizes) == (4096, 6, [0, 1, 2, 3, 4, 5])
        assert _ffi.colorize_ragged_plan([IIW[0]] * 2) == (4096, 86, [0, 43])
    assert _ffi.colorize_ragged_plan(sizes) == (256, 22, [0, 1, 2, 4, 6, 10])   # 5121 pixels: the rule's 256
    lib = _ffi.load_library()
    hs, p_h = _ints([15])
    ws, p_w = _ints([17])
    for bad in (300, 1, 255, 2049):
        with _ffi.debug_options(colorize_chunk_px=bad):
            with pytest.raises(ValueError) as err:
                _ffi.colorize_ragged_plan(sizes)
            assert "256" in str(err.value)
            assert lib.rf_debug_colorize_ragged_plan(1, p_h, p_w, None, 0) == _ffi.RF_E_BADARG
            assert lib.rf_colorize_ragged_workspace_bytes(1, p_h, p_w) == 0
    assert lib.rf_debug_colorize_ragged_plan(1, p_h, p_w, None, 0) == 1


def test_first_workgroups_are_the_running_sum(built):
    rng = np.random.default_rng(5)
    for chunk_opt in (0, 256, 768, 2048, 8192):
        sizes = [(int(rng.integers(1, 300)), int(rng.integers(1, 300))) for _ in range(int(rng.integers(1, 40)))]
        with _ffi.debug_options(colorize_chunk_px=chunk_opt):
            chunk, wgs, first = _ffi.colorize_ragged_plan(sizes)
        assert chunk % 256 == 0 and (chunk_opt == 0 or chunk == chunk_opt)
        want_first, want_wgs = _running(sizes, chunk)
        assert (wgs, first) == (want_wgs, want_first)
    # the plan query writes what fits `cap` ints and returns n
    lib = _ffi.load_library()
    hs, p_h = _ints([40, 40, 40])
    ws, p_w = _ints([40, 40, 40])
    out = np.full(5, -7, dtype=np.int32)
    assert lib.rf_debug_colorize_ragged_plan(3, p_h, p_w, out.ctypes.data, 3) == 3
    assert out.tolist() == [256, 21, 0, -7, -7]
    assert lib.rf_debug_colorize_ragged_plan(3, p_h, p_w, None, 1) == _ffi.RF_E_BADARG
    assert lib.rf_debug_colorize_ragged_plan(3, p_h, p_w, out.ctypes.data, -1) == _ffi.RF_E_BADARG
    assert lib.rf_debug_colorize_ragged_plan(0, None, None, None, 0) == 0


def test_workspace_is_the_image_table_plus_two_states_per_image(built):
    lib = _ffi.load_library()
    for n in (1, 6, 7, 16, 1000):
        hs, p_h = _ints([3 + i % 5 for i in range(n)])
        ws, p_w = _ints([2 + i % 7 for i in range(n)])
        got = lib.rf_colorize_ragged_workspace_bytes(n, p_h, p_w)
        assert got == _align256(RECORD * n) + n * 2 * SELSTATE
        assert got == _align256(RECORD * n) + lib.rf_colorize_workspace_bytes(n)
    assert _align256(RECORD * 6) == 256 and _align256(RECORD * 7) == 512
    hs, p_h = _ints([4, 5])
    ws, p_w = _ints([6, 7])
    # a size query that cannot answer
    assert lib.rf_colorize_ragged_workspace_bytes(0, p_h, p_w) == 0
    assert lib.rf_colorize_ragged_workspace_bytes(-1, p_h, p_w) == 0
    assert lib.rf_colorize_ragged_workspace_bytes(2, None, p_w) == 0
    assert lib.rf_colorize_ragged_workspace_bytes(2, p_h, None) == 0
    bad, p_bad = _ints([4, 0])
    assert lib.rf_colorize_ragged_workspace_bytes(2, p_bad, p_w) == 0
    big, p_big = _ints([37838, 5])
    bigw, p_bigw = _ints([37838, 7])
    assert lib.rf_colorize_ragged_workspace_bytes(2, p_big, p_bigw) == 0


def test_ragged_refusals_need_no_gpu(built):
    lib = _ffi.load_library()
    buf = ctypes.create_string_buffer(1 << 16)
    base = (ctypes.addressof(buf) + 255) & ~255
    bgr, r, ro, so, steps, wsp = (base + 4096 * i for i in range(6))
    hs, p_h = _ints([8, 3, 5])
    wd, p_w = _ints([8, 7, 2])                                 # 64, 21 and 10 pixels
    kr, p_kr = _u64([191, 62, 29])                             # the last rank inside each image
    ks, p_ks = _u64([63, 20, 9])
    need = lib.rf_colorize_ragged_workspace_bytes(3, p_h, p_w)
    assert need == 256 + 6 * SELSTATE

    def call(bgr=bgr, r=r, ro=ro, so=so, n=3, ph=p_h, pw=p_w, pkr=p_kr, pks=p_ks, steps=steps,
             ws=wsp, ws_bytes=need - 1):
        # a call that passes every argument rule ends at the workspace that is one byte short
        return lib.rf_colorize_ragged_srgb_u8(bgr, r, ro, so, n, ph, pw, pkr, pks, steps, ws, ws_bytes,
                                              None)

    def refused(code, word, **kw):
        assert call(**kw) == code, kw
        msg = lib.rf_last_error()
        assert b"rf_colorize_ragged_srgb_u8" in msg and word in msg, (kw, msg)

    refused(_ffi.RF_E_WORKSPACE, b"workspace")
    refused(_ffi.RF_E_WORKSPACE, b"workspace", ws_bytes=0)
    refused(_ffi.RF_E_WORKSPACE, b"workspace", ro=None)           # one output is enough
    refused(_ffi.RF_E_WORKSPACE, b"workspace", so=None)
    for kw in ({"bgr": None}, {"r": None}, {"steps": None}, {"ws": None}, {"ph": None}, {"pw": None},
               {"pkr": None}, {"pks": None}, {"ro": None, "so": None}):
        refused(_ffi.RF_E_BADARG, b"NULL", **kw)
    # an empty list is valid whatever the pointers are
    assert call(n=0, bgr=None, r=None, ro=None, so=None, ph=None, pw=None, ws=None) == _ffi.RF_OK
    refused(_ffi.RF_E_BADARG, b"n=-1", n=-1)
    for bad_h, bad_w in (([8, 0, 5], [8, 7, 2]), ([8, 3, 5], [8, 7, 0]), ([8, -3, 5], [8, 7, 2]),
                         ([8, 3, 5], [8, -7, 2])):
        a, p_a = _ints(bad_h)
        b, p_b = _ints(bad_w)
        refused(_ffi.RF_E_BADARG, b"size of image", ph=p_a, pw=p_b)
    # a rank outside its image, on the image in the middle: 3 * 21 = 63 values, 21 pixels
    a, p_a = _u64([191, 63, 29])
    refused(_ffi.RF_E_BADARG, b"rank outside image 1", pkr=p_a)
    a, p_a = _u64([63, 21, 9])
    refused(_ffi.RF_E_BADARG, b"rank outside image 1", pks=p_a)
    a, p_a = _u64([191, 62, 30])
    refused(_ffi.RF_E_BADARG, b"rank outside image 2", pkr=p_a)
    a, p_a = _u64([191, 64, 29])                               # inside image 0's range, not image 1's
    refused(_ffi.RF_E_BADARG, b"rank outside image 1", pkr=p_a)
    # 3 * 37838^2 = 4295142732 >= 2^32; 3 * 37837^2 = 4294915707 is below it
    z, p_z = _u64([0, 0, 0])
    a, p_a = _ints([8, 37838, 5])
    b, p_b = _ints([8, 37838, 2])
    refused(_ffi.RF_E_UNSUPPORTED, b"image 1", ph=p_a, pw=p_b, pkr=p_z, pks=p_z)
    a, p_a = _ints([8, 37837, 5])
    b, p_b = _ints([8, 37837, 2])
    refused(_ffi.RF_E_WORKSPACE, b"workspace", ph=p_a, pw=p_b, pkr=p_z, pks=p_z)
    # more workgroups than one grid of 256-thread workgroups takes (2^24 - 1 = 16777215): an image of
    # 30000x40000 in chunks of 256 pixels is 4687500 of them, so three fit and four do not; under the
    # rule four are 4 * 64 workgroups
    a, p_a = _ints([30000] * 4)
    b, p_b = _ints([40000] * 4)
    z4, p_z4 = _u64([0] * 4)
    with _ffi.debug_options(colorize_chunk_px=256):
        refused(_ffi.RF_E_WORKSPACE, b"workspace", n=3, ph=p_a, pw=p_b, pkr=p_z4, pks=p_z4)
        refused(_ffi.RF_E_UNSUPPORTED, b"workgroups", n=4, ph=p_a, pw=p_b, pkr=p_z4, pks=p_z4)
        assert lib.rf_debug_colorize_ragged_plan(4, p_a, p_b, None, 0) == _ffi.RF_E_UNSUPPORTED
    refused(_ffi.RF_E_WORKSPACE, b"workspace", n=4, ph=p_a, pw=p_b, pkr=p_z4, pks=p_z4)
    with _ffi.debug_options(colorize_chunk_px=1000):
        refused(_ffi.RF_E_BADARG, b"multiple of 256")
    refused(_ffi.RF_E_BADARG, b"aligned", ws=wsp + 8, ws_bytes=need)


def test_the_python_forms_raise_without_a_gpu(built, monkeypatch):
    """No CPU fallback: like the other operators, the list forms raise where no device is visible."""
    import torch
    import reflectance_filtering_amd as rf
    import decompose_with_trained_CNN as shim
    assert shim.decompose_list is rf.decompose_with_trained_CNN.decompose_list
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    img = torch.zeros((4, 5, 3), dtype=torch.uint8)
    with pytest.raises(_ffi.RFError):
        ops.colorize_ragged_srgb_u8([img], [torch.zeros((4, 5))])
    with pytest.raises(_ffi.RFError):
        rf.decompose_with_trained_CNN.decompose_list([img])
    with pytest.raises(_ffi.RFError):
        rf.decompose_with_trained_CNN.decompose_packed([img])
