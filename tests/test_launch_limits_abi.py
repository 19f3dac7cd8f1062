"""CPU suite: the launch rule of the C ABI ("Sizes" in include/reflectance_filtering.h).  The runtime
supports no launch whose gridDim x blockDim reaches 2^32 work-items in a dimension (hip_runtime_api.h at
hipModuleLaunchKernel); rf::launch_fits (rf_common.hpp) is the one place that says so, and every entry or
plan query whose check needs no device refuses with RF_E_UNSUPPORTED one workgroup beyond the largest
launch it admits.  Host arrays only; a call that would be admitted is never made here (it would reach
the device), only the size and plan queries see the largest admitted list."""
import ctypes

import numpy as np
import pytest

from reflectance_filtering_amd import _ffi

MOST_1024 = (1 << 32) // 1024 - 1       # 4,194,303 workgroups of 1024 threads
MOST_256 = (1 << 32) // 256 - 1         # 16,777,215 of 256
MOST_64 = (1 << 32) // 64 - 1           # 67,108,863 of 64


def _ones(n):
    a = np.ones(n, np.int32)
    return a, a.ctypes.data


@pytest.mark.parametrize("sigma_space,query", [(22.0, "rf_debug_jbf_ragged_plan"),
                                               (36.0, "rf_debug_jbf_ragged_slab_plan")], ids=["r33", "r54-slabs"])
def test_jbf_ragged_takes_4194303_tiles_and_refuses_one_more(built, sigma_space, query):
    lib = _ffi.load_library()
    ones, p = _ones(MOST_1024 + 1)
    out = (ctypes.c_int * 16)()
    assert lib.rf_jbf_ragged_workspace_bytes(MOST_1024, p, p, 1, 1, -1, sigma_space, 0) == (32 * MOST_1024 + 255) & ~255
    assert getattr(lib, query)(MOST_1024, p, p, 1, 1, -1, 20.0, sigma_space, 0, out, 4) == 1
    assert MOST_1024 in list(out)                               # one launch of that many tiles
    assert lib.rf_jbf_ragged_workspace_bytes(MOST_1024 + 1, p, p, 1, 1, -1, sigma_space, 0) == 0
    assert b"too many tiles for one launch" in lib.rf_last_error()
    assert getattr(lib, query)(MOST_1024 + 1, p, p, 1, 1, -1, 20.0, sigma_space, 0, out, 4) == _ffi.RF_E_UNSUPPORTED
    # the entry itself, before it looks at the workspace or touches the device (the pointers are never read)
    rc = lib.rf_jbf_ragged_u8(1 << 40, 2 << 40, 3 << 40, MOST_1024 + 1, p, p, 1, 1, -1, 20.0, sigma_space, 4, 0,
                              None, 0, None)
    assert rc == _ffi.RF_E_UNSUPPORTED and b"rf_jbf_ragged_u8: too many tiles for one launch" in lib.rf_last_error()
    # fewer, larger images: the tiles count, not the images
    hs, ws = np.full(4097, 64 * 32, np.int32), np.full(4097, 64 * 32 + 1, np.int32)      # 32 x 33 tiles each
    assert lib.rf_jbf_ragged_workspace_bytes(3971, hs.ctypes.data, ws.ctypes.data, 3, 3, -1, sigma_space, 0) > 0
    assert lib.rf_jbf_ragged_workspace_bytes(3972, hs.ctypes.data, ws.ctypes.data, 3, 3, -1, sigma_space, 0) == 0


def test_jbf_two_wg_plan_stops_at_the_launch_rule(built):
    plan = _ffi.jbf_two_wg_plan(MOST_1024, 64, 64, 1, 1, -1, 20.0, 22.0)
    assert plan is not None and plan[1] == MOST_1024
    assert _ffi.jbf_two_wg_plan(MOST_1024 + 1, 64, 64, 1, 1, -1, 20.0, 22.0) is None


def test_the_point_plan_takes_67108860_waves_and_refuses_one_more(built):
    """64 sets of one sigma_space: one chunk, a point per wave, four waves per workgroup of 256 threads."""
    lib = _ffi.load_library()
    ss = np.full(64, 22.0)
    most = 4 * MOST_256

    def call(total):
        return lib.rf_debug_jbf_points_plan(64, ss.ctypes.data, -1, 3, 0, total, None, 0)
    assert _ffi.jbf_points_plan(ss, -1, 3, 0, most) == [(33, 64, 1, most)]
    assert call(most + 1) == _ffi.RF_E_UNSUPPORTED and b"too many points for one launch" in lib.rf_last_error()


def test_gf_ragged_takes_16777215_items_and_refuses_one_more(built):
    """Images of 1 x 1: one stage-1 item and one row-state item each, 256 threads per item."""
    lib = _ffi.load_library()
    ones, p = _ones(MOST_256 + 1)
    assert lib.rf_gf_ragged_workspace_bytes(MOST_256, p, p, 3, 1, 9, 0) > 0
    assert lib.rf_gf_ragged_workspace_bytes(MOST_256 + 1, p, p, 3, 1, 9, 0) == 0
    assert b"too many work items for one launch" in lib.rf_last_error()


def test_the_uniform_guided_filter_lowers_its_chunk_to_the_launch_rule(built):
    """rf_gf_u8, rf_gf_ex_u8 and rf_gf_f32 fold a chunk's images into gridDim.x of their row and column walks;
    rf_debug_gf_launch_chunk answers from the function the entries take their chunk from."""
    lib = _ffi.load_library()
    assert "rf_debug_gf_launch_chunk" in _ffi.DEBUG_EXPORTS
    chunk = lib.rf_debug_gf_launch_chunk
    # ordinary images: the caps alone (16383 images for the 8-bit kernels, 65535 for the float ones)
    assert chunk(1 << 20, 1080, 1920, 3, 0) == 16383 and chunk(1 << 20, 1080, 1920, 3, 1) == 65535
    assert chunk(100, 1080, 1920, 3, 0) == 100 and chunk(0, 5, 7, 1, 0) == 0
    # row walk, 8-bit: m * src_cn * ceil(h / 64) workgroups of 256 threads; 21,888 rows are 342 blocks
    assert chunk(16383, 21888, 1, 3, 0) == MOST_256 // (3 * 342) == 16352
    assert 16352 * 3 * 342 * 256 < 1 << 32 <= 16353 * 3 * 342 * 256
    assert chunk(16383, 21888, 1, 1, 0) == 16383
    # row sums, float: m * (9 + 4 * src_cn) * ceil(h / 64) workgroups of 64 threads; 3,073 rows are 49 blocks
    assert chunk(65535, 3073, 1, 3, 1) == MOST_64 // (21 * 49) == 65217
    assert chunk(65535, 3073, 1, 1, 1) == 65535 and chunk(65535, 3073 * 2, 1, 1, 1) == MOST_64 // (13 * 97)
    # column walk, 8-bit: 8 * (ceil(m * nb / 8) + 64) * src_cn workgroups of 128 threads; 65,536 columns are 4096 blocks
    most = max(m for m in range(1, 16384) if 8 * ((m * 4096 + 7) // 8 + 64) * 3 * 128 < 1 << 32)
    assert chunk(16383, 1, 65536, 3, 0) == most == 2730
    # one image too tall for a launch: 0, and the entries refuse it before any device work
    assert chunk(5, (1 << 31) - 1, 1, 1, 0) == 0 and chunk(5, (1 << 31) - 1, 1, 1, 1) == 0
    assert chunk(5, 64 * (MOST_256 // 3), 1, 3, 0) == 1 and chunk(5, 64 * (MOST_256 // 3) + 1, 1, 3, 0) == 0
    assert chunk(-1, 5, 7, 1, 0) == _ffi.RF_E_BADARG and chunk(1, 5, 7, 2, 0) == _ffi.RF_E_BADARG
    fake, h = 1 << 40, (1 << 31) - 1
    assert lib.rf_gf_u8(fake, 2 * fake, 3 * fake, 1, h, 1, 3, 1, 9, 3.0, 1, 4 * fake, 1 << 50, None) == _ffi.RF_E_UNSUPPORTED
    assert b"rf_gf_u8: an image of 1 x 2147483647 is too large for one launch" in lib.rf_last_error()
    assert lib.rf_gf_u8(fake, 2 * fake, 3 * fake, 1, h, 1, 3, 1, 130, 3.0, 1, 4 * fake, 1 << 50, None) == _ffi.RF_E_UNSUPPORTED
    assert b"too large for one launch" in lib.rf_last_error()
    assert lib.rf_gf_f32(fake, 2 * fake, 3 * fake, 1, h, 1, 3, 1, 9, 1e-3, 1, 4 * fake, 1 << 50, None) == _ffi.RF_E_UNSUPPORTED
    assert b"rf_gf_f32: an image of 1 x 2147483647 is too large for one launch" in lib.rf_last_error()


def test_png_unfilter_takes_4194303_images_and_16777215_unpack_workgroups(built):
    lib = _ffi.load_library()
    ones, p = _ones(MOST_1024 + 1)
    fm = np.full(MOST_1024 + 1, 8 << 8, np.int32)               # depth 8, greyscale
    assert lib.rf_png_unfilter_workspace_bytes(MOST_1024, p, p, fm.ctypes.data) > 0
    assert lib.rf_png_unfilter_workspace_bytes(MOST_1024 + 1, p, p, fm.ctypes.data) == 0
    assert b"too many images for one launch" in lib.rf_last_error()
    # 65535 x 32767 pixels are 524,264 unpack workgroups of 4096 pixels: 32 images fit, 33 do not
    hs, ws = np.full(33, 65535, np.int32), np.full(33, 32767, np.int32)
    assert 33 * 524264 > MOST_256 >= 32 * 524264
    assert lib.rf_png_unfilter_workspace_bytes(32, hs.ctypes.data, ws.ctypes.data, fm.ctypes.data) > 0
    assert lib.rf_png_unfilter_workspace_bytes(33, hs.ctypes.data, ws.ctypes.data, fm.ctypes.data) == 0
    assert b"more pixels than one grid takes" in lib.rf_last_error()


def test_the_colourise_plan_takes_8388607_images_and_refuses_one_more(built):
    """Two selection states per image, a workgroup of 256 threads each."""
    lib = _ffi.load_library()
    ones, p = _ones(MOST_256 // 2 + 2)
    assert lib.rf_colorize_ragged_workspace_bytes(MOST_256 // 2, p, p) > 0
    assert lib.rf_colorize_ragged_workspace_bytes(MOST_256 // 2 + 1, p, p) == 0
    assert b"more workgroups than one grid takes" in lib.rf_last_error()


def test_whdr_refuses_beyond_67108863_workgroups_of_one_wave(built):
    """(the refusals alone: an admitted call launches)"""
    lib = _ffi.load_library()
    fake = 1 << 40
    assert lib.rf_whdr_points_u8(fake, 2, 16, 3, (MOST_64 + 1) // 2, fake, fake, fake, fake, 0.1, fake,
                                 None) == _ffi.RF_E_UNSUPPORTED
    assert b"too large for one launch" in lib.rf_last_error()
    assert lib.rf_whdr_f32(fake, MOST_64 + 1, 3, 1, 1, fake, fake, fake, 0.1, fake, None) == _ffi.RF_E_UNSUPPORTED
    assert b"too large for one launch" in lib.rf_last_error()
