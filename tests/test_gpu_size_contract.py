"""GPU suite: the size contract of the C ABI (include/reflectance_filtering.h, "Sizes"): every offset into
a caller's buffer is formed in 64 bits, and a call whose work does not fit one launch is refused before
any device work.  The cases are those of tests/size_cases.py, which runs the builders and oracles of
tests/abi_cases.py over buffers that pass 2^31 and 2^32 bytes (its docstring has the method).

Per case (size_cases.run):
  1. the call returns RF_OK;
  2. the outputs of the first period A and of the tail B equal the same entry called on A and on B alone;
  3. those two small calls equal the oracle (the builder's own check);
  4. every later period of an output equals the first, compared on the device in slices of 256 MiB at
     most; a failure names the first differing period and where it lies relative to each mark;
  5. the outputs start as the complement of A's result, so a period that was not written differs.
A case skips only where the device has less free memory than 1.25 times its need (both in the reason);
no case needs more than 32 GiB.  Marks that this bound cuts: the pixel index of r and shading_out of the
colourise entries stops at 2^31 (2^32 needs 32 GiB for bgr, r and shading_out alone); rf_gf_ragged_u8,
whose workspace holds 16 bytes and more per pixel, crosses byte 2^32 of a colour guide (pixel index
2^30.4) and pixel index 2^30 under a one-channel guide (there element index 2^32 of its float workspace).
Printed per case: wall time of the large call, peak device memory (profiles/size_contract_time.txt).

Entries of the header that have no case here: rf_png_deflate_ragged_u8 refuses a stream bound of 2^31 or
more, so its buffers cannot cross a mark (tests/test_png_abi.py pins the refusal); rf_cnn_pack_weights
has no size.  The point entries and the two WHDR entries have index lists beside their
images and runs of their own (size_cases.run_points, run_whdr_f32, run_whdr_points_u8).

The largest launch: rf_jbf_ragged_u8 takes 4,194,303 images of 1 x 1 (as many tiles of 1024 threads: one
short of 2^32 work-items, the runtime's limit) and refuses one more with RF_E_UNSUPPORTED, dst untouched.
At radius 54 (slabs) the admitted call took 18.4 s on an MI355X against 6.3 s at radius 33, so that half
runs at radius 33 alone; the refusal runs at both.
"""
import ctypes
import time

import numpy as np
import pytest

from tests import size_cases as S
from tests.test_gpu_fuzz import env  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

MOST_TILES = (1 << 32) // 1024 - 1


@pytest.mark.parametrize("name", sorted(S.CASES))
def test_offsets_past_the_marks(env, name):
    print("\n" + S.run(env, name))


@pytest.mark.parametrize("jkind,skind", [("colour", "grey3"), ("joint1", "grey1")], ids=["colour-bytes", "grey1-pixels"])
@pytest.mark.parametrize("ragged", [False, True], ids=["rf_jbf_points_u8", "rf_jbf_points_ragged_u8"])
def test_points_past_the_marks(env, ragged, jkind, skind):
    print("\n" + S.run_points(env, ragged, jkind, skind))


def test_whdr_f32_past_the_marks(env):
    print("\n" + S.run_whdr_f32(env))


def test_whdr_points_u8_with_the_mark_inside_the_second_set(env):
    print("\n" + S.run_whdr_points_u8(env))


@pytest.mark.parametrize("sigma_space", [22.0, 36.0], ids=["r33", "r54-slabs"])
def test_the_largest_ragged_launch_and_one_tile_more(env, sigma_space):
    """4,194,304 grey images of 1 x 1 are refused, dst untouched; 4,194,303 are taken (radius 33 alone, module
    docstring): image i has value i % 256 under a joint of value 7 i % 256, and each result is what the oracle
    gives for that image alone."""
    rf, co, torch = env
    lib = rf._ffi.load_library()
    n, d, sc = MOST_TILES + 1, -1, 20.0
    values = np.arange(256, dtype=np.uint8)
    want = np.array([co.joint_bilateral_filter((7 * values[v:v + 1]).reshape(1, 1, 1), values[v:v + 1].reshape(1, 1, 1),
                                               d, sc, sigma_space).reshape(()) for v in range(256)], np.uint8)
    ones = np.ones(n, np.int32)
    need = lib.rf_jbf_ragged_workspace_bytes(n - 1, ones.ctypes.data, ones.ctypes.data, 1, 1, d, sigma_space, 0)
    assert need > 0
    assert lib.rf_jbf_ragged_workspace_bytes(n, ones.ctypes.data, ones.ctypes.data, 1, 1, d, sigma_space, 0) == 0
    try:
        src = torch.arange(n, device="cuda").to(torch.uint8)
        joint = (torch.arange(n, device="cuda") * 7).to(torch.uint8)
        fill = torch.from_numpy(255 - want).cuda()[torch.arange(n, device="cuda") % 256]
        dst = fill.clone()
        ws = torch.full((need,), 0xA5, dtype=torch.uint8, device="cuda")
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()

        def call(count):
            return lib.rf_jbf_ragged_u8(joint.data_ptr(), src.data_ptr(), dst.data_ptr(), count, ones.ctypes.data,
                                        ones.ctypes.data, 1, 1, d, sc, sigma_space, 4, 0, ws.data_ptr(), need, stream)
        assert call(n) == rf._ffi.RF_E_UNSUPPORTED, lib.rf_last_error()
        assert b"for one launch" in lib.rf_last_error()
        torch.cuda.synchronize()
        assert bool((dst == fill).all()), "the refused call wrote to dst"
        if sigma_space != 22.0:
            return
        t0 = time.perf_counter()
        rc = call(n - 1)
        torch.cuda.synchronize()
        print("\nsize contract %d tiles of 1 x 1, sigma_space %g: %.2f s" % (n - 1, sigma_space,
                                                                            time.perf_counter() - t0))
        assert rc == rf._ffi.RF_OK, lib.rf_last_error()
        expect = torch.from_numpy(want).cuda()[torch.arange(n - 1, device="cuda") % 256]
        wrong = torch.nonzero(dst[:n - 1] != expect)
        assert wrong.numel() == 0, "%d images differ from the oracle, the first is image %d" % (
            wrong.shape[0], int(wrong[0]))
        assert int(dst[n - 1]) == int(fill[n - 1])
    finally:
        src = joint = fill = dst = ws = expect = wrong = None
        rf.ops.release_workspaces()
        torch.cuda.empty_cache()
