"""GPU suite: the buffer contract of every entry of the C ABI (include/reflectance_filtering.h).

Every buffer of a call - inputs, outputs, workspace - is a region of one guarded arena
(tests/arena.py).  Each case runs under five (layout, fill) pairs:

    L0  every base = 0 (mod 256)                                                 arena filled with 0xA5
    L1  uint8 buffers at the odd residues 1, 3, 5, ... 15 in turn, other element
        types at elem x 1 or elem x 3, the workspace at 16                       0x00, and again 0xFF
    L2  every uint8 buffer at 2, the others as L1                                0xFF
    L3  every uint8 buffer at 255, the others as L1                              0x00

The workspace holds exactly the bytes of the entry's size query and starts out as the arena's fill
(0xA5 bytes, zeros, or 0xFF: NaN as a float, -1 as a counter).  Asserted per case: RF_OK; no byte
outside the outputs and the workspace changes (guards, inputs, the bytes behind the workspace); the
L0 outputs equal the oracle under the entry's existing contract; every other layout's outputs are
bit-identical to L0's.

Shapes: S1 = 2 x 67 x 131 (w % 4 = 3, h % 64 = 3: 64x64 tiles with right and bottom strips; an image
is 26,331 or 8,777 bytes, both odd, so the second image of a batch is at an odd address even in L0),
S2 = 3 x 5 x 7 (smaller than every tile and window; 105 bytes), S3 = 1 x 1 x 1.

The cases themselves (buffers, host data, the call, the oracle check) are built by tests/abi_cases.py,
which tests/test_gpu_stream_contract.py runs as well.  tests/test_gpu_train_contract.py runs _contract on the
two entries of librf_train_hip.so (cases: tests/train_cases.py).
"""
import ctypes
import itertools

import numpy as np
import pytest

from tests import abi_cases as C
from tests import arena as A
from tests.abi_cases import S1, S2, S3
from tests.test_gpu_fuzz import env  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

PAIRS = (("L0", 0xA5), ("L1", 0x00), ("L1", 0xFF), ("L2", 0xFF), ("L3", 0x00))


def _residues(bufs, layout):
    odd, alt = itertools.cycle(range(1, 16, 2)), itertools.cycle((1, 3))
    out = []
    for b in bufs:
        if layout == "L0":
            out.append(0)
        elif b.role == "ws":
            out.append(16)
        elif b.fixed is not None:
            out.append(b.fixed)
        elif b.elem == 1:
            out.append({"L1": next(odd), "L2": 2, "L3": 255}[layout])
        else:
            out.append(b.elem * next(alt))
    return out


def _run(env, case, layout, fill, lib=None, last_error=None):
    """lib, last_error: the library the case calls and the getter of its error text (default: librf_hip.so and
    its rf_last_error; tests/test_gpu_train_contract.py passes librf_train_hip.so)."""
    rf, co, torch = env
    lib = rf._ffi.load_library() if lib is None else lib
    last_error = lib.rf_last_error if last_error is None else last_error
    ar = A.Arena(torch, "cuda", A.arena_bytes([b.nbytes for b in case.bufs]), fill)
    regs = {}
    for b, res in zip(case.bufs, _residues(case.bufs, layout)):
        regs[b.name] = ar.place(b.nbytes, res, b.elem, name=b.name)
        assert ar.ptr(regs[b.name]) % A.ALIGN == res
        if b.data is not None:
            ar.write(regs[b.name], b.data)
    torch.cuda.synchronize()
    ar.snapshot()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptrs = dict((name, ar.ptr(r)) for name, r in regs.items())
    if case.around is not None:
        with case.around():
            rc = case.call(lib, ptrs, stream)
    else:
        rc = case.call(lib, ptrs, stream)
    torch.cuda.synchronize()
    assert rc == rf._ffi.RF_OK, (layout, fill, rc, last_error())
    try:
        ar.assert_only_changed([regs[b.name] for b in case.bufs if b.role in ("out", "ws")])
    except AssertionError as err:
        raise AssertionError("layout %s, fill 0x%02X: %s" % (layout, fill, err))
    raw = dict((b.name, ar.bytes(regs[b.name]).cpu().numpy().copy()) for b in case.bufs if b.role == "out")
    return C.typed_outputs(case, raw)


def _contract(env, case, lib=None, last_error=None):
    base = None
    for layout, fill in PAIRS:
        outs = _run(env, case, layout, fill, lib, last_error)
        if case.after is not None:
            case.after()
        if base is None:
            case.check(outs)
            base = outs
            continue
        for name in base:
            a, b = base[name], outs[name]
            assert a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), \
                "%s differs from L0's under layout %s, fill 0x%02X (%d bytes)" % (
                    name, layout, fill, int(np.count_nonzero(a.view(np.uint8) != b.view(np.uint8))))


# ---- the entries -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [S1, S2], ids=["S1", "S2"])
@pytest.mark.parametrize("route", sorted(C.JBF_ROUTES))
@pytest.mark.parametrize("pair", sorted(C.JBF_PAIRS))
def test_jbf_u8(env, pair, route, shape):
    _contract(env, C.jbf_u8(env, pair, route, shape))


GF_ROUTES = {"r9": (9, False), "r45": (45, False), "r45_two_kernel": (45, True), "r129_float": (129, False)}


@pytest.mark.parametrize("shape", [S1, S2], ids=["S1", "S2"])
@pytest.mark.parametrize("iterations", [1, 2])
@pytest.mark.parametrize("skind", ["colour", "grey3", "grey1"])
@pytest.mark.parametrize("route", sorted(GF_ROUTES))
def test_gf_u8(env, route, skind, iterations, shape):
    radius, two_kernel = GF_ROUTES[route]
    _contract(env, C.gf_u8(env, shape, skind, radius, iterations, two_kernel=two_kernel))


@pytest.mark.parametrize("ws_images", [1, 3], ids=["chunked", "full"])
@pytest.mark.parametrize("radius", [45, 129])
def test_gf_u8_three_images_on_a_one_image_and_on_the_full_workspace(env, radius, ws_images):
    _contract(env, C.gf_u8(env, (3, 67, 131), "colour", radius, 2, ws_images=ws_images))


def test_gf_u8_in_place(env):
    _contract(env, C.gf_u8(env, S1, "colour", 9, 2, in_place=True))


@pytest.mark.parametrize("radius,skind", [(9, "grey1"), (45, "grey3"), (45, "colour")])
def test_gf_ex_u8_grey_guide(env, radius, skind):
    _contract(env, C.gf_u8(env, S1, skind, radius, 1, grey_guide=True))


@pytest.mark.parametrize("shape", [S1, S2, S3], ids=["S1", "S2", "S3"])
@pytest.mark.parametrize("want", ["both", "float", "u8"])
@pytest.mark.parametrize("entry", ["u8", "f32_nchw_rgb", "f32_nhwc_bgr"])
def test_cnn_reflectance(env, entry, want, shape):
    _contract(env, C.cnn_reflectance(env, entry, want, shape))


@pytest.mark.parametrize("shape", [S1, S3], ids=["S1", "S3"])
@pytest.mark.parametrize("want", ["both", "reflectance", "shading"])
def test_colorize_srgb_u8(env, want, shape):
    _contract(env, C.colorize_srgb_u8(env, want, shape))


@pytest.mark.parametrize("cn", [3, 1], ids=["colour", "one_channel"])
def test_jbf_f32(env, cn):
    _contract(env, C.jbf_f32(env, cn))


@pytest.mark.parametrize("radius", [9, 150])
@pytest.mark.parametrize("cn", [3, 1], ids=["colour", "one_channel"])
def test_gf_f32(env, cn, radius):
    _contract(env, C.gf_f32(env, cn, radius))


@pytest.mark.parametrize("ragged", [False, True], ids=["rf_jbf_points_u8", "rf_jbf_points_ragged_u8"])
def test_jbf_points(env, ragged):
    _contract(env, C.jbf_points(env, ragged))


@pytest.mark.parametrize("c", [3, 1])
def test_whdr_f32(env, c):
    _contract(env, C.whdr_f32(env, c))


@pytest.mark.parametrize("c", [3, 1])
def test_whdr_points_u8(env, c):
    """Two sets of whole images taken as point lists (pixel y * w + x of image i behind i * h * w)."""
    _contract(env, C.whdr_points_u8(env, c))


def test_jbf_ragged_u8(env):
    _contract(env, C.jbf_ragged_u8(env))


def test_gf_ragged_u8(env):
    _contract(env, C.gf_ragged_u8(env))


@pytest.mark.parametrize("entry", ["rf_colorize_ragged_srgb_u8", "rf_colorize_ragged_r8_srgb_u8"])
def test_colorize_ragged(env, entry):
    _contract(env, C.colorize_ragged(env, entry))


def test_png_deflate_ragged_u8(env):
    """The streams' used bytes and the offsets are the outputs; each stream inflates to the Up-filtered
    rows of its image (RGB order)."""
    _contract(env, C.png_deflate_ragged_u8(env))


def test_png_unfilter_ragged_u8(env):
    """raw is reconstructed in place, so it is an output; its bytes are not compared across layouts."""
    _contract(env, C.png_unfilter_ragged_u8(env))


# ---- the harness bites on the device -----------------------------------------------------------------------

def test_a_device_write_one_byte_past_an_output_is_reported(env):
    rf, co, torch = env
    ar = A.Arena(torch, "cuda", A.arena_bytes([105, 105]), 0xA5)
    src = ar.place(105, 1, name="src")
    dst = ar.place(105, 3, name="dst")
    ar.snapshot()
    view = ar.view(dst, (5, 7, 3), torch.uint8)
    view[:] = 7
    ar.assert_only_changed([dst])
    past = torch.tensor([dst.end], device="cuda")
    ar.buf[past] = 0                                  # an indexed write just past the output view
    torch.cuda.synchronize()
    with pytest.raises(AssertionError, match=r"1 byte\(s\) changed after dst .*first at offset 0 relative to its end"):
        ar.assert_only_changed([dst])
    ar.buf[torch.tensor([src.offset + 4], device="cuda")] = 1
    with pytest.raises(AssertionError, match=r"1 byte\(s\) changed inside src .*first at offset 4 relative"):
        ar.assert_only_changed([dst, A.Region("the byte behind dst", dst.end, 1)])
