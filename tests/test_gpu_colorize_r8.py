"""GPU suite: the colourise of an 8-bit reflectance map (rf_colorize_ragged_r8_srgb_u8 /
ops.colorize_ragged_r8_srgb_u8).  Its bytes are compared with the reference's (the fixture
tests/golden/colorize_r8_write.npz), with the numpy oracle, and - the defining property - with
ops.colorize_ragged_srgb_u8 on the float32 map formed with numpy on the host,
r8.astype(float32) / float32(255).  Every comparison is on exact bytes."""
import ctypes
import os

import numpy as np
import pytest

from tests.test_gpu_fuzz import _image, env  # noqa: F401  (env is a fixture)

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TAGS = ("ramp", "photo", "dark", "nan")
SHAPES = ((1, 1), (1, 70), (70, 1), (5, 7), (33, 130))
GUARD = 512


def _as_float(r8):
    return r8.astype(np.float32) / np.float32(255)


def _case(rng, h, w):
    """A photo and a map with a few zero bytes (+inf, and NaN where the photo is black too)."""
    img = _image(rng, h, w, 3, int(rng.integers(0, 3)))
    r8 = rng.integers(1, 256, (h, w)).astype(np.uint8)
    if h * w >= 35:
        flat = rng.choice(h * w, 3, replace=False)
        r8.reshape(-1)[flat[:2]] = 0
        if rng.random() < 0.5:
            img.reshape(-1, 3)[flat[0]] = 0
    return img, r8


def _r8(rf, torch, imgs, r8s, **kw):
    refl_p, shad_p, refl, shad = rf.ops.colorize_ragged_r8_srgb_u8(
        [torch.from_numpy(np.ascontiguousarray(i)).cuda() for i in imgs],
        [torch.from_numpy(np.ascontiguousarray(r)).cuda() for r in r8s], **kw)
    return (None if refl_p is None else [v.cpu().numpy() for v in refl],
            None if shad_p is None else [v.cpu().numpy() for v in shad])


def _f32(rf, torch, imgs, r8s, **kw):
    refl_p, shad_p, refl, shad = rf.ops.colorize_ragged_srgb_u8(
        [torch.from_numpy(np.ascontiguousarray(i)).cuda() for i in imgs],
        [torch.from_numpy(_as_float(r)).cuda() for r in r8s], **kw)
    return (None if refl_p is None else [v.cpu().numpy() for v in refl],
            None if shad_p is None else [v.cpu().numpy() for v in shad])


def _same(got, want, what=""):
    for k, name in enumerate(("reflectance", "shading")):
        assert (got[k] is None) == (want[k] is None), (what, name)
        if got[k] is None:
            continue
        assert len(got[k]) == len(want[k])
        for i, (a, b) in enumerate(zip(got[k], want[k])):
            assert a.shape == b.shape and a.dtype == np.uint8 and np.array_equal(a, b), (what, i, name)


@pytest.fixture(scope="module")
def lists():
    """The photos and maps of the shapes above, made once and left alone."""
    rng = np.random.default_rng(2609)
    return [_case(rng, h, w) for h, w in SHAPES]


# ---- 1. the reference's bytes ------------------------------------------------------------------------

@pytest.mark.parametrize("chunk_px", [0, 256])
def test_the_fixture_in_one_call_gives_the_references_bytes(env, chunk_px):
    rf, co, torch = env
    d = np.load(os.path.join(G, "colorize_r8_write.npz"))
    imgs = [d[t + "_image"] for t in TAGS]
    r8s = [d[t + "_r8"] for t in TAGS]
    with rf._ffi.debug_options(colorize_chunk_px=chunk_px):
        got = _r8(rf, torch, imgs, r8s)
    _same(got, ([d[t + "_refl_png"] for t in TAGS], [d[t + "_shading_png"] for t in TAGS]), chunk_px)


# ---- 2. the defining property ------------------------------------------------------------------------

@pytest.mark.parametrize("which", list(range(len(SHAPES))) + ["forward", "reversed"])
def test_equals_the_float_entry_on_byte_over_255(env, lists, which):
    rf, co, torch = env
    if which == "forward":
        cases = lists
    elif which == "reversed":
        cases = lists[::-1]
    else:
        cases = [lists[which]]
    imgs, r8s = [c[0] for c in cases], [c[1] for c in cases]
    _same(_r8(rf, torch, imgs, r8s), _f32(rf, torch, imgs, r8s), which)


def _prepare(rf, torch, imgs, r8s, ws=None):
    """Everything a direct call of the entry needs, on the device, with outputs that stand inside guard
    bytes: (call(stream pointer or None) -> return code, guarded reflectance buffer, guarded shading
    buffer, workspace, pixels)."""
    from reflectance_filtering_amd import image_utils as iu
    lib = rf._ffi.load_library()
    shapes = [i.shape[:2] for i in imgs]
    npx = sum(h * w for h, w in shapes)
    bgr = torch.from_numpy(np.concatenate([i.reshape(-1, 3) for i in imgs])).cuda()
    r8 = torch.from_numpy(np.concatenate([r.reshape(-1) for r in r8s])).cuda()
    refl = torch.full((GUARD + 3 * npx + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    shad = torch.full((GUARD + npx + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    steps = torch.from_numpy(iu.srgb_write_steps()).cuda()
    hs = np.array([h for h, _ in shapes], np.int32)
    wd = np.array([w for _, w in shapes], np.int32)
    kr = np.array([iu.percentile_rank(3 * h * w) for h, w in shapes], np.uint64)
    ks = np.array([iu.percentile_rank(h * w) for h, w in shapes], np.uint64)
    if ws is None:
        ws = torch.empty(lib.rf_colorize_ragged_workspace_bytes(len(imgs), hs.ctypes.data, wd.ctypes.data),
                         dtype=torch.uint8, device="cuda")

    def call(stream=None):
        if stream is None:
            stream = torch.cuda.current_stream().cuda_stream
        return lib.rf_colorize_ragged_r8_srgb_u8(bgr.data_ptr(), r8.data_ptr(), refl.data_ptr() + GUARD,
                                                 shad.data_ptr() + GUARD, len(imgs), hs.ctypes.data,
                                                 wd.ctypes.data, kr.ctypes.data, ks.ctypes.data,
                                                 steps.data_ptr(), ws.data_ptr(), ws.numel(),
                                                 ctypes.c_void_p(stream))

    return call, refl, shad, ws, npx


def _split(refl, shad, imgs, npx):
    refl = refl[GUARD:GUARD + 3 * npx].cpu().numpy().reshape(-1, 3)
    shad = shad[GUARD:GUARD + npx].cpu().numpy()
    out, first = ([], []), 0
    for i in imgs:
        h, w = i.shape[:2]
        out[0].append(refl[first:first + h * w].reshape(h, w, 3))
        out[1].append(shad[first:first + h * w].reshape(h, w))
        first += h * w
    return out


def test_guard_bytes_around_both_outputs_and_a_workspace_used_twice(env, lists):
    rf, co, torch = env
    imgs, r8s = [c[0] for c in lists], [c[1] for c in lists]
    want = _f32(rf, torch, imgs, r8s)
    call, refl, shad, ws, npx = _prepare(rf, torch, imgs, r8s)
    assert call() == rf._ffi.RF_OK
    torch.cuda.synchronize()
    for buf, fill, n in ((refl, 0xA5, 3 * npx), (shad, 0x5A, npx)):
        assert bool((buf[:GUARD] == fill).all()) and bool((buf[GUARD + n:] == fill).all())
    _same(_split(refl, shad, imgs, npx), want, "first")
    # the same workspace again, for another list: a call clears everything it reads
    imgs2, r8s2 = imgs[::-1][:4], r8s[::-1][:4]
    call, refl, shad, _, npx = _prepare(rf, torch, imgs2, r8s2, ws=ws)
    assert call() == rf._ffi.RF_OK
    torch.cuda.synchronize()
    for buf, fill, n in ((refl, 0xA5, 3 * npx), (shad, 0x5A, npx)):
        assert bool((buf[:GUARD] == fill).all()) and bool((buf[GUARD + n:] == fill).all())
    _same(_split(refl, shad, imgs2, npx), _f32(rf, torch, imgs2, r8s2), "second")


# ---- 3. an image over many workgroups ----------------------------------------------------------------

def test_an_image_that_spans_many_workgroups(env, lists):
    rf, co, torch = env
    from oracle import colorize_numpy as oc
    rng = np.random.default_rng(2610)
    shapes = [(9, 14), (120, 150), (31, 9)]
    chunk, wgs, first = rf._ffi.colorize_ragged_plan(shapes)
    assert chunk == 256 and first[2] - first[1] == 71 and wgs == 74          # 18000 pixels: 70.3 chunks
    chunk, wgs, first = rf._ffi.colorize_ragged_plan(SHAPES)
    assert chunk == 256 and wgs - first[4] == 17                              # 33x130 in the lists above
    imgs = [_image(rng, h, w, 3, int(rng.integers(0, 3))) for h, w in shapes]
    r8s = [rng.integers(1, 256, (h, w)).astype(np.uint8) for h, w in shapes]
    got = _r8(rf, torch, imgs, r8s)
    _same(got, _f32(rf, torch, imgs, r8s), "float entry")
    with np.errstate(all="ignore"):
        want = [oc.colorize_srgb_u8(i, _as_float(r)) for i, r in zip(imgs, r8s)]
    _same(got, ([w[0] for w in want], [w[1] for w in want]), "oracle")


# ---- 4. output selection -----------------------------------------------------------------------------

@pytest.mark.parametrize("kw", [{"want_shading": False}, {"want_reflectance": False}])
def test_one_output_alone(env, lists, kw):
    rf, co, torch = env
    imgs, r8s = [c[0] for c in lists], [c[1] for c in lists]
    got = _r8(rf, torch, imgs, r8s, **kw)
    assert (got[0] is None) == ("want_reflectance" in kw) and (got[1] is None) == ("want_shading" in kw)
    _same(got, _f32(rf, torch, imgs, r8s, **kw), kw)
    both = _r8(rf, torch, imgs, r8s)
    k = 0 if got[1] is None else 1
    _same((both[0] if k == 0 else None, both[1] if k == 1 else None), got, "both")


def test_the_argument_checks_of_the_operator(env):
    rf, co, torch = env
    img = torch.zeros((4, 5, 3), dtype=torch.uint8, device="cuda")
    r8 = torch.full((4, 5), 255, dtype=torch.uint8, device="cuda")
    op = rf.ops.colorize_ragged_r8_srgb_u8
    for images, rr in (([], []), ([img], [r8.float()]), ([img.cpu()], [r8]), ([img], [r8.cpu()]),
                       ([img], [r8.t()]), ([img[:, :, :1].contiguous()], [r8]), ([img], [r8[:3].contiguous()]),
                       ([img, img], [r8])):
        with pytest.raises(ValueError):
            op(images, rr)
    packed, flat = img.view(-1, 3), r8.view(-1)
    for images, rr, sizes in ((packed, flat, [(4, 4)]), (packed, flat[:19].contiguous(), [(4, 5)]),
                              (packed, flat, [(0, 5)]), (packed, flat, []), (packed, flat.float(), [(4, 5)])):
        with pytest.raises(ValueError):
            op(images, rr, sizes=sizes)
    refl_p, shad_p, refl, shad = op(packed, flat, sizes=[(2, 5), (2, 5)])            # the packed form
    assert tuple(refl_p.shape) == (20, 3) and [tuple(v.shape) for v in shad] == [(2, 5), (2, 5)]
    assert not refl_p.any() and not shad_p.any()


# ---- 5. capture --------------------------------------------------------------------------------------

def test_the_entry_is_refused_on_a_capturing_stream(env, lists):
    """As the float entry in tests/test_gpu_colorize_ragged.py: called with a capturing stream the
    entry returns its refusal and nothing enters the graph; an eager call on the same stream works
    afterwards."""
    rf, co, torch = env
    lib = rf._ffi.load_library()
    imgs, r8s = [c[0] for c in lists[2:4]], [c[1] for c in lists[2:4]]
    want = _f32(rf, torch, imgs, r8s)
    call, refl, shad, ws, npx = _prepare(rf, torch, imgs, r8s)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        rc = call(side.cuda_stream)
    msg = lib.rf_last_error()
    assert rc == rf._ffi.RF_E_UNSUPPORTED and b"captured" in msg and b"rf_colorize_ragged_r8_srgb_u8" in msg
    torch.cuda.synchronize()
    assert bool((refl == 0xA5).all()) and bool((shad == 0x5A).all())          # nothing was enqueued
    assert call(side.cuda_stream) == rf._ffi.RF_OK
    torch.cuda.synchronize()
    _same(_split(refl, shad, imgs, npx), want, "after the capture")
