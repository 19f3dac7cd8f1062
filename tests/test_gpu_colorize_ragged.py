"""GPU suite: the ragged colourise (rf_colorize_ragged_srgb_u8 / ops.colorize_ragged_srgb_u8: photos
of different sizes packed one after another; percentile, `max > 1` test and NaN rule per photo),
decompose_list and the ragged route of batch.decompose_files.  Bytes are compared with the numpy
oracle (oracle/colorize_numpy.py, pinned on the reference's bytes) image by image, never with another
kernel alone; the shapes are tiny so that the numpy sort answers in milliseconds."""
import os

import numpy as np
import pytest

from tests.test_gpu_fuzz import _colorize_floats, _colorize_shape, _image, env  # noqa: F401  (env is a fixture)

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_BYTE_256 = 1.0874      # as tests/test_gpu_fuzz.py: numpy's uint8 cast overflows above


def _run(rf, torch, imgs, rs, chunk_px=0, **kw):
    """One ragged call on host images: (list of reflectance bytes or None, list of shading bytes or
    None) as numpy arrays."""
    with rf._ffi.debug_options(colorize_chunk_px=chunk_px):
        refl_p, shad_p, refl, shad = rf.ops.colorize_ragged_srgb_u8(
            [torch.from_numpy(np.ascontiguousarray(i)).cuda() for i in imgs],
            [torch.from_numpy(np.ascontiguousarray(r, dtype=np.float32)).cuda() for r in rs], **kw)
    npx = sum(i.shape[0] * i.shape[1] for i in imgs)
    assert refl_p is None or tuple(refl_p.shape) == (npx, 3)
    assert shad_p is None or tuple(shad_p.shape) == (npx,)
    return (None if refl_p is None else [v.cpu().numpy() for v in refl],
            None if shad_p is None else [v.cpu().numpy() for v in shad])


def _oracle(imgs, rs):
    from oracle import colorize_numpy as oc
    with np.errstate(all="ignore"):
        return [oc.colorize_srgb_u8(i, np.asarray(r, dtype=np.float32)) for i, r in zip(imgs, rs)]


def _check(got, want, what=""):
    refl, shad = got
    for i, (want_refl, want_shad) in enumerate(want):
        if refl is not None:
            assert refl[i].shape == want_refl.shape and np.array_equal(refl[i], want_refl), (what, i, "reflectance")
        if shad is not None:
            assert shad[i].shape == want_shad.shape and np.array_equal(shad[i], want_shad), (what, i, "shading")


def _class(x):
    """How numpy's imwrite treats a float64 result: 'nan' and 'plain' are written as they are."""
    if np.isnan(x).any():
        return "nan"
    return "norm" if x.max() > 1 else "plain"


def _classes(img, r):
    sh, refl = _colorize_floats(img, np.asarray(r, dtype=np.float32))
    return _class(refl), _class(sh)


def _photo(rng, h, w):
    return _image(rng, h, w, 3, int(rng.integers(0, 3)))


# ---- 1. the reference's bytes ------------------------------------------------------------------------

@pytest.mark.parametrize("chunk_px", [0, 256, 4096])
def test_the_golden_cases_in_one_call_give_the_references_bytes(env, chunk_px):
    rf, co, torch = env
    d = np.load(os.path.join(G, "colorize_write.npz"))
    g = np.load(os.path.join(G, "decompose_outputs.npz"))
    tags = ("natural", "dark", "holes", "tiny")
    imgs = [d[t + "_image"] for t in tags] + [g["scene"]]
    rs = [d[t + "_r"] for t in tags] + [g["r"]]
    assert [i.shape[:2] for i in imgs] == [(48, 64), (20, 24), (33, 31), (1, 3), (24, 20)]
    want = [(d[t + "_refl_png"], d[t + "_shading_png"]) for t in tags] + \
           [(g["r_colorized_png"], g["s_colorized_png"])]
    _check(_run(rf, torch, imgs, rs, chunk_px), want, chunk_px)


# ---- 2. state per image ------------------------------------------------------------------------------

@pytest.mark.parametrize("order", ["forward", "reversed"])
def test_state_does_not_leak_between_neighbours(env, order):
    rf, co, torch = env
    rng = np.random.default_rng(41)
    imgs, rs = [], []
    imgs.append(_image(rng, 40, 50, 3, 2))                         # both results normalised
    rs.append(rng.uniform(0.05, 0.95, (40, 50)))
    imgs.append(np.zeros((30, 33, 3), np.uint8))                   # all black: both as they are, bytes 0
    rs.append(np.full((30, 33), 0.5))
    imgs.append(rng.integers(0, 2, (35, 28, 3)).astype(np.uint8))  # 0/1 image, r = 1: shading <= 1
    rs.append(np.ones((35, 28)))
    # 0/0 on a black pixel: NaN in both results, written as they are - so the other values stay below
    # the byte-256 overflow of numpy's cast (1 / r of bytes 1, as test_colorize_nan_result_is_written_unnormalised)
    img, r = np.ones((31, 47, 3), np.uint8), rng.uniform(0.95, 0.999, (31, 47))
    img[7, 9], r[7, 9] = 0, 0
    imgs.append(img)
    rs.append(r)
    img, r = _image(rng, 29, 37, 3, 2), rng.uniform(0.05, 0.95, (29, 37))
    img[5, 6], r[5, 6] = (9, 120, 33), 0                           # shading +inf
    imgs.append(img)
    rs.append(r)
    imgs.append(np.array([[[10, 20, 30]]], np.uint8))              # 1x1
    rs.append(np.array([[0.5]]))
    assert [_classes(i, r) for i, r in zip(imgs[:5], rs[:5])] == \
        [("norm", "norm"), ("plain", "plain"), ("norm", "plain"), ("nan", "nan"), ("norm", "norm")]
    sh, _ = _colorize_floats(imgs[4], np.asarray(rs[4], np.float32))
    assert np.isinf(sh).any()
    if order == "reversed":
        imgs, rs = imgs[::-1], rs[::-1]
    want = _oracle(imgs, rs)
    black = 1 if order == "forward" else 4
    assert not want[black][0].any() and not want[black][1].any()
    _check(_run(rf, torch, imgs, rs), want, order)


# ---- 3. chunk boundaries -----------------------------------------------------------------------------

def test_chunk_boundaries_at_256_pixels(env):
    rf, co, torch = env
    rng = np.random.default_rng(43)
    shapes = [(15, 17), (16, 16), (1, 257), (16, 32), (769, 1), (64, 48)]      # 255 256 257 512 769 3072
    with rf._ffi.debug_options(colorize_chunk_px=256):
        chunk, wgs, first = rf._ffi.colorize_ragged_plan(shapes)
    counts = [b - a for a, b in zip(first, first[1:] + [wgs])]
    assert chunk == 256 and counts == [1, 1, 2, 2, 4, 12]
    px = [h * w for h, w in shapes]
    assert any(c == 1 and p < chunk for c, p in zip(counts, px))               # inside one workgroup
    assert any(p % chunk == 0 for p in px)                                     # ends on a chunk end
    assert any(c >= 3 and p % chunk != 0 for c, p in zip(counts, px))          # partial last chunk
    imgs = [_photo(rng, h, w) for h, w in shapes]
    rs = [10.0 ** rng.uniform(-2, 0, (h, w)) for h, w in shapes]
    _check(_run(rf, torch, imgs, rs, 256), _oracle(imgs, rs))


# ---- 4. percentile ranks per image -------------------------------------------------------------------

def test_percentile_rank_boundaries_per_image(env):
    rf, co, torch = env
    from reflectance_filtering_amd import image_utils as iu
    rng = np.random.default_rng(44)
    shapes = [(9, 37), (2, 167), (27, 37), (25, 40), (7, 143), (6, 167), (3, 667)]
    assert [h * w for h, w in shapes] == [333, 334, 999, 1000, 1001, 1002, 2001]
    ranks = [(iu.percentile_rank(3 * h * w), iu.percentile_rank(h * w)) for h, w in shapes]
    assert len(set(3 * h * w - 1 - k for (h, w), (k, _) in zip(shapes, ranks))) > 1   # the rule moves
    imgs = [_image(rng, h, w, 3, 2) for h, w in shapes]
    rs = [10.0 ** rng.uniform(-2, 0, (h, w)) for h, w in shapes]
    assert all(_classes(i, r) == ("norm", "norm") for i, r in zip(imgs, rs))
    _check(_run(rf, torch, imgs, rs), _oracle(imgs, rs))


# ---- 5. equal sizes ----------------------------------------------------------------------------------

def test_equal_sizes_give_the_bytes_of_the_uniform_entry(env):
    rf, co, torch = env
    rng = np.random.default_rng(45)
    imgs = [_photo(rng, 37, 29) for _ in range(8)]
    rs = [(10.0 ** rng.uniform(-2, 0, (37, 29))).astype(np.float32) for _ in range(8)]
    rs[3][:] = 300.0                                                # shading <= 1: as it is
    refl, shad = rf.ops.colorize_srgb_u8(torch.from_numpy(np.stack(imgs)).cuda(),
                                         torch.from_numpy(np.stack(rs)).cuda())
    got = _run(rf, torch, imgs, rs)
    _check(got, list(zip(refl.cpu().numpy(), shad.cpu().numpy())))
    _check(got, _oracle(imgs, rs))


# ---- 6. output selection, workspace reuse ------------------------------------------------------------

def test_output_selection_and_a_reused_workspace(env):
    """Three calls back to back on the cached workspace, lists of 5, 2 and 9 images: every call finds
    the states and the image table of the one before."""
    rf, co, torch = env
    rng = np.random.default_rng(46)
    rf.ops.release_workspaces()
    calls = []
    for n, kw in ((5, {"want_shading": False}), (2, {"want_reflectance": False}), (9, {})):
        shapes = [_colorize_shape(rng) for _ in range(n)]
        imgs = [_photo(rng, h, w) for h, w in shapes]
        rs = [10.0 ** rng.uniform(-3, 0.3, (h, w)) for h, w in shapes]
        calls.append((kw, _run(rf, torch, imgs, rs, **kw), imgs, rs))
    assert len(rf.ops._colorize_ragged_workspaces) == 1
    for kw, got, imgs, rs in calls:
        assert (got[0] is None) == (not kw.get("want_reflectance", True))
        assert (got[1] is None) == (not kw.get("want_shading", True))
        _check(got, _oracle(imgs, rs), kw)
    rf.ops.release_workspaces()
    assert not rf.ops._colorize_ragged_workspaces


# ---- 7. seeded fuzz ----------------------------------------------------------------------------------

def _fuzz_case(rf, torch, rng, mode, h, w):
    """The r mixes of test_colorize_random_cases_match_the_oracle (modes 0..5), and mode 6: values
    that stay at or below 1, written as they are."""
    from reflectance_filtering_amd import image_utils as iu
    img = _image(rng, h, w, 3, int(rng.integers(0, 3)))
    if mode == 0:                                    # the CNN's own r
        r = rf.ops.cnn_reflectance_u8(torch.from_numpy(img[None]).cuda(), want_u8=False)[0].cpu().numpy()[0]
    elif mode == 1:
        r = (10.0 ** rng.uniform(-4, 0, (h, w))).astype(np.float32)
    elif mode == 2:                                  # denormals and exact 1.0 among them
        r = (10.0 ** rng.uniform(-3, 0, (h, w))).astype(np.float32)
        u = rng.random((h, w))
        r[u < 0.05] = np.float32(1.0)
        r[u > 0.97] = (rng.integers(1, 1 << 23, (h, w)).astype(np.uint32).view(np.float32))[u > 0.97]
    elif mode in (3, 4):                             # r == 0 on non-black pixels
        r = rng.uniform(0.05, 1.0, (h, w)).astype(np.float32)
        lit = np.flatnonzero(img.reshape(-1, 3).max(axis=1) > 0)
        room = h * w - 1 - iu.percentile_rank(h * w)
        count = int(rng.integers(1, room + 1)) if mode == 3 and room else room + int(rng.integers(1, 4))
        if lit.size:
            r.reshape(-1)[rng.choice(lit, min(count, lit.size), replace=False)] = 0
    elif mode == 5:                                  # a NaN result: 0/0 on black pixels
        img = rng.integers(0, 2, (h, w, 3)).astype(np.uint8)
        img.reshape(-1, 3)[rng.integers(0, h * w)] = 0
        mean = img.astype(np.float64).sum(axis=2) / 3.0
        r = (mean / rng.uniform(0.93, 1.08, (h, w))).astype(np.float32)
        sh, refl = _colorize_floats(img, r)
        assert not (sh >= _BYTE_256).any() and not (refl >= _BYTE_256).any()
    else:                                            # nothing above 1
        img = np.repeat(rng.integers(0, 2, (h, w, 1)), 3, axis=2).astype(np.uint8)
        r = rng.uniform(1.0, 4.0, (h, w)).astype(np.float32)
    return img, r


def test_seeded_random_lists_match_the_oracle(env):
    rf, co, torch = env
    rng = np.random.default_rng(47)
    seen = {"norm": 0, "plain": 0, "nan": 0}
    for case in range(30):
        n = int(rng.integers(1, 13))
        chunk_px = int(rng.choice([0, 256, 1024]))
        imgs, rs = [], []
        for i in range(n):
            h, w = _colorize_shape(rng)
            mode = (case * 5 + i) % 7 if case < 7 else int(rng.integers(0, 7))
            img, r = _fuzz_case(rf, torch, rng, mode, h, w)
            imgs.append(img)
            rs.append(r)
            for c in _classes(img, r):
                seen[c] += 1
        _check(_run(rf, torch, imgs, rs, chunk_px), _oracle(imgs, rs), (case, n, chunk_px))
    print("ragged colourise fuzz: results %s" % ", ".join("%s %d" % kv for kv in seen.items()))
    assert seen["norm"] and seen["plain"] and seen["nan"]


# ---- 8. decompose_list -------------------------------------------------------------------------------

def test_decompose_list_equals_decompose_batch_per_photo(env):
    rf, co, torch = env
    from tests import synth
    shapes = [(43, 64), (64, 43), (48, 64), (64, 43), (43, 64), (48, 64)]
    photos = [torch.from_numpy(synth.scene_u8(h, w, 3100 + i)).cuda() for i, (h, w) in enumerate(shapes)]
    rs, r8s, refls, shads = rf.decompose_list(photos)
    assert len(rs) == len(r8s) == len(refls) == len(shads) == len(shapes)
    for photo, r, r8, refl, shad in zip(photos, rs, r8s, refls, shads):
        want_r, want_r8, want_refl, want_shad = rf.decompose_batch(photo[None])
        assert r.dtype == torch.float32 and r.shape == photo.shape[:2]
        assert torch.equal(r.view(torch.int32), want_r[0].view(torch.int32))       # bit for bit
        assert torch.equal(r8, want_r8[0])
        assert refl.shape == photo.shape and torch.equal(refl, want_refl[0])
        assert shad.shape == photo.shape[:2] and torch.equal(shad, want_shad[0])
    with pytest.raises(ValueError):
        rf.decompose_list([])
    with pytest.raises(ValueError):
        rf.decompose_list([photos[0][:, :, :1].contiguous()])


def test_the_argument_checks_of_the_operator(env):
    rf, co, torch = env
    img = torch.zeros((4, 5, 3), dtype=torch.uint8, device="cuda")
    r = torch.ones((4, 5), dtype=torch.float32, device="cuda")
    op = rf.ops.colorize_ragged_srgb_u8
    for images, rr in (([], []), ([img.float()], [r]), ([img], [r.double()]), ([img.cpu()], [r]),
                       ([img], [r.cpu()]), ([img.transpose(0, 1)], [r.t().contiguous()]),
                       ([img], [r.t()]), ([img[:, :, :1].contiguous()], [r]), ([img], [r[:3].contiguous()]),
                       ([img, img], [r])):
        with pytest.raises(ValueError):
            op(images, rr)
    packed, flat = img.view(-1, 3), r.view(-1)
    for images, rr, sizes in ((packed, flat, [(4, 4)]), (packed, flat[:19].contiguous(), [(4, 5)]),
                              (packed, flat, [(0, 5)]), (packed, flat, []),
                              (packed[:, :2].contiguous(), flat, [(4, 5)])):
        with pytest.raises(ValueError):
            op(images, rr, sizes=sizes)
    refl_p, shad_p, refl, shad = op(packed, flat, sizes=[(2, 5), (2, 5)])            # the packed form
    assert tuple(refl_p.shape) == (20, 3) and [tuple(v.shape) for v in shad] == [(2, 5), (2, 5)]
    assert not refl_p.any() and not shad_p.any()


# ---- 9. one larger case ------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def larger():
    rng = np.random.default_rng(48)
    shapes = [(17, 23), (600, 700), (31, 9)]
    imgs = [_photo(rng, h, w) for h, w in shapes]
    rs = [10.0 ** rng.uniform(-2, 0, (h, w)) for h, w in shapes]
    return shapes, imgs, rs, _oracle(imgs, rs)


@pytest.mark.parametrize("chunk_px", [0, 4096])
def test_a_larger_image_beside_two_small_ones(env, larger, chunk_px):
    """0.4 MP.  Under the plan rule this list runs chunks of 512 pixels (420670 pixels are fewer than
    1024 chunks of 2048, so 256 * ceil(420670 / 262144)): two pixels per thread.  The rule gives a thread
    more than 8 only beyond 134 MP, so the second case asks for chunks of 4096 pixels - 16 per thread,
    103 chunks of the large image - through the debug option."""
    rf, co, torch = env
    shapes, imgs, rs, want = larger
    with rf._ffi.debug_options(colorize_chunk_px=chunk_px):
        chunk, wgs, first = rf._ffi.colorize_ragged_plan(shapes)
    assert (chunk, wgs) == ((512, 1 + 821 + 1) if chunk_px == 0 else (4096, 1 + 103 + 1))
    _check(_run(rf, torch, imgs, rs, chunk_px), want, chunk_px)


# ---- 10. batch.decompose_files -----------------------------------------------------------------------

def test_decompose_files_on_three_shapes_writes_the_files_of_the_single_image_tool(env, tmp_path,
                                                                                   monkeypatch):
    """Six PNGs in three shapes, no two neighbours equal: one step of batch.decompose_files is one
    decompose_packed (the device work of decompose_list); the files are those of decompose_image."""
    rf, co, torch = env
    from reflectance_filtering_amd import batch
    from reflectance_filtering_amd import decompose_with_trained_CNN as dc
    from reflectance_filtering_amd import image_utils as iu
    from tests import synth
    shapes = [(43, 64), (64, 43), (48, 64), (64, 43), (43, 64), (48, 64)]
    src_dir, out_a, out_b = tmp_path / "in", tmp_path / "list", tmp_path / "single"
    for d in (src_dir, out_a, out_b):
        d.mkdir()
    inputs = []
    for i, (h, w) in enumerate(shapes):
        inputs.append(str(src_dir / ("%03d.png" % i)))
        iu.imwrite(inputs[-1], synth.scene_u8(h, w, 3200 + i))
    lists, batches = [], []
    real_list, real_batch = dc.decompose_packed, dc.decompose_batch
    monkeypatch.setattr(dc, "decompose_packed", lambda images, **kw: (lists.append(len(images)),
                                                                      real_list(images, **kw))[1])
    monkeypatch.setattr(dc, "decompose_batch", lambda images, **kw: (batches.append(images.shape[0]),
                                                                     real_batch(images, **kw))[1])
    firsts = batch.decompose_files(inputs, str(out_a), rank=0, world=1)
    assert (lists, batches) == ([len(shapes)], [])
    assert [os.path.basename(f) for f in firsts] == ["%03d-r.png" % i for i in range(len(shapes))]
    assert sorted(os.listdir(str(out_a))) == sorted(
        "%03d%s" % (i, s) for i in range(len(shapes)) for s in ("-r.png", "-r_colorized.png", "-s_colorized.png"))
    for f in inputs:
        dc.decompose_image(f, str(out_b))
    for name in sorted(os.listdir(str(out_a))):
        with open(str(out_a / name), "rb") as fa, open(str(out_b / name), "rb") as fb:
            assert fa.read() == fb.read(), name
    # a step of one shape keeps the batch call
    del lists[:]
    batch.decompose_files([inputs[1], inputs[3]], str(out_a), rank=0, world=1)
    assert (lists, batches) == ([], [2])


# ---- 11. capture ------------------------------------------------------------------------------------

def test_the_ragged_entry_is_refused_on_a_capturing_stream(env):
    """As rf_cnn_reflectance_u8 in tests/test_gpu_parity.py: the entry called with a capturing stream
    returns its refusal and nothing enters the graph; the capture ends cleanly and an eager call on
    the same stream and buffers works afterwards."""
    import ctypes
    rf, co, torch = env
    from reflectance_filtering_amd import image_utils as iu
    lib = rf._ffi.load_library()
    rng = np.random.default_rng(49)
    shapes = [(9, 14), (12, 5)]
    imgs = [_photo(rng, h, w) for h, w in shapes]
    rs = [rng.uniform(0.05, 0.95, (h, w)).astype(np.float32) for h, w in shapes]
    bgr = torch.from_numpy(np.concatenate([i.reshape(-1, 3) for i in imgs])).cuda()
    r = torch.from_numpy(np.concatenate([x.reshape(-1) for x in rs])).cuda()
    refl = torch.zeros_like(bgr)
    shad = torch.zeros(bgr.shape[0], dtype=torch.uint8, device="cuda")
    steps = torch.from_numpy(iu.srgb_write_steps()).cuda()
    hs = np.array([h for h, _ in shapes], np.int32)
    wd = np.array([w for _, w in shapes], np.int32)
    kr = np.array([iu.percentile_rank(3 * h * w) for h, w in shapes], np.uint64)
    ks = np.array([iu.percentile_rank(h * w) for h, w in shapes], np.uint64)
    ws = torch.empty(lib.rf_colorize_ragged_workspace_bytes(2, hs.ctypes.data, wd.ctypes.data),
                     dtype=torch.uint8, device="cuda")

    def raw_call(stream_ptr):
        return lib.rf_colorize_ragged_srgb_u8(bgr.data_ptr(), r.data_ptr(), refl.data_ptr(), shad.data_ptr(),
                                              2, hs.ctypes.data, wd.ctypes.data, kr.ctypes.data,
                                              ks.ctypes.data, steps.data_ptr(), ws.data_ptr(), ws.numel(),
                                              ctypes.c_void_p(stream_ptr))

    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        rc = raw_call(side.cuda_stream)
    assert rc == rf._ffi.RF_E_UNSUPPORTED and b"captured" in lib.rf_last_error()
    torch.cuda.synchronize()
    assert not refl.any() and not shad.any()                     # nothing was enqueued
    assert raw_call(side.cuda_stream) == rf._ffi.RF_OK
    torch.cuda.synchronize()
    first = 0
    for (h, w), (want_refl, want_shad) in zip(shapes, _oracle(imgs, rs)):
        assert np.array_equal(refl[first:first + h * w].cpu().numpy().reshape(h, w, 3), want_refl)
        assert np.array_equal(shad[first:first + h * w].cpu().numpy().reshape(h, w), want_shad)
        first += h * w
