"""GPU suite: the network on float32 linear images (rf_cnn_reflectance_f32 / _packed_f32, both layouts)
against the uint8 entry bit for bit where the values are sRGB byte levels, against a float64 forward in
between, and the properties its header promises: a pixel's bits depend on its three values only,
non-finite values stay local, the caller's weights are used."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LAYOUTS = ("nchw_rgb", "nhwc_bgr")
TOL = 2e-6          # what tests/test_gpu_parity.py allows the u8 kernel against the float64 forward


@pytest.fixture(scope="module")
def env(built):
    import torch
    import reflectance_filtering_amd as rf
    if not torch.cuda.is_available():
        pytest.skip("no HIP device visible (run with -m 'not gpu' on CPU-only machines)")
    rf._ffi.load_library()
    return rf, torch


def _lut(rf, torch):
    return torch.from_numpy(rf.image_utils.srgb_byte_lut()).cuda()


def _to_layout(bgr_f32, layout):
    """float BGR [N,H,W,3] -> the entry's input in `layout` (contiguous)."""
    if layout == "nhwc_bgr":
        return bgr_f32.contiguous()
    return bgr_f32.flip(-1).permute(0, 3, 1, 2).contiguous()      # RGB planes


def _random_bytes(torch, n, h, w, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device="cuda", generator=g)


def _guarded(torch, npix, dtype, fill):
    """An output buffer of npix elements with 64 sentinel elements before and after it."""
    buf = torch.full((npix + 128,), fill, dtype=dtype, device="cuda")
    return buf, buf[64:64 + npix]


# ------------------------------------------------------------------ a. same bits as the u8 entry
@pytest.mark.parametrize("n,h,w", [(1, 1, 1), (1, 1, 2), (1, 1, 3), (1, 7, 5), (3, 5, 7), (2, 1, 129),
                                   (4, 33, 31)])
def test_byte_levels_give_the_bits_of_the_u8_entry(env, n, h, w):
    rf, torch = env
    lib = rf._ffi.load_library()
    bgr = _random_bytes(torch, n, h, w, 100 * n + 10 * h + w)
    want_r, want_r8 = rf.ops.cnn_reflectance_u8(bgr)
    packed, lut = rf.ops._cnn_device_consts(torch, bgr.device, None)
    linear = lut[bgr.long()]
    npix = n * h * w
    for layout in LAYOUTS:
        x = _to_layout(linear, layout)
        r, r8 = rf.ops.cnn_reflectance_f32(x, layout=layout)
        assert r.shape == (n, h, w) and r8.shape == (n, h, w)
        assert np.array_equal(r.cpu().numpy(), want_r.cpu().numpy()), layout
        assert np.array_equal(r8.cpu().numpy(), want_r8.cpu().numpy()), layout
        for want_float, want_u8 in ((True, True), (True, False), (False, True)):
            rbuf, rview = _guarded(torch, npix, torch.float32, -7.0)
            bbuf, bview = _guarded(torch, npix, torch.uint8, 0xA5)
            rc = lib.rf_cnn_reflectance_packed_f32(
                x.data_ptr(), rview.data_ptr() if want_float else None,
                bview.data_ptr() if want_u8 else None, n, h, w, rf._ffi.CNN_LAYOUTS[layout],
                packed.data_ptr(), rf._ffi.current_stream_ptr(torch))
            assert rc == rf._ffi.RF_OK
            got_r, got_b = rbuf.cpu().numpy(), bbuf.cpu().numpy()
            for got, want, asked, fill in ((got_r, want_r, want_float, np.float32(-7.0)),
                                           (got_b, want_r8, want_u8, 0xA5)):
                assert np.all(got[:64] == fill) and np.all(got[64 + npix:] == fill), (layout, "guard")
                if asked:
                    assert np.array_equal(got[64:64 + npix], want.cpu().numpy().ravel()), layout
                else:
                    assert np.all(got == fill), (layout, "an output that was not asked for")


def test_lds_column_kernel_takes_float_input_too(env):
    """The debug option that selects the LDS-column kernel means the same for float input: identical
    bits from both kernels, byte levels and values in between, odd pixel count, several images."""
    rf, torch = env
    n, h, w = 3, 5, 7
    photo = torch.from_numpy(np.random.RandomState(61).rand(n, h, w, 3).astype(np.float32)).cuda()
    levels = _lut(rf, torch)[_random_bytes(torch, n, h, w, 62).long()]
    want_r, want_r8 = rf.ops.cnn_reflectance_u8(_random_bytes(torch, n, h, w, 62))
    for layout in LAYOUTS:
        for bgr_f32 in (photo, levels):
            x = _to_layout(bgr_f32, layout)
            r, r8 = rf.ops.cnn_reflectance_f32(x, layout=layout)
            with rf._ffi.debug_options(cnn_lds_columns=1):
                r_lds, r8_lds = rf.ops.cnn_reflectance_f32(x, layout=layout)
            assert torch.equal(r.view(torch.int32), r_lds.view(torch.int32)) and torch.equal(r8, r8_lds), layout
        assert torch.equal(r_lds, want_r) and torch.equal(r8_lds, want_r8), layout


# ------------------------------------------------------------------ b. the grid-stride loop
def test_grid_stride_loop_on_one_large_image(env):
    """2897 x 2897 = 8,392,609 pixels: just past 256 * 128 workgroups of 256 pixels, so some lanes
    take a second trip.  Compared on the device; only the verdict comes back."""
    rf, torch = env
    side = 2897
    bgr = _random_bytes(torch, 1, side, side, 5)
    want_r, want_r8 = rf.ops.cnn_reflectance_u8(bgr)
    x = _to_layout(_lut(rf, torch)[bgr.long()], "nchw_rgb")
    r, r8 = rf.ops.cnn_reflectance_f32(x, layout="nchw_rgb")
    bad = ((r != want_r) | (r8 != want_r8)).view(-1)
    count = int(bad.sum().item())
    assert count == 0, (count, bad.nonzero()[:5].view(-1).tolist())


# ------------------------------------------------------------------ c. between the byte levels
def _forward_f64(x_rgb, weights):
    """Float64 forward of the shipped net on linear RGB values [P,3] (float32 values, taken as they
    are): the arithmetic of oracle.t0_numpy.cnn_reflectance_f64 behind its input stage."""
    wts = np.asarray(weights, dtype=np.float64).ravel()
    cur = np.maximum(x_rgb.astype(np.float64) @ wts[:96].reshape(32, 3).T + wts[96:128], 0)
    cat, q = [cur], 128
    for _ in range(4):
        cur = np.maximum(cur @ wts[q:q + 1024].reshape(32, 32).T + wts[q + 1024:q + 1056], 0)
        cat.append(cur)
        q += 1056
    z = np.concatenate(cat, axis=1) @ wts[q:q + 160] + wts[q + 160]
    return 1.0 / (1.0 + np.exp(-z))


def test_values_between_the_byte_levels_against_a_float64_forward(env):
    from oracle import t0_numpy
    rf, torch = env
    wts = rf.weights.load_weights()
    h, w = 64, 48
    rng = np.random.RandomState(11)
    # the test's forward is the oracle's on byte inputs
    bgr = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    lin_rgb = rf.image_utils.srgb_byte_lut()[bgr[:, :, ::-1]].reshape(-1, 3)
    assert np.array_equal(_forward_f64(lin_rgb, wts).reshape(h, w), t0_numpy.cnn_reflectance_f64(bgr, wts))
    photo = rng.rand(1, h, w, 3).astype(np.float32)                 # linear BGR, any float in [0,1)
    ref = _forward_f64(photo[0, :, :, ::-1].reshape(-1, 3), wts).reshape(h, w)
    scaled = ref * 255.0
    near_integer = np.abs(scaled - np.round(scaled)) <= TOL * 255.0
    for layout in LAYOUTS:
        x = _to_layout(torch.from_numpy(photo).cuda(), layout)
        r, r8 = rf.ops.cnn_reflectance_f32(x, layout=layout)
        r, r8 = r[0].cpu().numpy(), r8[0].cpu().numpy().astype(int)
        err = np.abs(r.astype(np.float64) - ref).max()
        print("%s: max |r - f64 forward| = %.3g" % (layout, err))
        assert err <= TOL, (layout, err)
        d8 = np.abs(r8 - np.trunc(scaled).astype(int))
        assert d8.max() <= 1 and not np.any(d8[~near_integer]), (layout, d8.max())


# ------------------------------------------------------------------ d. three values in, bits out
def _pixel_list():
    rng = np.random.RandomState(21)
    px = rng.rand(1000, 3).astype(np.float32)
    px[100:150] *= np.float32(4.0)                                  # above 1
    px[200:250] -= np.float32(0.5)                                  # some negative
    px[300:320] = np.float32(1e-40) * (1 + np.arange(60, dtype=np.float32).reshape(20, 3))   # denormal
    px[320] = (np.float32(-1e-41), np.float32(0.0), np.float32(-0.0))
    from reflectance_filtering_amd import image_utils as iu
    assert not np.isin(px, iu.srgb_byte_lut()[1:]).any()             # no byte level but (maybe) 0
    return px                                                        # [1000, 3] in B, G, R order


def test_a_pixels_bits_depend_on_its_three_values_only(env):
    rf, torch = env
    lib = rf._ffi.load_library()
    px = _pixel_list()
    assert np.any(px > 1) and np.any(px < 0) and np.any((px != 0) & (np.abs(px) < 1.1754944e-38))
    packed, _ = rf.ops._cnn_device_consts(torch, torch.device("cuda", torch.cuda.current_device()), None)

    def run(order, shape, layout, through_packed_entry=False):
        """bits of every listed pixel, in list order, from one arrangement of the list"""
        n, h, w = shape
        x = _to_layout(torch.from_numpy(px[order].reshape(n, h, w, 3)).cuda(), layout)
        if through_packed_entry:
            r = torch.empty((n, h, w), dtype=torch.float32, device="cuda")
            r8 = torch.empty((n, h, w), dtype=torch.uint8, device="cuda")
            rc = lib.rf_cnn_reflectance_packed_f32(x.data_ptr(), r.data_ptr(), r8.data_ptr(), n, h, w,
                                                   rf._ffi.CNN_LAYOUTS[layout], packed.data_ptr(),
                                                   rf._ffi.current_stream_ptr(torch))
            assert rc == rf._ffi.RF_OK
        else:
            r, r8 = rf.ops.cnn_reflectance_f32(x, layout=layout)
        back = np.empty(1000, dtype=np.int64)
        back[order] = np.arange(1000)
        return (r.cpu().numpy().ravel().view(np.uint32)[back], r8.cpu().numpy().ravel()[back])

    forward, reverse = np.arange(1000), np.arange(1000)[::-1].copy()
    base_r, base_r8 = run(forward, (1, 1, 1000), "nhwc_bgr")
    assert len(np.unique(base_r)) > 900
    for order, shape, layout, packed_entry in (
            (forward, (1, 1, 1000), "nchw_rgb", False), (reverse, (1, 1, 1000), "nhwc_bgr", False),
            (reverse, (1, 1, 1000), "nchw_rgb", False), (forward, (4, 10, 25), "nhwc_bgr", False),
            (forward, (4, 10, 25), "nchw_rgb", False), (reverse, (4, 10, 25), "nchw_rgb", False),
            (forward, (1, 1, 1000), "nchw_rgb", True), (forward, (4, 10, 25), "nhwc_bgr", True)):
        got_r, got_r8 = run(order, shape, layout, packed_entry)
        what = (shape, layout, packed_entry, order[0])
        assert np.array_equal(got_r, base_r), (what, np.flatnonzero(got_r != base_r)[:5])
        assert np.array_equal(got_r8, base_r8), what


# ------------------------------------------------------------------ e. the caller's weights
def test_callers_weights_are_used(env):
    rf, torch = env
    lib = rf._ffi.load_library()
    shipped = rf.weights.load_weights()
    mine = (shipped * np.float32(1.01)).astype(np.float32)
    x = torch.from_numpy(np.random.RandomState(31).rand(2, 3, 9, 11).astype(np.float32)).cuda()
    r, r8 = rf.ops.cnn_reflectance_f32(x, weights=mine)
    raw = torch.from_numpy(mine).cuda()
    packed = torch.empty(rf._ffi.CNN_NPACKED, dtype=torch.float32, device="cuda")
    stream = rf._ffi.current_stream_ptr(torch)
    assert lib.rf_cnn_pack_weights(raw.data_ptr(), packed.data_ptr(), stream) == rf._ffi.RF_OK
    r2 = torch.empty_like(r)
    r82 = torch.empty_like(r8)
    assert lib.rf_cnn_reflectance_packed_f32(x.data_ptr(), r2.data_ptr(), r82.data_ptr(), 2, 9, 11,
                                             rf._ffi.CNN_NCHW_RGB, packed.data_ptr(), stream) == rf._ffi.RF_OK
    assert torch.equal(r, r2) and torch.equal(r8, r82)
    # ... and the plain entry, which packs the raw weights itself on the caller's stream
    r3 = torch.empty_like(r)
    assert lib.rf_cnn_reflectance_f32(x.data_ptr(), r3.data_ptr(), None, 2, 9, 11, rf._ffi.CNN_NCHW_RGB,
                                      raw.data_ptr(), stream) == rf._ffi.RF_OK
    assert torch.equal(r, r3)
    r_shipped, _ = rf.ops.cnn_reflectance_f32(x)
    assert not torch.equal(r, r_shipped)


# ------------------------------------------------------------------ f. non-finite values stay local
def test_non_finite_inputs_stay_local(env):
    rf, torch = env
    n, h, w = 2, 13, 17
    clean = np.random.RandomState(41).rand(n, h, w, 3).astype(np.float32)
    dirty = clean.copy()
    planted = [(0, 0, 0, 0, np.nan), (0, 5, 16, 1, np.inf), (0, 12, 16, 2, -np.inf), (1, 0, 0, 2, np.nan),
               (1, 6, 3, 0, -np.inf), (1, 12, 16, 0, np.inf), (1, 12, 15, 1, np.nan)]
    touched = np.zeros((n, h, w), dtype=bool)
    for i, y, x, c, v in planted:
        dirty[i, y, x, c] = v
        touched[i, y, x] = True
    for layout in LAYOUTS:
        want_r, want_r8 = rf.ops.cnn_reflectance_f32(_to_layout(torch.from_numpy(clean).cuda(), layout), layout)
        got_r, got_r8 = rf.ops.cnn_reflectance_f32(_to_layout(torch.from_numpy(dirty).cuda(), layout), layout)
        torch.cuda.synchronize()                     # (a refusal or a failed launch would have raised)
        keep = ~touched
        assert np.array_equal(got_r.cpu().numpy().view(np.uint32)[keep],
                              want_r.cpu().numpy().view(np.uint32)[keep]), layout
        assert np.array_equal(got_r8.cpu().numpy()[keep], want_r8.cpu().numpy()[keep]), layout


# ------------------------------------------------------------------ g. the Python surface
def test_reflectance_net_and_batch_forms_on_the_device(env):
    rf, torch = env
    dc = rf.decompose_with_trained_CNN
    rng = np.random.RandomState(51)
    net = dc.ReflectanceNet()
    blob = rng.rand(2, 3, 9, 11).astype(np.float32)
    net.blobs["images"].reshape(2, 3, 9, 11)
    net.blobs["images"].data[...] = blob
    out = net.forward()["reflectance_intensity"]
    want, _ = rf.ops.cnn_reflectance_f32(torch.from_numpy(blob).cuda(), layout="nchw_rgb")
    assert out.shape == (2, 1, 9, 11) and np.array_equal(out[:, 0], want.cpu().numpy())
    # a byte-level blob keeps the byte route's bits
    bgr = rng.randint(0, 256, (2, 9, 11, 3)).astype(np.uint8)
    net.blobs["images"].data[...] = np.concatenate([dc.imgCV2_to_caffeBlob(b) for b in bgr])
    out = net.forward()["reflectance_intensity"]
    want, _ = rf.get_reflectance_batch(torch.from_numpy(bgr).cuda())
    assert np.array_equal(out[:, 0], want.cpu().numpy())
    # float photos through the batch forms
    photo = torch.from_numpy(rng.rand(2, 40, 56, 3).astype(np.float32)).cuda()
    r, r8 = rf.get_reflectance_batch(photo)
    want_r, want_r8 = rf.ops.cnn_reflectance_f32(photo, layout="nhwc_bgr")
    assert torch.equal(r, want_r) and torch.equal(r8, want_r8)
    r1 = r8.unsqueeze(-1).contiguous()
    for filter_type, sc, ss in (("bilateral", 20.0, 5.0), ("guided", 7.0, 9.0)):
        got_r8, got = dc.decompose_and_filter_batch(photo, sc, ss, filter_type=filter_type)
        want = rf.filter_reflectance.apply_filter_batch(filter_type, r1, r1, sc, ss, grey_as_bgr=True)
        assert torch.equal(got_r8, r8) and torch.equal(got, want.squeeze(-1)), filter_type
