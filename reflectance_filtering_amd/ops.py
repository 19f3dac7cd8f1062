"""Batched device operators: thin, torch-tensor-in / torch-tensor-out wrappers over the C ABI.

All tensors are CUDA(HIP) uint8, contiguous, shaped [N,H,W,C] (C in {1,3}) like a stack of
``cv2.imread`` results.  Work is enqueued on torch's current stream; nothing synchronises.
"""
import numpy as np

from . import _ffi

_gf_workspaces = {}
_GF_CACHE_PER_DEVICE = 4
_GF_CACHE_BYTES_PER_DEVICE = 64 << 30     # ... and at most this much scratch kept per device
_cnn_consts = {}
_jbf_ragged_workspaces = {}
_colorize_ragged_workspaces = {}
_gf_ragged_workspaces = {}
_png_workspaces = {}
_png_decode_workspaces = {}


def release_workspaces():
    """Drop the cached guided-filter, ragged-bilateral, ragged-colourise, ragged-guided and PNG-encode
    scratch buffers and CNN constants (device memory), and the tile-flag bytes the library keeps for
    joint_bilateral_u8 (rf_jbf_release_scratch: no such call may be in flight)."""
    if _ffi._lib is not None:
        _ffi._lib.rf_jbf_release_scratch()
    _png_workspaces.clear()
    _png_decode_workspaces.clear()
    del _png_host[:]
    _gf_workspaces.clear()
    _gf_ragged_workspaces.clear()
    _jbf_ragged_workspaces.clear()
    _colorize_ragged_workspaces.clear()
    _cnn_consts.clear()
    _steps_dev.clear()


def _chk_images(t, name, torch):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8
            and t.dim() == 4 and t.is_contiguous()):
        raise ValueError("%s must be a contiguous CUDA uint8 tensor [N,H,W,C]" % name)


def joint_bilateral_u8(joint, src, d, sigma_color, sigma_space, border=_ffi.BORDER_DEFAULT,
                       flags=0, out=None, grey_as_bgr=False):
    """Batched cv2.ximgproc.jointBilateralFilter(joint, src, d, sigmaColor, sigmaSpace).
    grey_as_bgr: a 1-channel joint is filtered as the 3-equal-channel image cv2.imread would
    have produced from it (no replicated copy is made)."""
    if grey_as_bgr:
        flags |= _ffi.JBF_GREY_AS_BGR
    torch = _ffi.require_gpu()
    lib = _ffi.load_library()
    _chk_images(joint, "joint", torch)
    _chk_images(src, "src", torch)
    if joint.shape[:3] != src.shape[:3]:
        raise ValueError("joint and src must have the same N,H,W")
    if out is None:
        out = torch.empty_like(src)
    n, h, w, scn = src.shape
    rc = lib.rf_jbf_u8(joint.data_ptr(), src.data_ptr(), out.data_ptr(), n, h, w,
                       joint.shape[3], scn, int(d), float(sigma_color), float(sigma_space),
                       int(border), int(flags), _ffi.current_stream_ptr(torch))
    _ffi.check(rc, "rf_jbf_u8")
    return out


def _points_host(points, point_offsets, n):
    """int64 host copies of a point list, [total,2] (x, y) and [n+1] offsets; the offsets checked."""
    pts = np.ascontiguousarray(np.asarray(points, dtype=np.int64).reshape(-1, 2))
    off = np.asarray(point_offsets, dtype=np.int64).ravel()
    if off.shape[0] != n + 1 or off[0] != 0 or off[-1] != pts.shape[0] or np.any(np.diff(off) < 0):
        raise ValueError("point_offsets must be %d non-decreasing values from 0 to the number of "
                         "points" % (n + 1))
    return pts, off


def _points_int32(pts, off):
    if pts.shape[0] >= 2 ** 31:
        raise ValueError("too many points")
    return pts.astype(np.int32), off.astype(np.int32)


def check_points(points, point_offsets, n, h, w):
    """Host copies of a point list for images of h x w: int32 [total,2] (x, y) and int32 [n+1]
    offsets, checked (the C entry cannot read device points to check them)."""
    pts, off = _points_host(points, point_offsets, n)
    if pts.shape[0] and (pts.min() < 0 or pts[:, 0].max() >= w or pts[:, 1].max() >= h):
        raise IndexError("point outside the %dx%d images" % (w, h))
    return _points_int32(pts, off)


def _to_host(a, torch):
    return a.cpu().numpy() if torch.is_tensor(a) else a


def _points_out(sigma_pairs, total, scn, dev, torch):
    """The sigma arrays of a point call (float64 [P] each) and its output [P, total, scn]."""
    pairs = np.asarray(sigma_pairs, dtype=np.float64).reshape(-1, 2)
    if pairs.shape[0] == 0:
        raise ValueError("sigma_pairs is empty")
    sc = np.ascontiguousarray(pairs[:, 0])
    ss = np.ascontiguousarray(pairs[:, 1])
    return sc, ss, torch.empty((pairs.shape[0], total, scn), dtype=torch.uint8, device=dev)


def _points_stage(need, pts, off, dev, torch):
    """The workspace of `need` bytes and the device copies of the points and their offsets."""
    if need == 0:   # arguments the entry refuses: let it say why
        need = 1
    return (torch.empty(need, dtype=torch.uint8, device=dev), torch.from_numpy(pts).to(dev),
            torch.from_numpy(off).to(dev))


def joint_bilateral_points_u8(joint, src, points, point_offsets, sigma_pairs, d=-1,
                              border=_ffi.BORDER_DEFAULT, flags=0, grey_as_bgr=False):
    """joint_bilateral_u8 evaluated at listed pixels only, for many (sigma_color, sigma_space)
    pairs in one launch (rf_jbf_points_u8): returns CUDA uint8 [P, total, src_cn] with
    out[p, k] = joint_bilateral_u8(joint, src, d, *sigma_pairs[p], border, flags)[i, y_k, x_k],
    byte for byte, where point k = (x_k, y_k) = points[k] belongs to image i
    (point_offsets[i] <= k < point_offsets[i+1]).  points / point_offsets are host arrays (or
    tensors, copied to the host) and are checked there.  Synchronises the current stream."""
    if grey_as_bgr:
        flags |= _ffi.JBF_GREY_AS_BGR
    torch = _ffi.require_gpu()
    lib = _ffi.load_library()
    _chk_images(joint, "joint", torch)
    _chk_images(src, "src", torch)
    if joint.shape[:3] != src.shape[:3]:
        raise ValueError("joint and src must have the same N,H,W")
    n, h, w, scn = src.shape
    pts, off = check_points(_to_host(points, torch), _to_host(point_offsets, torch), n, h, w)
    total = pts.shape[0]
    sc, ss, out = _points_out(sigma_pairs, total, scn, src.device, torch)
    need = lib.rf_jbf_points_workspace_bytes(sc.shape[0], ss.ctypes.data, int(d),
                                             joint.shape[3], int(flags))
    if n == 0 or total == 0:
        return out
    ws, d_pts, d_off = _points_stage(need, pts, off, src.device, torch)
    rc = lib.rf_jbf_points_u8(joint.data_ptr(), src.data_ptr(), n, h, w, joint.shape[3], scn,
                              d_pts.data_ptr(), d_off.data_ptr(), total, sc.shape[0],
                              sc.ctypes.data, ss.ctypes.data, int(d), int(border), int(flags),
                              out.data_ptr(), ws.data_ptr(), ws.numel(),
                              _ffi.current_stream_ptr(torch))
    _ffi.check(rc, "rf_jbf_points_u8")
    return out


def check_points_ragged(points, point_offsets, sizes):
    """check_points for images of different sizes: sizes is [n,2] (h, w), and every point is held to
    the size of its own image.  Returns int32 [total,2] (x, y) and int32 [n+1] offsets."""
    sizes = np.asarray(sizes, dtype=np.int64).reshape(-1, 2)
    n = sizes.shape[0]
    pts, off = _points_host(points, point_offsets, n)
    if n and sizes.min() <= 0:
        raise ValueError("image sizes must be positive")
    hw = np.repeat(sizes, np.diff(off), axis=0)                 # the (h, w) each point is held to
    bad = np.flatnonzero((pts < 0).any(axis=1) | (pts[:, 0] >= hw[:, 1]) | (pts[:, 1] >= hw[:, 0]))
    if bad.size:
        k = int(bad[0])
        raise IndexError("point %d (x %d, y %d) outside the %dx%d image %d" % (
            k, pts[k, 0], pts[k, 1], hw[k, 1], hw[k, 0], int(np.searchsorted(off, k, "right")) - 1))
    return _points_int32(pts, off)


def pack_images(images, name, torch):
    """A list of CUDA uint8 images [H_i, W_i, C] (equal C) tightly packed one after another:
    (tensor [total pixels, C], sizes int64 [n,2] (h, w)), with one torch.cat of flattened views."""
    images = list(images)
    if not images:
        raise ValueError("%s is empty" % name)
    for t in images:
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8
                and t.dim() == 3 and t.is_contiguous() and t.shape[2] == images[0].shape[2]):
            raise ValueError("%s must be contiguous CUDA uint8 tensors [H,W,C] with equal C" % name)
    sizes = np.array([t.shape[:2] for t in images], dtype=np.int64).reshape(-1, 2)
    return torch.cat([t.view(-1, t.shape[2]) for t in images]), sizes


def _packed_pair(joints, srcs, sizes, torch):
    """The image arguments of the ragged ops as packed tensors: lists of images are packed
    (pack_images; joints is srcs stays one pack), packed tensors are checked against sizes.
    Returns (joints [total pixels, C], srcs [total pixels, C], sizes int64 [n,2] (h, w))."""
    if sizes is None:
        same = joints is srcs
        srcs, sizes = pack_images(srcs, "srcs", torch)
        if same:
            joints = srcs
        else:
            joints, jsizes = pack_images(joints, "joints", torch)
            if not np.array_equal(sizes, jsizes):
                raise ValueError("joints and srcs must have the same sizes image by image")
    else:
        sizes = np.asarray(sizes, dtype=np.int64).reshape(-1, 2)
        if sizes.shape[0] and sizes.min() <= 0:
            raise ValueError("image sizes must be positive")
        npx = int((sizes[:, 0] * sizes[:, 1]).sum())
        for t, name in ((joints, "joints"), (srcs, "srcs")):
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8
                    and t.dim() == 2 and t.is_contiguous() and t.shape[0] == npx):
                raise ValueError("%s must be a contiguous CUDA uint8 tensor [%d, C]: the pixels of "
                                 "all images" % (name, npx))
    return joints, srcs, sizes


def split_packed(packed, sizes):
    """The [H_i, W_i, C] views of a packed tensor [total pixels, C], image by image."""
    views, first = [], 0
    for h, w in np.asarray(sizes, dtype=np.int64).reshape(-1, 2).tolist():
        views.append(packed[first:first + h * w].view(h, w, packed.shape[1]))
        first += h * w
    return views


def _stream_workspace(cache, need, device, torch):
    """A scratch buffer of at least `need` bytes for the CURRENT stream of `device`, cached in `cache`
    per (device, stream) and grown on demand (work on one stream is ordered, so the next call's
    copy cannot overtake the kernels still reading the buffer)."""
    dev = device.index if device.index is not None else torch.cuda.current_device()
    key = (dev, torch.cuda.current_stream(dev).cuda_stream)
    ws = cache.get(key)
    if ws is None or ws.numel() < need:
        if len(cache) >= 16:                        # streams come and go
            cache.clear()
        ws = torch.empty(max(need, 1 << 16), dtype=torch.uint8, device=device)
        cache[key] = ws
    return ws


def _jbf_ragged_workspace(need, device, torch):
    """The tile-record scratch of joint_bilateral_ragged_u8; release_workspaces() drops it."""
    return _stream_workspace(_jbf_ragged_workspaces, need, device, torch)


def joint_bilateral_ragged_u8(joints, srcs, d, sigma_color, sigma_space, border=_ffi.BORDER_DEFAULT,
                              flags=0, grey_as_bgr=False, sizes=None, out=None):
    """joint_bilateral_u8 over images of different sizes in one call (rf_jbf_ragged_u8: radius <= 52
    runs the tiles of all images in one launch per tile shape, radius 53..468 in one launch of
    tap-row slabs; a larger radius takes one launch per image).  joints / srcs: lists of n CUDA uint8 tensors [H_i, W_i, C] (equal C within a
    list; image i of both has the same H_i, W_i), or, with sizes = [n,2] (h, w), the images
    already packed one after another as contiguous CUDA uint8 tensors [total pixels, C].
    out: the packed result buffer [total pixels, src C], if the caller has one.
    Returns (packed result [total pixels, src C], list of its [H_i, W_i, C] views); image i is,
    byte for byte, joint_bilateral_u8(joints[i][None], srcs[i][None], ...)[0].  Synchronises
    the current stream."""
    if grey_as_bgr:
        flags |= _ffi.JBF_GREY_AS_BGR
    torch = _ffi.require_gpu()
    lib = _ffi.load_library()
    joints, srcs, sizes = _packed_pair(joints, srcs, sizes, torch)
    if sizes.size and sizes.max() >= 2 ** 31:
        raise ValueError("image too large")
    if out is None:
        out = torch.empty_like(srcs)
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.uint8
              and out.is_contiguous() and out.shape == srcs.shape):
        raise ValueError("out must be a contiguous CUDA uint8 tensor shaped like the packed srcs")
    n = sizes.shape[0]
    if n == 0:
        return out, []
    hs = np.ascontiguousarray(sizes[:, 0], dtype=np.int32)
    wds = np.ascontiguousarray(sizes[:, 1], dtype=np.int32)
    need = lib.rf_jbf_ragged_workspace_bytes(n, hs.ctypes.data, wds.ctypes.data, joints.shape[1],
                                             srcs.shape[1], int(d), float(sigma_space), int(flags))
    ws = _jbf_ragged_workspace(need, srcs.device, torch)   # need == 0: the entry says why
    rc = lib.rf_jbf_ragged_u8(joints.data_ptr(), srcs.data_ptr(), out.data_ptr(), n,
                              hs.ctypes.data, wds.ctypes.data, joints.shape[1], srcs.shape[1],
                              int(d), float(sigma_color), float(sigma_space), int(border),
                              int(flags), ws.data_ptr(), ws.numel(), _ffi.current_stream_ptr(torch))
    _ffi.check(rc, "rf_jbf_ragged_u8")
    return out, split_packed(out, sizes)


def joint_bilateral_points_ragged_u8(joints, srcs, points, point_offsets, sigma_pairs, d=-1,
                                     border=_ffi.BORDER_DEFAULT, flags=0, grey_as_bgr=False,
                                     sizes=None):
    """joint_bilateral_points_u8 over images of different sizes, in one launch
    (rf_jbf_points_ragged_u8).  joints / srcs: lists of n CUDA uint8 tensors [H_i, W_i, C] (equal
    C within a list; image i of both has the same H_i, W_i), or, with sizes = [n,2] (h, w), the
    images already packed one after another as contiguous CUDA uint8 tensors [total pixels, C].
    Returns CUDA uint8 [P, total, src_cn] with
    out[p, k] = joint_bilateral_u8(joints[i][None], srcs[i][None], d, *sigma_pairs[p], ...)[0, y_k, x_k],
    byte for byte, where point k = (x_k, y_k) = points[k] belongs to image i.  points /
    point_offsets are host arrays, checked there against each image's own size.  Synchronises
    the current stream."""
    if grey_as_bgr:
        flags |= _ffi.JBF_GREY_AS_BGR
    torch = _ffi.require_gpu()
    lib = _ffi.load_library()
    joints, srcs, sizes = _packed_pair(joints, srcs, sizes, torch)
    n = sizes.shape[0]
    scn = srcs.shape[1]
    pts, off = check_points_ragged(_to_host(points, torch), _to_host(point_offsets, torch), sizes)
    if sizes.size and sizes.max() >= 2 ** 31:
        raise ValueError("image too large")
    total = pts.shape[0]
    sc, ss, out = _points_out(sigma_pairs, total, scn, srcs.device, torch)
    if n == 0 or total == 0:
        return out
    need = lib.rf_jbf_points_ragged_workspace_bytes(n, sc.shape[0], ss.ctypes.data, int(d),
                                                    joints.shape[1], int(flags))
    ws, d_pts, d_off = _points_stage(need, pts, off, srcs.device, torch)
    hs = np.ascontiguousarray(sizes[:, 0], dtype=np.int32)
    wds = np.ascontiguousarray(sizes[:, 1], dtype=np.int32)
    rc = lib.rf_jbf_points_ragged_u8(joints.data_ptr(), srcs.data_ptr(), n, hs.ctypes.data,
                                     wds.ctypes.data, joints.shape[1], scn, d_pts.data_ptr(),
                                     d_off.data_ptr(), total, sc.shape[0], sc.ctypes.data,
                                     ss.ctypes.data, int(d), int(border), int(flags),
                                     out.data_ptr(), ws.data_ptr(), ws.numel(),
                                     _ffi.current_stream_ptr(torch))
    _ffi.check(rc, "rf_jbf_points_ragged_u8")
    return out


def gf_workspace(n, h, w, scn, radius, device, torch):
    """Guided-filter scratch for the CURRENT stream of `device`, cached per (device, stream):
    two streams (or threads with their own streams) never share planes.  The cache keeps one
    buffer per key, sized by rf_gf_workspace_bytes (capped at 1/8 of the device's memory, at most
    32 GiB), at most four buffers and 64 GiB per device; release_workspaces() drops them."""
    lib = _ffi.load_library()
    need = lib.rf_gf_workspace_bytes(n, h, w, 3, scn, radius)
    dev = device.index if device.index is not None else torch.cuda.current_device()
    key = (dev, torch.cuda.current_stream(dev).cuda_stream)
    ws = _gf_workspaces.pop(key, None)       # re-inserted below: dict order = least recently used first
    if ws is None or ws.numel() < need:
        ws = None
        # streams come and go: keep at most _GF_CACHE_PER_DEVICE buffers per device (dropping a
        # buffer is safe: torch's stream-ordered allocator does not recycle the block before the
        # stream it was allocated on has passed the work that used it)
        mine = [k for k in _gf_workspaces if k[0] == dev]
        for k in mine[:max(0, len(mine) - (_GF_CACHE_PER_DEVICE - 1))]:
            del _gf_workspaces[k]
        mine = [k for k in _gf_workspaces if k[0] == dev]       # least recently used first
        held = sum(_gf_workspaces[k].numel() for k in mine)
        while mine and held + need > _GF_CACHE_BYTES_PER_DEVICE:
            held -= _gf_workspaces.pop(mine.pop(0)).numel()
        ws = torch.empty(need, dtype=torch.uint8, device=device)
    _gf_workspaces[key] = ws
    return ws


def guided_filter_u8(guide, src, radius, eps, iterations=1, out=None, workspace=None,
                     grey_as_bgr=False):
    """Batched cv2.ximgproc.guidedFilter(guide, src, radius, eps), applied `iterations` times
    with the uint8 result fed back as src (the reference's chained CLI runs).
    grey_as_bgr: the guide is [N,H,W,1] and is filtered as the 3-equal-channel image cv2.imread
    would have produced from it (rf_gf_ex_u8 with RF_GF_GREY_AS_BGR; no replicated copy is made) -
    the same bytes as the replicated guide, not OpenCV's 1-channel-guide arithmetic."""
    torch = _ffi.require_gpu()
    lib = _ffi.load_library()
    _chk_images(guide, "guide", torch)
    _chk_images(src, "src", torch)
    if guide.shape[:3] != src.shape[:3]:
        raise ValueError("guide and src must have the same N,H,W")
    if out is None:
        out = torch.empty_like(src)
    n, h, w, scn = src.shape
    if workspace is None:
        workspace = gf_workspace(n, h, w, scn, int(radius), src.device, torch)
    if grey_as_bgr:
        rc = lib.rf_gf_ex_u8(guide.data_ptr(), src.data_ptr(), out.data_ptr(), n, h, w,
                             guide.shape[3], scn, int(radius), float(eps), int(iterations),
                             _ffi.GF_GREY_AS_BGR, workspace.data_ptr(), workspace.numel(),
                             _ffi.current_stream_ptr(torch))
        _ffi.check(rc, "rf_gf_ex_u8")
        return out
    rc = lib.rf_gf_u8(guide.data_ptr(), src.data_ptr(), out.data_ptr(), n, h, w, guide.shape[3],
                      scn, int(radius), float(eps), int(iterations), workspace.data_ptr(),
                      workspace.numel(), _ffi.current_stream_ptr(torch))
    _ffi.check(rc, "rf_gf_u8")
    return out


def gf_workspace_cap(device, torch):
    """The bytes rf_gf_workspace_bytes caps a guided-filter workspace at on `device`: an eighth of its
    memory, at least 6 and at most 32 GiB."""
    total = torch.cuda.get_device_properties(device).total_memory
    return min(max(6 << 30, total // 8), 32 << 30)


def guided_filter_ragged_u8(guides, srcs, radius, eps, iterations=1, grey_as_bgr=False, sizes=None,
                            out=None):
    """guided_filter_u8 over images of different sizes in one call (rf_gf_ragged_u8: a 1-channel src
    at radius 1..128 runs stage 1, the row walk and the column walk once per pass over all images;
    anything else takes one rf_gf_ex_u8 call per image).  guides / srcs: lists of n CUDA uint8 tensors
    [H_i, W_i, C] (equal C within a list; image i of both has the same H_i, W_i; `guides is srcs`
    stays one pack: a list that guides itself), or, with sizes = [n,2] (h, w), the images already
    packed one after another as contiguous CUDA uint8 tensors [total pixels, C].
    out: the packed result buffer [total pixels, src C], if the caller has one; it may be the packed
    srcs.  The scratch holds the whole list (18 bytes per pixel and more): a long list is split by
    the caller (filter_reflectance.apply_filter_list does).
    Returns (packed result [total pixels, src C], list of its [H_i, W_i, C] views); image i is, byte
    for byte, guided_filter_u8(guides[i][None], srcs[i][None], ...)[0].  Synchronises the current
    stream."""
    flags = _ffi.GF_GREY_AS_BGR if grey_as_bgr else 0
    torch = _ffi.require_gpu()
    lib = _ffi.load_library()
    guides, srcs, sizes = _packed_pair(guides, srcs, sizes, torch)
    if sizes.size and sizes.max() >= 2 ** 31:
        raise ValueError("image too large")
    if out is None:
        out = torch.empty_like(srcs)
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.uint8
              and out.is_contiguous() and out.shape == srcs.shape):
        raise ValueError("out must be a contiguous CUDA uint8 tensor shaped like the packed srcs")
    n = sizes.shape[0]
    if n == 0:
        return out, []
    hs = np.ascontiguousarray(sizes[:, 0], dtype=np.int32)
    wds = np.ascontiguousarray(sizes[:, 1], dtype=np.int32)
    need = lib.rf_gf_ragged_workspace_bytes(n, hs.ctypes.data, wds.ctypes.data, guides.shape[1],
                                            srcs.shape[1], int(radius), flags)
    ws = _stream_workspace(_gf_ragged_workspaces, need, srcs.device, torch)  # need == 0: the entry says why
    rc = lib.rf_gf_ragged_u8(guides.data_ptr(), srcs.data_ptr(), out.data_ptr(), n, hs.ctypes.data,
                             wds.ctypes.data, guides.shape[1], srcs.shape[1], int(radius), float(eps),
                             int(iterations), flags, ws.data_ptr(), ws.numel(),
                             _ffi.current_stream_ptr(torch))
    _ffi.check(rc, "rf_gf_ragged_u8")
    return out, split_packed(out, sizes)


def guided_filter_ragged_sweep_u8(guides, srcs, radius, eps_list, grey_as_bgr=False, sizes=None, out=None):
    """guided_filter_ragged_u8 for several eps at one radius (the guided half of a parameter sweep): the
    list is packed and checked once and filtered by one rf_gf_ragged_u8 call per eps.  (A stage 1 shared
    by the eps of a radius was built and measured: it did not beat these calls by more than the
    run-to-run spread of a sweep and was taken out - DESIGN.md 3.2.)  guides / srcs / sizes: as
    guided_filter_ragged_u8.  out: the result buffer [n_eps, total pixels, src C], if the caller has
    one; it must not overlap the packed srcs.
    Returns CUDA uint8 [n_eps, total pixels, src C]; slice e is, byte for byte, the packed result of
    guided_filter_ragged_u8(guides, srcs, radius, eps_list[e]).  Synchronises the current stream."""
    torch = _ffi.require_gpu()
    guides, srcs, sizes = _packed_pair(guides, srcs, sizes, torch)
    eps = np.ascontiguousarray(eps_list, dtype=np.float64).ravel()
    shape = (eps.shape[0],) + tuple(srcs.shape)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=srcs.device)
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.uint8
              and out.is_contiguous() and tuple(out.shape) == shape):
        raise ValueError("out must be a contiguous CUDA uint8 tensor [n_eps, total pixels, src C]")
    nbytes = srcs.numel()
    if eps.shape[0] and nbytes and out.data_ptr() < srcs.data_ptr() + nbytes \
            and srcs.data_ptr() < out.data_ptr() + eps.shape[0] * nbytes:
        raise ValueError("out must not overlap srcs: every eps reads them again")
    for e in range(eps.shape[0]):
        guided_filter_ragged_u8(guides, srcs, radius, float(eps[e]), grey_as_bgr=grey_as_bgr, sizes=sizes,
                                out=out[e])
    return out


def _cnn_device_consts(torch, device, weights):
    """(packed weights, sRGB table) on `device`.  Packing is the net-load step
    (rf_cnn_pack_weights): done once for the shipped weights (cached per device), once per call
    for caller-supplied ones; the forward pass itself keeps no state in the library."""
    from . import image_utils as iu
    from . import weights as wmod
    lib = _ffi.load_library()

    def pack(w_host):
        raw = torch.from_numpy(w_host).to(device)
        packed = torch.empty(_ffi.CNN_NPACKED, dtype=torch.float32, device=device)
        _ffi.check(lib.rf_cnn_pack_weights(raw.data_ptr(), packed.data_ptr(),
                                           _ffi.current_stream_ptr(torch)), "rf_cnn_pack_weights")
        return packed                       # `raw` may go: the pack is ordered on this stream

    if weights is None:
        key = (str(device), "default")
        if key not in _cnn_consts:
            lut = torch.from_numpy(iu.srgb_byte_lut()).to(device)
            _cnn_consts[key] = (pack(wmod.load_weights()), lut)
            # other streams may use the cached copy: make it visible to all of them once
            torch.cuda.current_stream(device).synchronize()
        return _cnn_consts[key]
    w = np.ascontiguousarray(weights, dtype=np.float32).ravel()
    if w.size != _ffi.CNN_NPARAMS:
        raise ValueError("weights must hold %d floats" % _ffi.CNN_NPARAMS)
    return (pack(w), torch.from_numpy(iu.srgb_byte_lut()).to(device))


def cnn_reflectance_u8(bgr, weights=None, want_float=True, want_u8=True):
    """Batched reflectance prediction: uint8 BGR [N,H,W,3] -> (r float32 [N,H,W], r_u8 [N,H,W]).
    r_u8 = trunc(r*255) is the content of the reference's `<base>-r.png`."""
    torch = _ffi.require_gpu()
    lib = _ffi.load_library()
    _chk_images(bgr, "bgr", torch)
    if bgr.shape[3] != 3:
        raise ValueError("bgr must have 3 channels")
    n, h, w, _ = bgr.shape
    packed, lut = _cnn_device_consts(torch, bgr.device, weights)
    r = torch.empty((n, h, w), dtype=torch.float32, device=bgr.device) if want_float else None
    r8 = torch.empty((n, h, w), dtype=torch.uint8, device=bgr.device) if want_u8 else None
    rc = lib.rf_cnn_reflectance_packed_u8(bgr.data_ptr(), r.data_ptr() if want_float else None,
                                          r8.data_ptr() if want_u8 else None, n, h, w,
                                          packed.data_ptr(), lut.data_ptr(),
                                          _ffi.current_stream_ptr(torch))
    _ffi.check(rc, "rf_cnn_reflectance_packed_u8")
    return r, r8


def cnn_reflectance_f32(x, layout="nchw_rgb", weights=None, want_float=True, want_u8=True):
    """cnn_reflectance_u8 for float32 LINEAR images, i.e. whatever a Caffe blob holds: a contiguous
    CUDA float32 tensor, layout "nchw_rgb" [N,3,H,W] (channels R, G, B: blobs['images'].data) or
    "nhwc_bgr" [N,H,W,3] (channels B, G, R: the float twin of the uint8 form) -> (r float32 [N,H,W],
    r_u8 [N,H,W]).  On values that are sRGB byte levels the results are bit for bit those of
    cnn_reflectance_u8 on the bytes."""
    torch = _ffi.require_gpu()
    lib = _ffi.load_library()
    if layout not in _ffi.CNN_LAYOUTS:
        raise ValueError("layout must be 'nchw_rgb' or 'nhwc_bgr'")
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32
            and x.dim() == 4 and x.is_contiguous()):
        raise ValueError("x must be a contiguous CUDA float32 tensor [N,3,H,W] or [N,H,W,3]")
    if layout == "nchw_rgb":
        n, c, h, w = x.shape
    else:
        n, h, w, c = x.shape
    if c != 3:
        raise ValueError("x must have 3 channels (%s: dimension %d)"
                         % (layout, 1 if layout == "nchw_rgb" else 3))
    packed, _ = _cnn_device_consts(torch, x.device, weights)
    r = torch.empty((n, h, w), dtype=torch.float32, device=x.device) if want_float else None
    r8 = torch.empty((n, h, w), dtype=torch.uint8, device=x.device) if want_u8 else None
    rc = lib.rf_cnn_reflectance_packed_f32(x.data_ptr(), r.data_ptr() if want_float else None,
                                           r8.data_ptr() if want_u8 else None, n, h, w,
                                           _ffi.CNN_LAYOUTS[layout], packed.data_ptr(),
                                           _ffi.current_stream_ptr(torch))
    _ffi.check(rc, "rf_cnn_reflectance_packed_f32")
    return r, r8


_steps_dev = {}


def _srgb_steps(dev, torch):
    """iu.srgb_write_steps() on `dev`, uploaded once per device."""
    from . import image_utils as iu
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    steps = _steps_dev.get(key)
    if steps is None:
        steps = torch.from_numpy(iu.srgb_write_steps()).to(dev)
        _steps_dev[key] = steps
    return steps


def colorize_srgb_u8(images, r, want_reflectance=True, want_shading=True):
    """Device form of iu.colorize(r, image) followed by iu.imwrite(..., sRGB=True) of both
    results (/root/reference/decompose_with_trained_CNN.py:121-128): returns the uint8 bytes of
    `<base>-r_colorized.png` [N,H,W,3] (BGR) and `<base>-s_colorized.png` [N,H,W].
    images: CUDA uint8 [N,H,W,3]; r: CUDA float32 [N,H,W] (the CNN's reflectance intensity)."""
    from . import image_utils as iu
    torch = _ffi.require_gpu()
    lib = _ffi.load_library()
    _chk_images(images, "images", torch)
    if images.shape[3] != 3:
        raise ValueError("images must have 3 channels")
    if (not torch.is_tensor(r) or not r.is_cuda or r.dtype != torch.float32
            or tuple(r.shape) != tuple(images.shape[:3]) or not r.is_contiguous()):
        raise ValueError("r must be a contiguous CUDA float32 tensor [N,H,W] matching images")
    n, h, w, _ = images.shape
    dev = images.device
    steps = _srgb_steps(dev, torch)
    refl = torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev) if want_reflectance else None
    shad = torch.empty((n, h, w), dtype=torch.uint8, device=dev) if want_shading else None
    if n == 0 or (refl is None and shad is None):
        return refl, shad
    ws = torch.empty(lib.rf_colorize_workspace_bytes(n), dtype=torch.uint8, device=dev)
    rc = lib.rf_colorize_srgb_u8(images.data_ptr(), r.data_ptr(),
                                 refl.data_ptr() if refl is not None else None,
                                 shad.data_ptr() if shad is not None else None, n, h, w,
                                 iu.percentile_rank(3 * h * w), iu.percentile_rank(h * w),
                                 steps.data_ptr(), ws.data_ptr(), ws.numel(),
                                 _ffi.current_stream_ptr(torch))
    _ffi.check(rc, "rf_colorize_srgb_u8")
    return refl, shad


def _colorize_ragged(entry, images, r, r_dtype, r_kind, sizes, want_reflectance, want_shading):
    """The two ragged colourise ops: `entry` reads a map of torch dtype `r_dtype` (`r_kind` names it
    in the messages); everything else - argument checks, ranks, steps, workspace - is shared."""
    from . import image_utils as iu
    torch = _ffi.require_gpu()
    lib = _ffi.load_library()
    if sizes is None:
        r = list(r)
        images, sizes = pack_images(images, "images", torch)
        if len(r) != sizes.shape[0]:
            raise ValueError("images and r must hold the same number of images")
        for t, (h, w) in zip(r, sizes.tolist()):
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == r_dtype
                    and t.is_contiguous() and tuple(t.shape) == (h, w)):
                raise ValueError("r must be contiguous CUDA %s tensors [H,W] matching images" % r_kind)
        r = torch.cat([t.view(-1) for t in r])
    else:
        sizes = np.asarray(sizes, dtype=np.int64).reshape(-1, 2)
        if sizes.shape[0] == 0:
            raise ValueError("sizes is empty")
        if sizes.min() <= 0:
            raise ValueError("image sizes must be positive")
        npx = int((sizes[:, 0] * sizes[:, 1]).sum())
        if not (isinstance(images, torch.Tensor) and images.is_cuda and images.dtype == torch.uint8
                and images.dim() == 2 and images.is_contiguous() and images.shape[0] == npx):
            raise ValueError("images must be a contiguous CUDA uint8 tensor [%d, 3]: the pixels of "
                             "all images" % npx)
        if not (isinstance(r, torch.Tensor) and r.is_cuda and r.dtype == r_dtype
                and r.is_contiguous() and tuple(r.shape) == (npx,)):
            raise ValueError("r must be a contiguous CUDA %s tensor [%d]: the pixels of all "
                             "images" % (r_kind, npx))
    if images.shape[1] != 3:
        raise ValueError("images must have 3 channels")
    if r.device != images.device:
        raise ValueError("images and r must be on the same device")
    if sizes.max() >= 2 ** 31:
        raise ValueError("image too large")
    dev = images.device
    n, npx = sizes.shape[0], images.shape[0]
    refl = torch.empty((npx, 3), dtype=torch.uint8, device=dev) if want_reflectance else None
    shad = torch.empty((npx,), dtype=torch.uint8, device=dev) if want_shading else None
    if refl is None and shad is None:
        return None, None, [], []
    steps = _srgb_steps(dev, torch)
    hs = np.ascontiguousarray(sizes[:, 0], dtype=np.int32)
    wds = np.ascontiguousarray(sizes[:, 1], dtype=np.int32)
    counts = (sizes[:, 0] * sizes[:, 1]).tolist()
    k_refl = np.array([iu.percentile_rank(3 * c) for c in counts], dtype=np.uint64)
    k_shad = np.array([iu.percentile_rank(c) for c in counts], dtype=np.uint64)
    need = lib.rf_colorize_ragged_workspace_bytes(n, hs.ctypes.data, wds.ctypes.data)
    # need == 0: the entry says why
    ws = _stream_workspace(_colorize_ragged_workspaces, need, dev, torch)
    rc = getattr(lib, entry)(images.data_ptr(), r.data_ptr(),
                             refl.data_ptr() if refl is not None else None,
                             shad.data_ptr() if shad is not None else None, n,
                             hs.ctypes.data, wds.ctypes.data, k_refl.ctypes.data,
                             k_shad.ctypes.data, steps.data_ptr(), ws.data_ptr(),
                             ws.numel(), _ffi.current_stream_ptr(torch))
    _ffi.check(rc, entry)
    return (refl, shad, split_packed(refl, sizes) if refl is not None else [],
            [v.squeeze(-1) for v in split_packed(shad.view(-1, 1), sizes)] if shad is not None else [])


def colorize_ragged_srgb_u8(images, r, sizes=None, want_reflectance=True, want_shading=True):
    """colorize_srgb_u8 over photos of different sizes in one call (rf_colorize_ragged_srgb_u8): the
    percentile, the `max > 1` test and the NaN rule stay per image.  images: a list of n CUDA uint8
    tensors [H_i, W_i, 3] and r a list of CUDA float32 tensors [H_i, W_i], or, with sizes = [n,2]
    (h, w), the images already packed one after another as contiguous CUDA tensors: images uint8
    [total pixels, 3], r float32 [total pixels].  Returns (packed reflectance bytes [total pixels, 3]
    or None, packed shading bytes [total pixels] or None, list of reflectance views [H_i, W_i, 3],
    list of shading views [H_i, W_i]); image i is, byte for byte, colorize_srgb_u8(images[i][None],
    r[i][None]).  Synchronises the current stream."""
    torch = _ffi.require_gpu()
    return _colorize_ragged("rf_colorize_ragged_srgb_u8", images, r, torch.float32, "float32", sizes,
                            want_reflectance, want_shading)


def colorize_ragged_r8_srgb_u8(images, r8, sizes=None, want_reflectance=True, want_shading=True):
    """colorize_ragged_srgb_u8 of 8-bit reflectance maps - filtered `-r.png` bytes that are on the
    device (rf_colorize_ragged_r8_srgb_u8): r8 is a list of CUDA uint8 tensors [H_i, W_i] or, with
    sizes, one packed uint8 tensor [total pixels]; the reflectance of a pixel is the float32 nearest
    to byte / 255, formed inside the kernels.  Same returns; byte for byte what
    colorize_ragged_srgb_u8 makes of the float32 maps r8.astype(float32) / float32(255).
    Synchronises the current stream."""
    torch = _ffi.require_gpu()
    return _colorize_ragged("rf_colorize_ragged_r8_srgb_u8", images, r8, torch.uint8, "uint8", sizes,
                            want_reflectance, want_shading)


_png_host = []
_png_threads = []


def _png_host_buffer(need, torch):
    """A page-locked host buffer of at least `need` bytes for the encoder's streams on their way back
    and the decoder's raw streams on their way up (a copy from or into pageable memory runs at a
    fraction of the link's rate); release_workspaces() drops it."""
    if not _png_host or _png_host[0].numel() < need:
        del _png_host[:]
        _png_host.append(torch.empty(max(need, 1 << 20), dtype=torch.uint8, pin_memory=True))
    return _png_host[0]


def _png_pool():
    if not _png_threads:
        import os
        from concurrent.futures import ThreadPoolExecutor
        cpus = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
        _png_threads.append(ThreadPoolExecutor(max_workers=max(1, min(8, cpus))))
    return _png_threads[0]


def png_encode_ragged_u8(images, sizes=None, grey_as_rgb=False):
    """PNG files of images of different sizes, deflated on the device in one call
    (rf_png_deflate_ragged_u8: Up filter, runs and literals in one dynamic-Huffman block per chunk).
    images: a list of n CUDA uint8 tensors [H_i, W_i], [H_i, W_i, 1] (written as grey, colour type 0)
    or [H_i, W_i, 3] (BGR, written as colour type 2), all of one kind - or, with sizes = [n,2] (h, w),
    the images already packed one after another as one contiguous CUDA tensor [total pixels, C] (or
    [total pixels] for C = 1).  grey_as_rgb: one-channel images are written as colour type 2 with
    three equal samples per pixel - the file cv2.imwrite makes of np.repeat(image, 3, axis=2) -
    without that copy.  Returns a list of n `bytes`, each a complete PNG file that decodes to the
    image's pixels (its bytes differ from image_utils._png_encode's: another deflate).  What crosses
    to the host is the n + 1 stream offsets and then the compressed bytes, in one copy; the host adds
    the container (image_utils.png_container).  Synchronises the current stream."""
    from . import image_utils as iu
    torch = _ffi.require_gpu()
    lib = _ffi.load_library()
    if sizes is None:
        images = list(images)
        if not images:
            return []
        flat = []
        for t in images:
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8
                    and t.dim() in (2, 3) and t.is_contiguous()):
                raise ValueError("images must be contiguous CUDA uint8 tensors [H,W] or [H,W,C]")
            flat.append(t if t.dim() == 3 else t.unsqueeze(-1))
        images, sizes = pack_images(flat, "images", torch)
    else:
        sizes = np.asarray(sizes, dtype=np.int64).reshape(-1, 2)
        if sizes.shape[0] == 0:
            return []
        if sizes.min() <= 0:
            raise ValueError("image sizes must be positive")
        npx = int((sizes[:, 0] * sizes[:, 1]).sum())
        if not (isinstance(images, torch.Tensor) and images.is_cuda and images.dtype == torch.uint8
                and images.dim() in (1, 2) and images.is_contiguous() and images.shape[0] == npx):
            raise ValueError("images must be a contiguous CUDA uint8 tensor [%d, C]: the pixels of "
                             "all images" % npx)
        if images.dim() == 1:
            images = images.view(-1, 1)
    if sizes.max() >= 2 ** 31:
        raise ValueError("image too large")
    cn = int(images.shape[1])
    flags = _ffi.PNG_GREY_AS_RGB if grey_as_rgb else 0
    dev = images.device
    n = sizes.shape[0]
    hs = np.ascontiguousarray(sizes[:, 0], dtype=np.int32)
    wds = np.ascontiguousarray(sizes[:, 1], dtype=np.int32)
    args = (n, hs.ctypes.data, wds.ctypes.data, cn, flags)
    bound = lib.rf_png_stream_bound(*args)
    need = lib.rf_png_workspace_bytes(*args)
    # bound == 0 or need == 0: the entry says why.  One cached buffer: workspace, offsets, streams.
    up = lambda b: (b + 255) & ~255
    off_at = up(need)
    str_at = off_at + up(8 * (n + 1))
    buf = _stream_workspace(_png_workspaces, str_at + max(bound, 1), dev, torch)
    offsets = buf[off_at:off_at + 8 * (n + 1)].view(torch.int64)
    rc = lib.rf_png_deflate_ragged_u8(images.data_ptr(), n, hs.ctypes.data, wds.ctypes.data, cn, flags,
                                      buf.data_ptr() + str_at, bound, offsets.data_ptr(),
                                      buf.data_ptr(), need, _ffi.current_stream_ptr(torch))
    _ffi.check(rc, "rf_png_deflate_ragged_u8")
    off = offsets.cpu().numpy()
    if off[0] != 0 or np.any(np.diff(off) <= 0) or off[-1] > bound:
        raise _ffi.RFError("rf_png_deflate_ragged_u8 returned stream offsets outside its bound")
    used = int(off[-1])
    host = _png_host_buffer(used, torch)
    host[:used].copy_(buf[str_at:str_at + used], non_blocking=True)
    torch.cuda.current_stream(dev).synchronize()
    data = host.numpy()
    ctype = 2 if (cn == 3 or grey_as_rgb) else 0
    jobs = [(data[int(off[i]):int(off[i + 1])], int(h), int(w), ctype)
            for i, (h, w) in enumerate(sizes.tolist())]
    if used < (1 << 20) or n == 1:
        return [iu.png_container(*job) for job in jobs]
    # the checksums of large streams run side by side (zlib.crc32 releases the GIL); every file is a
    # copy of its own, so the host buffer is free again when the call returns
    return list(_png_pool().map(lambda job: iu.png_container(*job), jobs))


def png_decode_ragged_u8(parsed):
    """The pixels of PNG files of different sizes and formats, reconstructed and unpacked on the
    device in one call (rf_png_unfilter_ragged_u8: the row filters undone as a skewed wavefront, the
    samples unpacked to BGR).  parsed: a list of n image_utils.png_parse results (height, width, bit
    depth, colour type, palette or None, raw bytes).  The raw streams (and the palettes, if any)
    cross in one upload from one page-locked staging buffer; what comes back is the n flag bytes.
    Returns (images, grey): a list of n CUDA uint8 [H_i, W_i, 3] views (BGR, what image_utils.imread
    returns for the file) of one packed tensor, and a list of n bools - the image's three channels
    are equal at every pixel.  Raises RFError naming the image if a row's filter byte is above 4.
    Synchronises the current stream."""
    torch = _ffi.require_gpu()
    lib = _ffi.load_library()
    parsed = list(parsed)
    n = len(parsed)
    if n == 0:
        return [], []
    hs = np.ascontiguousarray([p[0] for p in parsed], dtype=np.int32)
    wds = np.ascontiguousarray([p[1] for p in parsed], dtype=np.int32)
    fmts = np.ascontiguousarray([(int(p[2]) << 8) | int(p[3]) for p in parsed], dtype=np.int32)
    offs = np.zeros(n + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(p[5]) for p in parsed], dtype=np.uint64)
    total = int(offs[-1])
    with_palette = [i for i, p in enumerate(parsed) if p[4] is not None]
    up = lambda b: (b + 255) & ~255
    pal_bytes = 768 * n if with_palette else 0
    staged = up(total) + pal_bytes
    host = _png_host_buffer(staged, torch)
    data = host.numpy()
    for i, p in enumerate(parsed):
        data[int(offs[i]):int(offs[i + 1])] = np.frombuffer(p[5], np.uint8)
    if with_palette:
        pals = data[up(total):staged].reshape(n, 768)
        pals[:] = 0
        for i in with_palette:
            entries = np.asarray(parsed[i][4], dtype=np.uint8).reshape(-1)[:768]
            pals[i, :entries.size] = entries
    need = lib.rf_png_unfilter_workspace_bytes(n, hs.ctypes.data, wds.ctypes.data, fmts.ctypes.data)
    # need == 0: the entry says why.  One cached buffer: workspace, flags, raw streams, palettes.
    dev = torch.device("cuda", torch.cuda.current_device())
    flags_at = up(need)
    raw_at = flags_at + up(n)
    buf = _stream_workspace(_png_decode_workspaces, raw_at + staged, dev, torch)
    buf[raw_at:raw_at + staged].copy_(host[:staged], non_blocking=True)
    npx = int((hs.astype(np.int64) * wds.astype(np.int64)).sum())
    packed = torch.empty((max(npx, 0), 3), dtype=torch.uint8, device=dev)
    rc = lib.rf_png_unfilter_ragged_u8(buf.data_ptr() + raw_at, offs.ctypes.data, n, hs.ctypes.data,
                                       wds.ctypes.data, fmts.ctypes.data,
                                       buf.data_ptr() + raw_at + up(total) if with_palette else None,
                                       packed.data_ptr(), buf.data_ptr() + flags_at, buf.data_ptr(),
                                       need, _ffi.current_stream_ptr(torch))
    if rc != _ffi.RF_OK:   # refused before its synchronisation: the upload still reads the staging buffer
        torch.cuda.current_stream(dev).synchronize()
    _ffi.check(rc, "rf_png_unfilter_ragged_u8")
    flags = buf[flags_at:flags_at + n].cpu().numpy()
    bad = np.flatnonzero(flags & _ffi.PNG_FLAG_BAD_FILTER)
    if bad.size:
        raise _ffi.RFError("rf_png_unfilter_ragged_u8: image %d has a row filter byte above 4"
                           % int(bad[0]))
    sizes = np.stack([hs, wds], axis=1)
    return split_packed(packed, sizes), [bool(f & _ffi.PNG_FLAG_GREY) for f in flags]


def _chk_images_f32(t, name, torch):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32
            and t.dim() == 4 and t.is_contiguous()):
        raise ValueError("%s must be a contiguous CUDA float32 tensor [N,H,W,C]" % name)


def joint_bilateral_f32(joint, src, d, sigma_color, sigma_space, border=_ffi.BORDER_DEFAULT,
                        out=None):
    """Batched cv2.ximgproc.jointBilateralFilter on float32 images (CV_32F path: interpolated
    colour table over each joint image's value range).  Synchronises the current stream."""
    torch = _ffi.require_gpu()
    lib = _ffi.load_library()
    _chk_images_f32(joint, "joint", torch)
    _chk_images_f32(src, "src", torch)
    if joint.shape[:3] != src.shape[:3]:
        raise ValueError("joint and src must have the same N,H,W")
    if out is None:
        out = torch.empty_like(src)
    n, h, w, scn = src.shape
    ws = torch.empty(max(1, lib.rf_jbf_f32_workspace_bytes(n, joint.shape[3])), dtype=torch.uint8,
                     device=src.device)
    rc = lib.rf_jbf_f32(joint.data_ptr(), src.data_ptr(), out.data_ptr(), n, h, w, joint.shape[3],
                        scn, int(d), float(sigma_color), float(sigma_space), int(border),
                        ws.data_ptr(), ws.numel(), _ffi.current_stream_ptr(torch))
    _ffi.check(rc, "rf_jbf_f32")
    return out


def guided_filter_f32(guide, src, radius, eps, iterations=1, out=None):
    """Batched cv2.ximgproc.guidedFilter on float32 guide/src: float32 result, no rounding."""
    torch = _ffi.require_gpu()
    lib = _ffi.load_library()
    _chk_images_f32(guide, "guide", torch)
    _chk_images_f32(src, "src", torch)
    if guide.shape[:3] != src.shape[:3]:
        raise ValueError("guide and src must have the same N,H,W")
    if out is None:
        out = torch.empty_like(src)
    n, h, w, scn = src.shape
    ws = torch.empty(max(1, lib.rf_gf_f32_workspace_bytes(n, h, w, 3, scn, int(radius))),
                     dtype=torch.uint8, device=src.device)
    rc = lib.rf_gf_f32(guide.data_ptr(), src.data_ptr(), out.data_ptr(), n, h, w, guide.shape[3],
                       scn, int(radius), float(eps), int(iterations), ws.data_ptr(), ws.numel(),
                       _ffi.current_stream_ptr(torch))
    _ffi.check(rc, "rf_gf_f32")
    return out


class CapturedCall(object):
    """A fixed sequence of operator calls captured once into a HIP graph and replayed.

    The launch-bound cases (single small images: the 3x guided-filter chain is 16 launches, the
    colourise path 18) pay one graph launch instead.  `fn` must only call operators of this
    module on pre-allocated tensors (out= arguments, an explicit guided-filter workspace): it is
    run once eagerly first, so that the parameter tables a call uploads on first use exist
    before the capture, then captured on a side stream.  rf_jbf_f32 cannot be captured (it
    synchronises).  replay() re-runs the sequence on the same buffers."""

    def __init__(self, fn):
        torch = _ffi.require_gpu()
        self._torch = torch
        fn()                                   # warm-up: table uploads, kernel attribute calls
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.result = fn()

    def replay(self):
        self.graph.replay()
        return self.result
