"""GPU suite: the ragged point sweep (rf_jbf_points_ragged_u8: images of different sizes packed one
after another, one launch) and the list paths of whdr.sweep / sweep.run built on it.  Everything
is held, byte for byte, to the ORACLE run on each image alone (and the WHDR values to host
arithmetic on the oracle's bytes); no tolerance anywhere.

  a  degenerate and mixed shapes in one call, every pixel a point, radii larger than the images
  b  many points per wave (ppw 2 and 8, asserted from the plan) with waves that span three images
  c  equal sizes: the bytes of rf_jbf_points_u8; one radius-33 image
  d  whdr.sweep on an interleaved list: one ragged call, values of oracle filter -> host whdr
  e  sweep.run on photos of three sizes: the CNN once per pack, equal to the per-photo path
"""
import json

import numpy as np
import pytest

from tests.test_gpu_fuzz import _image, env  # noqa: F401  (env is a fixture)
from tests.test_gpu_points_fuzz import (B101, BCONST, BREFLECT, BREP, BWRAP, GREY_AS_BGR,
                                        TRUE_DIVISION, _host_whdr, _mismatch, _offsets,
                                        _oracle_filter, _oracle_full, _plan)

pytestmark = pytest.mark.gpu


def _every_pixel(shapes, empty, rng):
    """Every pixel of every image as a point, per image in a shuffled order; the images `empty`
    get none.  (points [total,2] (x, y), offsets [n+1])."""
    parts, counts = [], []
    for i, (h, w) in enumerate(shapes):
        if i in empty:
            counts.append(0)
            continue
        yy, xx = np.mgrid[0:h, 0:w]
        every = np.stack([xx.ravel(), yy.ravel()], axis=1)
        parts.append(every[rng.permutation(h * w)])
        counts.append(h * w)
    return np.concatenate(parts).astype(np.int32), _offsets(counts)


def _images(rng, shapes, cn, first_kind=0):
    return [_image(rng, h, w, cn, (first_kind + i) % 3) for i, (h, w) in enumerate(shapes)]


def _ragged_call(rf, torch, joints, srcs, pts, off, pairs, d=-1, border=B101, flags=0, grey=False):
    dev = (lambda images: [torch.from_numpy(np.ascontiguousarray(im)).cuda() for im in images])
    out = rf.ops.joint_bilateral_points_ragged_u8(dev(joints), dev(srcs), pts, off, pairs, d=d,
                                                  border=border, flags=flags, grey_as_bgr=grey)
    return out.cpu().numpy()


def _oracle_ragged(co, joints, srcs, pts, off, sc, ss, d, border, flags, grey):
    """The oracle on each image alone, read at that image's points: [total, scn]."""
    want = np.zeros((int(off[-1]), srcs[0].shape[-1]), np.uint8)
    for i in range(len(joints)):
        k0, k1 = int(off[i]), int(off[i + 1])
        if k1 > k0:
            full = _oracle_full(co, joints[i], srcs[i], sc, ss, d, border, flags, grey)
            want[k0:k1] = full[pts[k0:k1, 1], pts[k0:k1, 0]]
    return want


def _check(rf, co, torch, joints, srcs, pts, off, pairs, d=-1, border=B101, flags=0, grey=False,
           what=""):
    got = _ragged_call(rf, torch, joints, srcs, pts, off, pairs, d, border, flags, grey)
    assert got.shape == (len(pairs), int(off[-1]), srcs[0].shape[-1])
    for p, (sc, ss) in enumerate(pairs):
        want = _oracle_ragged(co, joints, srcs, pts, off, sc, ss, d, border, flags, grey)
        assert np.array_equal(got[p], want), _mismatch(
            got[p], want, pts, off, "%s set %d (sc %g ss %g) border %d flags %d grey %s shapes %s" % (
                what, p, sc, ss, border, flags, grey, [j.shape for j in joints]))
    return got


# ---- a. degenerate and mixed shapes in one call -------------------------------------------------

A_SHAPES = [(1, 1), (1, 17), (23, 1), (5, 7), (9, 11), (40, 33), (33, 40), (64, 48), (7, 5)]
A_EMPTY = (4, 8)                      # no points: one in the middle of the list, one at its end
# radii 9 (larger than 5x7, 1x17, 23x1 and 1x1), 3 (larger than 1x17's height) and 1; 0 counts as 1
A_PAIRS = [(20.0, 6.0), (7.0, 2.0), (60.0, 0.7), (15.0, 6.0), (0.0, 2.0)]


@pytest.mark.parametrize("border", [BCONST, BREP, BREFLECT, BWRAP, B101])
@pytest.mark.parametrize("jcn,scn,grey,flags", [
    (1, 1, False, 0), (3, 1, False, 0), (3, 3, False, 0), (1, 3, False, 0),
    (1, 1, True, 0), (1, 3, True, TRUE_DIVISION),
])
def test_mixed_and_degenerate_shapes_in_one_call_match_the_oracle(env, border, jcn, scn, grey,
                                                                  flags):
    """Nine images from 1x1 to 64x48 in one call, every pixel of seven of them a point (5,788
    points, shuffled per image; images 4 and 8 have none), radii 9, 3 and 1 so that disks cover
    whole images and fold several times at the border: a wrong width, or a base that is off by one
    image, shows as wrong bytes.  No border is left out: the oracle takes all five."""
    rf, co, torch = env
    rng = np.random.default_rng(900 + 10 * border + 3 * jcn + scn)
    joints, srcs = _images(rng, A_SHAPES, jcn), _images(rng, A_SHAPES, scn, 1)
    pts, off = _every_pixel(A_SHAPES, A_EMPTY, rng)
    assert int(off[-1]) == 5788 and off[5] == off[4] and off[9] == off[8]
    plan = _plan(A_PAIRS, -1, jcn, flags | (GREY_AS_BGR if grey else 0), 5788)
    assert [c[:3] for c in plan] == [(9, 2, 4), (3, 2, 4), (1, 1, 4)], plan   # 5788 * 3 // 4096 = 4
    _check(rf, co, torch, joints, srcs, pts, off, A_PAIRS, border=border, flags=flags, grey=grey,
           what="case a")


# ---- b. many points per wave across image boundaries --------------------------------------------

B_CYCLE = [(5, 7), (9, 4), (1, 1), (2, 1), (6, 6), (3, 11), (8, 5), (1, 3)]      # 186 pixels
B_SHAPES = B_CYCLE * 6                                                           # 1,116 points
# eight sigma_space values = 8 chunks of one set: 1116 * 8 // 4096 = 2 points per wave
B_PAIRS_2 = [(float(sc), float(ss)) for sc, ss in zip((20, 15, 4, 60, 25, 10, 7, 30),
                                                      (0.7, 1.3, 2.0, 2.7, 3.3, 4.0, 6.0, 8.0))]
# 32 sigma_space values = 32 chunks of one set: 1116 * 32 // 4096 = 8 points per wave
B_PAIRS_8 = [(float(5 + 2 * i), 0.7 + 0.23 * i) for i in range(32)]              # radii 1 .. 12


def _images_in_a_wave(off, ppw):
    """The largest number of images that have points in one wave of ppw consecutive points."""
    img_of = np.repeat(np.arange(len(off) - 1), np.diff(off))
    return max(len(set(img_of[k:k + ppw].tolist())) for k in range(0, len(img_of), ppw))


@pytest.mark.parametrize("pairs,want_ppw,jcn,scn,grey,border", [
    (B_PAIRS_2, 2, 3, 3, False, B101),
    (B_PAIRS_8, 8, 1, 1, True, BWRAP),
    (B_PAIRS_8, 8, 3, 1, False, BREFLECT),
])
def test_waves_that_span_images_of_different_sizes_match_the_oracle(env, pairs, want_ppw, jcn, scn,
                                                                    grey, border):
    """48 images of eight small shapes (1x1 to 9x4), every pixel a point: at ppw 2 and at ppw 8
    the lanes of one wave sit on two or three images with different widths and bases.  The ppw of
    every chunk is asserted from the plan the entry launches from, so a rule change fails the test
    instead of emptying it."""
    rf, co, torch = env
    rng = np.random.default_rng(1000 + want_ppw + jcn)
    joints, srcs = _images(rng, B_SHAPES, jcn), _images(rng, B_SHAPES, scn, 2)
    pts, off = _every_pixel(B_SHAPES, (), rng)
    total = int(off[-1])
    assert total == 1116 and total * len(pairs) // 4096 >= 2
    plan = _plan(pairs, -1, jcn, GREY_AS_BGR if grey else 0, total)
    assert len(plan) == len(pairs) and max(c[0] for c in plan) <= 12
    assert all(nsets == 1 and ppw == want_ppw for _, nsets, ppw, _ in plan), plan
    assert _images_in_a_wave(off, want_ppw) >= (3 if want_ppw == 8 else 2)
    assert any(b % want_ppw for b in off[1:-1])                # a wave with two images in it
    _check(rf, co, torch, joints, srcs, pts, off, pairs, border=border, grey=grey, what="case b")


# ---- c. equal sizes, and one large radius -------------------------------------------------------

def test_equal_sizes_give_the_bytes_of_the_uniform_entry(env):
    rf, co, torch = env
    rng = np.random.default_rng(1100)
    shapes = [(20, 30)] * 5
    joints, srcs = _images(rng, shapes, 3), _images(rng, shapes, 1, 1)
    pts, off = _every_pixel(shapes, (2,), rng)
    pairs = [(20.0, 4.0), (7.0, 1.0), (15.0, 4.0)]
    ragged = _check(rf, co, torch, joints, srcs, pts, off, pairs, border=BREP, what="case c")
    uniform = rf.ops.joint_bilateral_points_u8(
        torch.from_numpy(np.stack(joints)).cuda(), torch.from_numpy(np.stack(srcs)).cuda(), pts,
        off, pairs, border=BREP).cpu().numpy()
    assert np.array_equal(ragged, uniform)
    # the packed form of the arguments: the same call
    packed = rf.ops.joint_bilateral_points_ragged_u8(
        torch.from_numpy(np.stack(joints).reshape(-1, 3)).cuda(),
        torch.from_numpy(np.stack(srcs).reshape(-1, 1)).cuda(), pts, off, pairs, border=BREP,
        sizes=shapes).cpu().numpy()
    assert np.array_equal(packed, uniform)


def test_a_radius_33_image_after_a_small_one(env):
    """sigma_space 22 (radius 33, the reference's own parameter) on a single 48x64 image that is
    not the first of its call, so its base is not 0."""
    rf, co, torch = env
    rng = np.random.default_rng(1200)
    shapes = [(3, 5), (48, 64)]
    joints = _images(rng, shapes, 1)
    pts, off = _every_pixel(shapes, (0,), rng)
    _check(rf, co, torch, joints, joints, pts[::7], _offsets([0, len(pts[::7])]), [(20.0, 22.0)],
           grey=True, what="radius 33")


def test_ops_refuses_points_outside_their_own_image(env):
    rf, co, torch = env
    imgs = [torch.zeros((5, 9, 1), dtype=torch.uint8).cuda(),
            torch.zeros((9, 5, 1), dtype=torch.uint8).cuda()]
    ok = rf.ops.joint_bilateral_points_ragged_u8(imgs, imgs, [[8, 4], [4, 8]], [0, 1, 2], [(20, 2)])
    assert ok.shape == (1, 2, 1)
    with pytest.raises(IndexError):
        rf.ops.joint_bilateral_points_ragged_u8(imgs, imgs, [[4, 8], [8, 4]], [0, 1, 2], [(20, 2)])
    with pytest.raises(ValueError):
        rf.ops.joint_bilateral_points_ragged_u8(imgs, imgs[::-1], [[0, 0]], [0, 1, 1], [(20, 2)])


# ---- d. whdr.sweep on an interleaved list -------------------------------------------------------

D_SHAPES = [(43, 64), (64, 43), (48, 64), (43, 64), (64, 43), (43, 64), (48, 64), (64, 43), (43, 64)]
D_PAIRS = [(20, 8), (15, 6), (25, 4), (10, 4), (7, 2.7), (30, 1.2)]               # radii 12 .. 2
D_COUNTS = (70, 60, 0, 80, 65, 75, 1, 70, 66)                                     # comparisons


@pytest.mark.parametrize("scn", [1, 3])
def test_sweep_of_an_interleaved_list_is_one_call_and_equals_oracle_then_host_whdr(env, scn,
                                                                                   monkeypatch):
    """Nine grey maps of three IIW shapes scaled down (341x512 -> 43x64, 512x341 -> 64x43, 384x512
    -> 48x64) in an order with no two neighbours equal, ~40 judged points each, BF(CNN, CNN) over
    six pairs: float64 bit for bit host whdr on the oracle's bytes as float32 / 255, from ONE
    ragged call."""
    rf, co, torch = env
    from reflectance_filtering_amd import whdr as W
    from tests import synth
    from tests.test_gpu_jbf_points import _comparisons
    assert all(a != b for a, b in zip(D_SHAPES, D_SHAPES[1:]))
    rng = np.random.default_rng(1300)
    joint = [np.ascontiguousarray(synth.reflectance_like_u8(h, w, 1310 + i)[:, :, :1])
             for i, (h, w) in enumerate(D_SHAPES)]
    src = joint if scn == 1 else [synth.scene_u8(h, w, 1330 + i)
                                  for i, (h, w) in enumerate(D_SHAPES)]
    comps = [_comparisons(h, w, rng, m, n_points=40) for (h, w), m in zip(D_SHAPES, D_COUNTS)]
    comps[4][:, 5] = 0.0                                       # zero total weight -> 0
    comps[3][:7, 4] = 0                                        # 'E' judgements
    want = np.array([[_host_whdr(W, _oracle_filter(co, "bilateral", joint[i], src[i], sc, ss),
                                 comps[i], 0.1) for i in range(len(D_SHAPES))]
                     for sc, ss in D_PAIRS], dtype=np.float64)
    assert np.all(want[:, [2, 4]] == 0) and np.any(want > 0)
    calls = []
    real = rf.ops.joint_bilateral_points_ragged_u8

    def counting(*args, **kwargs):
        calls.append(len(kwargs["sizes"]))
        return real(*args, **kwargs)

    monkeypatch.setattr(rf.ops, "joint_bilateral_points_ragged_u8", counting)
    got = W.sweep("bilateral", src, joint, comps, D_PAIRS, grey_as_bgr=True)
    assert calls == [len(D_SHAPES)]
    assert got.dtype == np.float64 and got.shape == want.shape
    assert np.array_equal(got, want), (np.argwhere(got != want).tolist(), got[got != want],
                                       want[got != want])
    # device tensors in the list, and a list whose channel counts differ: one call per kind
    del calls[:]
    dev = [torch.from_numpy(im).cuda() for im in joint]
    assert np.array_equal(W.sweep("bilateral", dev, dev, comps, D_PAIRS, grey_as_bgr=True),
                          got if scn == 1 else W.sweep("bilateral", joint, joint, comps, D_PAIRS,
                                                       grey_as_bgr=True))
    assert calls[0] == len(D_SHAPES)


def test_guided_sweep_of_an_interleaved_list_equals_oracle_then_host_whdr(env):
    rf, co, torch = env
    from reflectance_filtering_amd import whdr as W
    from tests import synth
    from tests.test_gpu_jbf_points import _comparisons
    rng = np.random.default_rng(1400)
    shapes = D_SHAPES[:5]
    joint = [np.ascontiguousarray(synth.reflectance_like_u8(h, w, 1410 + i)[:, :, :1])
             for i, (h, w) in enumerate(shapes)]
    comps = [_comparisons(h, w, rng, 50, n_points=40) for h, w in shapes]
    pairs = [(20, 5), (3, 9)]
    want = np.array([[_host_whdr(W, _oracle_filter(co, "guided", joint[i], joint[i], sc, ss),
                                 comps[i], 0.1) for i in range(len(shapes))] for sc, ss in pairs])
    got = W.sweep("guided", joint, joint, comps, pairs, grey_as_bgr=True)
    assert np.array_equal(got, want), (got, want)


# ---- e. sweep.run on photos of three sizes ------------------------------------------------------

@pytest.mark.parametrize("guidance", ["cnn", "image"])
def test_sweep_run_on_mixed_sizes_equals_the_per_photo_path(env, tmp_path, guidance, monkeypatch):
    """Photos of three sizes with IIW judgement files beside them: the per-image WHDR matrix of
    sweep.run (one packed CNN call, one ragged filter call) equals the per-photo path - the CNN on
    each photo alone, the oracle filter on its bytes, host whdr."""
    rf, co, torch = env
    from reflectance_filtering_amd import image_utils as iu
    from reflectance_filtering_amd import sweep as sweep_cli
    from reflectance_filtering_amd import whdr as W
    from tests import synth
    from tests.test_gpu_jbf_points import _comparisons, _write_iiw_json
    rng = np.random.default_rng(1500)
    shapes = [(43, 64), (64, 43), (48, 64), (64, 43), (43, 64)]
    files = []
    for i, (h, w) in enumerate(shapes):
        path = str(tmp_path / ("%03d.png" % i))
        iu.imwrite(path, synth.scene_u8(h, w, 1510 + i))
        _write_iiw_json(sweep_cli.judgements_for(path), _comparisons(h, w, rng, 0 if i == 2 else 45),
                        h, w)
        files.append(path)
    cnn_calls = []
    real = rf.ops.cnn_reflectance_u8
    monkeypatch.setattr(rf.ops, "cnn_reflectance_u8",
                        lambda bgr, **kw: (cnn_calls.append(tuple(bgr.shape)), real(bgr, **kw))[1])
    sigma_color, sigma_spatial = [20.0, 7.0], [8.0, 2.7]
    pairs, per_image, has = sweep_cli.run(files, "bilateral", sigma_color, sigma_spatial, guidance)
    assert cnn_calls == [(1, 1, sum(h * w for h, w in shapes), 3)]
    monkeypatch.undo()
    assert pairs.tolist() == [[20, 8], [20, 2.7], [7, 8], [7, 2.7]]
    assert has.tolist() == [True, True, False, True, True]
    for i, path in enumerate(files):
        photo = iu.imread(path)
        h, w = photo.shape[:2]
        comp = W.to_pixels(W.load_judgements(sweep_cli.judgements_for(path)), h, w)
        _, r8 = rf.ops.cnn_reflectance_u8(torch.from_numpy(photo[None]).cuda(), want_float=False)
        r1 = r8[0].cpu().numpy()[:, :, None]
        joint = np.repeat(r1, 3, axis=2) if guidance == "cnn" else photo
        for p, (sc, ss) in enumerate(pairs):
            f = co.joint_bilateral_filter(joint, r1, -1, sc, ss).reshape(r1.shape)
            assert per_image[p, i] == _host_whdr(W, f, comp, 0.1), (guidance, i, p)
    assert np.all(per_image[:, 2] == 0) and np.any(per_image > 0)
    # the command line writes the same numbers
    out = str(tmp_path / "sweep.json")
    assert sweep_cli.main(["--inputs", str(tmp_path / "*.png"), "--sigma_color", "20,7",
                           "--sigma_spatial", "8,2.7", "--guidance", guidance, "--out", out]) == 0
    with open(out) as fh:
        result = json.load(fh)
    assert result["images"] == 5 and result["images_with_judgements"] == 4
    assert np.allclose(result["mean_whdr"], per_image[:, has].mean(axis=1), rtol=0, atol=0)
