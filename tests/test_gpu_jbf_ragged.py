"""GPU suite: the ragged full-image joint bilateral (rf_jbf_ragged_u8: images of different sizes
packed one after another, one launch per tile class) and the list paths built on it
(filter_reflectance.apply_filter_list, decompose_and_filter_list, batch.filter_files).  Everything
is held, byte for byte, to the ORACLE run on each image alone; no tolerance anywhere.

  a  degenerate and mixed shapes in one call, all four tile classes, guard bytes around dst
  b  radius 42 (row pitch 176)
  c  the routes that fall back to one launch per image: radius 54, RF_JBF_FORCE_GENERIC
  d  equal sizes: the bytes of the uniform entry
  e  apply_filter_list: two bilateral passes; guided against apply_filter_batch per shape group
  f  decompose_and_filter_list against decompose_and_filter_batch per photo
  g  batch.filter_files on a directory of three shapes against read_filter_write per file
"""
import os

import numpy as np
import pytest

from tests.test_gpu_fuzz import _image, env  # noqa: F401  (env is a fixture)
from tests.test_gpu_points_fuzz import (B101, BCONST, BREFLECT, BREP, BWRAP, FORCE_GENERIC,
                                        GREY_AS_BGR, TRUE_DIVISION, _oracle_full)

pytestmark = pytest.mark.gpu

GUARD = 4096
SENTINEL = 0xA5


def _images(rng, shapes, cn, first_kind=0):
    """Kinds alternate (smooth, posterised, noise), so neighbours in the pack differ strongly:
    a read into the neighbouring image changes bytes."""
    return [_image(rng, h, w, cn, (first_kind + i) % 3) for i, (h, w) in enumerate(shapes)]


def _plan(rf, shapes, jcn, scn, sc, ss, flags=0, grey=False):
    return rf._ffi.jbf_ragged_plan(shapes, jcn, scn, -1, sc, ss, flags | (GREY_AS_BGR if grey else 0))


def _ragged(rf, torch, joints, srcs, sc, ss, border=B101, flags=0, grey=False):
    """One ragged call into a dst with GUARD sentinel bytes on either side; returns the images."""
    scn = srcs[0].shape[2]
    total = sum(s.shape[0] * s.shape[1] for s in srcs)
    dev = (lambda images: [torch.from_numpy(np.ascontiguousarray(im)).cuda() for im in images])
    buf = torch.full((total * scn + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    out = buf[GUARD:GUARD + total * scn].view(total, scn)
    packed, views = rf.ops.joint_bilateral_ragged_u8(dev(joints), dev(srcs), -1, sc, ss,
                                                     border=border, flags=flags, grey_as_bgr=grey,
                                                     out=out)
    assert packed.data_ptr() == out.data_ptr() and len(views) == len(srcs)
    host = buf.cpu().numpy()
    assert np.all(host[:GUARD] == SENTINEL), "bytes before dst were written"
    assert np.all(host[GUARD + total * scn:] == SENTINEL), "bytes after dst were written"
    return [v.cpu().numpy() for v in views]


def _check(rf, co, torch, joints, srcs, sc, ss, border=B101, flags=0, grey=False, what=""):
    got = _ragged(rf, torch, joints, srcs, sc, ss, border, flags, grey)
    for i, (g, j, s) in enumerate(zip(got, joints, srcs)):
        want = _oracle_full(co, j, s, sc, ss, -1, border, flags, grey)
        assert g.shape == want.shape
        bad = np.argwhere((g != want).any(axis=2))
        assert bad.size == 0, "%s image %d %s sc %g ss %g border %d flags %d grey %s: %d pixels " \
            "differ, first (y %d, x %d) got %s want %s" % (
                what, i, s.shape, sc, ss, border, flags, grey, len(bad), bad[0][0], bad[0][1],
                g[tuple(bad[0])], want[tuple(bad[0])])
    return got


# ---- a. degenerate and mixed shapes in one call -------------------------------------------------

A_SHAPES = [(1, 1), (1, 70), (70, 1), (64, 64), (65, 65), (81, 200), (112, 520), (7, 5)]
ROWS = [(1, 1, False, 0), (3, 1, False, 0), (3, 3, False, 0), (1, 3, False, 0),
        (1, 1, True, 0), (1, 3, True, TRUE_DIVISION)]


@pytest.mark.parametrize("border", [BCONST, BREP, BREFLECT, BWRAP, B101])
@pytest.mark.parametrize("jcn,scn,grey,flags", ROWS)
def test_mixed_and_degenerate_shapes_in_one_call_match_the_oracle(env, border, jcn, scn, grey, flags):
    """Eight images from 1x1 to 112x520 in one call, at sigma_space 22 (radius 33: larger than five
    of the images, so their disks fold several times at the border) and at sigma_space 2.  A wrong
    width, or a base that is off by one image, shows as wrong bytes; the sentinel bytes around dst
    show a store outside it.  No border is left out: the oracle takes all five."""
    rf, co, torch = env
    rng = np.random.default_rng(2000 + 10 * border + 3 * jcn + scn)
    joints, srcs = _images(rng, A_SHAPES, jcn), _images(rng, A_SHAPES, scn, 1)
    plan = _plan(rf, A_SHAPES, jcn, scn, 20.0, 22.0, flags, grey)
    if scn == 1:     # all four tile classes run
        assert [c[:3] for c in plan] == [(64, 64, 144), (32, 128, 208), (16, 256, 336),
                                         (128, 32, 136)], plan
    else:
        assert [c[:3] for c in plan] == [(64, 64, 144), (32, 128, 208)], plan
    for sc, ss in ((20.0, 22.0), (12.0, 2.0)):
        _check(rf, co, torch, joints, srcs, sc, ss, border=border, flags=flags, grey=grey,
               what="case a")


def test_one_pack_as_joint_and_src_and_the_packed_form_of_the_arguments(env):
    rf, co, torch = env
    rng = np.random.default_rng(2100)
    shapes = [(7, 5), (81, 200), (1, 70)]
    imgs = _images(rng, shapes, 1)
    dev = [torch.from_numpy(im).cuda() for im in imgs]
    _, views = rf.ops.joint_bilateral_ragged_u8(dev, dev, -1, 20.0, 22.0, grey_as_bgr=True)
    for v, im in zip(views, imgs):
        assert np.array_equal(v.cpu().numpy(), _oracle_full(co, im, im, 20.0, 22.0, -1, B101, 0, True))
    pack = torch.cat([t.view(-1, 1) for t in dev])
    packed, views2 = rf.ops.joint_bilateral_ragged_u8(pack, pack, -1, 20.0, 22.0, grey_as_bgr=True,
                                                      sizes=shapes)
    assert packed.shape == pack.shape
    assert all(torch.equal(a, b) for a, b in zip(views, views2))
    with pytest.raises(ValueError):
        rf.ops.joint_bilateral_ragged_u8(dev, dev[::-1], -1, 20.0, 22.0)
    with pytest.raises(ValueError):
        rf.ops.joint_bilateral_ragged_u8(pack, pack, -1, 20.0, 22.0, sizes=shapes[:2])
    with pytest.raises(ValueError):
        rf.ops.joint_bilateral_ragged_u8(dev, dev, -1, 20.0, 22.0, out=pack[:-1])
    rf.ops.release_workspaces()
    _, views3 = rf.ops.joint_bilateral_ragged_u8(dev, dev, -1, 20.0, 22.0, grey_as_bgr=True)
    assert all(torch.equal(a, b) for a, b in zip(views, views3))


# ---- b. radius 42 ---------------------------------------------------------------------------------

@pytest.mark.parametrize("jcn,scn,grey", [(1, 1, True), (3, 3, False), (3, 1, False)])
def test_radius_42_at_pitch_176_matches_the_oracle(env, jcn, scn, grey):
    """The reference's c15 s28: 64x64 tiles alone at row pitch 176; the colour src takes the
    one-pass colour tile, 130 rows leave a tile of two rows."""
    rf, co, torch = env
    shapes = [(81, 200), (64, 64), (130, 70)]
    rng = np.random.default_rng(2200 + jcn + scn)
    joints, srcs = _images(rng, shapes, jcn, 2), _images(rng, shapes, scn)
    assert _plan(rf, shapes, jcn, scn, 15.0, 28.0, 0, grey) == [(64, 64, 176, 8 + 1 + 6)]
    _check(rf, co, torch, joints, srcs, 15.0, 28.0, border=BREFLECT, grey=grey, what="case b")


# ---- c. the fall-back: one launch per image ---------------------------------------------------

@pytest.mark.parametrize("ss,flags", [(36.0, 0), (22.0, FORCE_GENERIC)])
@pytest.mark.parametrize("jcn,scn,grey", [(1, 1, True), (3, 3, False)])
def test_the_fallback_routes_write_the_same_bytes(env, ss, flags, jcn, scn, grey):
    rf, co, torch = env
    shapes = [(70, 90), (1, 1), (64, 64)]
    rng = np.random.default_rng(2300 + jcn)
    joints, srcs = _images(rng, shapes, jcn), _images(rng, shapes, scn, 1)
    assert _plan(rf, shapes, jcn, scn, 20.0, ss, flags, grey) is None
    _check(rf, co, torch, joints, srcs, 20.0, ss, border=BWRAP, flags=flags, grey=grey,
           what="case c")


# ---- d. equal sizes ---------------------------------------------------------------------------------

@pytest.mark.parametrize("jcn,scn,grey", [(1, 1, True), (3, 3, False)])
def test_equal_sizes_give_the_bytes_of_the_uniform_entry(env, jcn, scn, grey):
    rf, co, torch = env
    shapes = [(81, 200)] * 3
    rng = np.random.default_rng(2400 + jcn)
    joints, srcs = _images(rng, shapes, jcn), _images(rng, shapes, scn, 1)
    ragged = _ragged(rf, torch, joints, srcs, 20.0, 22.0, grey=grey)
    uniform = rf.ops.joint_bilateral_u8(torch.from_numpy(np.stack(joints)).cuda(),
                                        torch.from_numpy(np.stack(srcs)).cuda(), -1, 20.0, 22.0,
                                        grey_as_bgr=grey).cpu().numpy()
    assert uniform.shape == (3, 81, 200, scn)
    assert np.array_equal(np.stack(ragged), uniform)


# ---- e. apply_filter_list ---------------------------------------------------------------------------

E_SHAPES = [(43, 64), (64, 43), (48, 64), (43, 64), (64, 43), (48, 64), (43, 64)]


def test_two_bilateral_passes_over_an_interleaved_list_match_the_oracle_applied_twice(env,
                                                                                      monkeypatch):
    rf, co, torch = env
    from reflectance_filtering_amd import filter_reflectance as fr
    rng = np.random.default_rng(2500)
    joints, srcs = _images(rng, E_SHAPES, 3), _images(rng, E_SHAPES, 3, 1)
    calls = []
    real = rf.ops.joint_bilateral_ragged_u8
    monkeypatch.setattr(rf.ops, "joint_bilateral_ragged_u8",
                        lambda *a, **kw: (calls.append(len(kw["sizes"])), real(*a, **kw))[1])
    dev = (lambda images: [torch.from_numpy(im).cuda() for im in images])
    got = fr.apply_filter_list("bilateral", dev(srcs), dev(joints), 20.0, 22.0, iterations=2)
    assert calls == [len(E_SHAPES)] * 2                          # one ragged call per pass
    for g, j, s in zip(got, joints, srcs):
        once = _oracle_full(co, j, s, 20.0, 22.0, -1, B101, 0, False)
        assert np.array_equal(g.cpu().numpy(), _oracle_full(co, j, once, 20.0, 22.0, -1, B101, 0, False))
    # three passes end in the first buffer again; a grey list filtered by itself
    greys = _images(rng, E_SHAPES[:4], 1)
    got = fr.apply_filter_list("bilateral", dev(greys), dev(greys), 20.0, 5.0, iterations=3,
                               grey_as_bgr=True)
    for g, im in zip(got, greys):
        want = im
        for _ in range(3):
            want = _oracle_full(co, im, want, 20.0, 5.0, -1, B101, 0, True)
        assert np.array_equal(g.cpu().numpy(), want)


def test_guided_over_an_interleaved_list_equals_the_batch_per_shape_group(env):
    rf, co, torch = env
    from reflectance_filtering_amd import filter_reflectance as fr
    rng = np.random.default_rng(2600)
    joints, srcs = _images(rng, E_SHAPES, 3), _images(rng, E_SHAPES, 3, 1)
    dev = (lambda images: [torch.from_numpy(im).cuda() for im in images])
    got = fr.apply_filter_list("guided", dev(srcs), dev(joints), 3.0, 9.0, iterations=2)
    assert len(got) == len(E_SHAPES)
    for shape in sorted(set(E_SHAPES)):
        idx = [i for i, s in enumerate(E_SHAPES) if s == shape]
        want = fr.apply_filter_batch("guided", torch.from_numpy(np.stack([srcs[i] for i in idx])).cuda(),
                                     torch.from_numpy(np.stack([joints[i] for i in idx])).cuda(),
                                     3.0, 9.0, iterations=2)
        for k, i in enumerate(idx):
            assert torch.equal(got[i], want[k]), (shape, i)


# ---- f. decompose_and_filter_list ---------------------------------------------------------------------

@pytest.mark.parametrize("filter_type,sc,ss", [("bilateral", 20.0, 22.0), ("guided", 7.0, 9.0)])
def test_decompose_and_filter_list_equals_the_batch_per_photo(env, filter_type, sc, ss):
    rf, co, torch = env
    from tests import synth
    shapes = [(43, 64), (64, 43), (48, 64), (64, 43), (81, 70)]
    photos = [torch.from_numpy(synth.scene_u8(h, w, 2700 + i)).cuda() for i, (h, w) in enumerate(shapes)]
    r8s, outs = rf.decompose_and_filter_list(photos, sc, ss, filter_type=filter_type)
    assert len(r8s) == len(outs) == len(shapes)
    for photo, r8, out in zip(photos, r8s, outs):
        want_r8, want = rf.decompose_and_filter_batch(photo[None], sc, ss, filter_type=filter_type)
        assert r8.shape == photo.shape[:2] and torch.equal(r8, want_r8[0])
        assert torch.equal(out, want[0])


# ---- g. batch.filter_files ------------------------------------------------------------------------------

@pytest.mark.parametrize("guided_by", ["itself", "photo"])
def test_filter_files_on_three_shapes_writes_the_files_of_the_single_image_tool(env, tmp_path,
                                                                                guided_by,
                                                                                monkeypatch):
    """Six PNGs in three shapes, no two neighbours equal: one step of batch.filter_files goes
    through apply_filter_list; the files are those of read_filter_write, file by file."""
    rf, co, torch = env
    from reflectance_filtering_amd import batch
    from reflectance_filtering_amd import filter_reflectance as fr
    from reflectance_filtering_amd import image_utils as iu
    from tests import synth
    shapes = [(43, 64), (64, 43), (48, 64), (64, 43), (43, 64), (48, 64)]
    src_dir, out_a, out_b = tmp_path / "in", tmp_path / "list", tmp_path / "single"
    for d in (src_dir, out_a, out_b):
        d.mkdir()
    inputs = []
    for i, (h, w) in enumerate(shapes):
        iu.imwrite(str(src_dir / ("%03d.png" % i)), synth.scene_u8(h, w, 2800 + i))
        path = str(src_dir / ("%03d-r.png" % i))
        iu.imwrite(path, synth.reflectance_like_u8(h, w, 2810 + i)[:, :, 0])
        inputs.append(path)
    pattern = None if guided_by == "itself" else str(src_dir / "{base}.png")
    lists = []
    real = fr.apply_filter_list
    monkeypatch.setattr(fr, "apply_filter_list",
                        lambda *a, **kw: (lists.append(len(a[1])), real(*a, **kw))[1])
    written = batch.filter_files("bilateral", inputs, pattern, 20.0, 22.0, str(out_a), rank=0, world=1)
    assert lists == [len(shapes)]
    assert [os.path.basename(f) for f in written] == ["%03d-r_bilateral_c20.0s22.0.png" % i
                                                      for i in range(len(shapes))]
    for f in inputs:
        fr.read_filter_write("bilateral", f, batch.guidance_for(f, pattern), 20.0, 22.0, str(out_b))
    for f in written:
        with open(f, "rb") as fa, open(str(out_b / os.path.basename(f)), "rb") as fb:
            assert fa.read() == fb.read(), f
    # a step of one shape keeps the batch calls
    del lists[:]
    batch.filter_files("bilateral", [inputs[1], inputs[3]], pattern, 20.0, 22.0, str(out_a),
                       rank=0, world=1)
    assert lists == []
