"""GPU suite: the whole filtered decomposition of a list of photos
(decompose_with_trained_CNN.decompose_filter_list / _packed) and its file-to-file form
(batch.decompose_filter_files).  Every field is compared, on exact bytes, with the functions it
composes - decompose_list, decompose_and_filter_list, apply_filter_list - and the two new outputs with
the numpy oracle on float32(filtered) / 255; the files with what `decompose` followed by `filter`
writes."""
import os

import numpy as np
import pytest

from tests.test_gpu_fuzz import env  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

SHAPES = ((24, 40), (40, 24), (31, 17), (40, 24), (24, 40))
RECIPES = (("bilateral", 20.0, 4.0), ("bilateral", 20.0, 22.0), ("guided", 7.0, 5.0))


@pytest.fixture(scope="module")
def photos(env):
    rf, co, torch = env
    from tests import synth
    return [torch.from_numpy(synth.scene_u8(h, w, 4100 + i)).cuda() for i, (h, w) in enumerate(SHAPES)]


@pytest.fixture(scope="module")
def plain(env, photos):
    """decompose_list of the photos: the maps every filter below starts from."""
    rf, co, torch = env
    return rf.decompose_list(photos)


def _equal(got, want):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and a.dtype == b.dtype, i
        assert np.array_equal(a.cpu().numpy().view(np.uint8), b.cpu().numpy().view(np.uint8)), i


def test_the_unfiltered_fields_are_those_of_decompose_list(env, photos, plain):
    rf, co, torch = env
    res = rf.decompose_filter_list(photos)
    assert res._fields == ("sizes", "r", "r_u8", "reflectance", "shading", "filtered",
                           "filtered_reflectance", "filtered_shading")
    assert res.sizes.tolist() == [list(s) for s in SHAPES]
    assert res.r[0].dtype == torch.float32
    for got, want in zip((res.r, res.r_u8, res.reflectance, res.shading), plain):
        _equal(got, want)
    for photo, f, fr_, fs in zip(photos, res.filtered, res.filtered_reflectance, res.filtered_shading):
        assert f.dtype == torch.uint8 and f.shape == photo.shape[:2]
        assert fr_.shape == photo.shape and fs.shape == photo.shape[:2]
    packed = rf.decompose_filter_packed(photos)
    npx = sum(h * w for h, w in SHAPES)
    assert tuple(packed.r.shape) == (npx,) and tuple(packed.filtered.shape) == (npx,)
    assert tuple(packed.filtered_reflectance.shape) == (npx, 3) and tuple(packed.filtered_shading.shape) == (npx,)
    assert torch.equal(packed.filtered, torch.cat([f.reshape(-1) for f in res.filtered]))
    one = rf.decompose_filter_list(photos[2:3])                      # one shape is a list too
    _equal(one.filtered, res.filtered[2:3])
    _equal(one.r_u8, res.r_u8[2:3])
    short = rf.decompose_filter_list(photos, colorize_filtered=False)
    assert short.filtered_reflectance is None and short.filtered_shading is None
    _equal(short.filtered, res.filtered)


@pytest.mark.parametrize("recipe", RECIPES, ids=lambda r: "%s_c%g_s%g" % r)
def test_filtered_and_its_decomposition(env, photos, recipe):
    """`filtered` is decompose_and_filter_list's; the two new outputs are the oracle's bytes for the
    float32 map filtered / 255."""
    rf, co, torch = env
    from oracle import colorize_numpy as oc
    ft, sc, ss = recipe
    res = rf.decompose_filter_list(photos, sc, ss, ft)
    r8s, want = rf.decompose_and_filter_list(photos, sc, ss, filter_type=ft)
    _equal(res.r_u8, r8s)
    _equal(res.filtered, want)
    for i, photo in enumerate(photos):
        f = res.filtered[i].cpu().numpy()
        with np.errstate(all="ignore"):
            refl, shad = oc.colorize_srgb_u8(photo.cpu().numpy(), f.astype(np.float32) / np.float32(255))
        assert np.array_equal(res.filtered_reflectance[i].cpu().numpy(), refl), (recipe, i)
        assert np.array_equal(res.filtered_shading[i].cpu().numpy(), shad), (recipe, i)


def test_iterations_and_other_guidance_equal_apply_filter_list(env, photos, plain):
    rf, co, torch = env
    maps = [m.unsqueeze(-1).contiguous() for m in plain[1]]
    apply = rf.apply_filter_list
    grey = lambda views: [v.squeeze(-1) for v in views]
    # the map guides itself, two passes
    for ft, sc, ss in (("bilateral", 20.0, 4.0), ("guided", 7.0, 5.0)):
        res = rf.decompose_filter_list(photos, sc, ss, ft, iterations=2)
        _equal(res.filtered, grey(apply(ft, maps, maps, sc, ss, iterations=2, grey_as_bgr=True)))
        once = rf.decompose_filter_list(photos, sc, ss, ft, colorize_filtered=False)
        assert any(not torch.equal(a, b) for a, b in zip(once.filtered, res.filtered))
    # the photos guide
    for ft, sc, ss, it in (("bilateral", 20.0, 4.0, 1), ("guided", 3.0, 5.0, 1), ("bilateral", 20.0, 4.0, 2)):
        res = rf.decompose_filter_list(photos, sc, ss, ft, guidance="image", iterations=it)
        _equal(res.filtered, grey(apply(ft, maps, photos, sc, ss, iterations=it)))
    # a colour guidance list, and a grey one of one channel (three equal channels)
    from tests import synth
    flat = [torch.from_numpy(synth.scene_u8(h, w, 4200 + i)).cuda() for i, (h, w) in enumerate(SHAPES)]
    for ft, sc, ss in (("guided", 3.0, 5.0), ("bilateral", 20.0, 4.0)):
        res = rf.decompose_filter_list(photos, sc, ss, ft, guidance=flat)
        _equal(res.filtered, grey(apply(ft, maps, flat, sc, ss)))
        one = [f[..., :1].contiguous() for f in flat]
        res = rf.decompose_filter_list(photos, sc, ss, ft, guidance=one)
        _equal(res.filtered, grey(apply(ft, maps, one, sc, ss, grey_as_bgr=True)))
    # refusals
    with pytest.raises(ValueError) as err:
        rf.decompose_filter_list(photos, guidance=flat[:2] + [flat[0]] + flat[3:])
    assert "image 2" in str(err.value)
    for bad in ({"guidance": flat[:4]}, {"guidance": "photo"}, {"iterations": 0}, {"filter_type": "box"},
                {"sigma_color": 0.0}):
        with pytest.raises(ValueError):
            rf.decompose_filter_list(photos, **bad)
    with pytest.raises(ValueError):
        rf.decompose_filter_list([])


# ---- file to file ------------------------------------------------------------------------------------

FILE_SHAPES = ((43, 64), (64, 43), (48, 64), (64, 43), (43, 64), (48, 64))


def _read_all(folder):
    out = {}
    for name in sorted(os.listdir(str(folder))):
        with open(str(folder / name), "rb") as fh:
            out[name] = fh.read()
    return out


def test_decompose_filter_files(env, tmp_path):
    rf, co, torch = env
    from oracle import colorize_numpy as oc
    from reflectance_filtering_amd import batch
    from reflectance_filtering_amd import image_utils as iu
    from tests import synth
    ft, sc, ss = "bilateral", 20.0, 4.0
    dirs = {k: tmp_path / k for k in ("in", "two", "one", "devdec", "devenc", "ranks")}
    for d in dirs.values():
        d.mkdir()
    inputs, scenes = [], []
    for i, (h, w) in enumerate(FILE_SHAPES):
        inputs.append(str(dirs["in"] / ("%03d.png" % i)))
        scenes.append(synth.scene_u8(h, w, 4300 + i))
        iu.imwrite(inputs[-1], scenes[-1])
    # A: the two commands with the PNG hand-off between them
    firsts = batch.decompose_files(inputs, str(dirs["two"]), rank=0, world=1)
    batch.filter_files(ft, firsts, None, sc, ss, str(dirs["two"]), rank=0, world=1)
    two = _read_all(dirs["two"])
    # B: one pass
    written = batch.decompose_filter_files(inputs, str(dirs["one"]), ft, sc, ss, rank=0, world=1)
    one = _read_all(dirs["one"])
    names = [batch.decompose_filter_names(f, "", ft, sc, ss) for f in inputs]
    assert [os.path.basename(w) for w in written] == [n[3] for n in names]
    assert sorted(one) == sorted(n for six in names for n in six)
    assert sorted(two) == sorted(n for six in names for n in six[:4])
    for name in two:                                              # the first four kinds of file
        assert one[name] == two[name], name
    for scene, six in zip(scenes, names):                         # the two new ones
        filtered = iu.imread(str(dirs["one"] / six[3]))
        assert np.array_equal(filtered[..., 0], filtered[..., 1]) and np.array_equal(filtered[..., 0], filtered[..., 2])
        with np.errstate(all="ignore"):
            refl, shad = oc.colorize_srgb_u8(scene, filtered[..., 0].astype(np.float32) / np.float32(255))
        assert np.array_equal(iu.imread(str(dirs["one"] / six[4])), refl), six[4]
        got = iu.imread(str(dirs["one"] / six[5]))
        assert np.array_equal(got, np.repeat(shad[:, :, None], 3, axis=2)), six[5]
    # the device decoder: the same files
    batch.decompose_filter_files(inputs, str(dirs["devdec"]), ft, sc, ss, rank=0, world=1, png_decoder="device")
    assert _read_all(dirs["devdec"]) == one
    # the device encoder: the same pixels
    batch.decompose_filter_files(inputs, str(dirs["devenc"]), ft, sc, ss, rank=0, world=1, png_encoder="device")
    assert sorted(os.listdir(str(dirs["devenc"]))) == sorted(one)
    for name in one:
        assert np.array_equal(iu.imread(str(dirs["devenc"] / name)), iu.imread(str(dirs["one"] / name))), name
    # two ranks, one after the other: together the full set
    a = batch.decompose_filter_files(inputs, str(dirs["ranks"]), ft, sc, ss, rank=0, world=2)
    half = set(os.listdir(str(dirs["ranks"])))
    b = batch.decompose_filter_files(inputs, str(dirs["ranks"]), ft, sc, ss, rank=1, world=2)
    assert len(a) + len(b) == len(inputs) and not set(a) & set(b) and 0 < len(half) < len(one)
    assert _read_all(dirs["ranks"]) == one


def test_decompose_filter_files_with_guidance_files(env, tmp_path):
    """`--guidance image` and a guidance pattern write the filtered file `filter` writes with that
    guidance, two passes included."""
    rf, co, torch = env
    from reflectance_filtering_amd import batch
    from reflectance_filtering_amd import image_utils as iu
    from tests import synth
    dirs = {k: tmp_path / k for k in ("in", "flat", "two", "image", "pattern")}
    for d in dirs.values():
        d.mkdir()
    inputs = []
    for i, (h, w) in enumerate(FILE_SHAPES[:4]):
        inputs.append(str(dirs["in"] / ("%03d.png" % i)))
        iu.imwrite(inputs[-1], synth.scene_u8(h, w, 4400 + i))
        iu.imwrite(str(dirs["flat"] / ("%03d.png" % i)), synth.scene_u8(h, w, 4500 + i))
    firsts = batch.decompose_files(inputs, str(dirs["two"]), rank=0, world=1)
    for key, pattern_one, pattern_two, ft, sc, ss, it in (
            ("image", "image", str(dirs["in"] / "{base}.png"), "guided", 3.0, 5.0, 2),
            ("pattern", str(dirs["flat"] / "{name}"), str(dirs["flat"] / "{base}.png"), "bilateral", 20.0, 4.0, 1)):
        want = batch.filter_files(ft, firsts, pattern_two, sc, ss, str(dirs["two"]), iterations=it,
                                  rank=0, world=1)
        got = batch.decompose_filter_files(inputs, str(dirs[key]), ft, sc, ss, guidance_pattern=pattern_one,
                                           iterations=it, rank=0, world=1)
        assert [os.path.basename(g) for g in got] == [os.path.basename(w) for w in want]
        for g, w in zip(got, want):
            with open(g, "rb") as fg, open(w, "rb") as fw:
                assert fg.read() == fw.read(), g
