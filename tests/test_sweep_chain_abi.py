"""CPU suite: the host logic of the chained WHDR sweep (whdr.sweep(iterations=K)) and of the sweep
tool's stored sources, guidance files, loader and options (reflectance_filtering_amd.sweep).  Stubs
only, no compute calls: what is held here is which op is called how often, on what, in which order,
and what is refused before any of them is called."""
import json
import random
import threading
import time

import numpy as np
import pytest

from reflectance_filtering_amd import image_utils as iu
from reflectance_filtering_amd import sweep as sweep_cli
from reflectance_filtering_amd import whdr

SHAPES = [(341, 512), (512, 341), (341, 512), (384, 512), (512, 341)]
COMP = np.array([[0, 0, 1, 1, 1, 1.0]])
BASE = ["--inputs", "x.png", "--sigma_color", "20", "--sigma_spatial", "22"]


# ---- parser ---------------------------------------------------------------------------------------

def test_new_options_and_their_defaults():
    args = sweep_cli.build_parser().parse_args(BASE)
    assert (args.src_files, args.guidance_files, args.iterations, args.png_decoder) == \
        (None, None, 1, "host")
    args = sweep_cli.build_parser().parse_args(
        BASE + ["--src_files", "{dir}/zoran/{stem}.png", "--guidance_files", "{dir}/flat/{base}.png",
                "--iterations", "3", "--png_decoder", "device"])
    assert args.src_files == "{dir}/zoran/{stem}.png" and args.guidance_files == "{dir}/flat/{base}.png"
    assert args.iterations == 3 and args.png_decoder == "device"


@pytest.mark.parametrize("bad", [["--iterations", "0"], ["--iterations", "-2"], ["--iterations", "x"],
                                 ["--png_decoder", "x"], ["--guidance", "flat"]])
def test_bad_option_values_are_argparse_errors(bad):
    good = [bad[0], {"--iterations": "2", "--png_decoder": "device", "--guidance": "image"}[bad[0]]]
    args = sweep_cli.build_parser().parse_args(BASE + ["--iterations", "1"] + good)
    assert getattr(args, bad[0][2:]) in (2, "device", "image")      # the option exists ...
    with pytest.raises(SystemExit):                                 # ... and refuses this value
        sweep_cli.build_parser().parse_args(BASE + bad)


def test_a_command_line_without_new_options_parses_as_before():
    args = sweep_cli.build_parser().parse_args(
        ["--inputs", "a/*.png", "b.png", "--filter_type", "guided", "--sigma_color", "3,7",
         "--sigma_spatial", "45,52", "--guidance", "image", "--delta", "0.2", "--out", "o.json",
         "--per_image", "o.npz"])
    assert args.iterations == 1     # (a new option: the rest is the namespace of the parent's parser)
    old = {k: v for k, v in vars(args).items()
           if k not in ("src_files", "guidance_files", "iterations", "png_decoder")}
    assert old == {"inputs": ["a/*.png", "b.png"], "filter_type": "guided", "sigma_color": [3.0, 7.0],
                   "sigma_spatial": [45.0, 52.0], "guidance": "image", "delta": 0.2, "out": "o.json",
                   "per_image": "o.npz"}
    args = sweep_cli.build_parser().parse_args(BASE)
    assert (args.filter_type, args.guidance, args.delta, args.out, args.per_image) == \
        ("bilateral", "cnn", 0.1, "sweep.json", None)
    assert sweep_cli.GUIDANCE == ("cnn", "image")


def test_patterns_evaluate_per_photo():
    assert sweep_cli.file_for("dir/123.png", "{dir}/zoran/{stem}.png") == "dir/zoran/123.png"
    assert sweep_cli.file_for("dir/123.png", "flat/{name}") == "flat/123.png"
    assert sweep_cli.file_for("dir/123.png", "{path}.flat{ext}") == "dir/123.png.flat.png"
    assert sweep_cli.file_for("dir/123-r.png", "{dir}/{base}.png") == "dir/123.png"
    assert sweep_cli.file_for("dir/123-r.png", "{dir}/{stem}.png") == "dir/123-r.png"


# ---- loader -----------------------------------------------------------------------------------------

def _write_judgements(path, comps_px, h, w):
    points, comparisons = [], []
    for row in comps_px:
        ids = []
        for x, y in ((row[0], row[1]), (row[2], row[3])):
            ids.append(len(points))
            points.append({"id": len(points), "x": (x + 0.5) / w, "y": (y + 0.5) / h})
        comparisons.append({"point1": ids[0], "point2": ids[1],
                            "darker": {0: "E", 1: "1", 2: "2"}[int(row[4])],
                            "darker_score": float(row[5])})
    with open(path, "w") as fh:
        json.dump({"intrinsic_points": points, "intrinsic_comparisons": comparisons}, fh)


def test_the_loader_keeps_file_order_and_reads_every_file_once(tmp_path, monkeypatch):
    photos = [str(tmp_path / ("%03d.png" % i)) for i in range(40)]
    for f in photos:
        _write_judgements(sweep_cli.judgements_for(f), COMP, 4, 4)
    reads, lock, rng = [], threading.Lock(), random.Random(7)
    delays = {}
    for f in photos:
        for name in (f, sweep_cli.file_for(f, "{dir}/src/{name}"), sweep_cli.file_for(f, "{dir}/flat/{name}")):
            delays[name] = rng.uniform(0.0, 0.004)

    def slow_imread(name):
        time.sleep(delays[name])
        with lock:
            reads.append(name)
        tag = np.zeros((4, 4, 3), dtype=np.uint8)
        tag[0, 0, 0] = int(name[-7:-4])
        tag[0, 0, 1] = {"src": 1, "flat": 2}.get(name.split("/")[-2], 0)
        return tag

    monkeypatch.setattr(iu, "imread", slow_imread)
    images, sources, guides, judgements, grey = sweep_cli.load(photos, "{dir}/src/{name}",
                                                               "{dir}/flat/{name}")
    assert grey == [False] * 40
    for kind, got in enumerate((images, sources, guides)):
        assert [(int(a[0, 0, 0]), int(a[0, 0, 1])) for a in got] == [(i, kind) for i in range(40)]
    assert sorted(reads) == sorted(delays) and len(reads) == 120
    from reflectance_filtering_amd import batch
    if batch.IO_THREADS > 1:    # 120 reads of random length finish out of order on a pool
        submitted = photos + [sweep_cli.file_for(f, "{dir}/%s/{name}" % d) for d in ("src", "flat")
                              for f in photos]
        assert reads != submitted, "the reads were serial"
    assert len(judgements) == 40 and all(j.shape == (1, 6) for j in judgements)
    # without patterns: the photos alone
    del reads[:]
    images, sources, guides, _, grey = sweep_cli.load(photos)
    assert sources is None and guides is None and grey is None and sorted(reads) == photos
    with pytest.raises(ValueError):
        sweep_cli.load(photos, png_decoder="x")


# ---- whdr.sweep(iterations=K): routes with stubbed ops ----------------------------------------------

class _Img(object):
    """Stands for a device image or a packed list: a shape, an id and a device."""
    device = "dev"
    is_cuda = True

    def __init__(self, shape, ident):
        self.shape, self.ident = tuple(shape), ident


class _Buf(object):
    """Stands for a tensor whose leading axis counts results: slot [j] (or [j, k]) is a name."""
    serial = 0

    def __init__(self, count):
        _Buf.serial += 1
        self.count, self.name = count, "buf%d" % _Buf.serial

    def __getitem__(self, j):
        return (self.name,) + (tuple(j) if isinstance(j, tuple) else (j,))

    def view(self, *shape):
        return self


def _stub(monkeypatch):
    from reflectance_filtering_amd import ops
    log = {"gf": [], "gf_sweep": [], "jbf": [], "points": [], "scores": [], "batches": [], "empty": []}

    def fake_gf(guides, srcs, radius, eps, iterations=1, grey_as_bgr=False, sizes=None, out=None):
        res = ("gf result", len(log["gf"]))
        log["gf"].append(dict(guides=guides, srcs=srcs, radius=radius, eps=eps, iterations=iterations,
                              grey_as_bgr=grey_as_bgr, sizes=[tuple(s) for s in sizes], out=out, res=res))
        return res, []

    def fake_gf_sweep(guides, srcs, radius, eps_list, grey_as_bgr=False, sizes=None, out=None):
        log["gf_sweep"].append((radius, list(eps_list)))
        return _Buf(len(eps_list))

    def fake_jbf(joints, srcs, d, sigma_color, sigma_space, grey_as_bgr=False, sizes=None, out=None):
        res = ("jbf result", len(log["jbf"]))
        log["jbf"].append(dict(joints=joints, srcs=srcs, d=d, pair=(sigma_color, sigma_space),
                               grey_as_bgr=grey_as_bgr, sizes=[tuple(s) for s in sizes], out=out, res=res))
        return res, []

    def fake_points(joints, srcs, points, point_offsets, sigma_pairs, d=-1, grey_as_bgr=False, sizes=None):
        log["points"].append(dict(joints=joints, srcs=srcs, pairs=[tuple(p) for p in sigma_pairs], d=d,
                                  grey_as_bgr=grey_as_bgr, n_points=len(points)))
        return _Buf(len(sigma_pairs))

    def fake_scores(samples, point_offsets, comps, weights, comp_offsets, delta=0.1):
        # [count, n]: the serial number of the WHDR call + image position / 100
        n = len(comp_offsets) - 1
        log["scores"].append(samples)
        return np.array([[len(log["scores"]) + i / 100.0 for i in range(n)]] * samples.count)

    def fake_sample(results, index):
        buf = _Buf(len(results))
        buf.of = list(results)
        return buf

    def fake_cat(parts):
        parts = list(parts)
        buf = _Buf(sum(p.count for p in parts))
        buf.of = parts
        return buf

    def fake_empty(shape, like):
        log["empty"].append(tuple(shape))
        return _Buf(shape[0])

    def fake_batch(*args):
        log["batches"].append(args)
        raise AssertionError("a mixed one-channel device list does not take the shape groups")

    monkeypatch.setattr(ops, "guided_filter_ragged_u8", fake_gf)
    monkeypatch.setattr(ops, "guided_filter_ragged_sweep_u8", fake_gf_sweep)
    monkeypatch.setattr(ops, "joint_bilateral_ragged_u8", fake_jbf)
    monkeypatch.setattr(ops, "joint_bilateral_points_ragged_u8", fake_points)
    monkeypatch.setattr(ops, "gf_workspace_cap", lambda device, torch: 1 << 40)
    monkeypatch.setattr(whdr, "whdr_points_u8", fake_scores)
    monkeypatch.setattr(whdr, "_pack_list",
                        lambda images, torch: _Img((sum(im.shape[0] * im.shape[1] for im in images),
                                                    images[0].shape[2]), [im.ident for im in images]))
    monkeypatch.setattr(whdr, "_sample", fake_sample)
    monkeypatch.setattr(whdr, "_cat", fake_cat)
    monkeypatch.setattr(whdr, "_empty", fake_empty)
    monkeypatch.setattr(whdr, "_index", lambda values, like: ("index", len(values)))
    monkeypatch.setattr(whdr, "_sweep_batch", fake_batch)
    monkeypatch.setattr(whdr, "_chain_batch", fake_batch)
    monkeypatch.setattr(whdr._ffi, "require_gpu", lambda: None)
    return log


TOTAL = sum(h * w for h, w in SHAPES)


def test_a_guided_chain_is_one_ragged_call_per_pass_and_distinct_pair(monkeypatch):
    log = _stub(monkeypatch)
    imgs = [_Img((h, w, 1), i) for i, (h, w) in enumerate(SHAPES)]
    guides = [_Img((h, w, 3), 100 + i) for i, (h, w) in enumerate(SHAPES)]
    # radius 2 with eps 3 (named twice: computed once), radius 4 with eps 5e-3
    pairs = [(3.0, 2.9), (5e-3, 4.0), (3.0, 2)]
    out = whdr.sweep("guided", imgs, guides, [COMP] * 5, pairs, iterations=3)
    assert out.shape == (3, 3, 5) and out.dtype == np.float64
    assert not log["gf_sweep"] and not log["jbf"] and not log["points"]
    calls = log["gf"]
    assert [(c["radius"], c["eps"]) for c in calls] == [(2, 3.0)] * 3 + [(4, 5e-3)] * 3
    for first in (0, 3):
        one, two, three = calls[first:first + 3]
        assert one["srcs"].ident == [0, 1, 2, 3, 4] and one["srcs"].shape == (TOTAL, 1)
        assert two["srcs"] is one["res"] and three["srcs"] is two["res"]
        assert len(set(c["out"] for c in (one, two, three))) == 3
    for c in calls:
        assert c["guides"].ident == [100, 101, 102, 103, 104] and c["iterations"] == 1
        assert c["sizes"] == SHAPES and c["grey_as_bgr"] is False
    # one WHDR call per pass and radius; the pair named twice shares its rows
    assert len(log["scores"]) == 6
    want = np.array([[[k + 1 + i / 100.0 for i in range(5)] for k in range(3)],
                     [[k + 4 + i / 100.0 for i in range(5)] for k in range(3)]])
    assert np.array_equal(out[:, 0], want[0]) and np.array_equal(out[:, 2], want[0])
    assert np.array_equal(out[:, 1], want[1])


def test_a_guided_chain_guiding_itself_and_its_eps_chunks(monkeypatch):
    log = _stub(monkeypatch)
    imgs = [_Img((h, w, 1), i) for i, (h, w) in enumerate(SHAPES)]
    # the bytes of a pass being written and of the one it reads: two eps per chunk at 4 x TOTAL
    monkeypatch.setattr(whdr, "SWEEP_GUIDED_BYTES", 4 * TOTAL)
    out = whdr.sweep("guided", imgs, imgs, [COMP] * 5, [(3, 4), (7, 4), (5, 4)], grey_as_bgr=True,
                     iterations=2)
    assert out.shape == (2, 3, 5)
    assert [c["eps"] for c in log["gf"]] == [3.0, 7.0, 3.0, 7.0, 5.0, 5.0]
    assert all(c["guides"] is log["gf"][0]["srcs"] and c["grey_as_bgr"] for c in log["gf"])
    assert log["gf"][2]["srcs"] is log["gf"][0]["res"] and log["gf"][3]["srcs"] is log["gf"][1]["res"]
    assert log["gf"][5]["srcs"] is log["gf"][4]["res"]
    assert log["empty"] == [(2, TOTAL, 1)] * 2 + [(1, TOTAL, 1)] * 2


def test_a_bilateral_chain_is_two_full_calls_and_one_point_call_per_pair(monkeypatch):
    log = _stub(monkeypatch)
    imgs = [_Img((h, w, 1), i) for i, (h, w) in enumerate(SHAPES)]
    guides = [_Img((h, w, 3), 100 + i) for i, (h, w) in enumerate(SHAPES)]
    pairs = [(20.0, 1.4), (7.0, 2.7)]
    out = whdr.sweep("bilateral", imgs, guides, [COMP] * 5, pairs, iterations=3)
    assert out.shape == (3, 2, 5)
    assert not log["gf"] and not log["gf_sweep"]
    full, pts = log["jbf"], log["points"]
    assert [c["pair"] for c in full] == [pairs[0], pairs[1], pairs[0], pairs[1]]
    assert [c["pairs"] for c in pts] == [[pairs[0]], [pairs[1]]]
    for g in (0, 1):
        one, two, last = full[g], full[2 + g], pts[g]
        assert one["srcs"].ident == [0, 1, 2, 3, 4] and two["srcs"] is one["res"]
        assert last["srcs"] is two["res"] and last["n_points"] == 10
        assert one["out"] != two["out"] and one["out"][0] == two["out"][0]   # two buffers of one group
        for c in (one, two, last):
            assert c["joints"].ident == [100, 101, 102, 103, 104] and c["d"] == -1
    assert log["empty"] == [(2, 2, TOTAL, 1)]
    # three WHDR calls, one per pass, for both pairs at once
    assert [s.count for s in log["scores"]] == [2, 2, 2]
    assert log["scores"][0].of == [full[0]["res"], full[1]["res"]]
    assert log["scores"][1].of == [full[2]["res"], full[3]["res"]]
    for k in range(3):
        assert out[k].tolist() == [[k + 1 + i / 100.0 for i in range(5)]] * 2
    # pairs in flight are bounded by bytes: one pair per group
    for key in log:
        del log[key][:]
    monkeypatch.setattr(whdr, "SWEEP_CHAIN_BYTES", 2 * TOTAL)
    whdr.sweep("bilateral", imgs, guides, [COMP] * 5, pairs, iterations=3)
    assert [c["pair"] for c in log["jbf"]] == [pairs[0], pairs[0], pairs[1], pairs[1]]
    assert log["empty"] == [(1, 2, TOTAL, 1)] * 2 and len(log["scores"]) == 6
    # K = 2: one full pass, one buffer per pair, so the same bytes hold both pairs
    for key in log:
        del log[key][:]
    out = whdr.sweep("bilateral", imgs, guides, [COMP] * 5, pairs, iterations=2)
    assert out.shape == (2, 2, 5) and len(log["jbf"]) == 2 and len(log["points"]) == 2
    assert log["empty"] == [(2, 1, TOTAL, 1)]


def test_a_single_pass_makes_exactly_the_calls_of_before(monkeypatch):
    log = _stub(monkeypatch)
    imgs = [_Img((h, w, 1), i) for i, (h, w) in enumerate(SHAPES)]
    pairs = [(3.0, 2.9), (5e-3, 4.0), (3.0, 2)]
    for kwargs in ({}, {"iterations": 1}):
        for key in log:
            del log[key][:]
        out = whdr.sweep("guided", imgs, imgs, [COMP] * 5, pairs, grey_as_bgr=True, **kwargs)
        assert out.shape == (3, 5)
        assert log["gf_sweep"] == [(2, [3.0]), (4, [5e-3])]
        assert not log["gf"] and not log["jbf"] and not log["points"] and not log["empty"]
        out = whdr.sweep("bilateral", imgs, imgs, [COMP] * 5, pairs, grey_as_bgr=True, **kwargs)
        assert out.shape == (3, 5)
        assert [c["pairs"] for c in log["points"]] == [[(3.0, 2.9), (5e-3, 4.0), (3.0, 2.0)]]
        assert not log["gf"] and not log["jbf"] and not log["empty"]
    for bad in (0, -1):
        with pytest.raises(ValueError):
            whdr.sweep("guided", imgs, imgs, [COMP] * 5, pairs, iterations=bad)


# ---- sweep.run: stored sources ------------------------------------------------------------------------

def _photo_set(tmp_path, grey_at, shapes=((5, 7), (9, 4), (3, 2), (6, 6), (4, 8))):
    """Photos, judgements, and sources under src/ (grey where grey_at says so, else colour) and
    guidance images under flat/; pixel [0, 0] of every file names its photo."""
    rng = np.random.default_rng(11)
    (tmp_path / "src").mkdir()
    (tmp_path / "flat").mkdir()
    photos = []
    for i, (h, w) in enumerate(shapes):
        path = str(tmp_path / ("%03d.png" % i))
        for name, grey in ((path, False), (sweep_cli.file_for(path, "{dir}/src/{name}"), i in grey_at),
                           (sweep_cli.file_for(path, "{dir}/flat/{name}"), False)):
            img = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
            if grey:
                img[:] = img[:, :, :1]
            img[0, 0] = (i, i, i) if grey else (i, 200, 100)
            assert iu.imwrite(name, img) is not False
        _write_judgements(sweep_cli.judgements_for(path), COMP, h, w)
        photos.append(path)
    return photos


def _stub_run(monkeypatch):
    from reflectance_filtering_amd import ops
    log = {"sweeps": [], "device": [], "cnn": []}

    def fake_device_list(images, channels=3):
        log["device"].append(channels)
        return [("dev", int(im[0, 0, 0]), tuple(im.shape[:2]), channels, tuple(im[0, 0, :channels]))
                for im in images]

    def fake_sweep(filter_type, src, joint, comparisons_px, sigma_pairs, delta=0.1, grey_as_bgr=False,
                   iterations=1):
        log["sweeps"].append(dict(filter_type=filter_type, src=src, joint=joint, same=joint is src,
                                  n_comps=len(comparisons_px), grey_as_bgr=grey_as_bgr,
                                  iterations=iterations))
        p = np.asarray(sigma_pairs).reshape(-1, 2).shape[0]
        one = np.array([[1000.0 * len(log["sweeps"]) + 10 * row + s[1] for s in src] for row in range(p)])
        return one if iterations == 1 else np.stack([one + 0.25 * k for k in range(iterations)])

    def no_cnn(*args, **kwargs):
        log["cnn"].append(args)
        raise AssertionError("the network is not called with src_files")

    monkeypatch.setattr(sweep_cli, "_device_list", fake_device_list)
    monkeypatch.setattr(whdr, "sweep", fake_sweep)
    monkeypatch.setattr(ops, "cnn_reflectance_u8", no_cnn)
    return log


def test_a_mixed_source_list_is_split_by_signature_and_put_back_in_order(tmp_path, monkeypatch):
    photos = _photo_set(tmp_path, grey_at=(0, 2, 3))
    log = _stub_run(monkeypatch)
    pairs, per_image, has = sweep_cli.run(photos, "guided", [3.0, 7.0], [2.0], src_files="{dir}/src/{name}")
    assert not log["cnn"] and has.tolist() == [True] * 5
    grey, colour = log["sweeps"]
    assert [s[1] for s in grey["src"]] == [0, 2, 3] and all(s[3] == 1 for s in grey["src"])
    assert [s[1] for s in colour["src"]] == [1, 4] and all(s[3] == 3 for s in colour["src"])
    # guidance "cnn": the source guides itself, a grey one as three equal channels
    assert grey["same"] and grey["grey_as_bgr"] is True and grey["iterations"] == 1
    assert colour["same"] and colour["grey_as_bgr"] is False
    assert per_image.shape == (2, 5)
    assert per_image.tolist() == [[1000, 2001, 1002, 1003, 2004], [1010, 2011, 1012, 1013, 2014]]
    # a chain, guided by files: three channels as read, for both groups
    del log["sweeps"][:]
    _, per_image, _ = sweep_cli.run(photos, "bilateral", [20.0], [1.4, 2.7], "image", iterations=3,
                                    src_files="{dir}/src/{name}", guidance_files="{dir}/flat/{name}")
    grey, colour = log["sweeps"]
    assert [j[1] for j in grey["joint"]] == [0, 2, 3] and [j[1] for j in colour["joint"]] == [1, 4]
    for call in (grey, colour):
        assert all(j[3] == 3 and j[4][1:] == (200, 100) for j in call["joint"])     # a flat/ file
        assert not call["same"] and call["grey_as_bgr"] is False and call["iterations"] == 3
    assert per_image.shape == (3, 2, 5)
    assert per_image[2, 1].tolist() == [1010.5, 2011.5, 1012.5, 1013.5, 2014.5]
    # guidance "image" without guidance files: the photo guides
    del log["sweeps"][:]
    sweep_cli.run(photos, "bilateral", [20.0], [1.4], "image", src_files="{dir}/src/{name}")
    for call in log["sweeps"]:
        assert all(j[3] == 3 and j[4][1:] == (200, 100) for j in call["joint"]) and not call["same"]
    assert not log["cnn"]


def test_sizes_and_missing_files_are_refused_before_any_op(tmp_path, monkeypatch):
    photos = _photo_set(tmp_path, grey_at=(0, 1, 2, 3, 4))
    log = _stub_run(monkeypatch)
    bad = sweep_cli.file_for(photos[3], "{dir}/flat/{name}")
    iu.imwrite(bad, np.zeros((6, 7, 3), dtype=np.uint8))
    with pytest.raises(ValueError) as err:
        sweep_cli.run(photos, "guided", [3.0], [2.0], src_files="{dir}/src/{name}",
                      guidance_files="{dir}/flat/{name}")
    assert photos[3] in str(err.value) and bad in str(err.value)
    iu.imwrite(sweep_cli.file_for(photos[1], "{dir}/src/{name}"), np.zeros((4, 9, 3), dtype=np.uint8))
    with pytest.raises(ValueError) as err:
        sweep_cli.run(photos, "bilateral", [20.0], [1.4], src_files="{dir}/src/{name}")
    assert photos[1] in str(err.value)
    for kwargs in ({"src_files": "{dir}/none/{name}"},
                   {"src_files": "{dir}/src/{name}", "guidance_files": "{dir}/flat/{stem}.jpg"},
                   {"guidance_files": "{dir}/none/{name}"}):
        with pytest.raises(Exception) as err:
            sweep_cli.run(photos, "guided", [3.0], [2.0], **kwargs)
        assert "not readable" in str(err.value)
    with pytest.raises(ValueError):
        sweep_cli.run(photos, "guided", [3.0], [2.0], src_files="{dir}/src/{name}", iterations=0)
    assert not log["sweeps"] and not log["device"] and not log["cnn"]
