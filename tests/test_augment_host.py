"""Augmented comparisons, everything that needs no device: the numpy restatement against the
reference's own augment() (tests/golden/augment.npz), build_graphs, the C ABI of
librf_augment_hip.so and its refusals, pack() with and without a second comparison set, the per-step
subsample and the command lines."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests import augment_numpy as restate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_equals_the_reference_entry_for_entry(golden_dir):
    path = os.path.join(golden_dir, "augment.npz")
    assert os.path.getsize(path) < (1 << 20)
    data = np.load(path)
    names = [str(data["case%d_name" % c]) for c in range(int(data["n_cases"]))]
    assert names == ["chain", "two-components", "cycle", "equal-clique", "mixed", "tie", "duplicate",
                     "iiw-like"]
    assert list(data["modes"]) == ["0.25", "0.75", "seeded"]
    nodes, drawn = [], 0
    for c, name in enumerate(names):
        comparisons = [(int(a), int(b), int(d), float(w)) for a, b, d, w in data["case%d_comparisons" % c]]
        nodes.append(len(restate.number_nodes(restate.unify(comparisons))[1]))
        outs = []
        for q in range(3):
            draws, want = data["case%d_mode%d_draws" % (c, q)], data["case%d_mode%d_out" % (c, q)]
            got = np.array(restate.augment(comparisons, draws=draws), dtype=np.float64).reshape(-1, 4)
            assert got.shape == want.shape, (name, q)
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (name, q)
            if q < 2:       # a fixed draw is one coin everywhere: the matrix form gives the same list
                n = nodes[-1]
                coins = np.full((n, n), int(float(data["modes"][q]) > 0.5), dtype=np.uint8)
                assert restate.augment(comparisons, coins=coins) == got.tolist(), (name, q)
            outs.append(got)
            drawn += len(draws)
        if name in ("equal-clique", "iiw-like"):        # the coin shows
            assert not np.array_equal(outs[0], outs[1])
    assert max(nodes) == 127 and nodes[0] == 40 and drawn > 1000
    # the tie rule and the later duplicate, by hand
    tie = data["case5_mode0_out"].tolist()
    assert [2.0, 1.0, 2.0, 0.7] in tie and [1.0, 2.0, 2.0, 0.7] not in tie
    dup = data["case6_mode0_out"].tolist()
    assert [1.0, 2.0, 2.0, 0.5] in dup


def test_restatement_refuses_too_few_draws():
    with pytest.raises(ValueError):
        restate.augment([(1, 2, 0, 0.5)], draws=[])


def random_judgements(seed, count, points):
    rng = np.random.RandomState(seed)
    rows = []
    while len(rows) < count:
        a, b = rng.randint(0, points, 2)
        if a != b:
            rows.append((int(500 + 7 * a), int(500 + 7 * b), int(rng.randint(0, 3)),
                         float(rng.randint(1, 40)) / 16))
    return rows


def test_build_graphs_against_a_loop():
    from reflectance_filtering_amd import augment
    for seed, count, points in ((1, 60, 12), (2, 200, 90), (3, 1, 2), (4, 0, 5)):
        rows = random_judgements(seed, count, points)      # few points: duplicates and reversals
        edges, weights, node_point = augment.build_graphs(rows)
        assert (edges.dtype, weights.dtype, node_point.dtype) == (np.int32, np.float64, np.int64)
        assert edges.shape == (len(weights), 3)
        unified = restate.unify(rows)
        to_node, to_point = restate.number_nodes(unified)
        assert node_point.tolist() == to_point
        last = {}
        for x, y, r, w in unified:                          # the later one stands
            last[(to_node[x], to_node[y])] = (r, w)
        got = dict(((a, b), (r, w)) for (a, b, r), w in zip(edges.tolist(), weights.tolist()))
        assert len(got) == len(edges) and got == last
        if count > 50:
            assert len(last) < len(unified)
        assert (edges[:, 0] != edges[:, 1]).all()
        # and the whole photo through the restatement either way
        by_graph = restate.hull(len(node_point), edges, weights, node_point=node_point)
        by_list = restate.augment(rows)
        assert [[a, b, float(r), w] for (a, b, r), w in zip(by_graph[0].tolist(), by_graph[1].tolist())] \
            == by_list


def test_build_graphs_refusals():
    from reflectance_filtering_amd import augment
    with pytest.raises(ValueError, match="against itself"):
        augment.build_graphs([(1, 2, 0, 0.5), (3, 3, 1, 0.5)])
    with pytest.raises(ValueError, match="darker"):
        augment.build_graphs([(1, 2, 3, 0.5)])
    too_many = [(i, i + 1, 2, 1.0) for i in range(0, 2 * 1300, 2)]
    graph = augment.build_graphs(too_many)
    assert len(graph[2]) == 2600
    with pytest.raises(ValueError, match="at most 2560"):
        augment.pack_graphs([graph])


def test_pack_graphs_and_split_packs():
    from reflectance_filtering_amd import augment
    graphs = [augment.build_graphs(random_judgements(s, c, p)) for s, c, p in ((1, 30, 9), (2, 0, 3), (3, 50, 40))]
    host = augment.pack_graphs(graphs)
    nodes = [len(g[2]) for g in graphs]
    assert nodes[1] == 0 and host["nodes"].tolist() == nodes
    assert host["node_offsets"].tolist() == np.concatenate([[0], np.cumsum(nodes)]).tolist()
    assert host["matrix_offsets"].tolist() == np.concatenate([[0], np.cumsum(np.square(nodes))]).tolist()
    assert host["out_offsets"].tolist() == np.concatenate(
        [[0], np.cumsum([k * (k - 1) // 2 for k in nodes])]).tolist()
    assert host["matrix_offsets"].dtype == np.int64 and host["out_offsets"].dtype == np.int64
    assert host["edge_offsets"].tolist() == np.concatenate([[0], np.cumsum([len(g[0]) for g in graphs])]).tolist()
    assert np.array_equal(host["edges"][host["edge_offsets"][2]:], graphs[2][0])
    assert augment.split_packs([]) == []
    assert augment.split_packs([10, 10, 10], 9 * 200 + 48) == [(0, 2), (2, 3)]
    assert augment.split_packs([100, 5], 10) == [(0, 1), (1, 2)]       # over the cap alone: a run each
    assert augment.split_packs([3, 4, 5]) == [(0, 3)]


# ---- ABI ---------------------------------------------------------------------------------------------

def header_functions():
    with open(os.path.join(ROOT, "include", "reflectance_filtering_augment.h")) as fh:
        text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    return set(re.findall(r"\b(rf_augment_\w+)\s*\(", text))


def test_header_exports_and_symbols(built):
    from reflectance_filtering_amd import _ffi, _ffi_augment, _ffi_train
    assert header_functions() == set(_ffi_augment.EXPORTS)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _ffi_augment.LIB_PATH]).decode()
    syms = {line.split()[-1] for line in out.splitlines()
            if len(line.split()) == 3 and line.split()[1] == "T" and line.split()[-1].startswith("rf_")}
    assert syms == set(_ffi_augment.EXPORTS)
    others = set(_ffi.EXPORTS) | set(_ffi.DEBUG_EXPORTS) | set(_ffi_train.EXPORTS)
    assert not set(_ffi_augment.EXPORTS) & others
    for path in (_ffi.LIB_PATH, _ffi_train.LIB_PATH):
        other = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        assert "rf_augment_" not in other and "rfa" not in other
    assert "rf_train_" not in out and "rft" not in out
    with open(_ffi_augment.LIB_PATH, "rb") as fh:
        blob = fh.read()
    archs = set(re.findall(rb"amdgcn-amd-amdhsa--(gfx[0-9a-f]+)", blob))
    assert archs == {b"gfx950"}
    with open(os.path.join(ROOT, "include", "reflectance_filtering_augment.h")) as fh:
        text = fh.read()
    assert int(re.search(r"#define RF_AUGMENT_MAX_NODES (\d+)", text).group(1)) == _ffi_augment.MAX_NODES
    assert _ffi_augment.MAX_NODES >= 2362


def test_version_and_refusals(built):
    from reflectance_filtering_amd import _ffi_augment
    lib = _ffi_augment.load_library()
    assert lib.rf_augment_version() == 100
    err = (lambda: lib.rf_augment_last_error().decode())
    p = ctypes.c_void_p(0x1000)          # invented: every refusal comes before any device work
    hull = lib.rf_augment_hull_f64
    nodes, matrix = 150, 100 * 100 + 50 * 50
    rows = (matrix - nodes) // 2
    need = lib.rf_augment_hull_workspace_bytes(matrix)
    ok = [p, p, p, p, p, p, p, p, 2, 100, nodes, 300, matrix, rows, p, p, p, p, need, None]
    assert hull(*([None] * 8 + [0, 0, 0, 0, 0, 0, None, None, None, None, 0, None])) == 0
    assert hull(*([None] * 8 + [0, -1, -1, -1, -1, -1, None, None, None, None, 0, None])) == 0
    for i in (0, 1, 2, 3, 4, 5, 14, 15, 16):
        args = list(ok)
        args[i] = None
        assert hull(*args) == -1 and "NULL pointer" in err(), i
    for i in (8, 9, 10, 11, 12, 13):
        args = list(ok)
        args[i] = -1
        assert hull(*args) == -1 and "bad size" in err(), i
    for ws, size in ((None, need), (p, need - 1), (ctypes.c_void_p(0x1008), need), (p, 0)):
        args = list(ok)
        args[17], args[18] = ws, size
        assert hull(*args) == -1 and "16-byte aligned" in err()
    args = list(ok)
    args[13] = rows - 1
    assert hull(*args) == -1 and "cap=" in err()
    for i, value in ((10, 201), (12, 2 * 100 * 100 + 1)):
        args = list(ok)
        args[i] = value
        args[18] = 1 << 40
        assert hull(*args) == -1 and "totals larger" in err(), i
    limit = _ffi_augment.MAX_NODES
    args = list(ok)
    args[9] = limit + 1
    assert hull(*args) == -2 and err().endswith("the limit is %d" % limit)
    args = list(ok)
    args[8] = 1 << 22
    assert hull(*args) == -2 and err().endswith("too many images for one launch")
    for i in (10, 11):
        args = list(ok)
        args[i] = 1 << 31
        assert hull(*args) == -2 and "32-bit" in err()
    # the two optional pointers may be NULL: the refusal that follows is the workspace's
    args = list(ok)
    args[6], args[7], args[18] = None, None, need - 16
    assert hull(*args) == -1 and "16-byte aligned" in err()


def test_workspace_query_is_monotone(built):
    from reflectance_filtering_amd import _ffi_augment
    last = 0
    limit = _ffi_augment.MAX_NODES
    for entries in [0, 1, 4, 9, 15, 16, 17, 63 * 63, 64 * 64, 300 * 300, limit * limit,
                    40 * limit * limit, 1 << 40]:
        size = _ffi_augment.hull_workspace_bytes(entries)
        assert size >= 9 * entries and size % 16 == 0 and size >= last and size > 0
        last = size
    assert _ffi_augment.hull_workspace_bytes(-1) == 0
    assert _ffi_augment.hull_workspace_bytes((1 << 40) + 1) == 0


# ---- trainer -----------------------------------------------------------------------------------------

def on_the_host(monkeypatch):
    """pack() with its arrays left on the host: the device is only where the copies go."""
    import torch
    from reflectance_filtering_amd import _ffi, train
    monkeypatch.setattr(_ffi, "require_gpu", lambda: torch)
    return train, torch.device("cpu")


def small_set(seed, counts, size=(12, 20)):
    rng = np.random.RandomState(seed)
    images = [rng.randint(0, 256, size + (3,)).astype(np.uint8) for _ in counts]
    comps = []
    for m in counts:
        rows = np.zeros((m, 6))
        rows[:, 0], rows[:, 2] = rng.randint(0, size[1], m), rng.randint(0, size[1], m)
        rows[:, 1], rows[:, 3] = rng.randint(0, size[0], m), rng.randint(0, size[0], m)
        rows[:, 4], rows[:, 5] = rng.randint(0, 3, m), rng.randint(1, 30, m) / 8.0
        comps.append(rows)
    return images, comps


def pack_as_it_was(train, images, comparisons_px, order_seed, ratio, eval_dense):
    """The arrays pack() returned before it took a second set: a copy of its steps."""
    from reflectance_filtering_amd import image_utils as iu
    from reflectance_filtering_amd import whdr
    n = len(images)
    order = np.arange(n) if order_seed is None else np.random.RandomState(order_seed).permutation(n)
    images = [images[i] for i in order]
    comps_px = [train.select_comparisons(comparisons_px[i], ratio, eval_dense) for i in order]
    sizes = [tuple(int(v) for v in im.shape[:2]) for im in images]
    points, point_offsets, comps, weights, comp_offsets = whdr.dedup_points_ragged(comps_px, sizes)
    inc_offsets, inc = train.point_incidence(point_offsets, comps, comp_offsets)
    lut = iu.srgb_byte_lut()
    x = np.zeros((points.shape[0], 3), dtype=np.float32)
    for i, image in enumerate(images):
        p0, p1 = point_offsets[i], point_offsets[i + 1]
        x[p0:p1] = lut[image[points[p0:p1, 1], points[p0:p1, 0], :]]
    return dict(points=points, point_offsets=point_offsets, comps=comps, weights=weights,
                comp_offsets=comp_offsets, inc_offsets=inc_offsets, inc=inc, x=x, order=order)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_pack_without_a_second_set_is_what_it_was(monkeypatch):
    train, cpu = on_the_host(monkeypatch)
    images, comps = small_set(21, [30, 0, 7, 320])
    for seed, ratio, dense in ((None, 1.0, True), (4, 0.5, False)):
        packed = train.pack(images, comps, seed, ratio, dense, device=cpu)
        was = pack_as_it_was(train, images, comps, seed, ratio, dense)
        for name in ("points", "point_offsets", "comps", "weights", "comp_offsets", "inc_offsets",
                     "inc", "order"):
            assert same_bits(getattr(packed, name), was[name]), name
        assert same_bits(packed.x.numpy(), was["x"])
        for name in ("point_offsets", "comps", "weights", "comp_offsets", "inc_offsets", "inc"):
            assert same_bits(getattr(packed, "d_" + name).numpy(), was[name]), name
        # the true WHDR is taken on the same arrays as before
        assert packed.whdr_comps is packed.comps and packed.whdr_weights is packed.weights
        assert packed.whdr_comp_offsets is packed.comp_offsets


def decode(points, point_offsets, comps, weights, comp_offsets, image):
    """The comparisons of one packed image as rows (x1, y1, x2, y2, darker, weight)."""
    p0 = point_offsets[image]
    c = comps[comp_offsets[image]:comp_offsets[image + 1]]
    w = weights[comp_offsets[image]:comp_offsets[image + 1]]
    return np.concatenate([points[p0 + c[:, 0]], points[p0 + c[:, 1]], c[:, 2:3], w[:, None]], axis=1)


def test_pack_with_a_second_set(monkeypatch):
    train, cpu = on_the_host(monkeypatch)
    images, comps = small_set(22, [30, 5, 0, 40])
    _, second = small_set(23, [90, 0, 6, 310])
    for seed, ratio, dense in ((None, 1.0, True), (6, 0.5, False)):
        packed = train.pack(images, comps, seed, ratio, dense, device=cpu, hinge_comparisons_px=second)
        order = packed.order
        for i in range(4):
            chosen = train.select_comparisons(second[order[i]], ratio, dense)
            hinge = decode(packed.points, packed.point_offsets, packed.comps, packed.weights,
                           packed.comp_offsets, i)
            assert np.array_equal(hinge, chosen)            # the hinge arrays: the second set, selected
            true = decode(packed.points, packed.point_offsets, packed.whdr_comps, packed.whdr_weights,
                          packed.whdr_comp_offsets, i)
            assert np.array_equal(true, comps[order[i]])    # the true WHDR: ALL the judgements
            pts = packed.points[packed.point_offsets[i]:packed.point_offsets[i + 1]]
            union = np.concatenate([chosen[:, 0:2], chosen[:, 2:4], comps[order[i]][:, 0:2],
                                    comps[order[i]][:, 2:4]]).astype(np.int64)
            assert np.array_equal(pts, np.unique(union, axis=0).reshape(-1, 2))
        inc_offsets, inc = train.point_incidence(packed.point_offsets, packed.comps, packed.comp_offsets)
        assert same_bits(packed.inc_offsets, inc_offsets) and same_bits(packed.inc, inc)
        assert same_bits(packed.d_comps.numpy(), packed.comps)
        assert same_bits(packed.d_weights.numpy(), packed.weights)
        assert packed.x.shape == (packed.points.shape[0], 3)
    with pytest.raises(ValueError):
        train.pack(images, comps, device=cpu, hinge_comparisons_px=second[:3])


def test_subsample_keeps_exactly_k_of_an_oversize_image(monkeypatch):
    import torch
    train, cpu = on_the_host(monkeypatch)
    images, comps = small_set(24, [40, 12, 0, 25, 13])
    packed = train.pack(images, comps, device=cpu)
    offsets = packed.comp_offsets

    def draw(seed, first, count, k):
        generator = torch.Generator(device=cpu)
        generator.manual_seed(seed)
        return train.subsample_weights(packed, first, count, k, generator)

    w = draw(3, 0, 5, 12).numpy()
    assert w.dtype == np.float64 and w.shape == packed.weights.shape
    for i, m in enumerate(np.diff(offsets)):
        part, full = w[offsets[i]:offsets[i + 1]], packed.weights[offsets[i]:offsets[i + 1]]
        kept = part != 0
        assert kept.sum() == min(m, 12) and np.array_equal(part[kept], full[kept])
        if m <= 12:
            assert np.array_equal(part, full)               # smaller images stay whole
    assert np.array_equal(draw(3, 0, 5, 12).numpy(), w)     # reproducible from the seed
    assert not np.array_equal(draw(4, 0, 5, 12).numpy(), w)
    # only the images of the minibatch are thinned; nothing to drop: no copy, no draw
    part = draw(3, 1, 3, 12).numpy()
    assert np.array_equal(part[:offsets[1]], packed.weights[:offsets[1]])
    assert (part[offsets[3]:offsets[4]] != 0).sum() == 12
    assert np.array_equal(part[offsets[4]:], packed.weights[offsets[4]:])
    assert draw(3, 0, 5, 0) is None and draw(3, 0, 5, 40) is None and draw(3, 1, 2, 12) is None
    assert np.array_equal(packed.d_weights.numpy(), packed.weights)     # the packed weights are not touched


# ---- command lines -----------------------------------------------------------------------------------

def test_train_cli_options(capsys):
    from reflectance_filtering_amd import train
    _, args = train.parse_args(["--inputs", "a.png"])
    assert (args.comparisons, args.max_evaluated) == ("comparisons", 1500)
    _, args = train.parse_args(["--inputs", "a.png", "--comparisons", "augmented", "--max_evaluated", "0"])
    assert (args.comparisons, args.max_evaluated) == ("augmented", 0)
    for bad in (["--comparisons", "hull"], ["--max_evaluated", "-1"], ["--max_evaluated", "x"]):
        with pytest.raises(SystemExit) as stop:
            train.parse_args(["--inputs", "a.png"] + bad)
        assert stop.value.code == 2
    capsys.readouterr()


def test_train_cli_records_both_options_and_packs_the_hull(tmp_path, monkeypatch, capsys):
    from reflectance_filtering_amd import augment
    from tests import train_stubs
    from tests.test_train_host import photos_in
    train = train_stubs.install(monkeypatch.setattr)
    seen = []

    def pack(images, comparisons_px, order_seed=None, ratio=1.0, eval_dense=True, device=None,
             hinge_comparisons_px=None):
        seen.append((len(images), [np.asarray(h) for h in hinge_comparisons_px]))
        return train_stubs.FakePacked(len(images))

    def augment_files(paths, seed=None, workspace_cap=None):
        seen.append(("augment", list(paths), seed))
        return ([[[1, 2, 2.0, 0.5], [2, 3, 0.0, 0.25]] for _ in paths],
                [{1: (0.3, 0.3), 2: (0.6, 0.3), 3: (0.8, 0.9)} for _ in paths])

    monkeypatch.setattr(train, "pack", pack)
    monkeypatch.setattr(augment, "augment_files", augment_files)
    photos = photos_in(tmp_path, 3)
    log = str(tmp_path / "t.json")
    rc = train.main(["--inputs"] + photos + ["--comparisons", "augmented", "--max_evaluated", "700",
                                              "--iterations", "2", "--seed", "5",
                                              "--out", str(tmp_path / "w.caffemodel"), "--log", log])
    assert rc == 0
    assert seen[0] == ("augment", [os.path.splitext(f)[0] + ".json" for f in photos], 5)
    count, hull = seen[1]
    assert count == 3 and np.array_equal(hull[0], [[1, 1, 2, 1, 2, 0.5], [2, 1, 3, 3, 0, 0.25]])
    (_, _, options), = [c for c in train_stubs.CALLS if c[0] == "fit"]
    assert options["max_evaluated"] == 700
    with open(log) as fh:
        result = json.load(fh)
    assert result["comparisons_type"] == "augmented" and result["max_evaluated"] == 700
    capsys.readouterr()


def test_augment_cli(tmp_path, monkeypatch, capsys):
    from reflectance_filtering_amd import augment
    args = augment.build_parser().parse_args(["--inputs", "a.png", "b.png", "--write_json", "out"])
    assert (args.inputs, args.write_json, args.seed) == (["a.png", "b.png"], "out", None)
    for bad in ([], ["--inputs", "a.png"], ["--write_json", "out"],
                ["--inputs", "a.png", "--write_json", "out", "--seed", "x"]):
        with pytest.raises(SystemExit) as stop:
            augment.build_parser().parse_args(bad)
        assert stop.value.code == 2
    capsys.readouterr()
    iiw = {"intrinsic_points": [{"id": 11, "x": 0.25, "y": 0.5}, {"id": 12, "x": 0.75, "y": 0.5},
                                {"id": 13, "x": 0.5, "y": 0.125}],
           "intrinsic_comparisons": [{"point1": 11, "point2": 12, "darker": "1", "darker_score": 0.75},
                                     {"point1": 13, "point2": 12, "darker": "E", "darker_score": 0.5}]}
    for stem in ("101", "102"):
        (tmp_path / (stem + ".png")).write_bytes(b"")
        (tmp_path / (stem + ".json")).write_text(json.dumps(iiw))
    (tmp_path / "101_augmented.json").write_text("[]")
    files = augment.judgement_files([str(tmp_path / "*.png"), str(tmp_path / "*.json")])
    assert files == [str(tmp_path / "101.json"), str(tmp_path / "102.json")]
    rows, ids, points = augment.load_judgements_ids(files[0])
    from reflectance_filtering_amd import whdr
    assert np.array_equal(rows, whdr.load_judgements(files[0]))
    assert ids.tolist() == [[11, 12], [13, 12]] and points[13] == (0.5, 0.125)
    # the device stage replaced by the restatement: what main() writes is the reference's list, as data
    monkeypatch.setattr(augment, "hull", lambda graphs, seed=None, workspace_cap=None: [
        [[int(a), int(b), float(r), float(w)] for (a, b, r), w in
         zip(*[x.tolist() for x in restate.hull(len(g[2]), g[0], g[1], node_point=g[2])])] for g in graphs])
    out = tmp_path / "aug"
    assert augment.main(["--inputs", str(tmp_path / "*.png"), "--write_json", str(out)]) == 0
    with open(str(out / "102_augmented.json")) as fh:
        written = json.load(fh)
    assert written == restate.augment([(11, 12, 1, 0.75), (13, 12, 0, 0.5)])
    assert sorted(os.listdir(str(out))) == ["101_augmented.json", "102_augmented.json"]
    assert np.array_equal(augment.to_rows(written[:1], points)[0, :4],
                          points[written[0][0]] + points[written[0][1]])
    assert "2 photos" in capsys.readouterr().out
