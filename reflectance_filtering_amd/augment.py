"""Augmented comparisons: the transitive hull of a photo's judgements on the device.

The reference builds them with augment() and warshall() of
training/createNumpyArrayWithComparisonsForIIW.py (supplementary section 1.1): A < B and B < C give
A < C with the smaller of the two weights, '=' chains give '=', contradictions keep the heavier
direction, and of A = B, B = A one is kept by a coin.  Here `build_graphs` does the host part (the
reference's unify and its node numbering) and `hull` runs rf_augment_hull_f64 over many photos in one
call (include/reflectance_filtering_augment.h: semantics S1..S5).

    python -m reflectance_filtering_amd.augment --inputs 'iiw/*.png' --write_json iiw_augmented/

writes `<stem>_augmented.json` per photo in the reference's own list format, [[point 1, point 2,
relation, weight], ...] with IIW point ids, relation 0 = about equal, 2 = point 2 darker.  There is
no CPU fallback.
"""
from __future__ import division, print_function

import argparse
import json
import os
import sys

import numpy as np

from . import _ffi, _ffi_augment
from .whdr import DARKER_CODE

MAX_NODES = _ffi_augment.MAX_NODES
WORKSPACE_CAP = 1 << 30     # bytes of workspace one call may take; a larger single photo goes alone


def load_judgements_ids(json_path):
    """IIW `<id>.json` -> (rows, ids, points): rows float64 [m,6] exactly what whdr.load_judgements
    returns, ids int64 [m,2] the two IIW point ids of every row, points {id: (x, y)} normalised."""
    with open(json_path) as fh:
        data = json.load(fh)
    points = {p["id"]: (p["x"], p["y"]) for p in data["intrinsic_points"]}
    rows, ids = [], []
    for c in data["intrinsic_comparisons"]:
        x1, y1 = points[c["point1"]]
        x2, y2 = points[c["point2"]]
        rows.append([x1, y1, x2, y2, DARKER_CODE[c["darker"]], c["darker_score"]])
        ids.append([c["point1"], c["point2"]])
    return (np.array(rows, dtype=np.float64).reshape(-1, 6),
            np.array(ids, dtype=np.int64).reshape(-1, 2), points)


def build_graphs(comparisons):
    """One photo's judgements (point 1, point 2, darker, weight) -> (edges int32 [E,3] (from node, to
    node, relation), edge_weights float64 [E], node_point int64 [N]).  The reference's unify:
    '=' goes both ways with relation 0, 'point 1 darker' is turned round, relation 2 = `to` is
    darker; nodes are numbered by first appearance in that unified list.  A later duplicate of an
    ordered pair replaces an earlier one (the reference's matrix fill does), so the ordered pairs
    returned are distinct.  A judgement of a point against itself raises ValueError."""
    point_to_node, node_point, slot = {}, [], {}
    edges, weights = [], []
    for p1, p2, darker, weight in comparisons:
        p1, p2, darker = int(p1), int(p2), int(darker)
        if p1 == p2:
            raise ValueError("a judgement of point %d against itself" % p1)
        if darker == 0:
            both = ((p1, p2, 0), (p2, p1, 0))
        elif darker == 1:
            both = ((p2, p1, 2),)
        elif darker == 2:
            both = ((p1, p2, 2),)
        else:
            raise ValueError("darker is neither 0 (=E), 1, 2")
        for x, y, relation in both:
            for p in (x, y):
                if p not in point_to_node:
                    point_to_node[p] = len(node_point)
                    node_point.append(p)
            pair = (point_to_node[x], point_to_node[y])
            if pair in slot:
                edges[slot[pair]] = pair + (relation,)
                weights[slot[pair]] = float(weight)
            else:
                slot[pair] = len(edges)
                edges.append(pair + (relation,))
                weights.append(float(weight))
    return (np.array(edges, dtype=np.int32).reshape(-1, 3), np.array(weights, dtype=np.float64),
            np.array(node_point, dtype=np.int64))


def split_packs(node_counts, cap=WORKSPACE_CAP):
    """Runs [first, end) of consecutive graphs whose workspace stays under `cap` bytes per call (host
    arithmetic of the workspace query: 9 bytes per matrix entry).  A graph that is over the cap by
    itself is a run of its own."""
    runs, first, entries = [], 0, 0
    for i, nodes in enumerate(node_counts):
        own = int(nodes) * int(nodes)
        if i > first and 9 * (entries + own) + 48 > cap:
            runs.append((first, i))
            first, entries = i, 0
        entries += own
    if first < len(node_counts):
        runs.append((first, len(node_counts)))
    return runs


def pack_graphs(graphs):
    """The host arrays of one rf_augment_hull_f64 call over `graphs` (build_graphs results)."""
    nodes = np.array([len(g[2]) for g in graphs], dtype=np.int64)
    counts = np.array([len(g[0]) for g in graphs], dtype=np.int64)
    if nodes.size and nodes.max() > MAX_NODES:
        raise ValueError("a photo of %d judged points: the hull takes at most %d"
                         % (nodes.max(), MAX_NODES))
    run = (lambda sizes: np.concatenate([[0], np.cumsum(sizes, dtype=np.int64)]))
    node_offsets, edge_offsets = run(nodes), run(counts)
    if node_offsets[-1] >= 2 ** 31 or edge_offsets[-1] >= 2 ** 31:
        raise ValueError("too many judgements for one call")

    def cat(k, dt, width):
        parts = [np.asarray(g[k], dtype=dt).reshape((-1,) + width) for g in graphs]
        return np.concatenate(parts, axis=0) if parts else np.zeros((0,) + width, dtype=dt)

    node_point = cat(2, np.int64, ())
    if node_point.size and (node_point.min() < -2 ** 31 or node_point.max() >= 2 ** 31):
        raise ValueError("point ids must fit 32 bits")
    return dict(edges=cat(0, np.int32, (3,)), edge_weights=cat(1, np.float64, ()),
                edge_offsets=edge_offsets.astype(np.int32), node_offsets=node_offsets.astype(np.int32),
                matrix_offsets=run(nodes * nodes), out_offsets=run(nodes * (nodes - 1) // 2),
                node_point=node_point.astype(np.int32), nodes=nodes)


def hull_arrays(graphs, coins=None, seed=None, device=None, workspace=None, node_point=True):
    """One rf_augment_hull_f64 call over all `graphs`: (comps int32 [m,3], weights float64 [m],
    counts int64 [n]) on the host, the photos' lists one behind the other.  coins: None (all zero), a
    CUDA or host uint8 array of one byte per matrix entry, or drawn from `seed` by a torch generator
    on the device.  workspace: a CUDA uint8 tensor to use, else one is allocated; node_point=False
    writes node ids in place of the graphs' point ids."""
    torch = _ffi.require_gpu()
    lib = _ffi_augment.load_library()
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    host = pack_graphs(graphs)
    n = len(graphs)
    total_matrix, cap = int(host["matrix_offsets"][-1]), int(host["out_offsets"][-1])
    if n == 0:
        return np.zeros((0, 3), np.int32), np.zeros(0, np.float64), np.zeros(0, np.int64)

    def up(array):      # never of zero length: the entry refuses NULL pointers
        array = np.ascontiguousarray(array)
        if array.size == 0:
            array = np.zeros((1,) + array.shape[1:], dtype=array.dtype)
        return torch.from_numpy(array).to(dev)

    d = dict((k, up(host[k])) for k in ("edges", "edge_weights", "edge_offsets", "node_offsets",
                                        "matrix_offsets", "out_offsets", "node_point"))
    if coins is None and seed is not None:
        generator = torch.Generator(device=dev)
        generator.manual_seed(int(seed))
        coins = torch.randint(0, 2, (max(total_matrix, 1),), generator=generator, device=dev,
                              dtype=torch.uint8)
    elif coins is not None:
        if not hasattr(coins, "is_cuda"):
            coins = torch.from_numpy(np.ascontiguousarray(coins, dtype=np.uint8).ravel())
        coins = coins.to(dev).contiguous().view(-1)
        if coins.dtype != torch.uint8 or coins.numel() < total_matrix:
            raise ValueError("coins: one uint8 per matrix entry (%d)" % total_matrix)
    need = _ffi_augment.hull_workspace_bytes(total_matrix)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    comps = torch.zeros((max(cap, 1), 3), dtype=torch.int32, device=dev)
    weights = torch.zeros(max(cap, 1), dtype=torch.float64, device=dev)
    counts = torch.zeros(n, dtype=torch.int32, device=dev)
    rc = lib.rf_augment_hull_f64(
        d["edges"].data_ptr(), d["edge_weights"].data_ptr(), d["edge_offsets"].data_ptr(),
        d["node_offsets"].data_ptr(), d["matrix_offsets"].data_ptr(), d["out_offsets"].data_ptr(),
        d["node_point"].data_ptr() if node_point else None, coins.data_ptr() if coins is not None else None, n,
        int(host["nodes"].max()), int(host["node_offsets"][-1]), int(host["edge_offsets"][-1]),
        total_matrix, cap, comps.data_ptr(), weights.data_ptr(), counts.data_ptr(),
        workspace.data_ptr(), workspace.numel(), _ffi.current_stream_ptr(torch))
    _ffi_augment.check(rc, "rf_augment_hull_f64")
    counts_h = counts.cpu().numpy().astype(np.int64)
    comps_h, weights_h = comps.cpu().numpy(), weights.cpu().numpy()
    keep = np.zeros(max(cap, 1), dtype=bool)
    for start, count in zip(host["out_offsets"][:-1], counts_h):
        keep[start:start + count] = True
    return comps_h[keep], weights_h[keep], counts_h


def hull(graphs, coins=None, seed=None, workspace_cap=WORKSPACE_CAP, device=None):
    """The hull of a list of photos' graphs (build_graphs results): per photo the reference's list
    [[point 1, point 2, relation, weight], ...] (relation a float, as the reference's matrix gives it).
    The list is split so that one call's workspace stays under workspace_cap bytes.  coins: None (all
    zero: of A = B, B = A the one with the smaller node first is dropped), a list of one [N,N] uint8
    array per photo, or - with `seed` - drawn on the device by a torch generator seeded with seed +
    the index of the call; the draw is reproducible for one seed, list and cap."""
    out = []
    for call, (first, end) in enumerate(split_packs([len(g[2]) for g in graphs], workspace_cap)):
        part = graphs[first:end]
        given = None
        if coins is not None:
            given = np.concatenate([np.asarray(c, dtype=np.uint8).reshape(len(g[2]) ** 2)
                                    for c, g in zip(coins[first:end], part)] + [np.zeros(0, np.uint8)])
        comps, weights, counts = hull_arrays(part, given, None if seed is None else seed + call,
                                             device)
        ends = np.cumsum(counts)
        for i in range(len(part)):
            k0, k1 = ends[i] - counts[i], ends[i]
            out.append([[int(a), int(b), float(r), float(w)]
                        for (a, b, r), w in zip(comps[k0:k1].tolist(), weights[k0:k1].tolist())])
    return out


def to_rows(augmented, points):
    """An augmented list with IIW point ids -> float64 [m,6] rows (x1, y1, x2, y2, darker, weight) in
    the normalised coordinates of whdr.load_judgements; relation 2 is darker code 2 (point 2 darker)."""
    rows = [[points[a][0], points[a][1], points[b][0], points[b][1], r, w] for a, b, r, w in augmented]
    return np.array(rows, dtype=np.float64).reshape(-1, 6)


def augment_files(json_paths, seed=None, workspace_cap=WORKSPACE_CAP):
    """(augmented lists, points dicts) of IIW judgement files, through build_graphs and hull."""
    loaded = [load_judgements_ids(path) for path in json_paths]
    graphs = [build_graphs(np.concatenate([ids, rows[:, 4:6]], axis=1))
              for rows, ids, _ in loaded]
    return hull(graphs, seed=seed, workspace_cap=workspace_cap), [points for _, _, points in loaded]


# ---- command line -----------------------------------------------------------------------------------

def build_parser():
    p = argparse.ArgumentParser(description="Augment IIW judgements by their transitive hull "
                                            "(one process, one GPU).")
    p.add_argument("--inputs", nargs="+", required=True,
                   help="photos or judgement files (files or glob patterns); a photo's judgements "
                        "are <stem>.json beside it")
    p.add_argument("--write_json", required=True, metavar="DIR",
                   help="write <stem>_augmented.json into DIR, the reference's list format")
    p.add_argument("--seed", type=int, default=None,
                   help="draw the coins of the '=' pairs from this seed (default: no coin, the "
                        "direction from the later node is kept)")
    return p


def judgement_files(inputs):
    """<stem>.json of every input, once, in order; an *_augmented.json is never an input."""
    from .batch import expand_inputs
    out = []
    for name in expand_inputs(inputs):
        path = os.path.splitext(name)[0] + ".json"
        if path.endswith("_augmented.json") or path in out:
            continue
        out.append(path)
    return out


def main(argv=None):
    args = build_parser().parse_args(sys.argv[1:] if argv is None else argv)
    files = judgement_files(args.inputs)
    if not files:
        raise SystemExit("no input files")
    lists, _ = augment_files(files, seed=args.seed)
    os.makedirs(args.write_json, exist_ok=True)
    for path, augmented in zip(files, lists):
        stem = os.path.splitext(os.path.basename(path))[0]
        with open(os.path.join(args.write_json, stem + "_augmented.json"), "w") as fh:
            json.dump(augmented, fh)
    print("%d photos, %d augmented comparisons" % (len(files), sum(len(a) for a in lists)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
