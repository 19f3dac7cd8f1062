"""Time of the judgement hull (rf_augment_hull_f64, one call per list) on seeded synthetic graph lists
of about 40, 150, 400 and 1,200 nodes per photo with an IIW-like degree, against the numpy
restatement of the tests (tests/augment_numpy.py, one vectorised update per k) on the host.

    python tools/augment_time.py [--repeats 9] > profiles/augment_time.txt

Device: nine repeats per list between two events on the stream, inputs resident, after one warm call;
median with min - max in milliseconds.  Host: the restatement once per list (it is the slow side).
The reference's own triple loop is not run here.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from reflectance_filtering_amd import _ffi, _ffi_augment, augment   # noqa: E402
from tests import augment_numpy                                      # noqa: E402

LISTS = (("40 nodes", 40, 16), ("150 nodes", 150, 16), ("400 nodes", 400, 4), ("1,200 nodes", 1200, 1),
         ("mixed 40..400", None, 12))


def graph(rng, nodes):
    """Every node judged against one of its six predecessors (one component, as IIW's Delaunay edges
    make), 0.6 more judgements per node between random nodes, half of all '='."""
    rows = []
    for v in range(1, nodes):
        rows.append((v, rng.randint(max(0, v - 6), v), int(rng.choice([0, 0, 1, 2])),
                     round(rng.uniform(0.05, 2.4), 3)))
    for _ in range(int(0.6 * nodes)):
        a, b = rng.randint(0, nodes, 2)
        if a != b:
            rows.append((a, b, int(rng.choice([0, 0, 1, 2])), round(rng.uniform(0.05, 2.4), 3)))
    return augment.build_graphs(rows)


def device_times(graphs, repeats):
    lib = _ffi_augment.load_library()
    host = augment.pack_graphs(graphs)
    up = (lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda())
    d = dict((k, up(host[k])) for k in ("edges", "edge_weights", "edge_offsets", "node_offsets",
                                        "matrix_offsets", "out_offsets", "node_point"))
    total_matrix, cap = int(host["matrix_offsets"][-1]), int(host["out_offsets"][-1])
    need = _ffi_augment.hull_workspace_bytes(total_matrix)
    workspace = torch.empty(need, dtype=torch.uint8, device="cuda")
    comps = torch.zeros((cap, 3), dtype=torch.int32, device="cuda")
    weights = torch.zeros(cap, dtype=torch.float64, device="cuda")
    counts = torch.zeros(len(graphs), dtype=torch.int32, device="cuda")

    def call():
        rc = lib.rf_augment_hull_f64(
            d["edges"].data_ptr(), d["edge_weights"].data_ptr(), d["edge_offsets"].data_ptr(),
            d["node_offsets"].data_ptr(), d["matrix_offsets"].data_ptr(), d["out_offsets"].data_ptr(),
            d["node_point"].data_ptr(), None, len(graphs), int(host["nodes"].max()),
            int(host["node_offsets"][-1]), int(host["edge_offsets"][-1]), total_matrix, cap,
            comps.data_ptr(), weights.data_ptr(), counts.data_ptr(), workspace.data_ptr(), need,
            _ffi.current_stream_ptr(torch))
        _ffi_augment.check(rc, "rf_augment_hull_f64")

    call()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        call()
        stop.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_time(stop))
    return sorted(times), int(counts.sum().item()), need


def host_time(graphs):
    t0 = time.perf_counter()
    total = sum(len(augment_numpy.hull(len(g[2]), g[0], g[1])[1]) for g in graphs)
    return (time.perf_counter() - t0) * 1e3, total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--skip_host_above", type=int, default=1200,
                    help="do not run the numpy restatement on graphs of more nodes than this")
    args = ap.parse_args()
    print("judgement hull, ms: device median (min - max) of %d repeats per list; numpy restatement once; %s"
          % (args.repeats, torch.cuda.get_device_name(0)))
    for name, nodes, count in LISTS:
        rng = np.random.RandomState(count * 1000 + (nodes or 7))
        sizes = [nodes] * count if nodes else [int(s) for s in rng.randint(40, 401, count)]
        graphs = [graph(rng, s) for s in sizes]
        t, found, need = device_times(graphs, args.repeats)
        line = ("%-14s %3d photos %8d judgements -> %9d  workspace %7.1f MB  device %9.3f (%9.3f - %9.3f)"
                % (name, count, sum(len(g[0]) for g in graphs), found, need / 1e6, t[len(t) // 2],
                   t[0], t[-1]))
        if max(sizes) <= args.skip_host_above:
            ms, total = host_time(graphs)
            assert total == found, "the restatement finds %d comparisons" % total
            line += "  numpy %10.1f" % ms
        print(line)
        sys.stdout.flush()


if __name__ == "__main__":
    main()
