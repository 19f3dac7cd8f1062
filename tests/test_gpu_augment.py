"""The judgement hull on the device (librf_augment_hip.so) against tests/augment_numpy.py, exactly and in
order: one call over images of 0, 2, 3, 63, 64, 65, 257 and 300 nodes - no judgements, the smallest
graph, the contradiction cycle, a wave's edge, past a 256-thread stride, two components - with and
without coins and point ids, over dirty workspaces, twice; an image alone against the same image in
the list; the node limit; a captured call replayed on a decoy.  The trainer on an augmented set:
tests/test_gpu_augment_train.py."""
import numpy as np
import pytest
import torch

from tests import augment_numpy as restate

pytestmark = pytest.mark.gpu
GUARD = 256
NODES = (0, 2, 3, 63, 64, 65, 257, 300)


def random_graph(seed, nodes, components=1, extra=0.8, first_id=1000):
    """A build_graphs-shaped graph (edges, weights, node_point) in which every node has an edge: per
    component a random tree over nearby nodes plus `extra` more judgements per node, about half '='
    (both directions), weights with two decimals so that ties happen, contradictions included."""
    rng = np.random.RandomState(seed)
    pairs = {}

    def judge(a, b):
        weight = round(rng.uniform(0.05, 2.4), 2)
        kind = rng.randint(0, 4)
        if kind < 2:
            pairs[(a, b)] = (0, weight)
            pairs[(b, a)] = (0, weight)
        elif kind == 2:
            pairs[(a, b)] = (2, weight)
        else:
            pairs[(b, a)] = (2, weight)

    bounds = np.linspace(0, nodes, components + 1).astype(int)
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        for v in range(lo + 1, hi):
            judge(v, rng.randint(max(lo, v - 6), v))
        for _ in range(int(extra * (hi - lo))):
            a, b = rng.randint(lo, hi, 2)
            if a != b:
                judge(a, b)
    keys = sorted(pairs)
    keys = [keys[i] for i in rng.permutation(len(keys))]
    edges = np.array([(a, b, pairs[(a, b)][0]) for a, b in keys], dtype=np.int32).reshape(-1, 3)
    weights = np.array([pairs[k][1] for k in keys], dtype=np.float64)
    return edges, weights, first_id + rng.permutation(10 * nodes + 1)[:nodes].astype(np.int64)


def the_graphs():
    graphs = []
    for k, nodes in enumerate(NODES):
        if nodes == 0:
            graphs.append((np.zeros((0, 3), np.int32), np.zeros(0), np.zeros(0, np.int64)))
        elif nodes == 3:        # A < B < C < A
            graphs.append((np.array([[0, 1, 2], [1, 2, 2], [2, 0, 2]], np.int32),
                           np.array([0.9, 0.7, 0.5]), np.array([7, 8, 9], np.int64)))
        else:
            graphs.append(random_graph(40 + k, nodes, components=2 if nodes == 300 else 1))
    return graphs


def the_coins(graphs, seed=5):
    rng = np.random.RandomState(seed)
    return [rng.randint(0, 2, (len(g[2]), len(g[2]))).astype(np.uint8) for g in graphs]


_EXPECTED = {}


def expected(graphs, coins, with_points, key):
    """The restatement's lists, computed once per key and never changed."""
    if key not in _EXPECTED:
        out = []
        for g, c in zip(graphs, coins if coins is not None else [None] * len(graphs)):
            comps, weights = restate.hull(len(g[2]), g[0], g[1], coins=c,
                                          node_point=g[2] if with_points else None)
            comps.setflags(write=False)
            weights.setflags(write=False)
            out.append((comps, weights))
        _EXPECTED[key] = out
    return _EXPECTED[key]


class Guarded(object):
    """A device buffer with 256 guard bytes of 0xA5 on both sides."""

    def __init__(self, array=None, nbytes=None, fill=0xA5):
        nbytes = max(array.nbytes if array is not None else nbytes, 16)
        self.raw = torch.full((nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        self.body = self.raw[GUARD:GUARD + nbytes]
        self.body.fill_(fill)
        if array is not None and array.nbytes:
            self.put(array)
        self.ptr = self.raw.data_ptr() + GUARD

    def put(self, array):
        flat = torch.from_numpy(np.ascontiguousarray(array).view(np.uint8).reshape(-1))
        self.body[:flat.numel()].copy_(flat)

    def host(self, dtype):
        return self.body.cpu().numpy().view(dtype)

    def intact(self):
        raw = self.raw.cpu().numpy()
        return (raw[:GUARD] == 0xA5).all() and (raw[-GUARD:] == 0xA5).all()


class Call(object):
    """The device buffers of one rf_augment_hull_f64 call over `graphs`, outputs pre-filled with 0xA5."""

    def __init__(self, graphs, coins=None, with_points=True, fill=0xA5):
        from reflectance_filtering_amd import _ffi_augment, augment
        self.lib = _ffi_augment.load_library()
        self.host = h = augment.pack_graphs(graphs)
        self.n = len(graphs)
        self.total_matrix, self.cap = int(h["matrix_offsets"][-1]), int(h["out_offsets"][-1])
        self.inputs = dict((k, Guarded(h[k])) for k in ("edges", "edge_weights", "edge_offsets",
                                                        "node_offsets", "matrix_offsets",
                                                        "out_offsets", "node_point"))
        self.coins = None
        if coins is not None:
            self.coins = Guarded(np.concatenate([c.reshape(-1) for c in coins] + [np.zeros(0, np.uint8)]))
        self.with_points = with_points
        self.comps = Guarded(nbytes=12 * self.cap)
        self.weights = Guarded(nbytes=8 * self.cap)
        self.counts = Guarded(nbytes=4 * self.n)
        self.need = _ffi_augment.hull_workspace_bytes(self.total_matrix)
        self.workspace = Guarded(nbytes=self.need, fill=fill)
        assert self.workspace.ptr % 16 == 0

    def args(self, stream, max_nodes=None):
        h, i = self.host, self.inputs
        return [i["edges"].ptr, i["edge_weights"].ptr, i["edge_offsets"].ptr, i["node_offsets"].ptr,
                i["matrix_offsets"].ptr, i["out_offsets"].ptr,
                i["node_point"].ptr if self.with_points else None,
                self.coins.ptr if self.coins is not None else None, self.n,
                int(h["nodes"].max()) if max_nodes is None else max_nodes, int(h["node_offsets"][-1]),
                int(h["edge_offsets"][-1]), self.total_matrix, self.cap, self.comps.ptr,
                self.weights.ptr, self.counts.ptr, self.workspace.ptr, self.need, stream]

    def run(self):
        from reflectance_filtering_amd import _ffi, _ffi_augment
        rc = self.lib.rf_augment_hull_f64(*self.args(_ffi.current_stream_ptr(torch)))
        _ffi_augment.check(rc, "rf_augment_hull_f64")
        torch.cuda.synchronize()
        return self.raw_outputs()

    def raw_outputs(self):
        return (self.comps.host(np.uint8).copy(), self.weights.host(np.uint8).copy(),
                self.counts.host(np.uint8).copy())

    def lists(self):
        """Per image (comps, weights); the rows behind every list must still hold the fill."""
        comps = self.comps.host(np.int32)[:3 * self.cap].reshape(-1, 3)
        weights = self.weights.host(np.float64)[:self.cap]
        counts = self.counts.host(np.int32)[:self.n]
        raw = self.weights.host(np.uint8)[:8 * self.cap].reshape(-1, 8)
        out = []
        for b in range(self.n):
            o0, o1 = int(self.host["out_offsets"][b]), int(self.host["out_offsets"][b + 1])
            assert 0 <= counts[b] <= o1 - o0
            assert (raw[o0 + counts[b]:o1] == 0xA5).all(), "a write behind the list of image %d" % b
            out.append((comps[o0:o0 + counts[b]], weights[o0:o0 + counts[b]]))
        for buf in list(self.inputs.values()) + [self.comps, self.weights, self.counts, self.workspace]:
            assert buf.intact()
        return out


def assert_lists_equal(got, want):
    assert len(got) == len(want)
    for b, ((gc, gw), (wc, ww)) in enumerate(zip(got, want)):
        assert gc.shape == wc.shape, "image %d: %d comparisons, the restatement has %d" % (
            b, len(gc), len(wc))
        assert np.array_equal(gc, wc), "image %d: comparisons differ" % b
        assert np.array_equal(gw.view(np.uint64), ww.view(np.uint64)), "image %d: weights differ" % b


@pytest.mark.parametrize("with_coins", (False, True), ids=("coins-null", "coins-seeded"))
@pytest.mark.parametrize("with_points", (True, False), ids=("point-ids", "node-ids"))
def test_hull_equals_the_restatement_in_order(built, with_coins, with_points):
    graphs = the_graphs()
    coins = the_coins(graphs) if with_coins else None
    want = expected(graphs, coins, with_points, (with_coins, with_points))
    assert [len(c) for c, _ in want][:3] == [0, 1, 3]
    assert any((w[0][:, 2] == 0).any() for w in want) and any((w[0][:, 2] == 2).any() for w in want)
    first = None
    for fill in (0xA5, 0x00, 0xFF):
        call = Call(graphs, coins, with_points, fill)
        raw = call.run()
        assert_lists_equal(call.lists(), want)
        if first is None:
            first = raw
            again = call.run()              # a second time over the workspace the first run left
            assert all(np.array_equal(a, b) for a, b in zip(again, first))
        assert all(np.array_equal(a, b) for a, b in zip(raw, first)), "fill 0x%02X" % fill
    if with_coins:      # the coins decide something here
        plain = expected(graphs, None, with_points, (False, with_points))
        assert any(not np.array_equal(a[0], b[0]) for a, b in zip(want, plain))


def test_an_image_alone_is_the_image_in_the_list(built):
    graphs, coins = the_graphs(), the_coins(the_graphs())
    packed = Call(graphs, coins)
    packed.run()
    inside = packed.lists()
    for b in (2, 5, 7):
        alone = Call([graphs[b]], [coins[b]])
        alone.run()
        assert_lists_equal(alone.lists(), [inside[b]])


def test_through_the_python_interface(built):
    from reflectance_filtering_amd import augment
    graphs, coins = the_graphs()[:6], the_coins(the_graphs())[:6]
    want = expected(the_graphs(), the_coins(the_graphs()), True, (True, True))[:6]
    # a cap that forces several calls: at most two of the small matrices fit
    lists = augment.hull(graphs, coins=coins, workspace_cap=9 * (65 * 65 + 64 * 64) + 48)
    assert len(augment.split_packs([len(g[2]) for g in graphs], 9 * (65 * 65 + 64 * 64) + 48)) > 1
    for got, (wc, ww) in zip(lists, want):
        assert [row[:3] for row in got] == [[a, b, float(r)] for a, b, r in wc.tolist()]
        assert [row[3] for row in got] == ww.tolist()
    seeded = augment.hull(graphs, seed=11)
    assert seeded == augment.hull(graphs, seed=11)
    assert [len(a) for a in seeded] == [len(c) for c, _ in want]       # a coin moves no count
    assert augment.hull([]) == []


def limit_graph(nodes):
    """`nodes` nodes: a random component of 10, then the pairs (10 -> 11), (12 -> 13), ...; its hull
    is the hull of the component followed by the pair edges, row by row."""
    head = random_graph(3, 10)
    tail = np.arange(10, nodes - 1, 2)
    edges = np.concatenate([head[0], np.stack([tail, tail + 1, 2 * (tail % 4 == 0)], axis=1)])
    weights = np.concatenate([head[1], 0.25 + (tail % 7) / 8.0])
    assert nodes % 2 == 0 and len(np.unique(edges[:, :2])) == nodes
    comps, w = restate.hull(10, head[0], head[1])
    want = (np.concatenate([comps, edges[len(head[0]):]]).astype(np.int32),
            np.concatenate([w, weights[len(head[1]):]]))
    return (edges.astype(np.int32), weights, np.arange(nodes, dtype=np.int64)), want


def test_node_limit(built):
    from reflectance_filtering_amd import _ffi, _ffi_augment
    limit = _ffi_augment.MAX_NODES
    assert limit >= 2362
    graph, want = limit_graph(limit)
    budget = 256 << 20                  # bytes this test may take for the matrices
    assert _ffi_augment.hull_workspace_bytes(limit * limit) <= budget
    call = Call([graph], with_points=False)
    call.run()
    assert_lists_equal(call.lists(), [want])
    # one node more: refused on the host, nothing written
    call.comps.body.fill_(0xA5)
    call.weights.body.fill_(0xA5)
    call.counts.body.fill_(0xA5)
    rc = call.lib.rf_augment_hull_f64(*call.args(_ffi.current_stream_ptr(torch), max_nodes=limit + 1))
    assert rc == -2 and b"limit" in call.lib.rf_augment_last_error()
    torch.cuda.synchronize()
    assert all((raw == 0xA5).all() for raw in call.raw_outputs())


def test_captured_call_replays_on_a_decoy(built):
    """One call captured into a graph on a side stream; replayed on the true inputs it gives their hull,
    replayed after the decoy's edges and weights were put into the same buffers it gives the decoy's."""
    graphs = [the_graphs()[k] for k in (2, 5, 3)]
    decoys = []
    for edges, weights, points in graphs:       # the same pairs, other relations and weights
        flipped = edges.copy()
        upper = flipped[:, 0] < flipped[:, 1]
        flipped[:, 2] = np.where(upper, 2, flipped[:, 2])
        decoys.append((flipped, weights[::-1].copy(), points))
    want = [restate.hull(len(g[2]), g[0], g[1], node_point=g[2]) for g in graphs]
    want_decoy = [restate.hull(len(g[2]), g[0], g[1], node_point=g[2]) for g in decoys]
    assert any(not np.array_equal(a[1], b[1]) for a, b in zip(want, want_decoy))
    call, decoy = Call(graphs), Call(decoys)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        assert call.lib.rf_augment_hull_f64(*call.args(side.cuda_stream)) == 0       # warm
    torch.cuda.synchronize()
    for buf in (call.comps, call.weights, call.counts):
        buf.body.fill_(0xA5)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        rc = call.lib.rf_augment_hull_f64(*call.args(side.cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    assert all((raw == 0xA5).all() for raw in call.raw_outputs()), "the captured call ran eagerly"
    graph.replay()
    torch.cuda.synchronize()
    assert_lists_equal(call.lists(), want)
    for name in ("edges", "edge_weights"):
        call.inputs[name].put(decoy.host[name])
    for buf in (call.comps, call.weights, call.counts):
        buf.body.fill_(0xA5)
    call.workspace.body.fill_(0xFF)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    got = call.lists()
    assert_lists_equal(got, want_decoy)
    with pytest.raises(AssertionError):
        assert_lists_equal(got, want)
    del graph
