"""The judgement hull in numpy: a restatement of augment(comparisons, 'actual', 'min') of the
reference's training/createNumpyArrayWithComparisonsForIIW.py with one vectorised update per k
(S1..S4 of include/reflectance_filtering_augment.h).  Iteration k of the reference's loop never
writes row k or column k - the diagonal is absent, so a candidate for them has an absent operand -
and so all (i, j) of one k can be taken from a snapshot of that row and column.
tests/golden/augment.npz pins it on the reference's own output, entry for entry and in order.
"""
import numpy as np


def unify(comparisons):
    """(point 1, point 2, darker, weight) -> the reference's one-way list (x, y, relation, weight):
    '=' both ways with relation 0, '1 darker' turned round, relation 2."""
    unified = []
    for p1, p2, darker, weight in comparisons:
        if darker == 0:
            unified.append((p1, p2, 0, weight))
            unified.append((p2, p1, 0, weight))
        elif darker == 1:
            unified.append((p2, p1, 2, weight))
        elif darker == 2:
            unified.append((p1, p2, 2, weight))
        else:
            raise ValueError("darker is neither 0, 1, 2")
    return unified


def number_nodes(unified):
    """Nodes by first appearance in the unified list: (point -> node, node -> point)."""
    point_to_node, node_to_point = {}, []
    for x, y, _, _ in unified:
        for p in (x, y):
            if p not in point_to_node:
                point_to_node[p] = len(node_to_point)
                node_to_point.append(p)
    return point_to_node, node_to_point


def closure(n, edges, edge_weights):
    """S1 + S2: (rel, w) float64 [n, n], NaN = absent.  A later edge of an ordered pair replaces an
    earlier one, as the reference's matrix fill does."""
    rel = np.full((n, n), np.nan)
    w = np.full((n, n), np.nan)
    for (i, j, r), weight in zip(edges, edge_weights):
        rel[i, j], w[i, j] = r, weight
    off_diagonal = ~np.eye(n, dtype=bool)
    for k in range(n):
        col_w, row_w = w[:, k].copy(), w[k, :].copy()
        col_r, row_r = rel[:, k].copy(), rel[k, :].copy()
        c = np.minimum(col_w[:, None], row_w[None, :])          # NaN where either is absent
        with np.errstate(invalid="ignore"):
            take = np.isfinite(c) & (np.isnan(w) | (w < c)) & off_diagonal
        new_rel = np.where(col_r[:, None] == row_r[None, :], col_r[:, None], 2.0)
        w[take] = c[take]
        rel[take] = np.broadcast_to(new_rel, (n, n))[take]
    return rel, w


def resolve(rel, w, coins=None, draws=None):
    """S3 in place.  coins: [n, n], entry (i, j), i < j, non-zero drops (j, i) of a (0, 0) pair; or
    draws: a sequence handed to the (0, 0) pairs in row-major order as the reference consumes
    np.random.rand(), a draw > 0.5 being a non-zero coin.  Returns the number of draws taken."""
    n = rel.shape[0]
    upper = np.triu(np.ones((n, n), dtype=bool), 1)
    both = upper & np.isfinite(rel) & np.isfinite(rel.T)
    equal = both & (rel == 0) & (rel.T == 0)
    contra = both & ~equal
    with np.errstate(invalid="ignore"):
        drop_down = contra & (w > w.T)
    taken = int(equal.sum())
    if draws is not None:
        if len(draws) < taken:
            raise ValueError("%d draws for %d '=' pairs" % (len(draws), taken))
        flip = np.zeros((n, n), dtype=bool)
        flip[equal] = np.asarray(draws, dtype=np.float64)[:taken] > 0.5      # row-major
    elif coins is not None:
        flip = np.asarray(coins).reshape(n, n) != 0
    else:
        flip = np.zeros((n, n), dtype=bool)
    drop_down |= equal & flip
    drop_up = both & ~drop_down
    for drop in (drop_up, drop_down.T):
        rel[drop] = np.nan
        w[drop] = np.nan
    return taken


def hull(n, edges, edge_weights, coins=None, draws=None, node_point=None):
    """S1..S4 for one graph: (comps int32 [m,3] (index 1, index 2, relation), weights float64 [m])."""
    rel, w = closure(n, edges, edge_weights)
    resolve(rel, w, coins, draws)
    i, j = np.nonzero(np.isfinite(rel))                                      # row-major
    names = np.arange(n) if node_point is None else np.asarray(node_point)
    comps = np.stack([names[i], names[j], rel[i, j].astype(np.int64)], axis=1).astype(np.int32)
    return comps.reshape(-1, 3), w[i, j].astype(np.float64)


def augment(comparisons, coins=None, draws=None):
    """The reference's augment(): [[point 1, point 2, relation, weight], ...] of one photo."""
    unified = unify(comparisons)
    point_to_node, node_to_point = number_nodes(unified)
    edges = [(point_to_node[x], point_to_node[y], r) for x, y, r, _ in unified]
    comps, weights = hull(len(node_to_point), edges, [u[3] for u in unified], coins, draws,
                          node_to_point)
    return [[int(a), int(b), float(r), float(wt)] for (a, b, r), wt in zip(comps, weights)]
