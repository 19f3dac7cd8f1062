"""Writes tests/golden/augment.npz: the reference's own augment() (unify, node numbering, warshall,
consistency check), run on the CPU, on small judgement lists that exercise every rule of it.

    python tests/golden/make_augment.py /path/to/reference

training/createNumpyArrayWithComparisonsForIIW.py imports simplejson for its file reading; a
stand-in module (the standard json, set here) lets it import where simplejson is not installed.
Only the .npz is committed.

Cases (at most 130 nodes, which keeps the file small and the reference's triple loop to seconds):
a chain given in shuffled order (a long path needs many k), two components, the contradiction cycle
A<B<C<A, an '=' clique (which draws coins), mixed '=' and '<' paths, equal weights on both
directions of a contradicting pair (the tie rule), a duplicate ordered pair (the later one stands)
and a random IIW-like list.  Every case runs three times: np.random.rand fixed at 0.25, fixed at
0.75, and seeded - the draws the reference consumed are recorded, in order.

Per case c the file holds case<c>_comparisons [m,4] (point 1, point 2, darker, weight) and per mode
q case<c>_mode<q>_out [k,4], the list augment() returned, and case<c>_mode<q>_draws.
"""
import contextlib
import io
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
MODES = ("0.25", "0.75", "seeded")


def reference_augment(reference):
    sys.modules.setdefault("simplejson", json)
    sys.path.insert(0, os.path.join(reference, "training"))
    import createNumpyArrayWithComparisonsForIIW as builder
    return builder.augment


def cases():
    rng = np.random.RandomState(77)
    out = []
    # a chain 100 < 101 < ... < 139, its links in shuffled order and directions
    links = [(100 + i, 101 + i, 2, round(rng.uniform(0.3, 1.9), 3)) for i in range(39)]
    links = [links[i] for i in rng.permutation(39)]
    links = [(b, a, 1, w) if k % 3 == 0 else (a, b, d, w) for k, (a, b, d, w) in enumerate(links)]
    out.append(("chain", links))
    out.append(("two-components", [(1, 2, 2, 0.9), (2, 3, 2, 0.4), (3, 4, 0, 1.2), (10, 11, 1, 0.8),
                                   (11, 12, 1, 0.6), (12, 13, 0, 0.5), (10, 13, 2, 0.2)]))
    out.append(("cycle", [(7, 8, 2, 0.9), (8, 9, 2, 0.7), (9, 7, 2, 0.5)]))
    clique = [(20 + a, 20 + b, 0, round(rng.uniform(0.2, 1.5), 3))
              for a in range(8) for b in range(a + 1, 8)]
    out.append(("equal-clique", clique))
    out.append(("mixed", [(1, 2, 0, 0.8), (2, 3, 2, 0.6), (3, 4, 0, 0.9), (4, 5, 1, 0.7),
                          (6, 5, 0, 1.1), (1, 6, 2, 0.3), (7, 3, 0, 0.4), (7, 1, 2, 1.0)]))
    out.append(("tie", [(1, 2, 2, 0.7), (1, 2, 1, 0.7), (2, 3, 2, 0.7), (3, 1, 0, 0.7),
                        (4, 1, 2, 0.5), (1, 4, 2, 0.5)]))
    out.append(("duplicate", [(1, 2, 2, 0.3), (2, 3, 0, 0.8), (1, 2, 2, 0.9), (3, 2, 0, 0.1),
                              (3, 4, 1, 0.6), (1, 2, 2, 0.5)]))
    # IIW-like: 130 points (127 of them judged) with ids of no order, about 1.6 judgements per point between
    # neighbours in a random layout, two thirds of them '=', scores like darker_score
    ids = rng.permutation(100000)[:130] + 1000
    rows, seen = [], set()
    while len(rows) < 208:
        a = rng.randint(0, 130)
        b = (a + rng.randint(1, 9)) % 130
        if (a, b) in seen or (b, a) in seen:
            continue
        seen.add((a, b))
        darker = int(rng.choice([0, 0, 0, 0, 1, 2]))
        rows.append((int(ids[a]), int(ids[b]), darker, round(rng.uniform(0.05, 2.4), 4)))
    out.append(("iiw-like", rows))
    return out


def main(reference):
    augment = reference_augment(reference)
    real_rand = np.random.rand
    out = {"n_cases": np.array(len(cases())), "modes": np.array(MODES)}
    try:
        for c, (name, comparisons) in enumerate(cases()):
            out["case%d_name" % c] = np.array(name)
            out["case%d_comparisons" % c] = np.array(comparisons, dtype=np.float64).reshape(-1, 4)
            for q, mode in enumerate(MODES):
                draws = []
                source = (np.random.RandomState(500 + c).rand if mode == "seeded"
                          else (lambda value=float(mode): value))

                def rand():
                    draws.append(source())
                    return draws[-1]

                np.random.rand = rand
                with contextlib.redirect_stdout(io.StringIO()):
                    result = augment([list(row) for row in comparisons])
                out["case%d_mode%d_out" % (c, q)] = np.array(result, dtype=np.float64).reshape(-1, 4)
                out["case%d_mode%d_draws" % (c, q)] = np.array(draws, dtype=np.float64)
                print("%s, rand %s: %d comparisons -> %d, %d draws"
                      % (name, mode, len(comparisons), len(result), len(draws)))
    finally:
        np.random.rand = real_rand
    np.savez_compressed(os.path.join(HERE, "augment.npz"), **out)


if __name__ == "__main__":
    main(sys.argv[1])
