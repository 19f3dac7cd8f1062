"""Writes tests/golden/whdr_hinge.npz: the reference's own WhdrHingeLossLayer (forward and backward),
run on the CPU, on small batches that exercise every branch of it.

    python tests/golden/make_whdr_hinge.py /path/to/reference

The layer derives from caffe.Layer only to be found by Caffe; a two-line stand-in for the `caffe`
module (below, written here) lets it run under plain Python 3 / numpy.  Only the .npz is committed.

Cases (each a batch of 3 one-channel images of 24 x 40 with 5, 300 and 1,181 comparisons):
(delta, margin) = (0.1, 0), (0.12, 0.08), (0.1, 0.3) with every comparison evaluated, and
(0.1, 0) with ratio 0.5, eval_dense 0.  Points are shared by many comparisons (960 pixels), one
comparison of every image has coinciding ends, and two pixels are 0 (the lightness floor): one as
the second point of an active comparison, one as the first.  No ratio y lies within 1e-3 (relative)
of a hinge border - there a float32 evaluation may take the other branch and the gradient jumps by
the comparison's full weight - and the first comparison of every image is active, so that every
per-image loss is an array (the layer's np.mean refuses a mix of arrays and plain zeros).

Per case the file holds the inputs, the layer's per-image losses, batch loss and gradient, the
parameter string, and the distance of tests/whdr_hinge_numpy.py (float64) from the layer: max |gradient
difference| over max |gradient| per image (the largest of the three), and the relative loss difference.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

H, W = 24, 40
COUNTS = (5, 300, 1181)
CASES = ((0.1, 0.0, 1.0, 1), (0.12, 0.08, 1.0, 1), (0.1, 0.3, 1.0, 1), (0.1, 0.0, 0.5, 0))
GAP = 1e-3


class Blob(object):
    def __init__(self, data):
        self.data = data
        self.diff = np.zeros_like(data)

    def reshape(self, *shape):
        self.data = np.zeros(shape, dtype=np.float32)
        self.diff = np.ones(shape, dtype=np.float32)        # the loss weight Caffe puts there


def reference_layer(reference):
    caffe = types.ModuleType("caffe")
    caffe.Layer = type("Layer", (object,), {})
    sys.modules["caffe"] = caffe
    sys.path.insert(0, os.path.join(reference, "training", "layers"))
    from whdr_hinge_loss_layer import WhdrHingeLossLayer
    return WhdrHingeLossLayer


def draw_case(rng, delta, margin):
    from tests import whdr_hinge_numpy as restate
    refl = rng.uniform(0.02, 1.0, size=(3, 1, H, W)).astype(np.float32)
    refl[0, 0, 3, 5] = 0.0
    refl[1, 0, 7, 11] = 0.0
    limits = restate.borders(delta, margin)
    comps = []
    redrawn = 0
    for b, m in enumerate(COUNTS):
        rows = np.zeros((m, 6), dtype=np.float64)
        k = 0
        while k < m:
            x1, x2 = rng.randint(0, W, size=2)
            y1, y2 = rng.randint(0, H, size=2)
            darker = rng.randint(0, 3)
            if k == 1:                      # coinciding ends
                x2, y2 = x1, y1
            if k == 2 and b == 0:           # the floor as point 2 of an active comparison
                x2, y2, darker = 5, 3, 1
            if k == 2 and b == 1:           # the floor as point 1
                x1, y1, darker = 11, 7, 2
            l1 = max(restate.EPS, float(refl[b, 0, y1, x1]))
            l2 = max(restate.EPS, float(refl[b, 0, y2, x2]))
            y = l1 / l2
            # (coinciding ends: y is exactly 1 in every precision, also where 1 is a border)
            if k != 1 and any(abs(y - lim) <= GAP * lim for lim in limits):
                redrawn += 1
                continue
            row = np.array([[x1, y1, x2, y2, darker, rng.uniform(0.05, 1.5)]])
            if k == 0:
                loss, _, _ = restate.comparison_terms(np.array([l1]), np.array([l2]),
                                                      np.array([darker]), delta, margin)
                if not loss[0] > 0:
                    continue
            rows[k] = row
            k += 1
        rows[:, 5] = rows[:, 5].astype(np.float32)          # the blob is float32
        comps.append(rows)
    return refl, comps, redrawn


def comparison_blob(comps):
    """The layer's second bottom: [batch, MAX + 1, 1, 6] float32, coordinates normalised so that
    int(x * width) is the pixel, the last row holding the count (and a file name)."""
    blob = np.zeros((len(comps), max(COUNTS) + 1, 1, 6), dtype=np.float32)
    for b, rows in enumerate(comps):
        m = rows.shape[0]
        blob[b, :m, 0, :] = rows
        blob[b, :m, 0, 0] = (rows[:, 0] + 0.5) / W
        blob[b, :m, 0, 2] = (rows[:, 2] + 0.5) / W
        blob[b, :m, 0, 1] = (rows[:, 1] + 0.5) / H
        blob[b, :m, 0, 3] = (rows[:, 3] + 0.5) / H
        blob[b, -1, 0, 0] = m
        blob[b, -1, 0, 1] = b
    return blob


def main(reference):
    from reflectance_filtering_amd import train, whdr
    from tests import whdr_hinge_numpy as restate
    layer_class = reference_layer(reference)
    out = {"n_cases": np.array(len(CASES))}
    for c, (delta, margin, ratio, eval_dense) in enumerate(CASES):
        rng = np.random.RandomState(1000 + c)
        refl, comps, redrawn = draw_case(rng, delta, margin)
        layer = layer_class()
        layer.param_str = "%r_%r_%r_%d" % (delta, margin, ratio, eval_dense)
        bottom = [Blob(refl.copy()), Blob(comparison_blob(comps))]
        top = [Blob(np.zeros(1, dtype=np.float32))]
        layer.setup(bottom, top)
        layer.reshape(bottom, top)
        layer.forward(bottom, top)
        layer.backward(top, [True, False], bottom)
        loss = float(top[0].data[0])
        diff = bottom[0].diff.copy()
        layer.diff = np.zeros_like(refl)
        losses = np.array([float(np.asarray(layer._whdr_hinge_single_img(bottom, b)).reshape(-1)[0])
                           for b in range(3)])
        # the restatement on the same inputs, in point-array form
        chosen = [train.select_comparisons(rows, ratio, bool(eval_dense)) for rows in comps]
        points, po, cp, wt, co = whdr.dedup_points(chosen, H, W)
        image = np.repeat(np.arange(3), np.diff(po))
        r = refl[image, 0, points[:, 1], points[:, 0]]
        my_losses, my_grad = restate.hinge_points(r, po, cp, wt, co, delta, margin)
        ref_grad = diff[image, 0, points[:, 1], points[:, 0]].astype(np.float64)
        rest = diff.copy()
        rest[image, 0, points[:, 1], points[:, 0]] = 0
        assert not rest.any(), "gradient outside the judgement points"
        dist_grad = max(np.abs(my_grad[po[i]:po[i + 1]] - ref_grad[po[i]:po[i + 1]]).max()
                        / np.abs(ref_grad[po[i]:po[i + 1]]).max() for i in range(3))
        dist_loss = max(np.abs(my_losses - losses).max() / np.abs(losses).max(),
                        abs(my_losses.mean() - loss) / abs(loss))
        print("case %d %s: redrawn %d of %d, loss %.6g, distance grad %.3g loss %.3g"
              % (c, layer.param_str, redrawn, sum(COUNTS), loss, dist_grad, dist_loss))
        out["case%d_param_str" % c] = np.array(layer.param_str)
        out["case%d_params" % c] = np.array([delta, margin, ratio, eval_dense], dtype=np.float64)
        out["case%d_refl" % c] = refl
        out["case%d_comparisons" % c] = np.concatenate(comps, axis=0)
        out["case%d_counts" % c] = np.array([rows.shape[0] for rows in comps])
        out["case%d_losses" % c] = losses
        out["case%d_loss" % c] = np.array(loss)
        out["case%d_diff" % c] = diff
        out["case%d_distance" % c] = np.array([dist_grad, dist_loss])
    np.savez_compressed(os.path.join(HERE, "whdr_hinge.npz"), **out)


if __name__ == "__main__":
    main(sys.argv[1])
