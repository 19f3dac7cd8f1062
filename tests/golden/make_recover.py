"""Writes tests/golden/recover.npz: the reference's own RecoverReflectanceShadingLayer (forward and backward)
with its BoundaryLossLayer on both tops, run on the CPU.

    python tests/golden/make_recover.py /path/to/reference

Both layers derive from caffe.Layer only to be found by Caffe, and the recover layer imports cv2 and
skimage.color without using them in these modes; stand-ins for the four modules (below, written here) let
them run under plain Python 3 / numpy.  Only the .npz is committed.

Cases: the four norms (rRelMean, rRelMax, rRelY, rRelNorm) x the penalties (L1, L2), each on a batch of 3
images of 24 x 40: image channels uniform in [0.02, 1], e uniform in [0.01, 1.3] so that reflectance and
shading both leave [0, 1] upwards (in rRelNorm the reflectance cannot: its channel mean is at most
e / sqrt(3)).  Planted: a pixel with e = 0 (the floor of R_i), a black pixel (the floor
of the norm) and a pixel with a negative channel (mean reflectance < 0).  Both losses carry the weight 0.1.

Per case the file holds the inputs in the reference's layout (e [3,1,H,W], image [3,3,H,W] with channels
R, G, B), both tops, both losses (float32, np.mean), bottom[0].diff, and the relative distance of each
np.mean(loss) from the float64 sum of the layer's own per-pixel losses divided by their number.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

N, H, W = 3, 24, 40
MODES = ("rRelMean", "rRelMax", "rRelY", "rRelNorm")
PENALTIES = ("L1", "L2")
SCALE = 0.1


class Blob(object):
    def __init__(self, data):
        self.data = data
        self.diff = np.zeros_like(data)

    def reshape(self, *shape):
        self.data = np.zeros(shape, dtype=np.float32)
        self.diff = np.zeros(shape, dtype=np.float32)


def reference_layers(reference):
    caffe = types.ModuleType("caffe")
    caffe.Layer = type("Layer", (object,), {})
    skimage = types.ModuleType("skimage")
    color = types.ModuleType("skimage.color")
    color.rgb2lab = color.lab2rgb = None
    skimage.color = color
    sys.modules.update({"caffe": caffe, "cv2": types.ModuleType("cv2"), "skimage": skimage,
                        "skimage.color": color})
    sys.path.insert(0, os.path.join(reference, "training", "layers"))
    from boundary_loss_layer import BoundaryLossLayer
    from recover_reflectance_shading_layer import RecoverReflectanceShadingLayer
    return RecoverReflectanceShadingLayer, BoundaryLossLayer


def draw_inputs(rng):
    image = rng.uniform(0.02, 1.0, size=(N, 3, H, W)).astype(np.float32)
    e = rng.uniform(0.01, 1.3, size=(N, 1, H, W)).astype(np.float32)
    e[0, 0, 3, 5] = 0.0
    image[1, :, 7, 11] = 0.0
    image[2, :, 20, 33] = (-0.9, 0.1, 0.2)
    return e, image


def run_boundary(layer_class, penalty, blob):
    """The layer on one top: (loss float32, distance of np.mean from the float64 mean); leaves blob.diff."""
    layer = layer_class()
    layer.param_str = penalty
    top = [Blob(np.zeros(1, dtype=np.float32))]
    layer.setup([blob], top)
    layer.reshape([blob], top)
    layer.forward([blob], top)
    top[0].diff[0] = SCALE                                  # the loss weight Caffe puts there
    layer.backward(top, [True], [blob])
    loss = top[0].data[0]
    pixels, _ = layer.error_norm(np.mean(blob.data, axis=1, keepdims=True))
    assert pixels.dtype == np.float32 and np.mean(pixels) == loss
    exact = pixels.astype(np.float64).sum() / pixels.size
    return np.float32(loss), abs(float(loss) - exact) / exact


def main(reference):
    recover_class, boundary_class = reference_layers(reference)
    out = {"n_cases": np.array(len(MODES) * len(PENALTIES)), "scale": np.float32(SCALE)}
    c = 0
    for mode in MODES:
        for penalty in PENALTIES:
            e, image = draw_inputs(np.random.RandomState(2000 + c))
            layer = recover_class()
            layer.param_str = mode
            bottom = [Blob(e.copy()), Blob(image.copy())]
            top = [Blob(None), Blob(None)]
            layer.setup(bottom, top)
            layer.reshape(bottom, top)
            layer.forward(bottom, top)
            loss_r, dist_r = run_boundary(boundary_class, penalty, top[0])
            loss_s, dist_s = run_boundary(boundary_class, penalty, top[1])
            layer.backward(top, [True, False], bottom)
            for blob in (top[0].data, top[1].data, bottom[0].diff):
                assert blob.dtype == np.float32 and np.isfinite(blob).all()
            live = [int((np.mean(t.data, axis=1) > 1).sum()) for t in top] + \
                   [int((np.mean(top[0].data, axis=1) < 0).sum())]
            # the unit colour of rRelNorm has a channel mean of at most 1 / sqrt(3): e <= 1.3 cannot lift it above 1
            assert min(live[1:]) > 0 and (live[0] > 0 or mode == "rRelNorm")
            print("case %d %s %s: losses %.6g %.6g, pixels above 1: %d %d, below 0: %d, mean distance %.3g %.3g"
                  % (c, mode, penalty, loss_r, loss_s, live[0], live[1], live[2], dist_r, dist_s))
            out["case%d_mode" % c] = np.array(mode)
            out["case%d_penalty" % c] = np.array(penalty)
            out["case%d_e" % c] = e
            out["case%d_image" % c] = image
            out["case%d_reflectance" % c] = top[0].data.copy()
            out["case%d_shading" % c] = top[1].data.copy()
            out["case%d_losses" % c] = np.array([loss_r, loss_s], dtype=np.float32)
            out["case%d_mean_distance" % c] = np.array([dist_r, dist_s])
            out["case%d_diff" % c] = bottom[0].diff.copy()
            c += 1
    np.savez_compressed(os.path.join(HERE, "recover.npz"), **out)


if __name__ == "__main__":
    main(sys.argv[1])
