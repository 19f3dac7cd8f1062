"""Time of one dense training step of the rRelMean mode (train.loss_and_grad on train.pack_dense) on a minibatch
of 10 photos of 341 x 512, its stages each alone, the rDirectly step on the same pack, and the same dense step in
plain PyTorch on the device (six matmuls, the recover arithmetic, both boundary means, autograd).

    python tools/recover_step_time.py [--repeats 9] > profiles/recover_step_time.txt

Stages: the dense forward pass (rf_cnn_reflectance_packed_f32 over every pixel), the three launches of
librf_recover_hip.so (recover-forward at the points, boundary backward over every pixel, hinge scatter), the
dense backward pass (rf_train_cnn_points_backward_f32 over every pixel).  Nine alternating repeats (every
candidate once per round), each the mean of `--inner` runs between two device synchronisations after a warm-up;
min / median / max in milliseconds.  The whole step also holds the hinge entry, three read-backs of losses and the
host copy of the weights the forward pass packs.  The comparator lives here and is not part of the package.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from reflectance_filtering_amd import train, weights as wmod   # noqa: E402
from tools.train_step_time import timed, torch_arrays, torch_net   # noqa: E402

DELTA, MARGIN, NORM, MODE, PENALTY = 0.1, 0.0, 0, "rRelMean", "L1"
SCALE_WHDR, SCALE_BOUNDARIES = 1.0, 0.1
EPS = float(np.finfo(np.float32).eps)


def workload(n_images, comps_per_image, seed):
    """Synthetic photos of 341 x 512 with IIW-like judgement counts (points shared), packed densely."""
    rng = np.random.RandomState(seed)
    images, comps = [], []
    for _ in range(n_images):
        npts = max(2, comps_per_image // 2)
        pixels = rng.choice(341 * 512, npts, replace=False)
        py, px = np.divmod(pixels, 512)
        a, b = rng.randint(0, npts, comps_per_image), rng.randint(0, npts, comps_per_image)
        rows = np.zeros((comps_per_image, 6))
        rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3] = px[a], py[a], px[b], py[b]
        rows[:, 4], rows[:, 5] = rng.randint(0, 3, comps_per_image), rng.uniform(0.2, 1.5, comps_per_image)
        images.append(rng.randint(0, 256, (341, 512, 3)).astype(np.uint8))
        comps.append(rows)
    return train.pack_dense(images, comps)


def floor(v):
    return v + (EPS - v).clamp(min=0).detach()


def torch_dense_step(packed, w0, arrays, point_pixel):
    i1, i2, darker, weight, image, wsum = arrays
    w = w0.detach().requires_grad_(True)
    x = packed.x_dense
    e = floor(torch_net(x, w))
    b, g, r = x[:, 0], x[:, 1], x[:, 2]
    m = floor(((r + g) + b) / 3)
    refl = e * (((r + g) + b) / m) / 3
    shading = m / e
    zero = torch.zeros_like(e)
    b_refl = torch.where(refl < 0, -refl, torch.where(refl > 1, refl - 1, zero)).mean()
    b_shad = torch.where(shading < 0, -shading, torch.where(shading > 1, shading - 1, zero)).mean()
    light = floor(refl)[point_pixel]
    y = light[i1] / light[i2]
    up, bd = 1 + DELTA + MARGIN, 1 + DELTA - MARGIN
    loss = torch.where(darker == 1, (y - 1 / up).clamp(min=0),
                       torch.where(darker == 2, (up - y).clamp(min=0),
                                   torch.maximum((y - bd).clamp(min=0), (1 / bd - y).clamp(min=0))))
    hinge = (torch.zeros(packed.n, device=x.device).index_add_(0, image, weight * loss) / wsum).mean()
    total = SCALE_WHDR * hinge + SCALE_BOUNDARIES * (b_refl + b_shad)
    total.backward()
    total.item()
    return w.grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--images", type=int, default=10)
    args = ap.parse_args()
    packed = workload(args.images, 700, seed=args.images)
    n, total, pixels = packed.n, packed.total, packed.pixels
    w = torch.from_numpy(wmod.load_weights()).cuda()
    arrays = torch_arrays(packed)
    x, e = train.forward_dense(w, packed, 0, n)
    pixel = packed.d_point_pixel[:total].contiguous()
    _, grad_e = train.boundary(packed, x, e, NORM, PENALTY, SCALE_BOUNDARIES, SCALE_BOUNDARIES)

    def new_launches():
        train.recover_points(x, e, pixel, NORM, packed.r[:total])
        _, g = train.boundary(packed, x, e, NORM, PENALTY, SCALE_BOUNDARIES, SCALE_BOUNDARIES)
        train.hinge_scatter(x, e, packed.grad_r[:total], pixel, NORM, SCALE_WHDR, g)

    steps = [
        ("dense forward", lambda: train.forward_dense(w, packed, 0, n)),
        ("recover + boundary + scatter", new_launches),
        ("dense backward", lambda: train._backward_at(w, packed, x, grad_e)),
        ("rRelMean step", lambda: train.loss_and_grad(w, packed, 0, n, DELTA, MARGIN, rs_mode=MODE,
                                                      loss_scale_whdr=SCALE_WHDR,
                                                      loss_scale_boundaries=SCALE_BOUNDARIES,
                                                      boundary_penalty=PENALTY)),
        ("rDirectly step", lambda: train.loss_and_grad(w, packed, 0, n, DELTA, MARGIN)),
        ("torch dense step", lambda: torch_dense_step(packed, w, arrays, pixel)),
    ]
    print("one rRelMean training step and its stages, ms (min / median / max of %d alternating repeats of %d runs), %s"
          % (args.repeats, args.inner, torch.cuda.get_device_name(0)))
    print("%d images of 341 x 512: %d pixels, %d points, %d comparisons" % (n, pixels, total, packed.comps.shape[0]))
    for _, step in steps:
        timed(step, 2)
    times = dict((name, []) for name, _ in steps)
    for _ in range(args.repeats):
        for name, step in steps:
            times[name].append(timed(step, args.inner))
    for name, _ in steps:
        t = sorted(times[name])
        print("%-30s %9.3f / %9.3f / %9.3f" % (name, t[0], t[len(t) // 2], t[-1]))
    med = dict((name, sorted(t)[len(t) // 2]) for name, t in times.items())
    stages = ("dense forward", "recover + boundary + scatter", "dense backward")
    print("the largest stage is the %s: %.0f %% of the step; the three stages sum to %.3f ms of its %.3f ms"
          % (max(stages, key=med.get), 100 * max(med[s] for s in stages) / med["rRelMean step"],
             sum(med[s] for s in stages), med["rRelMean step"]))
    # bytes the three new launches must move: x and e read, grad_e written (the points are a few thousand)
    moved = 20.0 * pixels
    print("recover + boundary + scatter move at least %.1f MB: %.0f GB/s at the median"
          % (moved / 1e6, moved / med["recover + boundary + scatter"] / 1e6))


if __name__ == "__main__":
    main()
