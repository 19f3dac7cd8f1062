"""Time of one training step (forward at the points + hinge loss + backward + optimiser) through the
training library against the same step in plain PyTorch on the device (gather, six matmuls,
autograd), for three workloads: a minibatch of 10 IIW-sized images, 640 images, and 1 M points.

    python tools/train_step_time.py [--repeats 9] > profiles/train_step_time.txt

Nine alternating repeats per workload (library, torch, library, ...), each the mean of `--inner`
steps between two device synchronisations after a warm-up; min / median / max in milliseconds.
The comparator lives here and is not part of the package.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from reflectance_filtering_amd import train, weights as wmod   # noqa: E402

DELTA, MARGIN, LR, MOMENTUM = 0.1, 0.0, 1e-3, 0.9


def workload(n_images, comps_per_image, seed):
    """Synthetic photos of 341 x 512 with IIW-like judgement counts (points shared)."""
    rng = np.random.RandomState(seed)
    image = rng.randint(0, 256, (341, 512, 3)).astype(np.uint8)
    images, comps = [], []
    for _ in range(n_images):
        npts = max(2, comps_per_image // 2)
        px, py = rng.randint(0, 512, npts), rng.randint(0, 341, npts)
        a, b = rng.randint(0, npts, comps_per_image), rng.randint(0, npts, comps_per_image)
        rows = np.zeros((comps_per_image, 6))
        rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3] = px[a], py[a], px[b], py[b]
        rows[:, 4], rows[:, 5] = rng.randint(0, 3, comps_per_image), rng.uniform(0.2, 1.5, comps_per_image)
        images.append(image)
        comps.append(rows)
    return train.pack(images, comps)


def library_step(packed, state):
    _, _, grad = train.loss_and_grad(state["w"], packed, 0, packed.n, DELTA, MARGIN)
    state["v"].mul_(MOMENTUM).add_(grad, alpha=LR)
    state["w"].sub_(state["v"])


def torch_net(x, w):
    h = x.flip(1)
    acts = []
    h = torch.relu(h @ w[0:96].view(32, 3).t() + w[96:128])
    acts.append(h)
    for l in range(4):
        base = 128 + l * 1056
        h = torch.relu(h @ w[base:base + 1024].view(32, 32).t() + w[base + 1024:base + 1056])
        acts.append(h)
    return torch.sigmoid(torch.cat(acts, 1) @ w[4352:4512] + w[4512])


def torch_step(packed, state, dev_arrays):
    i1, i2, darker, weight, image, wsum = dev_arrays
    w = state["w"].detach().requires_grad_(True)
    r = torch_net(packed.x, w)
    eps = float(np.finfo(np.float32).eps)
    light = r + (r.clamp(min=eps) - r).detach()
    y = light[i1] / light[i2]
    up, b = 1 + DELTA + MARGIN, 1 + DELTA - MARGIN
    loss = torch.where(darker == 1, (y - 1 / up).clamp(min=0),
                       torch.where(darker == 2, (up - y).clamp(min=0),
                                   torch.maximum((y - b).clamp(min=0), (1 / b - y).clamp(min=0))))
    per_image = torch.zeros(packed.n, device=r.device).index_add_(0, image, weight * loss) / wsum
    total = per_image.mean()
    total.backward()
    total.item()                        # the library step reads its loss back too
    with torch.no_grad():
        state["v"].mul_(MOMENTUM).add_(w.grad, alpha=LR)
        state["w"].sub_(state["v"])


def torch_arrays(packed):
    dev = packed.x.device
    image = np.repeat(np.arange(packed.n), np.diff(packed.comp_offsets))
    base = packed.point_offsets[:-1][image].astype(np.int64)
    wsum = np.add.reduceat(packed.weights, packed.comp_offsets[:-1])
    up = (lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev))
    return (up(base + packed.comps[:, 0], np.int64), up(base + packed.comps[:, 1], np.int64),
            up(packed.comps[:, 2], np.int64), up(packed.weights, np.float32), up(image, np.int64),
            up(wsum, np.float32))


def timed(step, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--inner", type=int, default=10)
    args = ap.parse_args()
    print("one training step, ms (min / median / max of %d alternating repeats of %d steps), %s"
          % (args.repeats, args.inner, torch.cuda.get_device_name(0)))
    for name, n_images, per_image in (("10 images", 10, 700), ("640 images", 640, 700),
                                      ("1 M points", 1000, 2000)):
        packed = workload(n_images, per_image, seed=n_images)
        arrays = torch_arrays(packed)
        fresh = (lambda: {"w": torch.from_numpy(wmod.load_weights()).cuda(),
                          "v": torch.zeros(4513, device="cuda")})
        lib_state, torch_state = fresh(), fresh()
        steps = {"library": (lambda: library_step(packed, lib_state)),
                 "torch": (lambda: torch_step(packed, torch_state, arrays))}
        for step in steps.values():
            timed(step, 3)
        times = {"library": [], "torch": []}
        for _ in range(args.repeats):
            for which in ("library", "torch"):
                times[which].append(timed(steps[which], args.inner))
        for which in ("library", "torch"):
            t = sorted(times[which])
            print("%-12s %8d points %8d comparisons  %-8s %8.3f / %8.3f / %8.3f"
                  % (name, packed.total, packed.comps.shape[0], which, t[0], t[len(t) // 2], t[-1]))


if __name__ == "__main__":
    main()
