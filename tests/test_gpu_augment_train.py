"""The trainer on augmented comparisons, end to end on the device: a handful of synthetic photos,
their judgements' hull through augment.hull, train.pack with that second set, and loss_and_grad
against the float64 hinge restatement on the same arrays - all comparisons, and with a forced
subsample on the chosen ones alone.  The yardstick is that of tests/test_gpu_train.py: four times the
largest distance tests/golden/whdr_hinge.npz records."""
import os

import numpy as np
import pytest
import torch

from tests import augment_numpy, synth, whdr_hinge_numpy as restate

pytestmark = pytest.mark.gpu
SIZES = ((40, 56), (33, 47), (48, 48), (25, 64), (40, 40))
POINTS = (26, 9, 31, 2, 0)
GAP = 1e-5      # no ratio this close (relative) to a hinge border: float32 takes the float64 branch
DELTA, MARGIN = 0.12, 0.05


def photos():
    """Per photo: image, judgements (id 1, id 2, darker, weight), points {id: (x, y)} normalised."""
    out = []
    for k, ((h, w), count) in enumerate(zip(SIZES, POINTS)):
        rng = np.random.RandomState(300 + k)
        image = synth.scene_u8(h, w, seed=60 + k)
        cells = rng.permutation(h * w)[:count]
        points = dict((7000 + 13 * i, ((c % w + 0.5) / w, (c // w + 0.5) / h)) for i, c in enumerate(cells))
        ids = sorted(points)
        rows = []
        for i in range(1, count):
            rows.append((ids[i], ids[rng.randint(max(0, i - 4), i)], int(rng.randint(0, 3)),
                         float(rng.randint(2, 40)) / 16))
        for _ in range(count // 2):
            a, b = rng.randint(0, count, 2)
            if a != b:
                rows.append((ids[a], ids[b], int(rng.randint(0, 3)), float(rng.randint(2, 40)) / 16))
        out.append((image, rows, points))
    return out


def to_px(rows6, size):
    from reflectance_filtering_amd import whdr
    return whdr.to_pixels(rows6, size[0], size[1])


@pytest.fixture(scope="module")
def packed_sets(built):
    from reflectance_filtering_amd import augment, train
    sets = photos()
    graphs = [augment.build_graphs(rows) for _, rows, _ in sets]
    lists = augment.hull(graphs, seed=17)
    # the device's lists are the restatement's up to the coin: the same pairs survive, one direction each
    for got, (_, rows, _) in zip(lists, sets):
        want = augment_numpy.augment(rows)
        assert sorted(tuple(sorted(r[:2])) for r in got) == sorted(tuple(sorted(r[:2])) for r in want)
    images = [image for image, _, _ in sets]
    plain = [to_px(np.array([points[a] + points[b] + (d, w) for a, b, d, w in rows],
                            dtype=np.float64).reshape(-1, 6), image.shape)
             for image, rows, points in sets]
    hull = [to_px(augment.to_rows(a, points), image.shape) for a, (image, _, points) in zip(lists, sets)]
    assert sum(len(h) for h in hull) > 3 * sum(len(p) for p in plain)
    return images, plain, hull, train.pack(images, plain, hinge_comparisons_px=hull), train.pack(images, plain)


def bound(golden_dir):
    """The device's distance on arrays other than the fixture's own, as tests/test_gpu_train.py takes it
    (test_hinge_entry_empty_and_weightless_images): four times the LARGEST distance the file records, for
    the gradient and for the losses alike.  The largest is a gradient distance; the photo here with a
    single comparison shows why the losses need it too: its loss is one float32 hinge term y - border of
    about 0.15 that carries the two float32 roundings of y (about 1e-7 absolute, measured 6.5e-7 relative),
    where the fixture's images average five comparisons and more."""
    data = np.load(os.path.join(golden_dir, "whdr_hinge.npz"))
    recorded = np.array([data["case%d_distance" % c] for c in range(int(data["n_cases"]))])
    return 4 * recorded.max(), 4 * recorded.max()


def check_against_restatement(packed, per_image, comps, weights, comp_offsets, golden_dir):
    r = packed.r.cpu().numpy()
    po = packed.point_offsets
    y = restate.ratios(r, po, comps, comp_offsets)
    apart = comps[:, 0] != comps[:, 1]
    for lim in restate.borders(DELTA, MARGIN):
        assert (np.abs(y[apart] - lim) > GAP * lim).all(), "a ratio at a hinge border: draw other photos"
    want_l, want_g = restate.hinge_points(r, po, comps, weights, comp_offsets, DELTA, MARGIN)
    grad = packed.grad_r.cpu().numpy()[:packed.total].astype(np.float64)
    busy = [i for i in range(packed.n) if po[i + 1] > po[i] and np.abs(want_g[po[i]:po[i + 1]]).max() > 0]
    dg = max(np.abs(grad[po[i]:po[i + 1]] - want_g[po[i]:po[i + 1]]).max()
             / np.abs(want_g[po[i]:po[i + 1]]).max() for i in busy)
    dl = np.abs(per_image - want_l).max() / np.abs(want_l).max()
    limit_g, limit_l = bound(golden_dir)
    print("device-to-restatement gradient %.3g (limit %.3g) loss %.3g (limit %.3g)" % (dg, limit_g, dl, limit_l))
    assert len(busy) >= 3 and dg <= limit_g and dl <= limit_l
    idle = [i for i in range(packed.n) if i not in busy]
    assert all(not grad[po[i]:po[i + 1]].any() and per_image[i] == 0 for i in idle)
    return want_l


def test_pack_with_the_hull_and_loss_and_grad(packed_sets, golden_dir):
    from reflectance_filtering_amd import train, weights as wmod
    images, plain, hull, packed, packed_plain = packed_sets
    assert packed.n == 5 and np.diff(packed.comp_offsets).tolist() == [len(h) for h in hull]
    assert np.diff(packed.whdr_comp_offsets).tolist() == [len(p) for p in plain]
    w = wmod.load_weights()
    loss, per_image, grad_w = train.loss_and_grad(w, packed, 0, packed.n, DELTA, MARGIN)
    want_l = check_against_restatement(packed, per_image, packed.comps, packed.weights,
                                       packed.comp_offsets, golden_dir)
    assert abs(loss - want_l.mean()) <= 1e-6 * want_l.mean()
    assert grad_w.shape == (4513,) and bool(torch.isfinite(grad_w).all()) and bool(grad_w.abs().max() > 0)
    # the true WHDR is that of the original judgements: the figure the plain pack gives
    got = train.evaluate(w, packed, DELTA, MARGIN)
    want = train.evaluate(w, packed_plain, DELTA, MARGIN)
    assert got["whdr"] == want["whdr"] and got["hinge"] != want["hinge"]
    assert np.array_equal(train.whdr_at_points(packed, DELTA), train.whdr_at_points(packed_plain, DELTA))


def test_a_forced_subsample_is_the_loss_on_the_chosen_comparisons(packed_sets, golden_dir):
    from reflectance_filtering_amd import train, weights as wmod
    _, _, hull, packed, _ = packed_sets
    keep = 40
    sizes = np.diff(packed.comp_offsets)
    assert (sizes > keep).sum() >= 2 and (sizes <= keep).sum() >= 2
    chooser = torch.Generator(device=packed.x.device)
    chooser.manual_seed(23)
    step_weights = train.subsample_weights(packed, 0, packed.n, keep, chooser)
    chosen = step_weights.cpu().numpy() != 0
    assert [int(chosen[a:b].sum()) for a, b in zip(packed.comp_offsets[:-1], packed.comp_offsets[1:])] \
        == [min(int(m), keep) for m in sizes]
    w = wmod.load_weights()
    _, per_image, _ = train.loss_and_grad(w, packed, 0, packed.n, DELTA, MARGIN, hinge_weights=step_weights)
    offsets = np.concatenate([[0], np.cumsum([chosen[a:b].sum() for a, b in
                                              zip(packed.comp_offsets[:-1], packed.comp_offsets[1:])])])
    check_against_restatement(packed, per_image, packed.comps[chosen], packed.weights[chosen],
                              offsets.astype(np.int32), golden_dir)
    _, whole, _ = train.loss_and_grad(w, packed, 0, packed.n, DELTA, MARGIN)
    assert not np.array_equal(whole, per_image)
    # a fit step with the option draws the same way from its seed and stays finite
    final, _ = train.fit(packed, w, iterations=2, batch_size=2, base_lr=1e-3, max_evaluated=keep, seed=3)
    assert np.isfinite(final).all() and not np.array_equal(final, w)
