"""WHDR evaluator: the host mirror against values produced by the reference's
own whdr_layer.whdr (tests/golden/whdr.npz), the IIW JSON reader, and - on a GPU - the batch
kernel against both."""
import json
import os

import numpy as np
import pytest

from reflectance_filtering_amd import whdr as W

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TAGS = ("grey", "colour", "none", "single")
DELTAS = (0.1, 0.0, 0.25)


def test_host_whdr_matches_reference_values():
    d = np.load(os.path.join(G, "whdr.npz"))
    for tag in TAGS:
        refl, comp = d[tag + "_refl"], d[tag + "_comparisons"]
        px = W.to_pixels(comp, refl.shape[1], refl.shape[2])
        assert np.array_equal(px, d[tag + "_pixels"]), tag
        got = np.array([W.whdr(refl, px, dl) for dl in DELTAS])
        assert np.array_equal(got, d[tag + "_whdr"]), tag
    with pytest.raises(Exception, match="1 or 3 channels"):
        W.whdr(np.ones((2, 4, 4), np.float32), np.array([[0, 0, 1, 1, 1, 1.0]]))


def _whdr_by_definition(refl, px, delta):
    """[Bell 2014] spelled out one judgement at a time (float32 image, float64 judgements)."""
    wrong = total = 0.0
    for x1, y1, x2, y2, darker, weight in px:
        l = []
        for x, y in ((x1, y1), (x2, y2)):
            v = refl[:, int(y), int(x)]
            v = v[0] if len(v) == 1 else (v[0] + v[1] + v[2]) / np.float32(3)
            l.append(v if v > W.EPS else W.EPS)
        limit = np.float32(1 + delta)
        says = 1 if l[1] / l[0] > limit else (2 if l[0] / l[1] > limit else 0)
        wrong += weight * (says != int(darker))
        total += weight
    return wrong / total if total else 0.0


def test_host_whdr_edge_cases_match_the_definition():
    rng = np.random.default_rng(3)
    for trial in range(40):
        c = (1, 3)[trial % 2]
        refl = (rng.random((c, 9, 13)) ** 3).astype(np.float32)
        refl[:, 2, 3] = 0                         # floored at EPS
        refl[:, 4, 5] = np.nan                    # NaN lightness -> EPS
        k = (0, 1, 50)[trial % 3]
        comp = np.zeros((k, 6))
        comp[:, :4] = rng.random((k, 4)) * 0.999
        comp[:, 4] = rng.integers(0, 3, k)
        comp[:, 5] = rng.random(k) if trial % 5 else 0.0   # all-zero weights -> 0.0
        px = W.to_pixels(comp, 9, 13)
        if k:
            px[0, :4] = (3, 2, 5, 4)
        with np.errstate(all="ignore"):
            assert W.whdr(refl, px, 0.1) == _whdr_by_definition(refl, px, 0.1), trial


def test_load_judgements_reads_iiw_json(tmp_path):
    doc = {"intrinsic_points": [{"id": 7, "x": 0.25, "y": 0.5, "opaque": True},
                                {"id": 9, "x": 0.75, "y": 0.125, "opaque": True},
                                {"id": 11, "x": 0.0, "y": 0.99, "opaque": False}],
           "intrinsic_comparisons": [
               {"point1": 7, "point2": 9, "darker": "1", "darker_score": 0.5},
               {"point1": 9, "point2": 11, "darker": "E", "darker_score": 1.25},
               {"point1": 11, "point2": 7, "darker": "2", "darker_score": 0.0625}]}
    path = tmp_path / "123.json"
    path.write_text(json.dumps(doc))
    comp = W.load_judgements(str(path))
    assert comp.dtype == np.float64
    assert np.array_equal(comp, np.array([[0.25, 0.5, 0.75, 0.125, 1, 0.5],
                                          [0.75, 0.125, 0.0, 0.99, 0, 1.25],
                                          [0.0, 0.99, 0.25, 0.5, 2, 0.0625]]))
    px = W.to_pixels(comp, 100, 200)
    assert np.array_equal(px[:, :4], [[50, 50, 150, 12], [150, 12, 0, 99], [0, 99, 50, 50]])
    empty = tmp_path / "e.json"
    empty.write_text(json.dumps({"intrinsic_points": [], "intrinsic_comparisons": []}))
    assert W.load_judgements(str(empty)).shape == (0, 6)


@pytest.mark.gpu
def test_device_batch_matches_reference_and_host(built):
    import torch
    d = np.load(os.path.join(G, "whdr.npz"))
    for tag in TAGS:                       # one image per launch: the reference's numbers
        refl = d[tag + "_refl"]
        px = d[tag + "_pixels"]
        for dl, want in zip(DELTAS, d[tag + "_whdr"]):
            got = W.whdr_batch(torch.from_numpy(refl[None]).cuda(), [px], dl)
            assert got.shape == (1,) and got[0] == want, (tag, dl)
    rng = np.random.default_rng(5)
    for c in (1, 3):                       # ragged batch against the host mirror
        n, h, w = 9, 37, 51
        refl = (rng.random((n, c, h, w)) ** 3).astype(np.float32)
        comps = []
        for i in range(n):
            k = int(rng.integers(0, 400)) if i != 4 else 0
            comp = np.zeros((k, 6))
            comp[:, 0:4] = rng.random((k, 4)) * 0.999
            comp[:, 4] = rng.integers(0, 3, k)
            comp[:, 5] = rng.random(k)
            comps.append(W.to_pixels(comp, h, w))
        got = W.whdr_batch(torch.from_numpy(refl).cuda(), comps, 0.1)
        want = np.array([W.whdr(refl[i], comps[i], 0.1) for i in range(n)])
        assert np.array_equal(got, want), c
    g3 = W.whdr_batch(torch.from_numpy(refl[:, 0]).cuda().contiguous(), comps, 0.1)   # [N,H,W]
    assert g3.shape == (9,)
    with pytest.raises(IndexError):
        W.whdr_batch(torch.zeros((1, 1, 4, 4), device="cuda"), [np.array([[4, 0, 1, 1, 1, 1.0]])])


def _edge_case_batch(rng, c, n, h, w):
    """The generator of test_host_whdr_edge_cases_match_the_definition as a batch (0 and NaN
    lightness floored at EPS, 0 / 1 / 50 / 300 comparisons, all-zero weights), plus pairs whose
    float32 ratio is exactly float32(1 + delta) for delta 0.1 and 0 - "about equal", not darker."""
    refl = (rng.random((n, c, h, w)) ** 3).astype(np.float32)
    refl[:, :, 2, 3] = 0
    refl[:, :, 4, 5] = np.nan
    # row 6: (6, 0) lightness 0.5, (6, 1) its float32(1.1) multiple, (6, 2) equal to (6, 0)
    refl[:, :, 6, 0] = 0.5
    refl[:, :, 6, 1] = np.float32(0.5) * np.float32(1.1)
    refl[:, :, 6, 2] = 0.5
    comps = []
    for i in range(n):
        k = (0, 1, 50, 300)[i % 4]
        comp = np.zeros((k, 6))
        comp[:, :4] = rng.random((k, 4)) * 0.999
        comp[:, 4] = rng.integers(0, 3, k)
        comp[:, 5] = rng.random(k) if i % 5 else 0.0
        px = W.to_pixels(comp, h, w)
        if k:
            px[0, :4] = (3, 2, 5, 4)
        if k >= 50:
            exact = np.array([(0, 6, 1, 6), (1, 6, 0, 6), (0, 6, 2, 6), (2, 6, 0, 6), (0, 6, 0, 6)])
            px[1:6, :4] = exact
            px[6:11, :4] = exact
            px[1:11, 4] = rng.integers(0, 3, 10)
        comps.append(px)
    return refl, comps


@pytest.mark.gpu
@pytest.mark.parametrize("c", [1, 3])
def test_device_batch_edge_cases_match_host_and_definition(built, c):
    """Device WHDR on the edge cases the host mirror is held to, with more than 64 comparisons per
    image (the wave loop runs several times): the same float64 value as W.whdr and as the
    definition spelled out, bit for bit, for delta 0.1 and 0."""
    import torch
    rng = np.random.default_rng(17 + c)
    n, h, w = 12, 9, 13
    refl, comps = _edge_case_batch(rng, c, n, h, w)
    light = refl[0, :, 6, :3].mean(axis=0) if c == 3 else refl[0, 0, 6, :3]
    assert light[1] / light[0] == np.float32(1 + 0.1) and light[2] / light[0] == np.float32(1 + 0.0)
    for dl in (0.1, 0.0):
        got = W.whdr_batch(torch.from_numpy(refl).cuda(), comps, dl)
        assert got.shape == (n,)
        for i in range(n):
            with np.errstate(all="ignore"):
                host = W.whdr(refl[i], comps[i], dl)
                spelled = _whdr_by_definition(refl[i], comps[i], dl)
            assert got[i] == host == spelled, (c, dl, i, got[i], host, spelled)


def test_to_pixels_keeps_float32_products():
    """Coordinates of a float32 blob are multiplied in float32 (whdr_layer.py:248-249 multiplies
    the array by a Python int): k / w as float32 times w rounds back to k, where the float64
    product of the same float32 value is just below k and truncates to k - 1."""
    h, w = 333, 500
    ks = np.arange(w, dtype=np.float32)
    js = np.arange(h, dtype=np.float32)
    n = max(h, w)
    comp = np.zeros((n, 6), dtype=np.float32)
    comp[:, 0] = np.resize(ks / np.float32(w), n)
    comp[:, 2] = np.resize(ks[::-1] / np.float32(w), n)
    comp[:, 1] = np.resize(js / np.float32(h), n)
    comp[:, 3] = np.resize(js[::-1] / np.float32(h), n)
    px = W.to_pixels(comp, h, w)
    assert px.dtype == np.float32
    want = comp.copy()                       # the reference's two statements, spelled out
    want[:, [0, 2]] = (want[:, [0, 2]] * w).astype(int)
    want[:, [1, 3]] = (want[:, [1, 3]] * h).astype(int)
    assert np.array_equal(px, want)
    wrong = np.trunc(comp[:, :4].astype(np.float64) * np.array([w, h, w, h]))
    assert (wrong != px[:, :4]).any()        # the float64 product does land elsewhere
    # float64 judgements (load_judgements) are untouched by the change
    c64 = comp.astype(np.float64)
    p64 = W.to_pixels(c64, h, w)
    assert p64.dtype == np.float64
    assert np.array_equal(p64[:, :4], np.trunc(c64[:, :4] * np.array([w, h, w, h])))
