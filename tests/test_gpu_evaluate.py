"""Scoring on the device (csrc/postprocess.hip: fmri_seg_counts_u8, fmri_surface_u8, fmri_masked_stats_f64, fmri_masked_compact_f64; their
front-ends in fmri_hip.ops; fetal_net.evaluate) against the scipy form of medpy.metric.binary's hd / hd95 / assd written out below.

Tolerances (u = 2^-53)
  borders, counts: identical (integer work).
  distances: identical at unit spacing, rtol 1e-15 with zeros in the same places otherwise - the bound tests/test_gpu_distance.py derives
    for the distance field (7u).  The device returns them in no particular order, so both sides are sorted: sorting a vector perturbed
    elementwise by <= eps moves every sorted entry by <= eps.
  hd: a maximum of those distances - identical at unit spacing, rtol 1e-15 otherwise.
  hd95: identical at unit spacing (the select is exact, the lerp is numpy's own); rtol 2e-15 otherwise: the two order statistics carry the
    7u, the result lies between them and all are non-negative, so the input error does not amplify; the lerp adds two roundings.
  assd: rtol 1e-15 + 2 n u with n the larger surface count: any two summation orders of n non-negative fp64 terms are each within
    (n - 1) u of the true sum.  Two device runs are bit-identical (the reduction order is fixed).
"""
import functools
import math

import numpy as np
import pytest
import scipy.ndimage as ndi
import torch

pytestmark = pytest.mark.gpu

REF = (0.4, 0.4, 3.0)                       # the reference's voxel spacing
SKEW = (0.7, 1.3, 2.1)
SPACINGS = [None, REF, SKEW]
SWEEP = 2048 * 256                           # voxels one sweep of the capped grid covers (EV_GRID x EV_THREADS in postprocess.hip)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the GPU box"
    from fmri_hip import ops as o
    return o


def _ellipsoid(shape, centre, radii):
    g = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    return sum(((a - c) / float(r)) ** 2 for a, c, r in zip(g, centre, radii)) < 1


def _field(shape, seed, sigma, quantile):
    f = ndi.gaussian_filter(np.random.RandomState(seed).randn(*shape), sigma)
    return f > np.quantile(f, quantile)


@functools.lru_cache(maxsize=None)
def masks(name):
    if name == "ellipsoids":                 # B touches the z = 19 face
        a, b = _ellipsoid((40, 48, 20), (20, 22, 9), (12, 15, 6)), _ellipsoid((40, 48, 20), (23, 20, 11), (10, 16, 9))
    elif name == "fields":                   # odd extents, several components, holes
        a, b = _field((17, 9, 33), 3, 1.5, 0.6), _field((17, 9, 33), 4, 1.5, 0.55)
    elif name == "line":
        a, b = np.zeros((1, 1, 40), bool), np.zeros((1, 1, 40), bool)
        a[0, 0, 3:20] = True
        b[0, 0, 10:30] = True
        b[0, 0, 35] = True
    elif name == "slab":
        a, b = _field((12, 1, 21), 5, 1.0, 0.5), _field((12, 1, 21), 6, 1.0, 0.5)
    elif name == "full":                     # a volume of ones: its surface is the six faces
        a, b = np.ones((8, 7, 6), bool), np.zeros((8, 7, 6), bool)
        b[2:7, 1:5, 2:6] = True
    elif name == "sweep":                    # more voxels than one sweep of the grid: the grid-stride loops
        shape = (96, 96, 64)
        assert np.prod(shape) > SWEEP
        a, b = _ellipsoid(shape, (48, 50, 30), (30, 35, 20)), _ellipsoid(shape, (52, 46, 34), (33, 30, 22))
    a, b = a.astype(np.uint8), b.astype(np.uint8)
    assert a.any() and b.any() and (a != b).any()
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


SMALL = ["ellipsoids", "fields", "line", "slab", "full"]
CASES = [(n, s, c) for n in SMALL for s in SPACINGS for c in (1, 2, 3)] + [("sweep", REF, 1), ("sweep", None, 3)]
CASE_IDS = ["%s-%s-c%d" % (n, "unit" if s is None else "x".join(str(v) for v in s), c) for n, s, c in CASES]


def border(mask, connectivity):
    m = mask.astype(bool)
    return m ^ ndi.binary_erosion(m, structure=ndi.generate_binary_structure(3, connectivity), iterations=1)


@functools.lru_cache(maxsize=None)
def oracle(name, spacing, connectivity):
    """medpy.metric.binary restated with scipy: the two distance sets, hd, hd95, assd"""
    a, b = masks(name)
    ba, bb = border(a, connectivity), border(b, connectivity)
    d_ab = ndi.distance_transform_edt(~bb, sampling=spacing)[ba]
    d_ba = ndi.distance_transform_edt(~ba, sampling=spacing)[bb]
    for d in (d_ab, d_ba):
        d.setflags(write=False)
    return {"d_ab": d_ab, "d_ba": d_ba, "hd": max(d_ab.max(), d_ba.max()), "hd95": np.percentile(np.hstack((d_ab, d_ba)), 95),
            "assd": np.mean((d_ab.mean(), d_ba.mean())), "n": (int(ba.sum()), int(bb.sum()))}


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def unit(spacing):
    return spacing is None


def check_metrics(got, want, spacing, what):
    n = max(want["n"])
    print("%s: hd %.17g / %.17g  hd95 %.17g / %.17g  assd %.17g / %.17g  (n = %s)" % (
        what, got["hd"], want["hd"], got["hd95"], want["hd95"], got["assd"], want["assd"], want["n"]))
    assert want["hd"] > 0 and want["hd95"] > 0 and want["assd"] > 0, "a trivial case checks nothing"
    if unit(spacing):
        assert got["hd"] == want["hd"], what
        assert got["hd95"] == want["hd95"], what
    else:
        np.testing.assert_allclose(got["hd"], want["hd"], rtol=1e-15, atol=0, err_msg=what)
        np.testing.assert_allclose(got["hd95"], want["hd95"], rtol=2e-15, atol=0, err_msg=what)
    np.testing.assert_allclose(got["assd"], want["assd"], rtol=1e-15 + 2 * n * 2.0 ** -53, atol=0, err_msg=what)


def test_the_ellipsoids_are_the_stated_ones():
    assert oracle("ellipsoids", None, 1)["n"] == (1226, 1334)


@pytest.mark.parametrize("connectivity", [1, 2, 3])
@pytest.mark.parametrize("name", SMALL + ["sweep"])
def test_surface_is_scipys_border(ops, name, connectivity):
    for m in masks(name):
        inv, count = ops.surface_u8(dev(m), connectivity)
        want = border(m, connectivity)
        assert inv.dtype == torch.uint8 and tuple(inv.shape) == m.shape
        np.testing.assert_array_equal(1 - inv.cpu().numpy(), want.astype(np.uint8))
        assert count == int(want.sum())
    if name == "full":
        a = masks(name)[0]
        inner = np.zeros(a.shape, bool)
        inner[1:-1, 1:-1, 1:-1] = True
        np.testing.assert_array_equal(border(a, 1), ~inner)                  # scipy agrees: the six faces and nothing else
        np.testing.assert_array_equal(1 - ops.surface_u8(dev(a), 1)[0].cpu().numpy(), (~inner).astype(np.uint8))


def test_a_cube_of_27_has_26_surface_voxels(ops):
    inside = np.zeros((5, 5, 5), np.uint8)
    inside[1:4, 1:4, 1:4] = 1
    for connectivity in (1, 2, 3):
        assert ops.surface_u8(dev(inside), connectivity)[1] == 26
        assert ops.surface_u8(dev(np.ones((3, 3, 3), np.uint8)), connectivity)[1] == 26
    # any nonzero byte is foreground
    assert ops.surface_u8(dev(inside * 255), 1)[1] == 26
    for bad in (0, 4, 1.5):
        with pytest.raises(ValueError):
            ops.surface_u8(dev(inside), bad)


@pytest.mark.parametrize("name", SMALL + ["sweep"])
def test_seg_counts_are_numpys(ops, name):
    a, b = masks(name)
    want = (int(a.astype(bool).sum()), int(b.astype(bool).sum()), int((a.astype(bool) & b.astype(bool)).sum()))
    assert ops.seg_counts_u8(dev(a), dev(b)) == want
    assert ops.seg_counts_u8(dev(a * 7), dev(b * 128)) == want                # nonzero, not one
    # volumes that do not start on an 8-byte boundary take the byte loop
    flat_a, flat_b = torch.zeros(a.size + 8, dtype=torch.uint8, device="cuda"), torch.zeros(b.size + 8, dtype=torch.uint8, device="cuda")
    flat_a[3:3 + a.size] = dev(a).reshape(-1)
    flat_b[8:8 + b.size] = dev(b).reshape(-1)
    assert ops.seg_counts_u8(flat_a[3:3 + a.size].view(a.shape), flat_b[8:8 + b.size].view(b.shape)) == want


@pytest.mark.parametrize("name,spacing,connectivity", CASES, ids=CASE_IDS)
def test_surface_distances(ops, name, spacing, connectivity):
    a, b = masks(name)
    want = oracle(name, spacing, connectivity)
    for got, key in ((ops.surface_distances_f64(dev(a), dev(b), spacing, connectivity), "d_ab"),
                     (ops.surface_distances_f64(dev(b), dev(a), spacing, connectivity), "d_ba")):
        assert got.dtype == torch.float64 and got.dim() == 1
        g, w = np.sort(got.cpu().numpy()), np.sort(want[key])
        assert g.shape == w.shape
        if unit(spacing):
            np.testing.assert_array_equal(g, w)
        else:
            np.testing.assert_array_equal(g == 0, w == 0)
            np.testing.assert_allclose(g, w, rtol=1e-15, atol=0)


@pytest.mark.parametrize("name,spacing,connectivity", CASES, ids=CASE_IDS)
def test_surface_metrics(ops, name, spacing, connectivity):
    a, b = masks(name)
    want = oracle(name, spacing, connectivity)
    da, db = dev(a), dev(b)
    got = ops.surface_metrics_u8(da, db, spacing, connectivity)
    assert got["n_surface"] == want["n"]
    check_metrics(got, want, spacing, "surface_metrics_u8 %s" % name)
    again = ops.surface_metrics_u8(da, db, spacing, connectivity)
    assert again == got, "two runs of one input differ: the reduction is not in a fixed order"
    swapped = ops.surface_metrics_u8(db, da, spacing, connectivity)         # symmetric by definition
    assert swapped["hd"] == got["hd"] and swapped["hd95"] == got["hd95"] and swapped["n_surface"] == got["n_surface"][::-1]


def test_other_percentiles(ops):
    a, b = masks("ellipsoids")
    want = oracle("ellipsoids", None, 1)
    both = np.hstack((want["d_ab"], want["d_ba"]))
    for q in (0, 50, 99.5, 100):
        assert ops.surface_metrics_u8(dev(a), dev(b), None, 1, percentile=q)["hd95"] == np.percentile(both, q)


def test_empty_masks_give_nan_without_a_distance_transform(ops, monkeypatch):
    from fetal_net import evaluate as E

    def no_edt(*args, **kwargs):
        raise AssertionError("the distance transform ran on a volume without a surface")
    monkeypatch.setattr(ops, "_edt", no_edt)
    some = masks("fields")[0]
    empty = np.zeros_like(some)
    for a, b, n in ((empty, some, (0, None)), (some, empty, (None, 0)), (empty, empty, (0, 0))):
        got = ops.surface_metrics_u8(dev(a), dev(b), REF, 1)
        assert math.isnan(got["hd"]) and math.isnan(got["hd95"]) and math.isnan(got["assd"])
        assert all(w is None or g == w for g, w in zip(got["n_surface"], n))
        row, host = E.evaluate_case(a, b, spacing=REF, device=True), E.evaluate_case(a, b, spacing=REF, device=False)
        assert list(row) == list(host)
        for k in row:
            np.testing.assert_array_equal(row[k], host[k], err_msg=k)       # NaN equals NaN here
    assert ops.surface_distances_f64(dev(empty), dev(some)).numel() == 0
    d = ops.surface_distances_f64(dev(some), dev(empty))
    assert d.numel() == int(border(some, 1).sum()) and bool(torch.isinf(d).all())


@pytest.mark.parametrize("name,spacing,connectivity", CASES, ids=CASE_IDS)
def test_evaluate_case_device_against_host(ops, name, spacing, connectivity):
    from fetal_net import evaluate as E
    a, b = masks(name)
    got = E.evaluate_case(a, b, spacing=spacing, connectivity=connectivity, device=True)
    host = E.evaluate_case(a, b, spacing=spacing, connectivity=connectivity, device=False)
    assert list(got) == list(host) == list(E.KEYS)
    for k in ("dice", "vod", "volume_truth", "volume_prediction", "volume_difference", "sensitivity", "precision"):
        assert got[k] == host[k], k                                           # ratios of the same integers
    want = oracle(name, spacing, connectivity)
    check_metrics(got, dict(host, n=want["n"]), spacing, "evaluate_case %s" % name)
    check_metrics(got, want, spacing, "evaluate_case %s vs the oracle" % name)


def test_evaluate_cases_through_the_device(ops, tmp_path):
    from fetal_net import evaluate as E
    from test_host_evaluate import write_cases
    cases = write_cases(str(tmp_path))
    rows = E.evaluate_cases(str(tmp_path), out_csv=str(tmp_path / "scores.csv"), device=True)
    host = E.evaluate_cases(str(tmp_path), device=False)
    assert list(rows) == list(host) == sorted(cases)
    for name, (t, p, spacing) in cases.items():
        for k in ("dice", "vod", "volume_truth", "volume_prediction", "volume_difference", "sensitivity", "precision"):
            assert rows[name][k] == host[name][k], (name, k)
        n = (int(border(t, 1).sum()), int(border(p, 1).sum()))
        check_metrics(rows[name], dict(host[name], n=n), None if spacing == (1.0, 1.0, 1.0) else spacing, "evaluate_cases %s" % name)
