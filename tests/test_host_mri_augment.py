"""The fetal acquisition augmenters on the host (fetal_net/augment.py): the draws of slice_motion / gamma / bias_field / slice_intensity and the
float64 forms of the four effects.  CPU only."""
import random

import numpy as np
import pytest

from fetal_net.augment import (apply_slice_motion, bias_field, bias_monomials, draw_augment_parameters, draw_mri_parameters, gamma_augment,
                               slice_gain)

ALL = {"slice_motion": {"prob": 1, "slice_prob": 0.5, "rotate": 3.0, "translate": 1.5}, "gamma": {"prob": 1, "range": (0.6, 1.8)},
       "bias_field": {"prob": 1, "order": 3, "coefficient": 0.4}, "slice_intensity": {"prob": 1, "slice_prob": 0.5, "sigma": 0.2}}
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def test_draws_have_the_documented_shapes_and_bounds():
    seen_low = seen_high = False
    for seed in range(20):
        r = draw_mri_parameters(ALL, (9, 8, 6), np.random.RandomState(seed))
        tab, moved = r["slice_table"], r["slice_moved"]
        assert tab.shape == (6, 6) and tab.dtype == np.float64 and moved.shape == (6,) and moved.dtype == bool
        assert all(tuple(row) == IDENTITY for row in tab[~moved])                         # exact, not cos(0) arithmetic
        for row in tab[moved]:
            assert tuple(row) != IDENTITY
            rot = row[[0, 1, 3, 4]].reshape(2, 2)
            np.testing.assert_allclose(rot.dot(rot.T), np.eye(2), atol=1e-12)            # a rotation ...
            assert row[0] == row[4] and row[1] == -row[3] and np.linalg.det(rot) > 0
            c = np.array([4.0, 3.5])                                                      # ... about the in-plane centre, then the shift
            assert np.abs(rot.dot(c) + row[[2, 5]] - c).max() < 6 * 1.5
        g = r["gamma"]
        assert isinstance(g, float) and 0.6 <= g <= 1.8
        seen_low, seen_high = seen_low or g < 1, seen_high or g > 1
        assert r["bias_coef"].shape == (20,) and r["bias_coef"].dtype == np.float64 and np.abs(r["bias_coef"]).max() <= 0.4
        gain = r["slice_gain"]
        assert gain.shape == (6,) and gain.dtype == np.float64 and (gain > 0).all()
    assert seen_low and seen_high                                                         # both branches of the gamma draw


def test_gamma_default_range_and_term_counts():
    assert [len(bias_monomials(o)) for o in (1, 2, 3)] == [4, 10, 20]
    assert bias_monomials(1) == [(0, 0, 0), (0, 0, 1), (0, 1, 0), (1, 0, 0)]              # lexicographic (a, b, c)
    assert bias_monomials(3) == sorted(bias_monomials(3)) and all(sum(t) <= 3 for t in bias_monomials(3))
    for order, n in ((1, 4), (2, 10), (3, 20)):
        r = draw_mri_parameters({"bias_field": {"prob": 1, "order": order}}, (4, 4, 3), np.random.RandomState(order))
        assert r["bias_coef"].shape == (n,) and np.abs(r["bias_coef"]).max() <= 0.5       # default coefficient
    r = draw_mri_parameters({"bias_field": {"prob": 1}}, (4, 4, 3), np.random.RandomState(0))
    assert r["bias_coef"].shape == (20,)                                                  # default order 3
    gs = [draw_mri_parameters({"gamma": {"prob": 1}}, (4, 4, 3), np.random.RandomState(s))["gamma"] for s in range(50)]
    assert 0.7 <= min(gs) < 1 < max(gs) <= 1.5
    with pytest.raises(ValueError):
        draw_mri_parameters({"bias_field": {"prob": 1, "order": 4}}, (4, 4, 3), np.random.RandomState(0))


def test_draw_order_is_the_documented_one():
    """slice_motion, gamma, bias_field, slice_intensity; decision first, parameters in the written order"""
    r = draw_mri_parameters(ALL, (9, 8, 6), np.random.RandomState(11))
    rs = np.random.RandomState(11)
    assert 1 > rs.random_sample()
    moved = rs.random_sample(6) < 0.5
    theta = np.deg2rad(rs.normal(0, 3.0, 6))
    t = rs.normal(0, 1.5, (6, 2))
    assert np.array_equal(moved, r["slice_moved"])
    for k in np.flatnonzero(moved):
        c = np.array([4.0, 3.5])
        R = np.array([[np.cos(theta[k]), -np.sin(theta[k])], [np.sin(theta[k]), np.cos(theta[k])]])
        for ij in ((0.0, 0.0), (8.0, 7.0), (2.0, 5.0)):
            want = R.dot(np.array(ij) - c) + c + t[k]
            row = r["slice_table"][k]
            got = np.array([row[0] * ij[0] + row[1] * ij[1] + row[2], row[3] * ij[0] + row[4] * ij[1] + row[5]])
            np.testing.assert_allclose(got, want, atol=1e-12)
    rs.random_sample()
    g = rs.uniform(0.6, 1.0) if rs.random_sample() < 0.5 else rs.uniform(1.0, 1.8)
    assert g == r["gamma"]
    rs.random_sample()
    assert np.array_equal(rs.uniform(-0.4, 0.4, 20), r["bias_coef"])
    rs.random_sample()
    chosen = rs.random_sample(6) < 0.5
    assert np.array_equal(np.where(chosen, np.exp(rs.normal(0, 0.2, 6)), 1.0), r["slice_gain"])
    assert (r["slice_gain"][~chosen] == 1.0).all()


def test_same_seed_same_arrays_and_prob_zero_draws_only_the_decision():
    a = draw_mri_parameters(ALL, (9, 8, 6), np.random.RandomState(5))
    b = draw_mri_parameters(ALL, (9, 8, 6), np.random.RandomState(5))
    c = draw_mri_parameters(ALL, (9, 8, 6), np.random.RandomState(6))
    for k in ("slice_table", "slice_moved", "bias_coef", "slice_gain"):
        assert np.array_equal(a[k], b[k])
    assert a["gamma"] == b["gamma"] and not np.array_equal(a["slice_table"], c["slice_table"])
    off = {k: dict(v, prob=0) for k, v in ALL.items()}
    rs, ref = np.random.RandomState(9), np.random.RandomState(9)
    r = draw_mri_parameters(off, (9, 8, 6), rs)
    assert r["slice_table"] is None and r["gamma"] == 0.0 and r["bias_coef"] is None and r["slice_gain"] is None
    ref.random_sample(4)                                                                  # four decisions, nothing else
    assert rs.random_sample() == ref.random_sample()
    rs, ref = np.random.RandomState(9), np.random.RandomState(9)
    assert draw_mri_parameters({"flip": [0, 0, 0]}, (9, 8, 6), rs)["slice_table"] is None  # absent keys: no draw at all
    assert rs.random_sample() == ref.random_sample()


def test_the_new_draws_leave_the_global_streams_alone():
    base = {"flip": [0.5, 0.5, 0.5], "scale": [0.1, 0.1, 0.0], "rotate": [0, 0, 10], "translate": [2, 2, 1], "gaussian_noise": {"prob": 0.5, "sigma": 0.1}}
    states = []
    for aug, draw in ((base, False), (dict(base, **ALL), True)):
        np.random.seed(21)
        random.seed(21)
        p = draw_augment_parameters(aug, 3, -1.0, 4.0)
        if draw:
            draw_mri_parameters(aug, (9, 8, 6), np.random.RandomState(3))
        states.append((p, np.random.get_state(), random.getstate()))
    (p0, n0, r0), (p1, n1, r1) = states
    assert r0 == r1 and n0[0] == n1[0] and np.array_equal(n0[1], n1[1]) and n0[2:] == n1[2:]
    assert np.array_equal(p0["scale_factor"], p1["scale_factor"]) and np.array_equal(p0["translate_factor"], p1["translate_factor"])
    assert np.array_equal(p0["flip_axis"], p1["flip_axis"]) and p0["apply_gaussian_noise"] == p1["apply_gaussian_noise"]


def test_host_forms():
    rs = np.random.RandomState(2)
    x = np.maximum(rs.randn(7, 6, 5), -1.5).astype(np.float32)
    ident = np.tile(np.array(IDENTITY), (5, 1))
    for order in (0, 1):
        assert np.array_equal(apply_slice_motion(x, ident, order=order), x)               # bit for bit
    shift = ident.copy()
    shift[2] = (1.0, 0.0, 1.0, 0.0, 1.0, -2.0)                                            # slice 2 reads (i + 1, j - 2)
    moved = apply_slice_motion(x, shift, order=1, cval=-9.0)
    assert np.array_equal(moved[..., [0, 1, 3, 4]], x[..., [0, 1, 3, 4]])
    assert np.array_equal(moved[:6, 2:, 2], x[1:, :4, 2]) and (moved[6, :, 2] == -9.0).all() and (moved[:, :2, 2] == -9.0).all()
    assert np.array_equal(apply_slice_motion(x[..., 1:3], shift, order=0, cval=-9.0, z_off=1)[..., 1], moved[..., 2])     # z_off: row k + 1
    const = np.full((4, 3, 2), 2.5, dtype=np.float32)
    assert np.array_equal(gamma_augment(const, 1.4), const)
    g = gamma_augment(x, 1.4)
    assert g.min() == x.min() and abs(g.max() - x.max()) < 1e-12 and (g <= x + 1e-12).all() and (g < x - 1e-3).any()      # range kept, mid-tones down
    assert np.array_equal(bias_field(x, np.zeros(20), -1.5), x) and np.array_equal(slice_gain(x, np.ones(5), -1.5), x)
    gains = np.ones(5)
    gains[3] = 2.0
    out = slice_gain(x, gains, -1.5)
    assert np.array_equal(out[..., 3] + 1.5, 2 * (x[..., 3].astype(np.float64) + 1.5)) and np.array_equal(out[..., [0, 1, 2, 4]], x[..., [0, 1, 2, 4]])
    coef = np.zeros(4)
    coef[3] = 0.3                                                                         # P = 0.3 x: e^-0.3 at i = 0 ... e^+0.3 at the far face
    b = bias_field(x, coef, -1.5)
    np.testing.assert_allclose(b[0] + 1.5, (x[0].astype(np.float64) + 1.5) * np.exp(-0.3), rtol=1e-12)
    np.testing.assert_allclose(b[6] + 1.5, (x[6].astype(np.float64) + 1.5) * np.exp(0.3), rtol=1e-12)
    np.testing.assert_allclose(b[3], x[3], rtol=1e-12)
    assert (bias_field(np.full((4, 4, 3), -1.5), rs.rand(20), -1.5) == -1.5).all()        # the background stays the background
    assert np.array_equal(bias_field(x[:, :, :1], np.array([0.0, 5.0, 0, 0]), -1.5), x[:, :, :1])     # an axis of length 1 sits at 0: z term off
