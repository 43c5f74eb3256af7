"""Gaussian-importance blending of the sliding-window tiles, host side (no GPU): the weight tables, the refusals, the four entry points in
header, binding table and library, and the host route of `patch_wise_prediction(blend="gaussian")` against the float64 restatement of
tests/blend_restatement.py, driven by deterministic fake models behind the reference's duck type."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import blend_restatement as R
from conftest import ROOT

NEW = ("fmri_tile_scatter_weighted", "fmri_tile_finalize_weighted", "fmri_tile_finalize_flip_weighted", "fmri_tile_finalize_labels_weighted")


# ---------------------------------------------------------------------------------------------------------------------------- tables
@pytest.mark.parametrize("p", [1, 2, 3, 16, 128, 129])
def test_tables_are_symmetric_peak_at_the_centre_and_stay_above_exp_minus_8(p):
    from fetal_net.prediction import gaussian_tile_tables
    g, h, one = gaussian_tile_tables((p, p, 1))
    assert g.dtype == np.float32 and g.shape == (p,) and g.tobytes() == h.tobytes()
    assert one.tobytes() == np.ones(1, dtype=np.float32).tobytes()
    assert g.tobytes() == R.tables((p,))[0].tobytes()                      # the header's formula, restated
    np.testing.assert_array_equal(g, g[::-1])
    assert float(g.min()) > math.exp(-8.0) and float(g.max()) <= 1.0
    if p % 2:
        assert g[p // 2] == 1.0 and int((g == g.max()).sum()) == 1          # one centre entry
    else:
        assert g[p // 2 - 1] == g[p // 2] == g.max() and int((g == g.max()).sum()) == 2 and g.max() < 1.0 + 1e-12
    assert np.all(np.diff(g[:(p + 1) // 2].astype(np.float64)) > 0)        # rises to the centre
    if p == 1:
        assert g.tolist() == [1.0]


def test_sigma_scale_changes_the_tables_and_is_checked():
    from fetal_net.prediction import gaussian_tile_tables
    wide, narrow = gaussian_tile_tables((16,), 0.25)[0], gaussian_tile_tables((16,), 0.125)[0]
    assert wide[0] > narrow[0] and wide.tobytes() == R.tables((16,), 0.25)[0].tobytes()
    for bad in (0, -0.125, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            gaussian_tile_tables((16,), bad)


# ---------------------------------------------------------------------------------------------------------------------- fake models
def _squash(x):
    """x / (1 + |x|): plain IEEE operations, the same bits however the tiles are batched"""
    return x / (1.0 + np.abs(x))


class Fake3d(object):
    """the reference's duck type, 3-D: (B, 1, px, py, pz) -> (B, C, px, py, pz).  positional: the output depends on the position inside the
    tile as well as on the tile's content, so the weights matter"""

    def __init__(self, patch, channels=1, positional=True):
        self.output_shape = (None, channels) + tuple(patch)
        n = int(np.prod(patch))
        self.ramp = np.linspace(0.5, 1.5, n).reshape(patch) if positional else np.ones(patch)
        self.channels = channels

    def predict(self, x):
        x = np.asarray(x, dtype=np.float64)[:, 0]
        return np.stack([_squash(x * self.ramp * (c + 1)) + 0.125 * c for c in range(self.channels)], axis=1)


class Fake2d(object):
    """2-D layout: (B, px, py, slices) -> (B, px, py, C); the output tile of the tiler is (px, py, 1)"""
    _input_layout = "channels_last_2d"

    def __init__(self, patch, channels=1):
        self.output_shape = (None, patch[0], patch[1], channels)
        self.ramp = np.linspace(0.5, 1.5, patch[0] * patch[1]).reshape(patch[0], patch[1])
        self.channels = channels

    def predict(self, x):
        x = np.asarray(x, dtype=np.float64)
        mid = x[..., x.shape[-1] // 2] + 0.25 * x.sum(axis=-1)
        return np.stack([_squash(mid * self.ramp * (c + 1)) for c in range(self.channels)], axis=-1)


class Constant(object):
    def __init__(self, patch, value):
        self.output_shape = (None, 1) + tuple(patch)
        self.value = value

    def predict(self, x):
        return np.full((np.asarray(x).shape[0],) + tuple(self.output_shape[1:]), self.value)


class RimError(object):
    """the true value (the tile's own content) plus an error proportional to the normalised distance from the tile centre,
    r = sqrt(sum_a ((i_a - (p_a - 1) / 2) / p_a)^2): a zero-padded network's rim, in caricature"""

    def __init__(self, patch, slope=0.5):
        self.output_shape = (None, 1) + tuple(patch)
        g = np.indices(patch).astype(np.float64)
        self.err = slope * np.sqrt(sum(((g[a] - (patch[a] - 1) / 2.0) / patch[a]) ** 2 for a in range(3)))

    def predict(self, x):
        return np.asarray(x, dtype=np.float64) + self.err


def _tiles_of(model, data, patch, overlap):
    """the tiler's geometry (unchanged package code) and the model's output for every tile, one tile per predict call:
    -> (preds (n, ox, oy, oz, C), corners, accumulator shape, pad_for_fit)"""
    from fetal_net import prediction as P
    is3d, pad0, fit, data_0, indices, data_shape = P._geometry(model, data, patch, overlap)
    preds = []
    for x, y, z in indices:
        tile = data_0[x:x + patch[0], y:y + patch[1], z:z + patch[2]]
        if is3d:
            preds.append(np.moveaxis(model.predict(tile[None, None])[0], 0, -1))
        else:
            preds.append(model.predict(tile[None])[0][:, :, None, :])
    return np.asarray(preds), np.asarray(indices), tuple(int(s) for s in data_shape), fit


def _want(model, data, patch, overlap, sigma=0.125):
    from fetal_net.prediction import _unpad
    preds, corners, ashape, fit = _tiles_of(model, data, patch, overlap)
    out, n_cover = R.blend_tiles(preds, corners, ashape, sigma)
    assert n_cover <= 64
    return _unpad(out, fit)


CASES = [("3d", (8, 8, 4), (11, 13, 6), 1), ("3d-single-tile", (8, 8, 4), (8, 8, 4), 1), ("3d-three-channels", (8, 8, 4), (11, 13, 6), 3),
         ("3d-content-only", (8, 8, 4), (11, 13, 6), 1), ("2d", (8, 8, 3), (11, 13, 5), 1), ("2d-three-channels", (8, 8, 3), (11, 13, 5), 3)]


def _case(name, patch, channels):
    if name.startswith("2d"):
        return Fake2d(patch, channels)
    return Fake3d(patch, channels, positional=name != "3d-content-only")


@pytest.mark.parametrize("overlap", [0, 0.5])
@pytest.mark.parametrize("name,patch,shape,channels", CASES)
def test_host_route_equals_the_restatement(name, patch, shape, channels, overlap):
    """both sides are float64 sums of the same terms, possibly in another order: n_cover * 2^-53 with n_cover <= 64 lies below 1e-13"""
    from fetal_net import prediction as P
    model = _case(name, patch, channels)
    data = np.random.RandomState(len(name) + int(10 * overlap)).randn(1, *shape)
    got = P.patch_wise_prediction(model, data, patch, overlap_factor=overlap, blend="gaussian")
    want = _want(model, data, patch, overlap)
    assert got.shape == tuple(shape) + (channels,) and got.dtype == np.float64
    np.testing.assert_allclose(got, want, rtol=1e-13, atol=0)
    if name.startswith("2d"):
        assert _tiles_of(model, data, patch, overlap)[0].shape[1:4] == (patch[0], patch[1], 1)       # weights in-plane only
    # blend=None is the call without the keyword, bit for bit
    plain = P.patch_wise_prediction(model, data, patch, overlap_factor=overlap)
    none = P.patch_wise_prediction(model, data, patch, overlap_factor=overlap, blend=None)
    assert plain.dtype == none.dtype and plain.tobytes() == none.tobytes()
    if overlap and name in ("3d", "2d", "3d-three-channels", "2d-three-channels") and max(shape) > max(patch):
        assert float(np.abs(got - plain).max()) > 1e-6        # positional model, overlapping tiles: the weights change the result
    # another sigma is another result, and the restatement's
    if overlap and name == "3d":
        wide = P.patch_wise_prediction(model, data, patch, overlap_factor=overlap, blend="gaussian", blend_sigma_scale=0.25)
        np.testing.assert_allclose(wide, _want(model, data, patch, overlap, 0.25), rtol=1e-13, atol=0)
        assert float(np.abs(wide - got).max()) > 1e-6


def test_refusals():
    from fetal_net import prediction as P
    from fetal_net.pipeline import Stage
    patch = (8, 8, 4)
    model = Fake3d(patch)
    data = np.zeros((1, 11, 13, 6))
    with pytest.raises(ValueError, match="blend"):
        P.patch_wise_prediction(model, data, patch, overlap_factor=0.5, blend="cosine")
    for sigma in (0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="blend_sigma_scale"):
            P.patch_wise_prediction(model, data, patch, overlap_factor=0.5, blend="gaussian", blend_sigma_scale=sigma)
    with pytest.raises(ValueError):
        P.patch_wise_prediction(model, data, patch, overlap_factor=0.5, blend_sigma_scale=0)
    with pytest.raises(ValueError, match="blend"):
        P.patch_wise_label_map(model, data, patch, blend="cosine")
    cfg = {"patch_shape": list(patch[:2]), "patch_depth": patch[2]}
    with pytest.raises(ValueError, match="blend"):
        P.predict_flips(data, model, 0.5, cfg, blend="cosine")
    with pytest.raises(ValueError, match="blend"):
        Stage(model, cfg, blend="cosine")
    with pytest.raises(TypeError):
        P.patch_wise_prediction(model, data, patch, 0.5, 5, False, None, None, None, "gaussian")        # keyword-only


def test_a_constant_model_stays_constant():
    """every tile predicts 0.25 everywhere: sum(w * 0.25) / sum(w) - the weights normalise"""
    from fetal_net import prediction as P
    patch = (8, 8, 4)
    got = P.patch_wise_prediction(Constant(patch, 0.25), np.random.RandomState(0).randn(1, 11, 13, 6), patch, overlap_factor=0.5,
                                  blend="gaussian")
    assert float(np.abs(got - 0.25).max()) <= 0.25 * 2.0 ** -52


def test_blending_lowers_the_error_of_a_model_that_is_worst_at_its_rim():
    """Why the feature exists.  The model returns the truth plus an error that grows with the distance r from the tile centre; the weight
    is a decreasing function of the same r, so at every voxel the blended mean is a mean of the same errors that leans towards the smaller
    ones (Chebyshev's sum inequality: strictly smaller unless all tiles on the voxel have one r).  A voxel that only ONE tile covers - the
    volume's own corners and faces always are such voxels, they lie on the rim of the first or last tile - has one prediction, which both
    rules return: there the two routes agree to the two roundings of (w * p) / w, and the maximum over the WHOLE volume is the same corner
    error on both routes.  The inequality is therefore asserted where a rule can act, over the voxels covered by more than one tile, with
    no threshold; the single-cover voxels are checked for agreement.  Geometry: tile 8 x 8 x 8 at overlap 0.5 steps by 5 (corners 0, 5, 8 in
    16), so no voxel lies on the rim of ALL the tiles that cover it (two tiles meeting at mirrored rim positions would share one r and leave the
    worst multiply-covered voxel as it is; patch 8 x 8 x 4 does that in z, where the step is 3)."""
    from fetal_net import prediction as P
    patch, shape = (8, 8, 8), (16, 16, 8)
    model = RimError(patch)
    data = np.random.RandomState(3).randn(1, *shape)
    uniform = P.patch_wise_prediction(model, data, patch, overlap_factor=0.5)[..., 0]
    blended = P.patch_wise_prediction(model, data, patch, overlap_factor=0.5, blend="gaussian")[..., 0]
    preds, corners, ashape, fit = _tiles_of(model, data, patch, 0.5)
    assert np.sum(fit) == 0
    cover = R.tile_scatter_weighted(preds.astype(np.float32), corners, R.tables(patch), np.zeros(ashape), np.zeros(ashape[:3]))[4]
    many = cover > 1
    assert many.any() and (~many).any()
    e_uniform, e_blended = np.abs(uniform - data[0]), np.abs(blended - data[0])
    print("max error where tiles overlap: uniform %.6f, blended %.6f; whole volume: uniform %.6f, blended %.6f" % (
        e_uniform[many].max(), e_blended[many].max(), e_uniform.max(), e_blended.max()))
    assert e_blended[many].max() < e_uniform[many].max()
    assert e_blended[many].mean() < e_uniform[many].mean()
    assert np.all(np.abs(blended[~many] - uniform[~many]) <= 2.0 ** -51 * np.abs(uniform[~many]))


@pytest.mark.parametrize("channels", [1, 3])
def test_label_map_on_the_host_route_is_the_label_rule_of_the_blended_means(channels):
    from fetal_net import prediction as P
    patch = (8, 8, 4)
    model = Fake3d(patch, channels)
    data = np.random.RandomState(8).randn(1, 11, 13, 6)
    labels = [3, 7, 9][:channels]
    means = P.patch_wise_prediction(model, data, patch, overlap_factor=0.5, blend="gaussian")
    got = P.patch_wise_label_map(model, data, patch, overlap_factor=0.5, threshold=0.1, labels=labels, blend="gaussian")
    want = np.asarray(P.prediction_to_image(np.moveaxis(means, -1, 0)[np.newaxis], label_map=True, threshold=0.1, labels=labels)).astype(np.uint8)
    assert got.dtype == np.uint8 and got.shape == (11, 13, 6) and got.tobytes() == want.tobytes()
    assert len(np.unique(got)) > 1
    # and the restatement's label rule agrees with prediction_to_image on these means
    ones = np.ones(means.shape[:3])
    np.testing.assert_array_equal(R.tile_finalize_labels_weighted(means, ones, 0.1, labels)[0], want)


def test_flips_and_stage_carry_the_keyword_on_the_host_route():
    from fetal_net import prediction as P
    from fetal_net.pipeline import Stage
    patch = (8, 8, 4)
    model = Fake3d(patch)
    cfg = {"patch_shape": list(patch[:2]), "patch_depth": patch[2]}
    vol = np.random.RandomState(4).randn(12, 10, 6)
    got = P.predict_flips(vol, model, 0.5, cfg, blend="gaussian")
    assert len(got) == 8
    for axes, g in zip(P.FLIP_AXES, got):
        flipped = P.flip_it(vol, axes)
        np.testing.assert_array_equal(g, P.flip_it(P.patch_wise_prediction(model, flipped[np.newaxis], patch, overlap_factor=0.5,
                                                                           blend="gaussian").squeeze(), axes))
    plain = P.predict_flips(vol, model, 0.5, cfg)
    assert float(np.abs(np.stack(got) - np.stack(plain)).max()) > 1e-6
    out = Stage(model, cfg, augment="flip", overlap=0.5, device=False, blend="gaussian").infer(vol)
    np.testing.assert_array_equal(out, np.median(np.stack(got), axis=0))
    np.testing.assert_array_equal(Stage(model, cfg, overlap=0.5, device=False, blend="gaussian").infer(vol), got[0])
    np.testing.assert_array_equal(Stage(model, cfg, overlap=0.5, device=False).infer(vol), plain[0])


# ----------------------------------------------------------------------------------------------------------------- header and binding
def test_header_binding_table_and_library_agree_on_the_new_entry_points():
    from fmri_hip import ops
    from fmri_hip._lib import LIB_PATH, SIGNATURES, lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fmri_hip.h")).read(), flags=re.S)
    for name in NEW:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, src)
        assert m, "%s is not declared in include/fmri_hip.h" % name
        params = [p.strip() for p in m.group(1).split(",")]
        assert name in SIGNATURES and len(SIGNATURES[name]) == len(params), name
        for param, ctype in zip(params, SIGNATURES[name]):
            want = ctypes.c_void_p if "*" in param or "fmri_stream_t" in param else ctypes.c_double if param.startswith("double") else \
                ctypes.c_int64 if param.startswith("int64_t") else ctypes.c_int
            assert ctype is want, (name, param, ctype)
        assert callable(getattr(ops, name[len("fmri_"):])), name
    if not os.path.exists(LIB_PATH):
        import __graft_entry__ as g
        g.build()
    L = lib()
    for name in NEW:
        assert hasattr(L, name), name


def test_refusals_of_the_entry_points_need_no_device():
    """every refusal is decided on the host before anything is enqueued: the codes come back without a GPU"""
    from fmri_hip._lib import LIB_PATH, lib
    if not os.path.exists(LIB_PATH):
        import __graft_entry__ as g
        g.build()
    L = lib()
    E_SHAPE, E_ALIGN = -1, -2
    lo = (ctypes.c_int32 * 3)(0, 0, 0)
    vals = (ctypes.c_uint8 * 1)(1)
    p, q = 4096, 8192                                         # never dereferenced
    sc = L.fmri_tile_scatter_weighted
    good = [p, p, 2, 3, 3, 3, 1, p, p, p, q, q, 4, 4, 4, None]
    for k in (0, 1, 7, 8, 9, 10, 11):
        args = list(good)
        args[k] = 0
        assert sc(*args) == E_SHAPE, k
    for k in (2, 3, 4, 5, 6, 12, 13, 14):
        for v in (0, -1):
            args = list(good)
            args[k] = v
            assert sc(*args) == E_SHAPE, k
    for k, off in ((0, 2), (1, 2), (7, 2), (10, 4), (11, 4)):
        args = list(good)
        args[k] += off
        assert sc(*args) == E_ALIGN, k
    fin = L.fmri_tile_finalize_weighted
    for k in range(4):
        args = [p, p, q, p, 8, 1, None]
        args[k] = 0
        assert fin(*args) == E_SHAPE, k
    assert fin(p, p, q, p, 0, 1, None) == E_SHAPE and fin(p, p, q, p, 8, 0, None) == E_SHAPE
    assert fin(p + 4, p, q, p, 8, 1, None) == E_ALIGN and fin(p, p + 4, q, p, 8, 1, None) == E_ALIGN and fin(p, p, q, p + 2, 8, 1, None) == E_ALIGN
    flip = L.fmri_tile_finalize_flip_weighted
    assert flip(0, p, 4, 4, 4, 1, q, 2, 2, 2, lo, 0, p, None) == E_SHAPE
    assert flip(p, 0, 4, 4, 4, 1, q, 2, 2, 2, lo, 0, p, None) == E_SHAPE
    assert flip(p, p, 4, 4, 4, 1, q, 2, 2, 2, None, 0, p, None) == E_SHAPE
    assert flip(p, p, 4, 4, 4, 1, q, 2, 2, 5, lo, 0, p, None) == E_SHAPE
    assert flip(p, p, 4, 4, 4, 1, q, 2, 2, 2, (ctypes.c_int32 * 3)(0, 3, 0), 0, p, None) == E_SHAPE
    assert flip(p, p, 4, 4, 4, 1, q, 2, 2, 2, lo, 8, p, None) == E_SHAPE
    assert flip(p + 4, p, 4, 4, 4, 1, q, 2, 2, 2, lo, 0, p, None) == E_ALIGN
    assert flip(p, p + 4, 4, 4, 4, 1, q, 2, 2, 2, lo, 0, p, None) == E_ALIGN
    lab = L.fmri_tile_finalize_labels_weighted
    assert lab(0, p, q, p, 8, 1, 0.5, vals, None) == E_SHAPE and lab(p, 0, q, p, 8, 1, 0.5, vals, None) == E_SHAPE
    assert lab(p, p, 0, p, 8, 1, 0.5, vals, None) == E_SHAPE and lab(p, p, q, 0, 8, 1, 0.5, vals, None) == E_SHAPE
    assert lab(p, p, q, p, 0, 1, 0.5, vals, None) == E_SHAPE and lab(p, p, q, p, 8, 1, 0.5, None, None) == E_SHAPE
    assert lab(p, p, q, p, 8, 2, 0.5, (ctypes.c_uint8 * 2)(3, 3), None) == E_SHAPE
    assert lab(p + 4, p, q, p, 8, 1, 0.5, vals, None) == E_ALIGN
