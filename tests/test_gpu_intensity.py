"""The intensity preparation in front of the model on the device (csrc/postprocess.hip: fmri_order_stats_f64, fmri_minmax_f64,
fmri_intensity_map_f64, fmri_laplace_f64, fmri_grad_magnitude_combine_f64, fmri_correlate1d_asym_f64;
fmri_hip.ops percentile_f64 / window_intensities_f64 / norm_minmax_f64 / normalize_f64 / laplace_f64 / gaussian_gradient_magnitude_f64)
and its wiring into fetal_net.preprocess and fetal_net.pipeline, against scipy.ndimage / numpy themselves.

Tolerances
  Everything but the zoom inside Stage.intensities / predict_volume: identical (np.testing.assert_array_equal, NaN positions included).
    Derived, not measured: every operation is an fp64 add, multiply, divide or square root in numpy's / scipy's own order, correctly
    rounded on gfx950 (no fast-math flag, fp contract off), and the order statistics are selected on the bit patterns.
  The `scale_data` zoom inside Stage.intensities keeps the bound of tests/test_gpu_resample.py, 1e-12 * max(1, max |want|); without the
    zoom the chain is identical again.
Measured on an MI355X (`pytest -s` prints them): every comparison of the first kind identical, at both digit widths of the select;
  Stage.intensities with the zoom 2.7e-15, predict_volume data 2.7e-15 / prediction 6.7e-16, two stages (laplace_norm) data 1.8e-14.
"""
import functools

import numpy as np
import pytest
import torch
from scipy import ndimage

pytestmark = pytest.mark.gpu

SHAPES = [(1, 4, 3), (2, 1, 5), (3, 3, 1), (7, 9, 5), (33, 40, 70)]          # the first three: axes shorter than the radius 4
BIG = (129, 128, 128)                                                       # more voxels than the grid has threads: the grid-stride loop
QS = [0, 1, 25, 37.5, 50, 99, 100]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the GPU box"
    from fmri_hip import ops as o
    return o


@functools.lru_cache(maxsize=None)
def volume(shape):
    v = np.random.RandomState(sum(shape)).randn(*shape) * 30 + 50
    v.setflags(write=False)
    return v


def dev(v):
    return torch.from_numpy(np.array(v, dtype=np.float64, order="C")).cuda()          # a copy: the cached volumes are read-only


def same(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.dtype == np.float64 and got.shape == np.shape(want), (what, got.dtype, got.shape, np.shape(want))
    np.testing.assert_array_equal(got, want, err_msg=what)


# ------------------------------------------------------------------------------------------------------------- laplace, correlation, gradient
@pytest.mark.parametrize("shape", SHAPES + [BIG], ids=str)
def test_laplace_equals_scipy(ops, shape):
    v = volume(shape)
    d = dev(v)
    same(ops.laplace_f64(d), ndimage.laplace(v), "laplace %s" % (shape,))
    np.testing.assert_array_equal(d.cpu().numpy(), v)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_both_correlation_branches_equal_scipy(ops, shape):
    from fmri_hip._lib import lib
    v = volume(shape)
    d = dev(v)
    X, Y, Z = shape
    for order, name in ((0, "fmri_correlate1d_f64"), (1, "fmri_correlate1d_asym_f64")):
        w = ops.gaussian_kernel1d(1.0, order, 4)
        wd = torch.from_numpy(w).cuda()
        for axis in range(3):
            out = torch.empty_like(d)
            assert getattr(lib(), name)(d.data_ptr(), out.data_ptr(), X, Y, Z, axis, wd.data_ptr(), 4, ops._s()) == 0
            same(out, ndimage.gaussian_filter1d(v, 1.0, axis=axis, order=order), "%s %s axis %d" % (name, shape, axis))
            same(out, ndimage.correlate1d(v, w, axis=axis), "%s %s axis %d against correlate1d" % (name, shape, axis))


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_gradient_magnitude_equals_scipy(ops, shape):
    v = volume(shape)
    d = dev(v)
    same(ops.gaussian_gradient_magnitude_f64(d, (1, 1, 1)), ndimage.gaussian_gradient_magnitude(v, sigma=(1, 1, 1)), "grad %s" % (shape,))
    np.testing.assert_array_equal(d.cpu().numpy(), v)
    if shape == (7, 9, 5):
        same(ops.gaussian_gradient_magnitude_f64(d, (0.6, 1.0, 1.7)), ndimage.gaussian_gradient_magnitude(v, sigma=(0.6, 1.0, 1.7)), "grad, 3 sigmas")
        with pytest.raises(NotImplementedError):
            ops.gaussian_gradient_magnitude_f64(d, (1, 0, 1))


# -------------------------------------------------------------------------------------------------------------- order statistics, percentiles
SELECT_NAMES = ["n=1", "n=2", "signed zeros", "heavy ties", "70% zeros", "last digit", "600 decades", "129x128x128 randn", "one NaN"]


@functools.lru_cache(maxsize=None)
def select_inputs():
    rs = np.random.RandomState(11)
    background = rs.rand(30000) * 900
    background[rs.rand(30000) < 0.7] = 0.0
    nan = rs.randn(1000)
    nan[517] = np.nan
    return {
        "n=1": np.array([3.25]),
        "n=2": np.array([2.0, -1.0]),
        "signed zeros": np.array([0.0, -0.0, 0.0, -0.0, 1.0]),
        "heavy ties": np.round(rs.randn(5000) * 3),
        "70% zeros": background,
        "last digit": 1.0 + rs.permutation(4097) * 2.0 ** -52,
        "600 decades": rs.randn(20000) * 10.0 ** rs.randint(-300, 300, 20000),
        "129x128x128 randn": rs.randn(129 * 128 * 128),
        "one NaN": nan,
    }


@pytest.mark.parametrize("bits", [8, 11])
@pytest.mark.parametrize("name", SELECT_NAMES)
def test_order_statistics_and_percentiles_equal_numpy(ops, monkeypatch, name, bits):
    monkeypatch.setenv("FMRI_SELECT_BITS", str(bits))
    v = select_inputs()[name]
    n = v.size
    d = dev(v)
    srt = np.sort(v)
    ranks = sorted({0, n - 1, n // 2, n // 100, (99 * n) // 100, min(1, n - 1), n // 3, (2 * n) // 3})
    vals, nans = ops.order_stats_f64(d, ranks)
    assert nans == int(np.isnan(v).sum())
    same(vals, srt[ranks], "order statistics of %s" % name)
    lo = np.floor(np.array(QS) / 100 * (n - 1)).astype(np.int64)
    more, _ = ops.order_stats_f64(d, np.concatenate([lo, np.minimum(lo + 1, n - 1)]))          # 14 ranks: two groups
    same(more, srt[np.concatenate([lo, np.minimum(lo + 1, n - 1)])], "14 order statistics of %s" % name)
    with np.errstate(invalid="ignore"):
        want = np.percentile(v, QS)
    assert np.isnan(want).all() == (name == "one NaN")
    same(ops.percentile_f64(d, QS), want, "percentiles of %s" % name)
    assert ops.percentile_f64(d, 37.5) == want[3] or name == "one NaN"
    np.testing.assert_array_equal(d.cpu().numpy(), v)


def test_eight_ranks_with_duplicates_in_one_call(ops):
    v = select_inputs()["heavy ties"]
    ranks = [7, 7, 0, 4999, 2500, 2500, 7, 1]
    vals, _ = ops.order_stats_f64(dev(v), ranks)
    same(vals, np.sort(v)[ranks], "8 ranks with duplicates")


def test_minmax_equals_numpy(ops):
    assert sorted(select_inputs()) == sorted(SELECT_NAMES)
    for name, v in select_inputs().items():
        with np.errstate(invalid="ignore"):
            want = (v.min(), v.max())
        np.testing.assert_array_equal(np.array(ops.minmax_f64(dev(v))), np.array(want), err_msg=name)


# ------------------------------------------------------------------------------------------------------------------------- invalid arguments
def test_invalid_arguments_are_refused(ops):
    import ctypes
    from fmri_hip._lib import lib
    L = lib()
    d = dev(volume((7, 9, 5)))
    out, nan = torch.empty(8, dtype=torch.float64, device="cuda"), torch.empty(1, dtype=torch.int64, device="cuda")
    ws = torch.empty(L.fmri_order_stats_workspace_bytes(), dtype=torch.uint8, device="cuda")
    p, s = d.data_ptr(), ops._s()

    def select(src, n, ranks, K, o=out.data_ptr(), c=nan.data_ptr(), w=ws.data_ptr()):
        R = (ctypes.c_int64 * 9)(*(list(ranks) + [0] * (9 - len(ranks))))
        return L.fmri_order_stats_f64(src, n, ctypes.addressof(R), K, o, c, w, s)

    assert select(p, 315, [0, 314], 2) == 0
    E = -1                                                                       # FMRI_E_SHAPE
    assert select(p, 315, [315], 1) == E and select(p, 315, [-1], 1) == E and select(p, 315, [0] * 9, 9) == E
    assert select(p, 315, [0], 0) == E and select(p, 2 ** 31, [0], 1) == E and select(p, 0, [0], 1) == E
    assert select(0, 315, [0], 1) == E and select(p, 315, [0], 1, o=0) == E and select(p, 315, [0], 1, c=0) == E
    assert select(p, 315, [0], 1, w=0) == E and L.fmri_order_stats_f64(p, 315, 0, 1, out.data_ptr(), nan.data_ptr(), ws.data_ptr(), s) == E
    o2 = torch.empty_like(d)
    assert L.fmri_minmax_f64(0, 315, out.data_ptr(), nan.data_ptr(), s) == E and L.fmri_minmax_f64(p, 0, out.data_ptr(), nan.data_ptr(), s) == E
    assert L.fmri_intensity_map_f64(p, o2.data_ptr(), 315, 3, 0.0, 1.0, 0.0, 0.0, s) == E
    assert L.fmri_intensity_map_f64(p, 0, 315, 0, 0.0, 1.0, 0.0, 0.0, s) == E
    assert L.fmri_laplace_f64(p, p, 7, 9, 5, s) == E and L.fmri_laplace_f64(p, o2.data_ptr(), 7, 0, 5, s) == E
    assert L.fmri_correlate1d_asym_f64(p, p, 7, 9, 5, 0, p, 1, s) == E and L.fmri_correlate1d_asym_f64(p, o2.data_ptr(), 7, 9, 5, 3, p, 1, s) == E
    assert L.fmri_grad_magnitude_combine_f64(p, p, 0, o2.data_ptr(), 315, s) == E
    torch.cuda.synchronize()
    np.testing.assert_array_equal(d.cpu().numpy(), volume((7, 9, 5)))
    for bad in (torch.zeros(3, 3, 3, device="cuda"), torch.zeros(0, 3, 3, dtype=torch.float64, device="cuda")):
        with pytest.raises(ValueError):
            ops.laplace_f64(bad)
        with pytest.raises(ValueError):
            ops.percentile_f64(bad, 50)
    with pytest.raises(ValueError):
        ops.percentile_f64(d, 101)
    with pytest.raises(RuntimeError):
        ops.laplace_f64(torch.zeros(3, 3, 3, dtype=torch.float64))


# ------------------------------------------------------------------------------------------------------------------ maps and the host API
def test_map_in_place_and_out_of_place(ops):
    v = volume((33, 40, 70))
    d = dev(v)
    same(ops.normalize_f64(d, 3.0, 7.0), (v - 3.0) / 7.0, "z-score")
    np.testing.assert_array_equal(d.cpu().numpy(), v)
    assert ops.intensity_map_f64(d, ops.MAP_ZSCORE, 3.0, 7.0, out=d) is d             # src == dst, asked for explicitly
    same(d, (v - 3.0) / 7.0, "z-score in place")
    w = v.copy()
    w[3, 4, 5] = np.nan
    lo, hi = np.percentile(v, 1), np.percentile(v, 99)
    same(ops.intensity_map_f64(dev(w), ops.MAP_WINDOW, lo, hi, 255.0 / (hi - lo), 0.0), (np.clip(w, lo, hi) - lo) * (255.0 / (hi - lo)) + 0.0,
         "window of a volume with a NaN")


@pytest.mark.parametrize("kind", ["randn", "constant"])
def test_host_api_device_equals_host(ops, kind):
    from fetal_net import preprocess
    from fetal_net.pipeline import normalize_data, window_intensities_data
    v = np.array(volume((33, 40, 70))) if kind == "randn" else np.full((9, 8, 7), 41.5)
    keep = v.copy()
    fns = [(n, getattr(preprocess, n)) for n in preprocess.__all__]
    fns += [("window", window_intensities_data), ("window 5-95 to [-1, 1]", lambda a, device: window_intensities_data(a, 5, 95, -1.0, 1.0, device=device)),
            ("normalize", lambda a, device: normalize_data(a, 12.5, 3.0, device=device))]
    for name, fn in fns:
        with np.errstate(invalid="ignore", divide="ignore"):
            want = fn(v, device=False)
        same(fn(v, device=True), want, "%s, %s" % (name, kind))
        same(fn(v, device=None), want, "%s, %s, default rule" % (name, kind))          # normalize: the host form, see its docstring
        t = fn(dev(v), device=None)
        assert isinstance(t, torch.Tensor) and t.is_cuda
        same(t, want, "%s, %s, tensor in" % (name, kind))
        np.testing.assert_array_equal(v, keep)
    if kind == "constant":
        assert (window_intensities_data(v, device=True) == 0.0).all() and np.isnan(preprocess.norm_minmax(v, device=True)).all()
        assert np.isnan(preprocess.grad_norm(v, device=True)).all()
    d = dev(v)
    preprocess.grad_norm(d)
    window_intensities_data(d)
    np.testing.assert_array_equal(d.cpu().numpy(), v)


# ---------------------------------------------------------------------------------------------------------------------------- wiring
class PointwiseModel:
    """predict(x) = sigmoid(gain * (x - offset)) voxel by voxel (the stand-in of tests/test_host_pipeline.py)"""

    def __init__(self, patch, gain, offset):
        self.output_shape = (None, 1) + tuple(patch)
        self.gain, self.offset = gain, offset

    def predict(self, x):
        return 1.0 / (1.0 + np.exp(-self.gain * (np.asarray(x, dtype=np.float64) - self.offset)))


def blob_volume(shape, seed):
    rs = np.random.RandomState(seed)
    g = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), -1).astype(np.float64)
    blob = np.exp(-(((g - np.array(shape) / 2.0) / (np.array(shape) / 4.0)) ** 2).sum(-1))
    return 100.0 + 400.0 * blob + 5.0 * rs.randn(*shape)


def close(got, want, what):
    assert got.dtype == np.float64 and got.shape == want.shape, (what, got.shape, want.shape)
    err = float(np.abs(got - want).max())
    print("%s: max |difference| %.3e" % (what, err))
    assert err <= 1e-12 * max(1.0, float(np.abs(want).max())), (what, err)


CFG = {"patch_shape": [16, 16], "patch_depth": 8, "scale_data": [0.5, 0.5, 1.0], "preproc": "grad_norm"}
NORM = {"mean": 0.1, "std": 0.5}


def test_stage_intensities_device_equals_host(ops):
    from fetal_net import preprocess
    from fetal_net.pipeline import Stage, normalize_data
    vol = blob_volume((32, 32, 16), 2)
    keep = vol.copy()
    sd, sh = Stage(None, CFG, "window_1_99", NORM, device=True), Stage(None, CFG, "window_1_99", NORM, device=False)
    steps_d, steps_h = [], []
    got, want = sd.intensities(vol, steps_d), sh.intensities(vol, steps_h)
    np.testing.assert_array_equal(vol, keep)
    assert len(steps_d) == len(steps_h) == 1 and steps_d[0].factors == steps_h[0].factors and want.shape == (16, 16, 16)
    # grad_norm divides by the gradient's range and the z-score by 0.5: |d result / d zoomed| stays below ~2 / range * 2, far under 1
    close(got, want, "Stage.intensities, all four steps")
    # without the zoom (the second stage's form, and a config without scale_data) nothing is left to differ
    same(sd.intensities(vol), sh.intensities(vol), "Stage.intensities, window and z-score")
    cfg = dict(CFG, scale_data=None)
    same(Stage(None, cfg, "window_1_99", NORM, device=True).intensities(vol, []), Stage(None, cfg, "window_1_99", NORM, device=False).intensities(vol, []),
         "Stage.intensities without the zoom")
    same(Stage(None, cfg, "window_1_99", NORM).intensities(vol, []), Stage(None, cfg, "window_1_99", NORM, device=False).intensities(vol, []),
         "Stage.intensities, default rule")
    # a caller's own callable is handed a numpy array
    seen = []

    def own(a):
        seen.append(type(a))
        return preprocess.laplace(a, device=False)

    cfg = dict(CFG, scale_data=None, preproc=own)
    same(Stage(None, cfg, "window_1_99", NORM, device=True).intensities(vol, []), Stage(None, cfg, "window_1_99", NORM, device=False).intensities(vol, []),
         "Stage.intensities with a callable")
    assert seen == [np.ndarray, np.ndarray]
    assert normalize_data(np.zeros((2, 2, 2)), 1.0, 2.0, device=True).dtype == np.float64


def test_predict_volume_device_intensities_equal_host(ops):
    from fetal_net.pipeline import predict_volume
    vol = blob_volume((32, 32, 16), 2)
    m = PointwiseModel((16, 16, 8), gain=1.0, offset=0.0)
    common = dict(overlap_factor=0.5, preprocess_method="window_1_99", norm_params=NORM)
    a = predict_volume(vol, m, CFG, device=True, **common)
    b = predict_volume(vol, m, CFG, device=False, **common)
    assert a["prediction"].shape == b["prediction"].shape and a["prediction"].squeeze().shape == vol.shape
    close(a["data"], b["data"], "predict_volume: data")
    close(a["prediction"], b["prediction"], "predict_volume: prediction")
    two = dict(common, model2=m, config2=dict(CFG, preproc=None), preprocess_method2="window_1_99", norm_params2={"mean": 100.0, "std": 50.0})
    a = predict_volume(vol, m, dict(CFG, preproc="laplace_norm"), device=True, **two)
    b = predict_volume(vol, m, dict(CFG, preproc="laplace_norm"), device=False, **two)
    close(a["data"], b["data"], "two stages: data")
    np.testing.assert_array_equal(a["mask"], b["mask"])
    same(a["prediction_roi"], b["prediction_roi"], "two stages: second stage (window and z-score of the box, no zoom)")
