"""scipy.ndimage's B-spline resampling and the variant median on the device (csrc/postprocess.hip: fmri_spline_filter1d_f64,
fmri_spline_affine_f64, fmri_median_stack_f64; fmri_hip.ops spline_filter_f64 / affine_transform_f64 / zoom_f64 / rotate_f64 /
median_stack_f64) and their wiring into fetal_net.pipeline and the test-time augmentation, against scipy.ndimage / numpy themselves.

Tolerances
  order 0: identical - a gather at indices computed by the same fp64 operations.
  orders 1-3 and the prefilter: max |got - want| <= 1e-12 * max(1, max |want|), the bound tests/test_host_spline_rotate.py holds the torch
    form to.  A plain-Python restatement of the same arithmetic differs from ndimage.zoom by at most 5.6e-16 on [0, 1) data of shape
    7x9x5 (orders 2, 3) and by 0.0 at orders 0 and 1.
  cval: on strictly positive input at order 1 the device result is 0 exactly where scipy's is (scipy drops the far edge of an axis when
    (m - 1) * ((n - 1) / (m - 1)) > n - 1 in floating point: n = 4 -> m = 188 is such a pair).
  median: identical to np.median.
Measured maxima on an MI355X (every test prints its own; `pytest -s`), randn / [0.5, 1.5) data:
  prefilter: one axis 4.4e-15, all three axes 2.8e-14 (orders 2 and 3, the 1027-sample line included)
  zoom: order 0 identical, order 1 4.4e-16, order 2 1.6e-15, order 3 2.4e-15; the zero voxels agree in every order-1 case
  rotate: order 2 1.7e-14, order 3 1.7e-14;  affine, full matrix: order 3 2.9e-15, order 1 identical
  Zoom.forward on a volume of values around 300: 4.5e-13 (1.5e-15 relative), Zoom.backward 2.8e-14; predict_volume 5.8e-15;
  _TTAVariant.forward / inverse 6.1e-16 / 1.0e-15; median identical
"""
import functools

import numpy as np
import pytest
import torch
from scipy import ndimage

pytestmark = pytest.mark.gpu

ANGLES = (17.3, -29.9, 30.0, 90, 0.0, 45.0, 180, -90.0, 270.0)        # the list of tests/test_host_spline_rotate.py


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the GPU box"
    from fmri_hip import ops as o
    return o


@functools.lru_cache(maxsize=None)
def volume(shape, kind="randn"):
    rs = np.random.RandomState(sum(shape) + 7 * len(kind))
    v = rs.randn(*shape) if kind == "randn" else rs.rand(*shape) + 0.5          # "pos": strictly positive
    v.setflags(write=False)
    return v


def dev(v):
    return torch.from_numpy(np.array(v, dtype=np.float64, order="C")).cuda()          # a copy: the cached volumes are read-only


def check_close(got, want, order, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.dtype == np.float64 and got.shape == want.shape, (what, got.shape, want.shape)
    err = float(np.abs(got - want).max()) if want.size else 0.0
    print("%s: max |difference| %.3e" % (what, err))
    if order == 0:
        np.testing.assert_array_equal(got, want, err_msg=what)
    else:
        assert err <= 1e-12 * max(1.0, float(np.abs(want).max())), (what, err)


# ------------------------------------------------------------------------------------------------------------------------- prefilter
PREFILTER_SHAPES = [(1, 4, 3), (2, 1, 5), (3, 3, 1), (7, 9, 5), (33, 40, 70), (3, 2, "lds_max+3")]


@pytest.mark.parametrize("shape", PREFILTER_SHAPES, ids=str)
@pytest.mark.parametrize("order", [2, 3])
def test_prefilter_equals_scipy(ops, shape, order):
    from fmri_hip._lib import lib
    if shape[2] == "lds_max+3":
        shape = shape[:2] + (lib().fmri_spline_lds_max_line() + 3,)               # the global-memory form of the contiguous axis
    v = volume(shape)
    for axis in range(3):
        want = ndimage.spline_filter1d(v, order, axis, mode="mirror")
        check_close(ops.spline_filter_f64(dev(v), order, axes=(axis,)), want, order, "prefilter %s order %d axis %d" % (shape, order, axis))
    check_close(ops.spline_filter_f64(dev(v), order), ndimage.spline_filter(v, order, mode="mirror"), order,
                "prefilter %s order %d all axes" % (shape, order))


def test_prefilter_leaves_its_input_alone_and_copies_low_orders(ops):
    v = volume((7, 9, 5))
    d = dev(v)
    ops.spline_filter_f64(d, 3)
    np.testing.assert_array_equal(d.cpu().numpy(), v)
    np.testing.assert_array_equal(ops.spline_filter_f64(d, 1).cpu().numpy(), v)


# ------------------------------------------------------------------------------------------------------------------------------ zoom
FACTORS = [(1.6, 0.7, 2.0), (0.5, 1.3, 1.0), (1 / 0.7, 1 / 0.7, 1 / 1.3)]
ZOOM_CASES = [((7, 9, 5), f) for f in FACTORS] + [((33, 40, 6), f) for f in FACTORS] + [
    ((1, 4, 3), (3.0, 0.5, 1.0)),          # an input axis of length 1
    ((4, 5, 3), (0.25, 1, 1)),             # an output axis of length 1
    ((5, 4, 3), (0.5, 1, 1)),              # banker's rounding: 2.5 -> 2
]


@pytest.mark.parametrize("shape,factors", ZOOM_CASES, ids=str)
@pytest.mark.parametrize("order", [0, 1, 2, 3])
def test_zoom_equals_scipy(ops, shape, factors, order):
    v = volume(shape, "pos")
    want = ndimage.zoom(v, factors, order=order)
    got = ops.zoom_f64(dev(v), factors, order=order).cpu().numpy()
    check_close(got, want, order, "zoom %s x %s order %d" % (shape, factors, order))
    if order == 1:
        np.testing.assert_array_equal(got == 0, want == 0)


def test_zoom_returns_cval_where_scipy_does(ops):
    v = np.ones((4, 3, 2))
    want = ndimage.zoom(v, (47.0, 1, 1), order=1)
    assert want.shape == (188, 3, 2) and (want[-1] == 0).all() and (want[:-1] > 0).all()        # scipy drops the far edge here
    got = ops.zoom_f64(dev(v), (47.0, 1, 1), order=1).cpu().numpy()
    np.testing.assert_array_equal(got == 0, want == 0)
    check_close(got, want, 1, "zoom 4 -> 188 order 1")


# ---------------------------------------------------------------------------------------------------------------------------- rotate
@pytest.mark.parametrize("shape", [(24, 20, 6), (7, 9, 3), (2, 5, 2)], ids=str)
@pytest.mark.parametrize("order", [2, 3])
def test_rotate_equals_scipy(ops, shape, order):
    v = volume(shape)
    d = dev(v)
    worst = 0.0
    for angle in ANGLES:
        for reshape in (False, True):
            want = ndimage.rotate(v, angle, order=order, reshape=reshape)
            got = ops.rotate_f64(d, angle, order=order, reshape=reshape).cpu().numpy()
            assert got.shape == want.shape, (angle, reshape, got.shape, want.shape)
            err = float(np.abs(got - want).max())
            worst = max(worst, err)
            assert err <= 1e-12 * max(1.0, float(np.abs(want).max())), (angle, reshape, err)
    print("rotate %s order %d: max |difference| over %d angles %.3e" % (shape, order, len(ANGLES), worst))


# ---------------------------------------------------------------------------------------------------------------------------- affine
def test_affine_transform_with_a_full_matrix_equals_scipy(ops):
    v = volume((9, 8, 7))
    M = np.array([[0.81, 0.23, -0.17], [-0.29, 0.74, 0.31], [0.12, -0.19, 0.66]])
    t = np.array([1.3, 2.1, 0.9])
    want = ndimage.affine_transform(v, M, t, (11, 6, 10), order=3)
    assert (want != 0).mean() > 0.2 and (want == 0).any()                      # inside and outside voxels both occur
    got = ops.affine_transform_f64(dev(v), M, t, (11, 6, 10), 3)
    check_close(got, want, 3, "affine (9, 8, 7) -> (11, 6, 10) order 3")
    np.testing.assert_array_equal(got.cpu().numpy() == 0, want == 0)
    want = ndimage.affine_transform(v, M, t, (11, 6, 10), order=1, cval=-2.5)
    check_close(ops.affine_transform_f64(dev(v), M, t, (11, 6, 10), 1, cval=-2.5), want, 1, "affine order 1 cval -2.5")


# ---------------------------------------------------------------------------------------------------------------------------- median
@pytest.mark.parametrize("K", [1, 2, 3, 8, 9, 32, 64])
def test_median_stack_equals_numpy(ops, K):
    rs = np.random.RandomState(K)
    stack = rs.rand(K, 1000)
    stack[:, ::3] = np.round(stack[:, ::3], 1)                                 # repeated values within a voxel's stack
    stack[:, 5] = 0.25
    got = ops.median_stack_f64(dev(stack.reshape(K, 10, 100))).cpu().numpy()
    assert got.shape == (10, 100)
    np.testing.assert_array_equal(got.ravel(), np.median(stack, axis=0))


def test_median_stack_refuses_more_than_64(ops):
    from fmri_hip._lib import FmriError
    with pytest.raises(FmriError):
        ops.median_stack_f64(torch.zeros(65, 10, dtype=torch.float64, device="cuda"))


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


def test_zoom_step_device_equals_host(ops):
    from fetal_net.pipeline import Zoom
    vol = blob_volume((20, 24, 12), 3)
    zd, zh = Zoom([0.5, 0.5, 1.0], 1, device=True), Zoom([0.5, 0.5, 1.0], 1, device=False)
    fd, fh = zd.forward(vol), zh.forward(vol)
    assert fh.shape == (10, 12, 12)
    check_close(fd, fh, 3, "Zoom.forward")
    check_close(zd.backward(fh), zh.backward(fh), 1, "Zoom.backward")
    assert zh.backward(fh).shape == vol.shape
    pair = np.stack([fh, fh[::-1].copy()])
    check_close(zd.backward(pair), zh.backward(pair), 1, "Zoom.backward of a stack of two")
    assert zd.backward(pair).shape == (2,) + vol.shape
    check_close(Zoom([0.5, 0.5, 1.0], 1).forward(vol), fh, 3, "Zoom.forward, default device rule")


def test_predict_volume_device_resampling_equals_host(ops):
    from fetal_net.pipeline import predict_volume
    vol = blob_volume((32, 32, 16), 2)
    cfg = {"patch_shape": [16, 16], "patch_depth": 8}
    m = PointwiseModel((16, 16, 8), gain=1.0, offset=0.0)
    common = dict(overlap_factor=0.5, norm_params={"mean": 100.0, "std": 100.0})
    for extra in (dict(xy_scale=0.5, z_scale=1.0), dict(augment="flip")):
        a = predict_volume(vol, m, cfg, device=True, **common, **extra)
        b = predict_volume(vol, m, cfg, device=False, **common, **extra)
        assert a["prediction"].shape == b["prediction"].shape and a["prediction"].squeeze().shape == vol.shape
        check_close(a["prediction"], b["prediction"], 1, "predict_volume %s" % sorted(extra))
        check_close(a["data"], b["data"], 3, "predict_volume %s: data" % sorted(extra))


def test_tta_variant_default_rotation_equals_the_scipy_form(ops, monkeypatch):
    """_TTAVariant.forward / inverse with the HIP rotations (the default on a GPU) against the scipy ones; the draw of
    tests/test_host_spline_rotate.py"""
    from fetal_net import prediction as P
    rs = np.random.RandomState(3)
    vol = rs.rand(20, 24, 10)
    np.random.seed(5)
    v = P._TTAVariant.draw(vol.min(), vol.max())
    monkeypatch.setenv("FMRI_TTA_TORCH_ROTATE", "0")
    a0 = v.forward(vol)
    b0 = v.inverse(a0)
    monkeypatch.delenv("FMRI_TTA_TORCH_ROTATE")
    calls = []
    real = ops.rotate_f64
    monkeypatch.setattr(ops, "rotate_f64", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    a1 = v.forward(vol)
    b1 = v.inverse(a1)
    assert len(calls) == 2, "the default rotation did not go through fmri_hip.ops.rotate_f64"
    assert a0.shape == a1.shape and b0.shape == b1.shape
    check_close(a1, a0, 2, "_TTAVariant.forward")
    check_close(b1, b0, 3, "_TTAVariant.inverse")
