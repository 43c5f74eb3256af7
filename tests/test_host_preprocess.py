"""fetal_net.preprocess - the filters a config names with "preproc" (reference fetal_net/preprocess.py:5-27) - in its host form, and the
way fetal_net.pipeline resolves such a name (reference prod/predict_nifti2.py:57-74), against the reference's expressions written out
with scipy / numpy.  The device forms are held to the host forms in tests/test_gpu_intensity.py."""
import numpy as np
import pytest
from scipy import ndimage


def _nm(d):
    return -1 + 2 * (d - d.min()) / (d.max() - d.min())


WRITTEN_OUT = {
    "norm_minmax": _nm,
    "laplace": ndimage.laplace,
    "laplace_norm": lambda d: _nm(ndimage.laplace(d)),
    "grad": lambda d: ndimage.gaussian_gradient_magnitude(d, sigma=(1, 1, 1)),
    "grad_norm": lambda d: _nm(ndimage.gaussian_gradient_magnitude(d, sigma=(1, 1, 1))),
}


class PointwiseModel:
    """predict(x) = sigmoid(gain * (x - offset)) voxel by voxel (the stand-in of tests/test_host_pipeline.py)"""

    def __init__(self, patch, gain, offset):
        self.output_shape = (None, 1) + tuple(patch)
        self.gain, self.offset = gain, offset

    def predict(self, x):
        return 1.0 / (1.0 + np.exp(-self.gain * (np.asarray(x, dtype=np.float64) - self.offset)))


def _volume(shape=(20, 24, 12), seed=0):
    return np.random.RandomState(seed).randn(*shape) * 30 + 50


@pytest.mark.parametrize("name", sorted(WRITTEN_OUT))
def test_host_form_equals_the_reference_expression(name):
    from fetal_net import preprocess
    assert sorted(preprocess.__all__) == sorted(WRITTEN_OUT)
    d = _volume()
    keep = d.copy()
    got = getattr(preprocess, name)(d, device=False)
    np.testing.assert_array_equal(got, WRITTEN_OUT[name](d))
    np.testing.assert_array_equal(d, keep)
    if name.endswith("norm") or name == "norm_minmax":
        assert got.min() == -1.0 and abs(got.max() - 1.0) < 1e-12


def test_host_form_keeps_the_dtype_rules_of_the_reference():
    from fetal_net import preprocess
    d = _volume().astype(np.float32)
    for name, fn in WRITTEN_OUT.items():
        got = getattr(preprocess, name)(d, device=False)
        assert got.dtype == fn(d).dtype
        np.testing.assert_array_equal(got, fn(d))
    const = np.full((4, 5, 3), 7.0)
    with np.errstate(invalid="ignore"):
        assert np.isnan(preprocess.norm_minmax(const, device=False)).all()          # 0 / 0, as in the reference


def test_stage_resolves_a_named_preproc():
    from fetal_net import preprocess
    from fetal_net.pipeline import Stage
    cfg = {"patch_shape": [8, 8], "patch_depth": 4, "preproc": "laplace_norm"}
    st = Stage(None, cfg, device=False)
    assert st.preproc is preprocess.laplace_norm
    d = _volume()
    np.testing.assert_array_equal(st.intensities(d, []), WRITTEN_OUT["laplace_norm"](d))
    np.testing.assert_array_equal(st.intensities(d), d)                             # no hook at the second stage (no resampling stack)
    for bad in ("by_name", "np", "ndimage", "_dispatch", 3):
        with pytest.raises(TypeError):
            Stage(None, {"patch_shape": [8, 8], "patch_depth": 4, "preproc": bad})
    own = Stage(None, {"patch_shape": [8, 8], "patch_depth": 4, "preproc": lambda v: v * 2.0}, device=False)
    np.testing.assert_array_equal(own.intensities(d, []), d * 2.0)


def test_window_and_normalize_keep_their_host_forms():
    from fetal_net.pipeline import normalize_data, window_intensities_data
    d = _volume()
    lo, hi = np.percentile(d, 1), np.percentile(d, 99)
    np.testing.assert_array_equal(window_intensities_data(d, device=False), (np.clip(d, lo, hi) - lo) * (255.0 / (hi - lo)) + 0.0)
    np.testing.assert_array_equal(normalize_data(d, 3.0, 7.0, device=False), (d - 3.0) / 7.0)
    np.testing.assert_array_equal(window_intensities_data(np.full((3, 4, 5), 2.0), device=False), np.zeros((3, 4, 5)))


@pytest.mark.parametrize("name", ["grad_norm", "laplace"])
def test_predict_volume_with_a_named_preproc_equals_the_written_out_chain(name):
    from fetal_net.pipeline import predict_volume
    vol = _volume((32, 32, 16), seed=2) + 200.0
    cfg = {"patch_shape": [16, 16], "patch_depth": 8, "preproc": name, "scale_data": [0.5, 0.5, 1.0]}
    m = PointwiseModel((16, 16, 8), gain=0.02, offset=0.0)
    norm = {"mean": 0.1, "std": 0.5}
    out = predict_volume(vol, m, cfg, overlap_factor=0.5, preprocess_method="window_1_99", norm_params=norm, device=False)
    lo, hi = np.percentile(vol, 1), np.percentile(vol, 99)
    data = (np.clip(vol, lo, hi) - lo) * (255.0 / (hi - lo)) + 0.0
    data = ndimage.zoom(data, [0.5, 0.5, 1.0])
    data = (WRITTEN_OUT[name](data) - 0.1) / 0.5
    np.testing.assert_array_equal(out["data"], data)
    want = ndimage.zoom(m.predict(data), [2.0, 2.0, 1.0], order=0)
    assert out["prediction"].squeeze().shape == vol.shape
    np.testing.assert_allclose(out["prediction"].squeeze(), want, rtol=0, atol=1e-9)
