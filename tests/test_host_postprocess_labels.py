"""fetal_net.postprocess.postprocess_label_map on the host: the scipy / numpy form that is its definition, the argument rules, and the
`postprocess_labels` keyword of run_validation_case.  No GPU: every call forces device=False or runs a stub model."""
import os

import numpy as np
import pytest
from scipy import ndimage


def _field(shape, n_labels, seed):
    rs = np.random.RandomState(seed)
    p = np.stack([ndimage.gaussian_filter(rs.rand(*shape), 2.0) for _ in range(n_labels)], axis=-1)
    return (p - p.min()) / (p.max() - p.min())


def _definition(pred, values, gaussian_std=1, threshold=0.5, fill_holes=True, connected_component=True):
    """the issue's definition, voxel by voxel in plain loops over the channels (no argmax, no -inf trick)"""
    from fetal_net.postprocess import postprocess_prediction
    n_labels = pred.shape[-1]
    out = np.zeros(pred.shape[:3], np.uint8)
    top = np.full(pred.shape[:3], -np.inf)
    for l in range(n_labels):
        s = ndimage.gaussian_filter(pred[..., l], gaussian_std)
        m = postprocess_prediction(pred[..., l], gaussian_std, threshold, fill_holes, connected_component, device=False)
        win = m & ((out == 0) | (s > top))                  # strictly larger than every lower channel that holds the voxel
        out[win] = values[l]
        top[win] = s[win]
    return out


@pytest.mark.parametrize("kw", [dict(), dict(gaussian_std=0.5), dict(fill_holes=False), dict(connected_component=False),
                                dict(gaussian_std=(1.0, 0.0, 2.0))])
def test_host_path_is_the_definition(kw):
    from fetal_net.postprocess import postprocess_label_map
    pred = _field((17, 33, 9), 5, 0)
    sm = np.stack([ndimage.gaussian_filter(pred[..., l], kw.get("gaussian_std", 1)) for l in range(5)])
    thr = float(np.quantile(sm, 0.6))
    labels = (3, 1, 200, 7, 9)
    got = postprocess_label_map(pred, threshold=thr, labels=labels, device=False, **kw)
    ref = _definition(pred, labels, threshold=thr, **kw)
    assert got.dtype == np.uint8 and got.shape == (17, 33, 9)
    assert np.array_equal(got, ref)
    assert len(np.unique(got)) >= 4 and int(((sm > thr).sum(0) > 1).sum()) > 100          # several labels present, masks overlap
    default = postprocess_label_map(pred, threshold=thr, device=False, **kw)               # labels default to 1..L
    assert np.array_equal(default, _definition(pred, (1, 2, 3, 4, 5), threshold=thr, **kw))


def test_one_label_and_three_dimensions():
    from fetal_net.postprocess import postprocess_label_map, postprocess_prediction
    pred = _field((20, 24, 28), 1, 3)
    thr = float(np.quantile(ndimage.gaussian_filter(pred[..., 0], 1), 0.6))
    mask = postprocess_prediction(pred[..., 0], threshold=thr, device=False)
    assert 0 < mask.sum() < mask.size
    got = postprocess_label_map(pred, threshold=thr, labels=[7], device=False)
    assert np.array_equal(got, (7 * mask).astype(np.uint8))
    assert np.array_equal(postprocess_label_map(pred[..., 0], threshold=thr, labels=[7], device=False), got)
    assert np.array_equal(postprocess_label_map(pred[..., 0], threshold=thr, device=False), mask.astype(np.uint8))


def test_identical_channels_resolve_to_the_lower_index():
    from fetal_net.postprocess import postprocess_label_map
    one = _field((16, 18, 20), 1, 4)[..., 0]
    pred = np.stack([one, one, one], axis=-1)
    thr = float(np.quantile(ndimage.gaussian_filter(one, 1), 0.6))
    got = postprocess_label_map(pred, threshold=thr, labels=(9, 4, 2), device=False)
    assert set(np.unique(got)) == {0, 9}


def test_a_filled_voxel_competes_with_its_smoothed_value():
    """channel 0: a shell whose closed hole is filled; channel 1: a block inside that hole with a high probability - inside the block
    channel 1 wins although channel 0 holds the voxels too, elsewhere in the hole channel 0 keeps them with S_0 <= threshold"""
    from fetal_net.postprocess import postprocess_label_map
    shell = np.zeros((20, 24, 28))
    shell[4:16, 4:20, 4:24] = 1
    shell[7:13, 8:16, 8:20] = 0
    block = np.zeros_like(shell)
    block[8:12, 9:15, 9:19] = 1
    pred = np.stack([0.1 + 0.8 * shell, 0.1 + 0.8 * block], axis=-1)
    got = postprocess_label_map(pred, gaussian_std=0.5, device=False)
    assert got[10, 12, 14] == 2 and got[7, 8, 8] == 1 and got[5, 5, 5] == 1 and got[0, 0, 0] == 0
    assert ndimage.gaussian_filter(pred[..., 0], 0.5)[7, 8, 8] <= 0.5


def test_argument_rules():
    from fetal_net.postprocess import postprocess_label_map
    pred = np.zeros((4, 5, 6, 3))
    for bad in [(1, 2), (1, 2, 3, 4), (1, 1, 2), (0, 1, 2), (1, 2, 256), (1, 2, 2.5), (1, 2, -1)]:
        with pytest.raises(ValueError):
            postprocess_label_map(pred, labels=bad, device=False)
    with pytest.raises(ValueError):
        postprocess_label_map(np.zeros((4, 5, 6, 33)), device=False)
    with pytest.raises(ValueError):
        postprocess_label_map(np.zeros((4, 5)), device=False)
    with pytest.raises(ValueError):
        postprocess_label_map(np.zeros((4, 5, 6)), labels=(1, 2), device=False)
    assert postprocess_label_map(np.zeros((4, 5, 6, 32)), device=False).sum() == 0
    from fetal_net import postprocess
    from fmri_hip import ops
    assert postprocess.MAX_LABELS == ops.MAX_LABELS == 32                                 # the host path keeps its own copy of the bound


class _Stub(object):
    """a foreign model object (no device path): three label channels computed from the patch, channels first"""
    _input_layout = "channels_first_3d"
    output_shape = (None, 3, 8, 8, 8)

    def predict(self, x):
        x = np.asarray(x, np.float64)[:, 0]
        return np.stack([x, 1.0 - x, 0.9 * x], axis=1)


def test_run_validation_case_writes_the_cleaned_map_when_asked(tmp_path):
    from fetal_net.postprocess import postprocess_label_map
    from fetal_net.prediction import get_prediction_labels, patch_wise_prediction, run_validation_case
    from fetal_net.utils.nifti import load_nifti

    class Root(object):
        pass

    class DataFile(object):
        root = Root()

    vol = _field((16, 24, 16), 1, 6)[..., 0]
    DataFile.root.data = [vol]
    DataFile.root.truth = [(vol > 0.5).astype(np.uint8)]
    kw = dict(patch_shape=(8, 8, 8), overlap_factor=0, output_label_map=True, threshold=0.55, labels=(2, 5, 9))
    pred = patch_wise_prediction(_Stub(), vol[np.newaxis], (8, 8, 8))
    assert pred.shape == (16, 24, 16, 3)
    today = get_prediction_labels(np.moveaxis(pred, -1, 0)[np.newaxis], threshold=0.55, labels=(2, 5, 9))[0]
    clean = postprocess_label_map(pred, threshold=0.55, labels=(2, 5, 9), device=False)
    rough = postprocess_label_map(pred, threshold=0.55, labels=(2, 5, 9), gaussian_std=0.5, connected_component=False, device=False)
    assert not np.array_equal(today, clean) and not np.array_equal(clean, rough)

    def labels_of(name, **more):
        out = str(tmp_path / name)
        run_validation_case(0, out, _Stub(), DataFile, ["volume"], **dict(kw, **more))
        return out, load_nifti(os.path.join(out, "prediction_labels.nii.gz"), scaled=False)

    plain_dir, plain = labels_of("plain")
    none_dir, none = labels_of("none", postprocess_labels=None)
    assert np.array_equal(plain, today) and np.array_equal(none, today)
    clean_dir, got = labels_of("clean", postprocess_labels={})
    assert got.dtype == np.uint8 and np.array_equal(got, clean)
    assert np.array_equal(labels_of("rough", postprocess_labels=dict(gaussian_std=0.5, connected_component=False))[1], rough)
    for name in ("prediction.nii.gz", "truth.nii.gz", "data_volume.nii.gz"):              # every other file is today's
        assert np.array_equal(load_nifti(os.path.join(plain_dir, name)), load_nifti(os.path.join(clean_dir, name)))
    out = str(tmp_path / "off")                                                           # without output_label_map the keyword does nothing
    run_validation_case(0, out, _Stub(), DataFile, ["volume"], patch_shape=(8, 8, 8), postprocess_labels={})
    assert not os.path.exists(os.path.join(out, "prediction_labels.nii.gz"))


@pytest.mark.parametrize("sigma", [0.5, 1, 2.0, 2.3])
def test_order0_gaussian_weights_are_the_same_doubles_reversed(sigma):
    """the device gaussians take their weights from ops.gaussian_kernel1d(sd, 0, radius), which reverses the kernel as scipy's
    gaussian_filter1d does: the order-0 kernel is symmetric, so that is bit for bit the unreversed phi / phi.sum()"""
    from fmri_hip import ops
    radius = int(4.0 * sigma + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    w = ops.gaussian_kernel1d(float(sigma), 0, radius)
    assert w.dtype == np.float64 and w.tobytes() == (phi / phi.sum()).tobytes() and w.tobytes() == w[::-1].tobytes()
