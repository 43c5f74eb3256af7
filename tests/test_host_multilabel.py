"""Several labels, host side: the reference's label-map helpers against literal arrays, per-label scoring, the generator's argument checks
and the builders' label-wise metric names.  The device side is tests/test_gpu_multilabel.py."""
import numpy as np
import pytest


def test_get_prediction_labels_literal_cases():
    from fetal_net.prediction import get_prediction_labels
    # (1 sample, 3 labels, 1, 1, 6): a clear winner per channel, a tie (lowest index wins), a maximum exactly AT the threshold (kept:
    # only < threshold is background), a maximum below it
    p = np.zeros((1, 3, 1, 1, 6))
    p[0, :, 0, 0, 0] = (0.9, 0.1, 0.2)
    p[0, :, 0, 0, 1] = (0.1, 0.8, 0.2)
    p[0, :, 0, 0, 2] = (0.1, 0.2, 0.7)
    p[0, :, 0, 0, 3] = (0.2, 0.6, 0.6)
    p[0, :, 0, 0, 4] = (0.1, 0.5, 0.3)
    p[0, :, 0, 0, 5] = (0.4, 0.3, 0.2)
    out = get_prediction_labels(p)
    assert isinstance(out, list) and len(out) == 1 and out[0].dtype == np.uint8 and out[0].shape == (1, 1, 6)
    assert out[0].ravel().tolist() == [1, 2, 3, 2, 2, 0]
    assert get_prediction_labels(p, labels=(4, 1, 9))[0].ravel().tolist() == [4, 1, 9, 1, 1, 0]
    assert get_prediction_labels(p, threshold=0.65)[0].ravel().tolist() == [1, 2, 3, 0, 0, 0]
    two = get_prediction_labels(np.concatenate([p, p[:, ::-1]]), labels=(4, 1, 9))
    assert len(two) == 2 and two[1].ravel().tolist() == [9, 1, 4, 4, 1, 0]          # reversed channels: the tie now sits at index 0 and 1
    with pytest.raises(ValueError):
        get_prediction_labels(p, labels=(1, 2))


def test_prediction_to_image_literal_cases():
    from fetal_net.prediction import multi_class_prediction, prediction_to_image
    one = np.array([0.2, 0.5, 0.500001, 0.9]).reshape(1, 1, 1, 1, 4)
    assert prediction_to_image(one) is not None and np.array_equal(prediction_to_image(one), one[0, 0])
    # one channel: strictly above the threshold - the value exactly at it is background (the two rules differ at equality, on purpose)
    assert prediction_to_image(one, label_map=True).ravel().tolist() == [0, 0, 1, 1]
    assert prediction_to_image(one, label_map=True, labels=(7,)).ravel().tolist() == [0, 0, 7, 7]
    assert prediction_to_image(one, label_map=True, threshold=0.1).ravel().tolist() == [1, 1, 1, 1]
    many = np.zeros((1, 2, 1, 1, 3))
    many[0, :, 0, 0, 0] = (0.5, 0.1)          # exactly at the threshold with several channels: kept
    many[0, :, 0, 0, 1] = (0.3, 0.3)          # below
    many[0, :, 0, 0, 2] = (0.6, 0.6)          # tie
    assert prediction_to_image(many, label_map=True, labels=(4, 9)).ravel().tolist() == [4, 0, 4]
    parts = prediction_to_image(many)
    assert len(parts) == 2 and np.array_equal(parts[1], many[0, 1])
    assert all(np.array_equal(a, b) for a, b in zip(parts, multi_class_prediction(many)))


def test_get_multi_class_labels_numpy_form():
    from fetal_net.device_generator import get_multi_class_labels
    data = np.array([0, 1, 2, 4, 9, 3, 1, 0], dtype=np.uint8).reshape(2, 1, 2, 2, 1)
    y = get_multi_class_labels(data, 3)
    assert y.shape == (2, 3, 2, 2, 1) and y.dtype == np.int8
    assert y.reshape(2, 3, 4).tolist() == [[[0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 0]], [[0, 0, 1, 0], [0, 0, 0, 0], [0, 1, 0, 0]]]
    y = get_multi_class_labels(data, 3, labels=(4, 1, 9))
    assert y.reshape(2, 3, 4).tolist() == [[[0, 0, 0, 1], [0, 1, 0, 0], [0, 0, 0, 0]], [[0, 0, 0, 0], [0, 0, 1, 0], [1, 0, 0, 0]]]
    with pytest.raises(ValueError):
        get_multi_class_labels(data, 3, labels=(1, 2))
    with pytest.raises(ValueError):
        get_multi_class_labels(data[:, 0], 3)


def _label_maps(seed=0, shape=(24, 24, 12)):
    rs = np.random.RandomState(seed)
    t = np.zeros(shape, np.uint8)
    t[3:12, 4:14, 2:8] = 1
    t[13:21, 5:17, 3:10] = 2
    t[5:10, 16:22, 4:9] = 4
    p = np.roll(t, (1, -1, 1), axis=(0, 1, 2))
    p[rs.rand(*shape) > 0.97] = 1
    p[p == 4] = 0                                       # label 4 is absent from the prediction
    return t, p


def test_evaluate_case_labels_host_equals_evaluate_case_per_label():
    from fetal_net.evaluate import KEYS, evaluate_case, evaluate_case_labels
    t, p = _label_maps()
    rows = evaluate_case_labels(t, p, (4, 1, 2), spacing=(0.5, 0.5, 2.0), device=False)
    assert list(rows) == [4, 1, 2]
    for v, row in rows.items():
        ref = evaluate_case(t == v, p == v, spacing=(0.5, 0.5, 2.0), device=False)
        assert tuple(row) == KEYS
        for k in KEYS:
            assert row[k] == ref[k] or (np.isnan(row[k]) and np.isnan(ref[k])), (v, k)
    assert rows[4]["dice"] == 0.0 and np.isnan(rows[4]["hd"]) and np.isnan(rows[4]["precision"]) and rows[4]["volume_difference"] == -1.0
    for bad in ((), (0, 1), (1, 1), (256,), tuple(range(1, 34))):
        with pytest.raises(ValueError):
            evaluate_case_labels(t, p, bad, device=False)


def test_evaluate_cases_per_label_csv(tmp_path):
    from fetal_net.evaluate import KEYS, evaluate_case_labels, evaluate_cases
    from fetal_net.utils.nifti import save_nifti
    t, p = _label_maps()
    for name, with_label_file in (("a", True), ("b", False)):
        d = tmp_path / name
        d.mkdir()
        save_nifti(t, str(d / "truth.nii.gz"))
        if with_label_file:
            save_nifti(np.full(t.shape, 0.25), str(d / "prediction.nii.gz"))
            save_nifti(p, str(d / "prediction_labels.nii.gz"))
        else:
            save_nifti(p, str(d / "prediction.nii.gz"))
    d = tmp_path / "c"                                   # probabilities only: nothing to score per label
    d.mkdir()
    save_nifti(t, str(d / "truth.nii.gz"))
    save_nifti(np.full(t.shape, 0.25), str(d / "prediction.nii.gz"))
    out = str(tmp_path / "scores.csv")
    rows = evaluate_cases(str(tmp_path), out_csv=out, spacing=1.0, device=False, labels=(1, 2, 4))
    assert list(rows) == ["a", "b"]
    ref = evaluate_case_labels(t, p, (1, 2, 4), spacing=1.0, device=False)
    for case in rows.values():
        assert list(case) == [1, 2, 4]
        for v in case:
            assert all(case[v][k] == ref[v][k] or np.isnan(ref[v][k]) for k in KEYS)
    lines = open(out).read().strip().splitlines()
    assert lines[0].split(",") == ["subject_id", "label"] + list(KEYS) and len(lines) == 1 + 2 * 3
    assert lines[1].split(",")[:2] == ["a", "1"] and lines[6].split(",")[:2] == ["b", "4"]
    # without labels: one row per case with the binary scores, header as before
    plain = evaluate_cases(str(tmp_path), out_csv=out, spacing=1.0, device=False)
    assert list(plain) == ["a", "b", "c"] and open(out).readline().strip().split(",") == ["subject_id"] + list(KEYS)


class _Root:
    pass


class _File:
    def __init__(self, masks=None):
        self.root = _Root()
        self.root.data = [np.zeros((24, 24, 12), np.float32)]
        self.root.truth = [np.zeros((24, 24, 12), np.uint8)]
        self.root.mask = masks if masks is not None else []


def test_generator_refuses_what_several_labels_cannot_mean():
    """raised by the call itself, before any volume goes to a device (none is needed here)"""
    from fetal_net.device_generator import device_data_generator
    kw = dict(batch_size=2, patch_shape=(16, 16, 5), truth_index=2, truth_size=1, is3d=False, categorical=False)
    with pytest.raises(ValueError, match="categorical"):
        device_data_generator(_File(), [0], n_labels=3, **dict(kw, categorical=True))
    with pytest.raises(ValueError, match="mask"):
        device_data_generator(_File(masks=[np.zeros((24, 24, 12), np.float32)]), [0], n_labels=3, **kw)
    with pytest.raises(ValueError, match="mask"):
        device_data_generator(_File(), [0], n_labels=3, distance_masks=True, **kw)
    with pytest.raises(ValueError, match="labels"):
        device_data_generator(_File(), [0], n_labels=3, labels=(1, 2), **kw)
    with pytest.raises(ValueError, match="truth_size"):
        device_data_generator(_File(), [0], n_labels=3, **dict(kw, truth_size=2))
    for bad in ((1, 1, 2), (0, 1, 2), (1, 2, 256)):
        with pytest.raises(ValueError):
            device_data_generator(_File(), [0], n_labels=3, labels=bad, **kw)
    # one label: none of this is looked at - the call hands back the generator without touching its arguments
    g = device_data_generator(_File(), [0], n_labels=1, labels=(1, 2), **dict(kw, categorical=True))
    assert hasattr(g, "__next__")


def test_builders_add_label_wise_metrics_only_when_asked_and_several_labels():
    import fetal_net.model as fmodel
    base = ["loss", "binary_accuracy", "vod_coefficient"]
    names = ["label_%d_dice_coef" % i for i in range(3)]
    builders = (
        (fmodel.unet_model_3d, dict(input_shape=(1, 16, 16, 16), depth=2, n_base_filters=8)),
        (fmodel.unet_model_2d, dict(input_shape=(32, 32, 5), depth=2, n_base_filters=8)),
        (fmodel.isensee2017_model_3d, dict(input_shape=(1, 16, 16, 16), depth=3, n_base_filters=8)),
        (fmodel.isensee2017_model, dict(input_shape=(32, 32, 5), depth=3, n_base_filters=8)),
    )
    for build, kw in builders:
        m = build(n_labels=3, include_label_wise_dice_coefficients=True, **kw)
        assert m.metrics_names == base + names, build.__name__
        assert m._builder_kwargs["include_label_wise_dice_coefficients"] is True
        assert m._label_metrics() == [0, 1, 2]
        for other in (dict(n_labels=3), dict(n_labels=3, include_label_wise_dice_coefficients=False),
                      dict(n_labels=1, include_label_wise_dice_coefficients=True)):
            m = build(**dict(kw, **other))
            assert m.metrics_names == base, (build.__name__, other)
            assert "include_label_wise_dice_coefficients" not in m._builder_kwargs and m._label_metrics() == []


def test_label_wise_metric_values_from_the_sums_behind_the_sixteen():
    import fetal_net.model as fmodel
    m = fmodel.unet_model_3d(input_shape=(1, 16, 16, 16), depth=2, n_base_filters=8, n_labels=2, include_label_wise_dice_coefficients=True)
    sums = np.zeros(16 + 6)
    sums[:8] = (3, 5, 4, 2, 5, 3, 90, 100)
    sums[16:] = (1.5, 2, 3, 0, 0, 0)
    logs = m._batch_logs(sums)
    assert list(logs) == m.metrics_names
    assert logs["label_0_dice_coef"] == (2 * 1.5 + 1) / (2 + 3 + 1) and logs["label_1_dice_coef"] == 1.0
