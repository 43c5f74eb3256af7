"""fetal_net.evaluate on the host (device=False): hand-computed surface distances, the reference's Dice expression, the loop over case
folders and its CSV."""
import csv
import math
import os

import numpy as np
import pytest
from scipy import ndimage

from fetal_net import evaluate as E
from fetal_net.utils.nifti import save_nifti


def surface_count(mask, connectivity):
    st = ndimage.generate_binary_structure(3, connectivity)
    return int((mask ^ ndimage.binary_erosion(mask, structure=st, iterations=1)).sum())


def test_two_single_voxels_are_their_distance_apart():
    t, p = np.zeros((3, 3, 6), bool), np.zeros((3, 3, 6), bool)
    t[1, 1, 1] = True
    p[1, 1, 4] = True
    r = E.evaluate_case(t, p, device=False)
    assert (r["hd"], r["hd95"], r["assd"]) == (3.0, 3.0, 3.0)
    r = E.evaluate_case(t, p, spacing=(1, 1, 2), device=False)
    assert (r["hd"], r["hd95"], r["assd"]) == (6.0, 6.0, 6.0)
    assert r["dice"] == 0.0 and r["vod"] == 0.0 and r["volume_truth"] == 2.0 and r["volume_prediction"] == 2.0
    assert r["volume_difference"] == 0.0 and r["sensitivity"] == 0.0 and r["precision"] == 0.0
    assert list(r) == list(E.KEYS)


@pytest.mark.parametrize("connectivity", [1, 2, 3])
def test_a_cube_of_27_has_26_surface_voxels(connectivity):
    inside = np.zeros((5, 5, 5), bool)
    inside[1:4, 1:4, 1:4] = True
    assert surface_count(inside, connectivity) == 26
    assert surface_count(np.ones((3, 3, 3), bool), connectivity) == 26       # the volume's faces count as background
    # and through the module: against the centre voxel every one of the 26 is 1, sqrt(2) or sqrt(3) away, the centre is 1 from the nearest
    centre = np.zeros((5, 5, 5), bool)
    centre[2, 2, 2] = True
    r = E.evaluate_case(inside, centre, connectivity=connectivity, device=False)
    d = np.array([1.0] * 6 + [math.sqrt(2)] * 12 + [math.sqrt(3)] * 8)
    assert r["hd"] == math.sqrt(3)
    assert r["assd"] == np.mean((d.mean(), 1.0))
    assert r["hd95"] == np.percentile(np.hstack((d, [1.0])), 95)
    assert r["sensitivity"] == 1 / 27 and r["precision"] == 1.0 and r["volume_difference"] == (1 - 27) / 27


def test_identical_masks():
    m = np.random.RandomState(0).rand(9, 8, 7) < 0.4
    for connectivity in (1, 2, 3):
        r = E.evaluate_case(m, m.copy(), spacing=(0.4, 0.4, 3.0), connectivity=connectivity, device=False)
        assert (r["hd"], r["hd95"], r["assd"]) == (0.0, 0.0, 0.0)
        assert r["dice"] == 1.0 and r["vod"] == 1.0 and r["sensitivity"] == 1.0 and r["precision"] == 1.0 and r["volume_difference"] == 0.0
        assert r["volume_truth"] == r["volume_prediction"] == int(m.sum()) * float(np.prod((0.4, 0.4, 3.0)))


def reference_dice(truth, prediction):
    return 2 * np.sum(truth * prediction) / (np.sum(truth) + np.sum(prediction))      # reference fetal/evaluate.py:17


def test_dice_coefficient_is_the_reference_expression():
    assert E.get_fetal_envelope_mask(np.array([-1.0, 0.0, 0.2, 3.0])).tolist() == [False, False, True, True]
    rs = np.random.RandomState(1)
    for shape, pt, pp in (((7, 5, 3), 0.5, 0.5), ((16, 16, 8), 0.1, 0.9), ((3, 3, 3), 0.9, 0.05), ((20, 11, 13), 0.3, 0.33)):
        t, p = rs.rand(*shape) < pt, rs.rand(*shape) < pp
        np.testing.assert_array_equal(E.dice_coefficient(t, p), reference_dice(t, p))
        np.testing.assert_array_equal(E.evaluate_case(t, p, device=False)["dice"], reference_dice(t, p))
    data_t, data_p = rs.randn(6, 6, 6), rs.randn(6, 6, 6)
    np.testing.assert_array_equal(E.dice_coefficient(E.get_fetal_envelope_mask(data_t), E.get_fetal_envelope_mask(data_p)),
                                  reference_dice(data_t > 0, data_p > 0))


def test_empty_masks_give_nan_not_an_exception():
    empty = np.zeros((4, 5, 6), bool)
    some = empty.copy()
    some[1:3, 2, 3] = True
    assert math.isnan(E.dice_coefficient(empty, empty))
    r = E.evaluate_case(empty, empty, device=False)
    assert all(math.isnan(r[k]) for k in ("dice", "vod", "volume_difference", "sensitivity", "precision", "hd", "hd95", "assd"))
    assert r["volume_truth"] == 0.0 and r["volume_prediction"] == 0.0
    for t, p in ((empty, some), (some, empty)):
        assert E.dice_coefficient(t, p) == 0.0
        r = E.evaluate_case(t, p, device=False)
        assert r["dice"] == 0.0 and r["vod"] == 0.0
        assert all(math.isnan(r[k]) for k in ("hd", "hd95", "assd"))
    r = E.evaluate_case(empty, some, device=False)
    assert r["volume_difference"] == math.inf and math.isnan(r["sensitivity"]) and r["precision"] == 0.0


def test_bad_arguments():
    m = np.ones((3, 3, 3), bool)
    for kw in ({"connectivity": 0}, {"connectivity": 4}, {"spacing": (1, 2)}, {"spacing": (1, 0, 1)}):
        with pytest.raises(ValueError):
            E.evaluate_case(m, m, device=False, **kw)
    with pytest.raises(ValueError):
        E.evaluate_case(m, np.ones((3, 3, 4), bool), device=False)
    with pytest.raises(ValueError):
        E.evaluate_case(m[0], m[0], device=False)


def write_cases(root):
    """two case folders as run_validation_cases writes them (one with a non-identity diagonal affine, its prediction as probabilities),
    a folder without a prediction and a plain file -> {subject: (truth mask, prediction mask, spacing)}"""
    rs = np.random.RandomState(2)
    x, y, z = np.meshgrid(np.arange(12), np.arange(14), np.arange(9), indexing="ij")
    truth = ((x - 6) / 4.0) ** 2 + ((y - 6) / 5.0) ** 2 + ((z - 4) / 3.0) ** 2 < 1
    prob = np.clip(1.2 - (((x - 7) / 4.0) ** 2 + ((y - 7) / 4.0) ** 2 + ((z - 4) / 3.5) ** 2) + 0.05 * rs.randn(12, 14, 9), 0, 1)
    labels = (((x - 5) / 3.0) ** 2 + ((y - 8) / 5.0) ** 2 + ((z - 5) / 3.0) ** 2 < 1).astype(np.uint8)
    spacing = (0.5, 0.75, 3.0)                               # exact in the float32 the affine is stored in
    for name in ("case_a", "case_b", "case_c"):
        os.makedirs(os.path.join(root, name))
    save_nifti(truth.astype(np.uint8), os.path.join(root, "case_a", "truth.nii.gz"))
    save_nifti(labels, os.path.join(root, "case_a", "prediction.nii.gz"))
    save_nifti(truth.astype(np.uint8), os.path.join(root, "case_b", "truth.nii.gz"), np.diag(spacing + (1.0,)))
    save_nifti(prob.astype(np.float32), os.path.join(root, "case_b", "prediction.nii.gz"), np.diag(spacing + (1.0,)))
    save_nifti(truth.astype(np.uint8), os.path.join(root, "case_c", "truth.nii.gz"))
    open(os.path.join(root, "notes.txt"), "w").write("not a case\n")
    return {"case_a": (truth, labels > 0, (1.0, 1.0, 1.0)), "case_b": (truth, prob.astype(np.float32) > 0.5, spacing)}


def same_row(got, want):
    assert list(got) == list(want)
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


def test_evaluate_cases_round_trip(tmp_path):
    cases = write_cases(str(tmp_path))
    out_csv = str(tmp_path / "scores.csv")
    rows = E.evaluate_cases(str(tmp_path), out_csv=out_csv, device=False)
    assert list(rows) == ["case_a", "case_b"]                # case_c has no prediction.nii.gz, notes.txt is no folder: both skipped
    for name, (t, p, spacing) in cases.items():
        same_row(rows[name], E.evaluate_case(t, p, spacing=spacing, device=False))
        assert 0 < rows[name]["dice"] < 1 and rows[name]["hd"] > rows[name]["hd95"] > rows[name]["assd"] > 0
    with open(out_csv, newline="") as f:
        lines = list(csv.reader(f))
    assert lines[0] == ["subject_id"] + list(E.KEYS)
    assert [l[0] for l in lines[1:]] == ["case_a", "case_b"]
    for l in lines[1:]:
        same_row(dict(zip(E.KEYS, (float(v) for v in l[1:]))), dict(rows[l[0]]))
    # a spacing given by the caller wins over the affine's
    forced = E.evaluate_cases(str(tmp_path), spacing=(2.0, 2.0, 2.0), device=False)
    same_row(forced["case_b"], E.evaluate_case(cases["case_b"][0], cases["case_b"][1], spacing=(2.0, 2.0, 2.0), device=False))


def test_a_folder_without_a_prediction_is_skipped(tmp_path):
    os.makedirs(str(tmp_path / "only_truth"))
    save_nifti(np.ones((3, 3, 3), np.uint8), str(tmp_path / "only_truth" / "truth.nii.gz"))
    assert E.evaluate_cases(str(tmp_path), device=False) == {}
    assert "skipped" in E.evaluate_cases.__doc__
