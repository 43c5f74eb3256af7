"""fetal_net.utils.create_distance_masks on the host path (scipy): the reference's formula, its folder loop and the data-file form."""
import os

import numpy as np
import pytest
import scipy.ndimage


def subjects():
    rs = np.random.RandomState(2)
    shapes = [(12, 10, 6), (9, 11, 5)]
    truths = [(scipy.ndimage.gaussian_filter(rs.randn(*s), 1.2) > 0.05).astype(np.uint8) for s in shapes]
    assert all(t.any() and not t.all() for t in truths)
    return [rs.randn(*s) for s in shapes], truths


def formula(mask, sampling):
    """the reference script's three lines"""
    dists = scipy.ndimage.distance_transform_edt(mask, sampling=sampling)
    dists_inv = scipy.ndimage.distance_transform_edt(1 - mask, sampling=sampling)
    return dists + dists_inv


def test_module_constants_are_the_reference_scripts():
    from fetal_net.utils import create_distance_masks as C
    assert C.sampling == (0.4, 0.4, 3.0) and C.ext == ".gz" and C.dataset_folder == ""


def test_create_distance_mask_is_the_reference_formula():
    from fetal_net.utils.create_distance_masks import create_distance_mask, sampling
    for t in subjects()[1]:
        got = create_distance_mask(t, device=False)
        assert got.dtype == np.float64
        np.testing.assert_array_equal(got, formula(t, sampling))
        np.testing.assert_array_equal(create_distance_mask(t, sampling=(1.0, 2.0, 0.5), device=False), formula(t, (1.0, 2.0, 0.5)))
        # nonzero means foreground, whatever the label's dtype or value
        np.testing.assert_array_equal(create_distance_mask(t.astype(np.float32) * 7, device=False), got)


def test_create_distance_masks_over_a_folder(tmp_path, capsys):
    from fetal_net.utils.create_distance_masks import create_distance_masks, sampling
    from fetal_net.utils.nifti import load_nifti, save_nifti
    truths = subjects()[1]
    for name, t in zip(("subj_a", "subj_b"), truths):
        os.makedirs(str(tmp_path / name))
        save_nifti(t, str(tmp_path / name / "truth.nii.gz"))
    os.makedirs(str(tmp_path / "no_truth_here"))
    written = create_distance_masks(dataset_folder=str(tmp_path), device=False)
    assert written == [str(tmp_path / n / "dists.nii.gz") for n in ("subj_a", "subj_b")]
    assert capsys.readouterr().out.split() == ["subj_a", "subj_b"]
    for path, t in zip(written, truths):
        got, affine = load_nifti(path, return_affine=True)
        assert got.dtype == np.float64
        np.testing.assert_array_equal(got, formula(t, sampling))
        np.testing.assert_array_equal(affine, np.eye(4))
    assert create_distance_masks(dataset_folder=str(tmp_path), ext="", device=False) == []          # no uncompressed truth.nii there


def test_add_distance_masks_round_trip(tmp_path):
    from fetal_net.data import open_data_file, write_plain_data_file
    from fetal_net.utils.create_distance_masks import add_distance_masks, sampling
    vols, truths = subjects()
    ids = [b"subj_a", b"subj_b"]
    src, dst = str(tmp_path / "data.h5"), str(tmp_path / "data_masks.h5")
    write_plain_data_file(src, vols, truths, subject_ids=ids)
    assert add_distance_masks(src, dst, device=False) == dst
    with open_data_file(dst) as f:
        assert "mask" in f.root and len(f.root.mask) == len(f.root.data) == 2
        for i in range(2):
            np.testing.assert_array_equal(f.root.data[i], vols[i])
            np.testing.assert_array_equal(f.root.truth[i], truths[i])
            assert f.root.mask[i].shape == truths[i].shape and f.root.mask[i].dtype == np.float64
            np.testing.assert_array_equal(f.root.mask[i], formula(truths[i], sampling))
        assert list(f.root.subject_ids) == ids
    with pytest.raises(ValueError):
        add_distance_masks(dst, str(tmp_path / "again.h5"), device=False)
    assert not os.path.exists(str(tmp_path / "again.h5"))
