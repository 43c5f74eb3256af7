"""From a folder of scans to a data file and to generators, without a GPU: the host form of fetal_net.data.write_data_to_file and
fetal_net.normalize against what the reference's own code made of the same files (tests/golden/dataset_golden.npz, written by
tests/golden/make_dataset_fixture.py), the argument surface and the split of fetal_net.generator, and fetal/utils.py."""
import inspect
import json
import os
import pickle
import random
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

SCALES = [None, (0.5, 0.5, 1)]
PREPROCS = [None, "laplace_norm"]
N_SUBJECTS = 3


def zoom_bound(want):
    """the bound tests/test_gpu_resample.py holds for zoom_f64"""
    return 1e-12 * max(1.0, float(np.abs(want).max()))


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(GOLDEN, "dataset_golden.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def scans(golden, tmp_path_factory):
    """the fixture's inputs as NIfTI files -> one (volume, truth, mask) tuple of paths per subject"""
    from fetal_net.utils.nifti import save_nifti
    d = tmp_path_factory.mktemp("dataset_scans")
    files = []
    for i in range(N_SUBJECTS):
        names = tuple(str(d / ("s%d_%s.nii.gz" % (i, k))) for k in ("volume", "truth", "mask"))
        for key, p in zip(("vol", "truth", "maskin"), names):
            save_nifti(golden["%s_%d" % (key, i)], p)
        files.append(names)
    return files


def check_against_golden(golden, f, si, pi, mi, normalize, mean, std):
    from fetal_net.data import PlainDataFile
    case, base = "s%dp%dm%d" % (si, pi, mi), "s%dp%dm0" % (si, pi)
    kind = {"all": "all", "each": "each"}.get(normalize, "data")
    assert isinstance(f, PlainDataFile) and len(f.root.data) == N_SUBJECTS
    for i in range(N_SUBJECTS):
        want, got = golden["%s_%s_%d" % (base, kind, i)], f.root.data[i]
        assert got.dtype == np.float64 and got.shape == want.shape
        if si == 0:
            np.testing.assert_array_equal(got, want)
        else:
            assert np.abs(got - want).max() <= zoom_bound(want)
        truth = f.root.truth[i]
        assert truth.dtype == np.uint8
        np.testing.assert_array_equal(truth, golden["%s_truth_%d" % (case, i)])
        if mi:
            assert f.root.mask[i].dtype == np.float64
            np.testing.assert_array_equal(f.root.mask[i], golden["%s_mask_%d" % (case, i)])
    if not mi:
        assert "mask" not in f.root
    if normalize == "all":
        want_mean, want_std = float(golden[base + "_mean"]), float(golden[base + "_std"])
        if si == 0:
            assert float(mean) == want_mean and float(std) == want_std
        else:
            assert abs(float(mean) - want_mean) <= zoom_bound(want_mean) and abs(float(std) - want_std) <= zoom_bound(want_std)
    else:
        assert mean is None and std is None


@pytest.mark.parametrize("normalize", ["all", "each", None])
@pytest.mark.parametrize("mi", [0, 1])
@pytest.mark.parametrize("pi", [0, 1])
@pytest.mark.parametrize("si", [0, 1])
def test_host_form_reproduces_the_reference(golden, scans, tmp_path, si, pi, mi, normalize):
    from fetal_net.data import open_data_file, write_data_to_file
    out = str(tmp_path / "data.h5")
    files = [s if mi else s[:2] for s in scans]
    kw = dict(subject_ids=["a", "b", "c"], normalize=normalize, scale=SCALES[si], preproc=PREPROCS[pi], device=False)
    if si and mi:
        with pytest.raises(ValueError, match="scale with mask"):
            write_data_to_file(files, out, **kw)
        assert not os.path.exists(out)
        return
    path, (mean, std) = write_data_to_file(files, out, **kw)
    assert path == out and not os.path.exists(out + ".tmp")
    with open_data_file(out) as f:
        check_against_golden(golden, f, si, pi, mi, normalize, mean, std)
        assert f.root.subject_ids == [b"a", b"b", b"c"]


def test_a_preproc_callable_is_the_named_filter(golden, scans, tmp_path):
    import fetal_net.preprocess
    from fetal_net.data import open_data_file, write_data_to_file
    out = str(tmp_path / "data.h5")
    _, (mean, std) = write_data_to_file([s[:2] for s in scans], out, preproc=fetal_net.preprocess.laplace_norm, device=False)
    with open_data_file(out) as f:
        check_against_golden(golden, f, 0, 1, 0, "all", mean, std)
        assert "subject_ids" not in f.root
    # a caller's own callable sees the volume as a float64 array
    seen = []

    def own(d):
        seen.append((type(d), d.dtype))
        return d * 2
    write_data_to_file([s[:2] for s in scans], out, normalize=False, preproc=own, device=False)
    assert seen == [(np.ndarray, np.float64)] * N_SUBJECTS
    with open_data_file(out) as f:
        np.testing.assert_array_equal(f.root.data[1], golden["vol_1"] * 2)


def test_normalize_data_storage_host_forms(golden):
    from fetal_net import normalize as N
    data = [golden["s0p0m0_data_%d" % i].copy(order="K") for i in range(N_SUBJECTS)]        # memory order kept: it decides numpy's summation order
    storage, mean, std = N.normalize_data_storage(data, device=False)
    assert storage is data and float(mean) == float(golden["s0p0m0_mean"]) and float(std) == float(golden["s0p0m0_std"])
    for i in range(N_SUBJECTS):
        np.testing.assert_array_equal(storage[i], golden["s0p0m0_all_%d" % i])
    data = [golden["s0p0m0_data_%d" % i].copy(order="K") for i in range(N_SUBJECTS)]        # memory order kept: it decides numpy's summation order
    storage, mean, std = N.normalize_data_storage_each(data, device=False)
    assert storage is data and mean is None and std is None
    for i in range(N_SUBJECTS):
        np.testing.assert_array_equal(storage[i], golden["s0p0m0_each_%d" % i])
    from fetal_net.pipeline import normalize_data
    assert N.normalize_data is normalize_data
    # a constant volume: 0 / 0, as numpy gives it
    with np.errstate(invalid="ignore"):
        const, _, _ = N.normalize_data_storage_each([np.full((3, 4, 5), 7.25)], device=False)
    assert np.isnan(const[0]).all()


def test_refusals(scans, tmp_path):
    from fetal_net.data import write_data_to_file
    out = str(tmp_path / "data.h5")
    for device in (False, True):               # refused before anything is read or uploaded
        with pytest.raises(ValueError, match="got 1 files"):
            write_data_to_file([s[:1] for s in scans], out, device=device)
        with pytest.raises(ValueError, match="got 4 files"):
            write_data_to_file([s + s[:1] for s in scans], out, device=device)
        with pytest.raises(ValueError, match="scale with mask"):
            write_data_to_file(scans, out, scale=(0.5, 0.5, 1), device=device)
        with pytest.raises(ValueError, match="normalize must be"):
            write_data_to_file([s[:2] for s in scans], out, normalize="some", device=device)
        with pytest.raises(ValueError, match="preproc"):
            write_data_to_file([s[:2] for s in scans], out, preproc="sharpen", device=device)
    assert os.listdir(str(tmp_path)) == []


def test_a_failed_build_leaves_no_file(scans, tmp_path, monkeypatch):
    from fetal_net import data as D
    out = str(tmp_path / "data.h5")
    calls = []

    def breaks_on_the_second(d):
        calls.append(1)
        if len(calls) == 2:
            raise RuntimeError("filter failed")
        return d
    with pytest.raises(RuntimeError, match="filter failed"):
        D.write_data_to_file([s[:2] for s in scans], out, preproc=breaks_on_the_second, device=False)
    files = [s[:2] for s in scans]
    files[2] = (files[2][0], str(tmp_path / "missing.nii.gz"))
    with pytest.raises(OSError):
        D.write_data_to_file(files, out, device=False)
    assert os.listdir(str(tmp_path)) == []
    # the write itself fails midway: the temporary file goes too
    from fetal_net.utils import hdf5
    real = hdf5.File.create_group

    def create_group(self, name):
        if name == "truth":
            raise OSError("disk full")
        return real(self, name)
    monkeypatch.setattr(hdf5.File, "create_group", create_group)
    with pytest.raises(OSError, match="disk full"):
        D.write_data_to_file([s[:2] for s in scans], out, device=False)
    assert os.listdir(str(tmp_path)) == []


def test_generator_signature_is_the_reference_one():
    from fetal_net.generator import get_training_and_validation_generators as fn
    import fetal_net.generator as G
    with open(os.path.join(GOLDEN, "signatures_golden.json")) as f:
        sig = json.load(f)["get_training_and_validation_generators"]
    spec = inspect.getfullargspec(fn)
    assert spec.args == sig["args"] and spec.varkw == sig["varkw"] and spec.varargs is None
    assert sorted(spec.kwonlyargs) == ["device", "distance_masks", "noise_seed", "prefetch"]
    assert spec.kwonlydefaults == {"device": "cuda", "noise_seed": 0, "distance_masks": None, "prefetch": 0}
    # the reference's defaults (generator.py:58-67)
    want = dict(patch_shape=None, data_split=0.8, overwrite=False, labels=None, augment=None, validation_batch_size=None,
                skip_blank_train=True, skip_blank_val=False, truth_index=-1, truth_size=1, truth_downsample=None, truth_crop=True,
                patches_per_epoch=1, categorical=True, is3d=False, prev_truth_index=None, prev_truth_size=None,
                drop_easy_patches_train=False, drop_easy_patches_val=False, samples_pad=3, val_augment=None)
    assert dict(zip(spec.args[-len(spec.defaults):], spec.defaults)) == want
    from fetal_net import data, device_generator
    assert G.get_validation_split is data.get_validation_split and G.split_list is data.split_list
    assert G.random_list_generator is device_generator.random_list_generator and G.list_generator is device_generator.list_generator


def test_split_and_step_counts_need_no_gpu(golden, scans, tmp_path, capsys):
    from fetal_net.data import get_validation_split, open_data_file, write_data_to_file
    from fetal_net.generator import get_training_and_validation_generators
    out = str(tmp_path / "data.h5")
    five = [s[:2] for s in scans] + [scans[0][:2], scans[1][:2]]
    write_data_to_file(five, out, subject_ids=["s%d" % i for i in range(5)], normalize="each", device=False)
    keys = [str(tmp_path / n) for n in ("train.pkl", "val.pkl", "test.pkl")]
    with open_data_file(out) as f:
        random.seed(5)
        tg, vg, nt, nv = get_training_and_validation_generators(f, 3, 1, keys[0], keys[1], keys[2], patch_shape=(8, 8, 4), data_split=0.75,
                                                                patches_per_epoch=14, is3d=True, truth_size=4, truth_index=0)
        assert (nt, nv) == (4, 4)                                 # validation_batch_size defaults to batch_size
        lists = [pickle.load(open(k, "rb")) for k in keys]
        random.seed(5)
        want = get_validation_split(f, str(tmp_path / "t2"), str(tmp_path / "v2"), str(tmp_path / "e2"), data_split=0.75)
        assert tuple(lists) == tuple(want) and sorted(sum(lists, [])) == list(range(5))
        assert len(lists[0]) == 3 and len(lists[1]) == 1 and len(lists[2]) == 1
        printed = capsys.readouterr().out
        assert "Training: %r" % ["s%d" % i for i in lists[0]] in printed and "Test: %r" % ["s%d" % i for i in lists[2]] in printed
        # nothing was uploaded: both generators wait for their first batch, and will share one DeviceDataFile
        assert tg.device_data_file is None and vg.device_data_file is None and tg._shared is vg._shared
        assert tg._kwargs["noise_seed"] == 0 and vg._kwargs["noise_seed"] == 1
        # an existing split is re-loaded, and validation_batch_size counts the validation steps
        _, _, nt, nv = get_training_and_validation_generators(f, 3, 1, keys[0], keys[1], keys[2], patch_shape=(8, 8, 4),
                                                              patches_per_epoch=14, validation_batch_size=7, noise_seed=4)
        assert (nt, nv) == (4, 2) and [pickle.load(open(k, "rb")) for k in keys] == lists
        with pytest.raises(NotImplementedError):
            get_training_and_validation_generators(f, 3, 1, keys[0], keys[1], keys[2], patch_shape=(8, 8, 4), truth_downsample=2)


def make_scans_dir(root, golden, ext=".gz", masks=()):
    from fetal_net.utils.nifti import save_nifti
    for name, i in (("fetus_b", 1), ("fetus_a", 0), ("fetus_c", 2)):
        os.makedirs(os.path.join(root, name))
        save_nifti(golden["vol_%d" % i], os.path.join(root, name, "volume.nii" + ext))
        save_nifti(golden["truth_%d" % i], os.path.join(root, name, "truth.nii" + ext))
        for m in masks:
            save_nifti(golden["maskin_%d" % i], os.path.join(root, name, m + ".nii" + ext))


def test_fetch_training_data_files(golden, tmp_path):
    from fetal.utils import fetch_training_data_files
    root = str(tmp_path / "scans")
    make_scans_dir(root, golden)
    cfg = {"scans_dir": root, "training_modalities": ["volume"], "weight_mask": None, "ext": ".gz"}
    files, ids = fetch_training_data_files(cfg, return_subject_ids=True)
    assert ids == ["fetus_a", "fetus_b", "fetus_c"]
    assert files == [(os.path.join(root, s, "volume.nii.gz"), os.path.join(root, s, "truth.nii.gz")) for s in ids]
    assert fetch_training_data_files(cfg) == files
    cfg.update(weight_mask=["dists"], ext="", training_modalities=["t1", "t2"])
    files = fetch_training_data_files(cfg)
    assert files[1] == tuple(os.path.join(root, "fetus_b", n + ".nii") for n in ("t1", "t2", "truth", "dists"))


@pytest.mark.parametrize("normalization", ["all", "each"])
def test_create_data_file_and_norm_params(golden, tmp_path, normalization):
    from fetal.utils import create_data_file, get_last_model_path
    from fetal_net.data import load_norm_params, open_data_file
    root = str(tmp_path / "scans")
    make_scans_dir(root, golden, masks=("dists",))
    cfg = {"scans_dir": root, "training_modalities": ["volume"], "weight_mask": ["dists"], "ext": ".gz", "base_dir": str(tmp_path),
           "data_file": str(tmp_path / "fetal_data.h5"), "normalization": normalization, "preproc": "laplace_norm"}
    mean, std = create_data_file(cfg, device=False)
    got = load_norm_params(str(tmp_path))
    if normalization == "all":
        assert got == (float(mean), float(std)) and got == (float(golden["s0p1m0_mean"]), float(golden["s0p1m0_std"]))
    else:
        assert got == (None, None) and mean is None and std is None
    with open_data_file(cfg["data_file"]) as f:
        assert f.root.subject_ids == [b"fetus_a", b"fetus_b", b"fetus_c"]
        check_against_golden(golden, f, 0, 1, 1, normalization, mean, std)
    for k, name in enumerate(("m-epoch01.h5", "m-epoch03.h5", "m-epoch02.h5")):
        p = str(tmp_path / name)
        open(p, "w").close()
        os.utime(p, (1000 + k, 1000 + k))
    assert get_last_model_path(str(tmp_path / "m")) == str(tmp_path / "m-epoch02.h5")


def test_moments_prototypes_are_declared_and_bound():
    from fmri_hip._lib import SIGNATURES
    import ctypes as C
    with open(os.path.join(ROOT, "include", "fmri_hip.h")) as f:
        header = f.read()
    assert re.search(r"^int64_t fmri_moments_workspace_bytes\(void\);", header, re.M)
    assert re.search(r"^int fmri_moments_f64\(const double\* src, int64_t n, double\* out5, int64_t\* nan_count, void\* workspace, "
                     r"fmri_stream_t stream\);", header, re.M)
    assert SIGNATURES["fmri_moments_workspace_bytes"] == []
    assert SIGNATURES["fmri_moments_f64"] == [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
