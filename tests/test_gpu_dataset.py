"""The first stage of a training run on the device: fmri_moments_f64 (csrc/postprocess.hip; fmri_hip.ops.moments_f64) against exact
arbiters, the device form of fetal_net.data.write_data_to_file against the host form, and the whole chain scans folder ->
create_data_file -> get_training_and_validation_generators -> train_model at the smallest sizes.

Bounds of the moments (u = 2^-53), derived, not tuned.  A compensated (Neumaier) lane sum is within about 2u * sum|x| of the exact sum,
and every combine of the fixed tree - 6 levels in the wave, 2 across the waves of a workgroup, up to 16 across workgroups - adds at
most one rounding of that size:
  sum:  |sum_dev - fsum(x)| <= 32 u sum|x|              (math.fsum is exact);   mean: the same bound divided by n
  std:  |std_dev - std_exact| <= 64 u std_exact         std_exact in np.longdouble around the exact mean; covers the per-term subtract and
        square, the tree, the division and the root.  The inputs keep std / |mean| >= 1e-6, so the rounding of the mean the second pass
        is taken around moves the result by (u |mean| / std)^2 <= 1e-20 relative.
numpy's own pairwise sums stay inside both on every input here.  Min and max are selections: identical.  Integer-valued volumes have
exactly representable partial sums: sum and mean identical to numpy's.
Every test prints its figures (`pytest -s`).
"""
import functools
import math
import os
import random

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
SHAPES = [(1,), (5, 3, 2), (255,), (256,), (257,), (37, 29, 23), (64, 64, 40)]          # n = 1 ... 163,840 (40 workgroups)
KINDS = ["uniform", "normal", "offset"]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the GPU box"
    from fmri_hip import ops as o
    return o


@functools.lru_cache(maxsize=None)
def volume(shape, kind):
    rs = np.random.RandomState(sum(shape) + 13 * len(kind))
    if kind == "uniform":
        v = rs.rand(*shape) * 255
    elif kind == "normal":
        v = rs.randn(*shape) * 3 + 0.5
    else:
        v = rs.randn(*shape) * 10 + 1e6                                               # std / |mean| = 1e-5
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def arbiters(shape, kind):
    """(exact sum, sum|x|, std in long double around the exact mean) - computed once per input"""
    x = volume(shape, kind).ravel()
    total, mag = math.fsum(x), math.fsum(np.abs(x))
    d = x.astype(np.longdouble) - np.longdouble(total) / x.size
    return total, mag, float(np.sqrt((d * d).sum() / x.size))


def raw_moments(ops, t):
    """{mean, std, min, max, sum} and the NaN count as the entry point leaves them"""
    host = ops.moments_f64_enqueue(t).cpu()
    return host[:5].numpy().copy(), int(host[5:].view(torch.int64).item())


def check_moments(ops, t, shape, kind, what):
    x = volume(shape, kind)
    total, mag, std_exact = arbiters(shape, kind)
    out, nans = raw_moments(ops, t)
    mean, std, lo, hi, s = (float(v) for v in out)
    print("%s %s %s: sum error %.2f u sum|x|, mean error %.2f u sum|x|/n, std error %.2f u std (numpy: %.2f, %.2f)" % (
        what, kind, shape, abs(s - total) / (U * mag), abs(mean - total / x.size) / (U * mag / x.size),
        abs(std - std_exact) / (U * std_exact) if std_exact else 0.0, abs(float(x.mean()) - total / x.size) / (U * mag / x.size),
        abs(float(x.std()) - std_exact) / (U * std_exact) if std_exact else 0.0))
    assert nans == 0 and lo == x.min() and hi == x.max()
    assert abs(s - total) <= 32 * U * mag
    assert abs(mean - total / x.size) <= 32 * U * mag / x.size
    assert abs(std - std_exact) <= 64 * U * std_exact
    assert ops.moments_f64(t) == (mean, std, lo, hi)
    return out


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_moments_against_exact_arbiters(ops, shape, kind):
    check_moments(ops, torch.from_numpy(volume(shape, kind).copy()).cuda(), shape, kind, "moments")


@pytest.mark.parametrize("shape", [(257,), (37, 29, 23)], ids=lambda s: "x".join(map(str, s)))
def test_moments_of_a_view_that_is_not_16_byte_aligned(ops, shape):
    x = volume(shape, "offset")
    store = torch.zeros(x.size + 1, dtype=torch.float64, device="cuda")
    view = store[1:].view(*shape)
    view.copy_(torch.from_numpy(x.copy()))
    assert view.data_ptr() % 16 == 8 and view.is_contiguous()
    got = check_moments(ops, view, shape, "offset", "unaligned view")
    aligned, _ = raw_moments(ops, torch.from_numpy(x.copy()).cuda())
    assert got.tobytes() == aligned.tobytes()                 # the order of the sums does not depend on how the pairs are loaded


def test_moments_special_values(ops):
    x = volume((37, 29, 23), "normal").copy()
    x[11, 7, 5] = np.nan
    got = ops.moments_f64(torch.from_numpy(x).cuda())
    assert len(got) == 4 and all(math.isnan(v) for v in got)
    out, nans = raw_moments(ops, torch.from_numpy(x).cuda())
    assert nans == 1 and out[2] == np.nanmin(x) and out[3] == np.nanmax(x)
    for shape in [(1,), (37, 29, 23), (64, 64, 40)]:
        const = torch.full(shape, 7.25, dtype=torch.float64, device="cuda")              # dyadic: n * 7.25 is exact
        assert ops.moments_f64(const) == (7.25, 0.0, 7.25, 7.25)
    for shape in [(5, 3, 2), (37, 29, 23), (64, 64, 40)]:
        ints = np.random.RandomState(3).randint(0, 4096, size=shape).astype(np.float64)
        out, _ = raw_moments(ops, torch.from_numpy(ints).cuda())
        assert out[4] == ints.sum() and out[0] == ints.mean() and out[2] == ints.min() and out[3] == ints.max()
    with pytest.raises(ValueError):
        ops.moments_f64(torch.zeros((4, 4, 4), dtype=torch.float32, device="cuda"))
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.moments_f64(torch.zeros((4, 4, 4), dtype=torch.float64, device="cuda")[:, :, ::2])


def test_moments_are_the_same_bits_on_every_call_and_stream(ops):
    t = torch.from_numpy(volume((64, 64, 40), "offset").copy()).cuda()
    first, _ = raw_moments(ops, t)
    second, _ = raw_moments(ops, t)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = ops.moments_f64_enqueue(t)
    side.synchronize()
    assert first.tobytes() == second.tobytes() == out.cpu()[:5].numpy().tobytes()


def test_moments_entry_point_refuses_bad_arguments(ops):
    from fmri_hip._lib import lib
    L = lib()
    t = torch.ones(64, dtype=torch.float64, device="cuda")
    out = torch.full((6,), -3.0, dtype=torch.float64, device="cuda")
    ws = torch.empty(L.fmri_moments_workspace_bytes(), dtype=torch.uint8, device="cuda")
    E_SHAPE = -1
    p, o, n, w = t.data_ptr(), out.data_ptr(), out.data_ptr() + 40, ws.data_ptr()
    assert L.fmri_moments_f64(0, 64, o, n, w, 0) == E_SHAPE
    assert L.fmri_moments_f64(p, 64, 0, n, w, 0) == E_SHAPE
    assert L.fmri_moments_f64(p, 64, o, 0, w, 0) == E_SHAPE
    assert L.fmri_moments_f64(p, 64, o, n, 0, 0) == E_SHAPE
    assert L.fmri_moments_f64(p, 0, o, n, w, 0) == E_SHAPE
    assert L.fmri_moments_f64(p, -5, o, n, w, 0) == E_SHAPE
    torch.cuda.synchronize()
    assert (out[:5] == -3.0).all()                            # nothing was launched
    assert L.fmri_moments_workspace_bytes() >= 2048 * 16


# ------------------------------------------------------------------------------------------------------ write_data_to_file on the device
SCALES = [None, (0.5, 0.5, 1)]
PREPROCS = [None, "laplace_norm"]
N_SUBJECTS = 3


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(GOLDEN, "dataset_golden.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def scans(golden, tmp_path_factory):
    from fetal_net.utils.nifti import save_nifti
    d = tmp_path_factory.mktemp("dataset_scans")
    files = []
    for i in range(N_SUBJECTS):
        names = tuple(str(d / ("s%d_%s.nii.gz" % (i, k))) for k in ("volume", "truth", "mask"))
        for key, p in zip(("vol", "truth", "maskin"), names):
            save_nifti(golden["%s_%d" % (key, i)], p)
        files.append(names)
    return files


@pytest.fixture(scope="module")
def host_files(scans, tmp_path_factory):
    """the host form's un-normalised arrays, one build per (scale, preproc, mask) - shared by the device tests and left unchanged"""
    from fetal_net.data import open_data_file, write_data_to_file
    d = tmp_path_factory.mktemp("dataset_host")
    built = {}

    def get(si, pi, mi):
        if (si, pi, mi) not in built:
            out = str(d / ("host_%d%d%d.h5" % (si, pi, mi)))
            write_data_to_file([s if mi else s[:2] for s in scans], out, normalize=False, scale=SCALES[si], preproc=PREPROCS[pi], device=False)
            with open_data_file(out) as f:
                built[si, pi, mi] = ([f.root.data[i] for i in range(N_SUBJECTS)], [f.root.truth[i] for i in range(N_SUBJECTS)],
                                     [f.root.mask[i] for i in range(N_SUBJECTS)] if mi else None)
        return built[si, pi, mi]
    return get


def read_all(path):
    from fetal_net.data import open_data_file
    with open_data_file(path) as f:
        n = len(f.root.data)
        return ([f.root.data[i] for i in range(n)], [f.root.truth[i] for i in range(n)],
                [f.root.mask[i] for i in range(n)] if "mask" in f.root else None)


def exact_stats(vol):
    x = np.ascontiguousarray(vol).ravel()
    total, mag = math.fsum(x), math.fsum(np.abs(x))
    d = x.astype(np.longdouble) - np.longdouble(total) / x.size
    return total / x.size, mag / x.size, float(np.sqrt((d * d).sum() / x.size))


@pytest.mark.parametrize("si,pi,mi", [(0, 0, 0), (0, 0, 1), (0, 1, 0), (1, 0, 0), (1, 1, 0)])
def test_device_build_against_the_host_build(ops, scans, host_files, tmp_path, si, pi, mi):
    from fetal_net.data import write_data_to_file
    files = [s if mi else s[:2] for s in scans]
    kw = dict(scale=SCALES[si], preproc=PREPROCS[pi], device=True)
    h_data, h_truth, h_mask = host_files(si, pi, mi)

    def close(got, want, what):
        assert got.dtype == np.float64 and got.shape == want.shape
        err = float(np.abs(got - want).max())
        print("%s: max |device - host| %.3e" % (what, err))
        if si == 0:
            np.testing.assert_array_equal(got, want, err_msg=what)
        else:
            assert err <= 1e-12 * max(1.0, float(np.abs(want).max())), (what, err)

    # un-normalised: truth and masks identical, data identical or within the zoom bound
    raw = str(tmp_path / "raw.h5")
    _, stats = write_data_to_file(files, raw, normalize=None, **kw)
    assert stats == (None, None)
    d_data, d_truth, d_mask = read_all(raw)
    for i in range(N_SUBJECTS):
        close(d_data[i], h_data[i], "data %d" % i)
        assert d_truth[i].dtype == np.uint8
        np.testing.assert_array_equal(d_truth[i], h_truth[i])
        if mi:
            np.testing.assert_array_equal(d_mask[i], h_mask[i])
    assert (d_mask is None) == (not mi)

    # 'all': mean and std within the bounds of the moments; the stored volumes are numpy's (x - mean) / std of the un-normalised ones
    res = str(tmp_path / "all.h5")
    _, (mean, std) = write_data_to_file(files, res, normalize="all", **kw)
    ex = [exact_stats(v) for v in d_data]
    # the per-volume bounds, averaged, plus the roundings of averaging three doubles (two adds and a divide, and the arbiter's own divide)
    mean_bound = float(np.mean([32 * U * e[1] for e in ex])) + 4 * U * abs(float(mean))
    std_bound = float(np.mean([64 * U * e[2] for e in ex])) + 4 * U * float(std)
    print("mean error %.3e (bound %.3e), std error %.3e (bound %.3e)" % (
        abs(float(mean) - np.mean([e[0] for e in ex])), mean_bound, abs(float(std) - np.mean([e[2] for e in ex])), std_bound))
    assert abs(float(mean) - float(np.mean([e[0] for e in ex]))) <= mean_bound
    assert abs(float(std) - float(np.mean([e[2] for e in ex]))) <= std_bound
    a_data, a_truth, _ = read_all(res)
    for i in range(N_SUBJECTS):
        np.testing.assert_array_equal(a_data[i], (d_data[i] - mean) / std)
        np.testing.assert_array_equal(a_truth[i], h_truth[i])
    # no device budget: every volume is downloaded un-normalised and normalised with numpy - the same bytes
    spill = str(tmp_path / "spill.h5")
    _, (mean0, std0) = write_data_to_file(files, spill, normalize="all", device_budget=0, **kw)
    assert (float(mean0), float(std0)) == (float(mean), float(std))
    s_data, _, _ = read_all(spill)
    for i in range(N_SUBJECTS):
        assert s_data[i].tobytes() == a_data[i].tobytes()
    # a budget for one volume: the first stays resident, the others spill
    _, (mean1, std1) = write_data_to_file(files, spill, normalize="all", device_budget=d_data[0].nbytes, **kw)
    assert (float(mean1), float(std1)) == (float(mean), float(std))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(read_all(spill)[0], a_data))

    # 'each': every volume with its own device moments
    each = str(tmp_path / "each.h5")
    _, stats = write_data_to_file(files, each, normalize="each", **kw)
    assert stats == (None, None)
    e_data, _, _ = read_all(each)
    for i in range(N_SUBJECTS):
        m, s = ops.moments_f64(torch.from_numpy(np.ascontiguousarray(d_data[i])).cuda())[:2]
        np.testing.assert_array_equal(e_data[i], (d_data[i] - m) / s)
        assert abs(m - ex[i][0]) <= 32 * U * ex[i][1] and abs(s - ex[i][2]) <= 64 * U * ex[i][2]


def test_each_on_a_constant_volume_gives_numpy_s_nans(ops, golden, tmp_path):
    from fetal_net import normalize as N
    from fetal_net.data import write_data_to_file
    from fetal_net.utils.nifti import save_nifti
    vols = [np.full((6, 5, 4), 7.25), golden["vol_0"]]
    files = []
    for i, v in enumerate(vols):
        files.append((str(tmp_path / ("v%d.nii" % i)), str(tmp_path / ("t%d.nii" % i))))
        save_nifti(v, files[-1][0])
        save_nifti((v > 300).astype(np.uint8), files[-1][1])
    out = str(tmp_path / "each.h5")
    write_data_to_file(files, out, normalize="each", device=True)
    data, _, _ = read_all(out)
    with np.errstate(invalid="ignore"):
        want = (vols[0] - vols[0].mean()) / vols[0].std()
    assert np.isnan(want).all() and np.isnan(data[0]).all()
    assert np.isfinite(data[1]).all() and abs(float(data[1].std()) - 1.0) < 1e-12
    # the storage functions take the same route
    storage, mean, std = N.normalize_data_storage_each([v.copy() for v in vols], device=True)
    assert mean is None and std is None and np.isnan(storage[0]).all()
    np.testing.assert_array_equal(storage[1], data[1])
    storage, mean, std = N.normalize_data_storage([v.copy() for v in vols], device=True)
    m = [ops.moments_f64(torch.from_numpy(np.ascontiguousarray(v)).cuda())[:2] for v in vols]
    assert float(mean) == np.mean([a[0] for a in m]) and float(std) == np.mean([a[1] for a in m])
    np.testing.assert_array_equal(storage[1], (vols[1] - mean) / std)


# ------------------------------------------------------------------------------------------------------------------------ the whole chain
def test_scans_folder_to_a_trained_epoch(tmp_path, monkeypatch):
    monkeypatch.setenv("FMRI_DTYPE", "fp32")
    import fetal_net.model as fmodel
    from fetal.utils import create_data_file
    from fetal_net.data import load_norm_params, open_data_file
    from fetal_net.device_generator import DeviceDataFile
    from fetal_net.generator import get_training_and_validation_generators
    from fetal_net.training import train_model
    from fetal_net.utils.nifti import save_nifti
    rs = np.random.RandomState(2)
    sp = (24, 24, 12)
    grid = np.stack(np.meshgrid(*[np.arange(n) for n in sp], indexing="ij"))
    for i in range(4):
        centre = np.array([8 + 2 * i, 14 - i, 6]).reshape(3, 1, 1, 1)
        blob = (((grid - centre) / np.array([6.0, 5.0, 3.0]).reshape(3, 1, 1, 1)) ** 2).sum(0) < 1
        os.makedirs(str(tmp_path / "scans" / ("case_%d" % i)))
        save_nifti(np.round(rs.rand(*sp) * 200 + 400 * blob), str(tmp_path / "scans" / ("case_%d" % i) / "volume.nii.gz"))
        save_nifti(blob.astype(np.uint8), str(tmp_path / "scans" / ("case_%d" % i) / "truth.nii.gz"))
    config = {"scans_dir": str(tmp_path / "scans"), "training_modalities": ["volume"], "weight_mask": None, "ext": ".gz",
              "base_dir": str(tmp_path), "data_file": str(tmp_path / "fetal_data.h5"), "normalization": "all",
              "patch_shape": (16, 16), "patch_depth": 8, "truth_index": 0, "truth_size": 8, "3D": True}
    mean, std = create_data_file(config)
    assert load_norm_params(str(tmp_path)) == (float(mean), float(std)) and 100 < mean < 400 and std > 50
    keys = [str(tmp_path / n) for n in ("training.pkl", "validation.pkl", "test.pkl")]
    patch = tuple(config["patch_shape"]) + (config["patch_depth"],)
    with open_data_file(config["data_file"]) as f:
        assert f.root.subject_ids == [("case_%d" % i).encode() for i in range(4)]
        random.seed(1)
        np.random.seed(1)
        tg, vg, nt, nv = get_training_and_validation_generators(
            f, 2, 1, keys[0], keys[1], keys[2], patch_shape=patch, patches_per_epoch=4, validation_batch_size=4, skip_blank_train=False,
            truth_index=config["truth_index"], truth_size=config["truth_size"], categorical=False, is3d=config["3D"])
        assert (nt, nv) == (2, 1) and all(os.path.exists(k) for k in keys)
        assert tg.device_data_file is None
        x, y = next(tg)
        assert x.is_cuda and x.dtype == torch.float32 and tuple(x.shape) == (2, 1) + patch
        assert y.is_cuda and y.dtype == torch.uint8 and tuple(y.shape) == (2, 1) + patch
        xv, yv = next(vg)
        assert xv.is_cuda and tuple(xv.shape) == (4, 1) + patch and tuple(yv.shape) == (4, 1) + patch
        assert isinstance(tg.device_data_file, DeviceDataFile) and tg.device_data_file is vg.device_data_file
        assert sorted(tg.device_data_file.indices) == sorted(tg._kwargs["index_list"] + vg._kwargs["index_list"])
        model = fmodel.unet_model_3d(input_shape=(1,) + patch, depth=2, n_base_filters=8, initial_learning_rate=1e-3)
        hist = train_model(model, str(tmp_path / "fetal_net_model"), tg, vg, steps_per_epoch=nt, validation_steps=nv, n_epochs=1,
                           output_folder=str(tmp_path))
    h = hist.history
    print("loss %.4f, val_loss %.4f" % (h["loss"][0], h["val_loss"][0]))
    assert len(h["loss"]) == 1 and np.isfinite(h["loss"][0]) and np.isfinite(h["val_loss"][0])
    assert any(n.startswith("fetal_net_model-epoch01") and n.endswith(".h5") for n in os.listdir(str(tmp_path)))
    assert os.path.exists(str(tmp_path / "norm_params.json"))


def test_experiment_scripts_import_what_they_name():
    import fetal.experiments.train_adv  # noqa: F401
    import fetal.experiments.train_semi  # noqa: F401
    from fetal.utils import create_data_file, get_last_model_path
    from fetal_net.generator import get_training_and_validation_generators
    assert callable(create_data_file) and callable(get_last_model_path) and callable(get_training_and_validation_generators)
