"""Previous-slice truth 2-D models on the device paths (reference fetal/config_utils.py:128-131, fetal_net/generator.py:272-305,
fetal_net/prediction.py:98-114, :151-160, :296-320): the 2 / 4 / 6-channel first-layer kernels, the tile gather that appends truth slices,
the device tile loop with truth channels and the batched sampler with truth channels."""
import os
import random

import numpy as np
import pytest
import scipy.ndimage
import torch
import torch.nn.functional as F

from gpu_util import assert_close, bar, f64, planar_kernel, ref_conv_fwd, rnd, to_ncdhw

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the GPU box"
    from fmri_hip import ops as o
    return o


# ------------------------------------------------------------------------------------------------ first layer, even channel counts
FIRST_CASES = [
    # C0, Cout, slices, H, W
    (2, 32, 4, 16, 32),
    (2, 64, 8, 32, 64),
    (4, 32, 8, 16, 64),
    (4, 64, 4, 32, 32),
    (6, 32, 12, 16, 32),
    (6, 64, 4, 32, 64),
]


@pytest.mark.parametrize("case", FIRST_CASES, ids=lambda c: "c%d_o%d_s%d_%dx%d" % c)
def test_planar_first_layer_even_channels_is_exact_on_dyadic_data(ops, case):
    """impl=MFMA takes the first-layer kernels for 2, 4, 6 input channels; on dyadic data (every product and partial sum exact in fp32) the
    bf16 forward and the fp32 weight / bias gradients equal the generic kernels' bit for bit"""
    from fmri_hip._lib import IMPL_GENERIC, IMPL_MFMA
    C0, Cout, S, H, W = case
    bf = torch.bfloat16
    g = torch.Generator().manual_seed(C0 * 100 + Cout + S + H + W)
    dy4 = lambda shape, lo=-4, hi=5, div=4.0: (torch.randint(lo, hi, shape, generator=g).float() / div)
    x = dy4((1, S, H, W, C0)).to(bf).cuda()
    w = dy4((27, Cout, C0), -2, 3, 8.0).to(bf).cuda()
    bias = dy4((Cout,)).cuda()
    dy = dy4((1, S, H, W, Cout), -2, 3, 2.0).to(bf).cuda()
    out = {}
    for impl in (IMPL_MFMA, IMPL_GENERIC):
        y = torch.full((1, S, H, W, Cout), float("nan"), dtype=bf, device="cuda")
        ops.conv3d_fwd(x, None, w, bias, y, act=1, impl=impl, planar=True)
        dw = torch.zeros((27, Cout, C0), dtype=torch.float32, device="cuda")
        db = torch.zeros((Cout,), dtype=torch.float32, device="cuda")
        ops.conv3d_wgrad(x, None, dy, dw, db, impl=impl, planar=True)
        torch.cuda.synchronize()
        out[impl] = (y.cpu(), dw.cpu(), db.cpu())
    (ym, dwm, dbm), (yg, dwg, dbg) = out[IMPL_MFMA], out[IMPL_GENERIC]
    assert torch.equal(ym.view(torch.int16), yg.view(torch.int16)), "forward"
    assert torch.equal(dwm, dwg), "weight gradient: max diff %g" % float((dwm - dwg).abs().max())
    assert torch.equal(dbm, dbg)
    assert torch.equal(dbm, dy.float().cpu().sum(dim=(0, 1, 2, 3)))


@pytest.mark.parametrize("case", FIRST_CASES, ids=lambda c: "c%d_o%d_s%d_%dx%d" % c)
def test_planar_first_layer_even_channels_vs_fp64(ops, case):
    from fmri_hip._lib import IMPL_MFMA
    C0, Cout, S, H, W = case
    bf = torch.bfloat16
    x = rnd((1, S, H, W, C0), 1, bf)
    w = rnd((27, Cout, C0), 3, bf, scale=0.2)
    bias = rnd((Cout,), 4, torch.float32)
    y = torch.full((1, S, H, W, Cout), float("nan"), dtype=bf, device="cuda")
    ops.conv3d_fwd(x, None, w, bias, y, act=1, impl=IMPL_MFMA, planar=True)
    dy = rnd((1, S, H, W, Cout), 11, bf)
    dw = torch.zeros((27, Cout, C0), dtype=torch.float32, device="cuda")
    db = torch.zeros((Cout,), dtype=torch.float32, device="cuda")
    ops.conv3d_wgrad(x, None, dy, dw, db, impl=IMPL_MFMA, planar=True)
    torch.cuda.synchronize()
    assert_close(y, ref_conv_fwd(f64(x), None, False, f64(w), f64(bias), 1, planar=True), 5e-3, 1e-4, what="first %d fwd" % C0)
    xr = to_ncdhw(f64(x))
    wk = torch.zeros((Cout, C0, 3, 3, 3), dtype=torch.float64, requires_grad=True)
    F.conv3d(xr, wk, None, padding=1).backward(to_ncdhw(f64(dy)))
    refg = planar_kernel(wk.grad).permute(2, 3, 4, 0, 1).reshape(27, Cout, C0)
    assert_close(dw, refg, 2e-6, 2e-6, what="first %d dw" % C0)
    assert_close(db, f64(dy).sum(dim=(0, 1, 2, 3)), 2e-6, 2e-6, what="first %d db" % C0)
    assert float(dw[:9].abs().max()) == 0.0 and float(dw[18:].abs().max()) == 0.0       # planar: only the centre kd plane


# ------------------------------------------------------------------------------------------------ tile gather with truth channels
GATHER_CASES = [
    # pz, aux_dz, aux_nz
    (5, 1, 1),
    (5, 0, 1),
    (5, -2, 1),
    (5, 7, 2),
    (3, -1, 1),
    (1, 1, 1),
    (11, 3, 5),
    (4, 2, 3),
]


def _corners(shape, patch):
    X, Y, Z = shape
    px, py, pz = patch
    return np.array([(0, 0, 0), (-3, -5, -2), (X - px + 4, Y - py + 2, Z - pz + 3), (X - 2, -4, Z - 1), (-px - 2, Y + 1, -pz - 3),
                     (5, 3, 2), (X - px, Y - py, Z - pz), (2, Y - py - 1, -1)], dtype=np.int32)


@pytest.mark.parametrize("case", GATHER_CASES, ids=lambda c: "pz%d_dz%d_nz%d" % c)
def test_tile_gather_stack_equals_host_batch_iterator(ops, case):
    from fetal_net.prediction import batch_iterator
    pz, dz, nz = case
    rs = np.random.RandomState(pz * 10 + nz)
    shape = (21, 17, 13)
    vol = rs.randn(*shape).astype(np.float32)
    truth = (rs.rand(*shape) > 0.6).astype(np.uint8)
    patch = (7, 5, pz)
    idx = _corners(shape, patch)
    (host, _), = list(batch_iterator(idx, len(idx), vol, patch, truth, dz, [patch[0], patch[1], nz]))
    host = np.asarray(host, dtype=np.float32)
    assert host.shape == (len(idx), 7, 5, pz + nz)
    vd = torch.from_numpy(vol).cuda()
    ad = torch.from_numpy(truth.astype(np.float32)).cuda()
    idd = torch.from_numpy(idx).cuda()
    t32 = torch.full(host.shape, float("nan"), device="cuda")
    ops.tile_gather_stack(vd, ad, idd, patch, dz, nz, t32)
    tbf = torch.full(host.shape, float("nan"), device="cuda", dtype=torch.bfloat16)
    ops.tile_gather_stack(vd, ad, idd, patch, dz, nz, tbf)
    # an odd-sized, 2-byte-aligned destination: the narrowest store form
    raw = torch.full((host.size + 1,), float("nan"), device="cuda", dtype=torch.bfloat16)
    tbo = raw[1:].view(host.shape)
    ops.tile_gather_stack(vd, ad, idd, patch, dz, nz, tbo)
    torch.cuda.synchronize()
    assert np.array_equal(t32.cpu().numpy(), host)
    want_bf = torch.from_numpy(host).to(torch.bfloat16)
    assert torch.equal(tbf.cpu().view(torch.int16), want_bf.view(torch.int16))
    assert torch.equal(tbo.cpu().view(torch.int16), want_bf.view(torch.int16))
    assert torch.isnan(raw[:1].float()).all()                          # nothing in front of the tiles was written


@pytest.mark.parametrize("pz", [1, 5, 8, 16])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_tile_gather_stack_without_truth_equals_tile_gather(ops, pz, dtype):
    rs = np.random.RandomState(pz)
    shape = (30, 26, 19)
    vd = torch.from_numpy(rs.randn(*shape).astype(np.float32)).cuda()
    patch = (9, 8, pz)
    idd = torch.from_numpy(_corners(shape, patch)).cuda()
    a = torch.full((idd.shape[0],) + patch, float("nan"), device="cuda", dtype=dtype)
    b = torch.full_like(a, float("nan"))
    ops.tile_gather(vd, idd, patch, a)
    ops.tile_gather_stack(vd, None, idd, patch, 0, 0, b)
    torch.cuda.synchronize()
    ai = a.view(torch.int32 if dtype == torch.float32 else torch.int16)
    bi = b.view(torch.int32 if dtype == torch.float32 else torch.int16)
    assert torch.equal(ai, bi)


# ------------------------------------------------------------------------------------------------ device tile loop with truth channels
class _Proxy:
    """not a fetal_net Model: patch_wise_prediction tiles on the host (reference batch_iterator) and calls .predict"""

    def __init__(self, model):
        self.model = model
        self.output_shape = model.output_shape

    def predict(self, x):
        return self.model.predict(x)


def _volumes(seed=3, shape=(48, 40, 12)):
    rs = np.random.RandomState(seed)
    vol = rs.randn(1, *shape)
    truth = (scipy.ndimage.gaussian_filter(rs.randn(1, *shape), (0, 2, 2, 1)) > 0.05).astype(np.uint8)
    return vol, truth


def test_2d_prev_truth_prediction_runs_on_the_device_and_equals_host_tiling(monkeypatch):
    import fetal_net.model as fmodel
    import fetal_net.prediction as P

    class NoHostTiles:
        def __init__(self, *a, **k):
            raise AssertionError("the device tile loop was not taken")

    model = fmodel.unet_model_2d(input_shape=(32, 32, 6), depth=3, n_base_filters=8, compute_dtype="fp32")
    vol, truth = _volumes()
    for bs in (5, 7):
        for pti in (1, -1):
            with monkeypatch.context() as mp:
                mp.setattr(P, "ThreadedGenerator", NoHostTiles)
                dev = P.patch_wise_prediction(model, vol, (32, 32, 5), overlap_factor=0.5, batch_size=bs, truth_data=truth,
                                              prev_truth_index=pti, prev_truth_size=1)
            st = model.__dict__.get("_tile_state")
            assert st is not None and st["key"][-2:] == (pti, 1) and st["aux"] is not None
            host = P.patch_wise_prediction(_Proxy(model), vol, (32, 32, 5), overlap_factor=0.5, batch_size=bs, truth_data=truth,
                                           prev_truth_index=pti, prev_truth_size=1)
            assert dev.shape == host.shape == (48, 40, 12, 1)
            np.testing.assert_allclose(dev, host, rtol=0, atol=2e-6)
    # the truth channel matters: a different truth volume gives a different prediction
    other = P.patch_wise_prediction(model, vol, (32, 32, 5), overlap_factor=0.5, truth_data=1 - truth, prev_truth_index=-1, prev_truth_size=1)
    assert float(np.abs(other - dev).max()) > 1e-4


def test_2d_prev_truth_prediction_bf16_against_fp32():
    """the bf16 engine (first layer on the 6-channel first-layer kernels) against the fp32 engine with the same weights, both on the device"""
    import fetal_net.model as fmodel
    from fetal_net.prediction import patch_wise_prediction
    m32 = fmodel.unet_model_2d(input_shape=(32, 32, 6), depth=3, n_base_filters=32, compute_dtype="fp32")
    mbf = fmodel.unet_model_2d(input_shape=(32, 32, 6), depth=3, n_base_filters=32, compute_dtype="bf16")
    mbf.set_weights_dict(m32.get_weights_dict())
    vol, truth = _volumes(5, (64, 64, 16))
    kw = dict(overlap_factor=0.5, truth_data=truth, prev_truth_index=1, prev_truth_size=1)
    a = patch_wise_prediction(m32, vol, (32, 32, 5), **kw)
    b = patch_wise_prediction(mbf, vol, (32, 32, 5), **kw)
    assert mbf.__dict__.get("_tile_state") is not None
    err = float(np.abs(a - b).max())
    print("bf16 vs fp32 prev-truth prediction: max abs diff %.3e" % err)
    bar("prev-truth prediction bf16 vs fp32 max abs", err, 2e-3)        # 9.7e-4 measured on MI355X


def test_run_validation_case_with_prev_truth_equals_host_path(tmp_path):
    import fetal_net.model as fmodel
    from fetal_net.prediction import run_validation_case
    from fetal_net.utils.nifti import load_nifti

    class Root:
        pass

    class DataFile:
        root = Root()

    vol, truth = _volumes(7, (40, 48, 10))
    DataFile.root.data = [vol[0]]
    DataFile.root.truth = [truth[0]]
    model = fmodel.unet_model_2d(input_shape=(32, 32, 6), depth=3, n_base_filters=8, compute_dtype="fp32")
    kw = dict(patch_shape=(32, 32, 5), overlap_factor=0.5, prev_truth_index=1, prev_truth_size=1)
    fn = run_validation_case(0, str(tmp_path / "dev"), model, DataFile, ["volume"], **kw)
    assert model.__dict__.get("_tile_state") is not None
    fh = run_validation_case(0, str(tmp_path / "host"), _Proxy(model), DataFile, ["volume"], **kw)
    for f in ("data_volume.nii.gz", "truth.nii.gz", "prediction.nii.gz"):
        assert os.path.exists(str(tmp_path / "dev" / f))
    pd, ph = load_nifti(fn), load_nifti(fh)
    assert pd.shape == ph.shape == (40, 48, 10)
    np.testing.assert_allclose(pd, ph, rtol=0, atol=2e-6)


# ------------------------------------------------------------------------------------------------ batched sampling with truth channels
class _Root:
    pass


class _DataFile:
    def __init__(self, vols, truths, masks=None):
        self.root = _Root()
        self.root.data, self.root.truth = vols, truths
        self.root.mask = masks if masks is not None else []
        self.root.subject_ids = [("s%d" % i).encode() for i in range(len(vols))]


def _synth(seed, shapes):
    rs = np.random.RandomState(seed)
    vols, truths = [], []
    for s in shapes:
        vols.append((scipy.ndimage.gaussian_filter(rs.randn(*s), 1.5) * 4.0 + 0.3 * rs.randn(*s)).astype(np.float64))
        truths.append((scipy.ndimage.gaussian_filter(rs.randn(*s), 2.0) > 0.02).astype(np.uint8))
    return vols, truths


@pytest.mark.parametrize("prev", [(-1, 1), (2, 2)])
def test_prev_truth_generator_batched_equals_patch_by_patch(monkeypatch, prev):
    from fetal_net import device_generator as DG
    aug = {"flip": [0.5, 0.5, 0], "translate": (5, 5, 0), "scale": (0.1, 0.1, 0), "rotate": (0, 0, 90), "poisson_noise": 0.5,
           "contrast": {"prob": 0.5, "min_factor": 0.2, "max_factor": 0.1}, "intensity_multiplication": (0.8, 1.2),
           "elastic_transform": {"alpha": 5, "sigma": 4}, "coarse_dropout": {"rate": 0.2, "size_percent": [0.10, 0.30], "per_channel": True},
           "gaussian_noise": {"prob": 0.5, "sigma": 0.05}, "speckle_noise": {"prob": 0.5, "sigma": 0.05}}
    vols, truths = _synth(9, [(56, 60, 24), (50, 64, 30)])
    mk = [np.random.RandomState(5).rand(*t.shape).astype(np.float32) for t in truths]
    df = _DataFile(vols, truths, mk)
    from fmri_hip import ops
    outs = []
    for batched in (False, True):
        with monkeypatch.context() as mp:
            # a prev-truth batch is launched together: the gather is entered 4 times per launch() call - image, labels, mask, previous truth -
            # whatever the number of plans
            calls = {"launch": 0, "gather": 0}

            def counted(name, inner):
                def f(*a, **k):
                    calls[name] += 1
                    return inner(*a, **k)
                return f
            mp.setattr(DG._Sampler, "launch", counted("launch", DG._Sampler.launch))
            mp.setattr(ops, "affine_sample_batch", counted("gather", ops.affine_sample_batch))
            np.random.seed(21)
            random.seed(21)
            gen = DG.device_data_generator(df, [0, 1], batch_size=7, augment=aug, patch_shape=(32, 32, 5), skip_blank=True, categorical=False,
                                           is3d=False, truth_index=2, truth_size=1, prev_truth_index=prev[0], prev_truth_size=prev[1],
                                           batched=batched, shuffle_index_list=False, noise_seed=4)
            b = []
            for _ in range(3):
                (x, m), y = next(gen)
                b += [x.cpu().numpy(), m.cpu().numpy(), y.cpu().numpy()]
            gen.close()
        assert calls["launch"] >= 3 and (not batched or calls["gather"] == 4 * calls["launch"]), calls
        outs.append(b)
    for a, b in zip(*outs):
        assert a.shape == b.shape and np.array_equal(a, b)
    x = outs[0][0]
    assert x.shape == (7, 32, 32, 5 + prev[1])
    assert set(np.unique(x[..., 5:])) <= {0.0, 1.0} and x[..., 5:].any()          # the truth channels: warped labels, nearest
    assert not np.array_equal(x[0], x[3])
