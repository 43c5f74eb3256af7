"""Agreement of the TTA variants on the device: fmri_tta_agreement_f64 / ops.tta_agreement_f64 against the numpy restatement written from
the definitions (tests/tta_agreement_restatement.py; the host form is proven against it in tests/test_host_tta_agreement.py), and the
flows that use it: prediction.tta_agreement, Stage.infer(agreement=True), predict_volume(return_agreement=True).

median, mean, variance, disagreement and the counts are required IDENTICAL: fp64, one rounding per operation, the same order on both
sides.  The entropy goes through the device's log2, which is not numpy's, so no bound can be derived for it here.  Measured on the MI355X
over every case of test_kernel_is_the_restatement (profiles/r19_tta_agreement.log): the largest |device - numpy| is ENTROPY_MEASURED;
the bar is 4x that, and has to stay below 1e-13 - beyond that something other than the rounding of log2 would be wrong."""
import ctypes
import functools
import itertools

import numpy as np
import pytest

import tta_agreement_restatement as R

pytestmark = pytest.mark.gpu

ENTROPY_MEASURED = 2.0 ** -52                                # 2.220e-16 in each of the 20 (K, C) rows: one unit in the last place of 1.0
ENTROPY_ATOL = 4 * ENTROPY_MEASURED                           # 8.882e-16
assert ENTROPY_ATOL <= 1e-13

KS = (1, 2, 3, 8, 9, 16, 17, 32, 33, 64)                     # both sides of every template boundary (8, 16, 32, 64), odd and even
NVOX = (1, 63, 64, 65, 257 * 3, 40 * 27 * 9)                  # below / at / above one wave, odd (the 8-byte route), more than one workgroup
E_SHAPE = -1
SENTINEL = -7.0


@pytest.fixture(scope="module")
def ops():
    from fmri_hip import ops as o
    return o


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()               # a copy: the shared cases are read-only


@functools.lru_cache(maxsize=None)
def _case(kind, K, nvox, C):
    """(stack (K, nvox[, C]), its restatement), computed once and shared"""
    seed = 1000 * K + 10 * (nvox % 97) + C
    stack = (R.dyadic_stack if kind == "dyadic" else R.smooth_stack)(K, nvox, C, seed)
    if C == 1:
        stack = stack[..., 0]
    stack.setflags(write=False)
    return stack, R.agreement(stack, 0.5, C)


def _same(got, want, what):
    for name in ("median", "mean", "variance", "disagreement"):
        if name in got:
            assert got[name].cpu().numpy().tobytes() == want[name].tobytes(), (what, name)
    if "counts" in got:
        assert np.array_equal(got["counts"].cpu().numpy(), want["counts"]), what
    if "entropy" in got:
        d = float(np.abs(got["entropy"].cpu().numpy() - want["entropy"]).max())
        assert d <= ENTROPY_ATOL, (what, d)
        return d
    return 0.0


# ------------------------------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("K", KS)
def test_kernel_is_the_restatement(ops, K, C):
    worst = 0.0
    for kind, nvox in itertools.product(("dyadic", "smooth"), NVOX):
        stack, want = _case(kind, K, nvox, C)
        if kind == "dyadic" and nvox >= 64:
            # a count test can hide a failure only behind empty or full sets
            sizes = want["counts"][:, :1 + K]                 # |M| and every |V_k|, per channel
            assert sizes.min() >= 0.1 * nvox and sizes.max() <= 0.9 * nvox, (K, nvox, C, sizes.min(), sizes.max())
        d_stack = _dev(stack)
        got = ops.tta_agreement_f64(d_stack, 0.5, channels=C)
        assert set(got) == {"median", "counts"} | set(R.MAPS)
        assert all(tuple(got[name].shape) == stack.shape[1:] for name in ("median",) + R.MAPS) and tuple(got["counts"].shape) == (C, 2 * K + 1)
        worst = max(worst, _same(got, want, (kind, K, nvox, C)))
        assert got["median"].cpu().numpy().tobytes() == ops.median_stack_f64(d_stack).cpu().numpy().tobytes(), (kind, K, nvox, C)
        ent = got["entropy"].cpu().numpy()
        assert ent.min() >= 0.0 and ent.max() <= 1.0
        mean = want["mean"]
        assert not ent[(mean <= 0.0) | (mean >= 1.0)].any()      # exactly 0 at p = 0 and p = 1
    print("entropy K=%d C=%d: max |device - numpy| = %.3e" % (K, C, worst))


def _raw(L, stack, K, nvox, C, thr, outs, counts):
    """the entry point itself; outs: five tensors or None in the header's order"""
    import torch
    return L.fmri_tta_agreement_f64(stack.data_ptr(), K, nvox, C, thr, *[0 if t is None else t.data_ptr() for t in outs],
                                    0 if counts is None else counts.data_ptr(), torch.cuda.current_stream().cuda_stream)


NAMES = ("median",) + R.MAPS


@pytest.mark.parametrize("C", [1, 3])
def test_every_subset_of_null_outputs(C):
    """a NULL map or NULL counts changes nothing in the outputs that are there; a tensor that was not handed over keeps its sentinel"""
    import torch
    from fmri_hip._lib import lib
    L = lib()
    K, nvox = 9, 257 * 3
    stack, want = _case("smooth", K, nvox, C)
    d_stack = _dev(stack)
    for r in range(5):
        for present in itertools.combinations(R.MAPS, r):
            for with_counts in (True, False):
                bufs = {name: torch.full(stack.shape[1:], SENTINEL, dtype=torch.float64, device="cuda") for name in NAMES}
                cnt = torch.full((C, 2 * K + 1), -7, dtype=torch.int64, device="cuda")
                outs = [bufs[name] if name == "median" or name in present else None for name in NAMES]
                assert _raw(L, d_stack, K, nvox, C, 0.5, outs, cnt if with_counts else None) == 0
                got = {name: bufs[name] for name in ("median",) + present}
                if with_counts:
                    got["counts"] = cnt
                else:
                    assert bool((cnt == -7).all())
                _same(got, want, (present, with_counts))
                for name in R.MAPS:
                    if name not in present:
                        assert bool((bufs[name] == SENTINEL).all()), (present, name)


@pytest.mark.parametrize("which", NAMES + ("stack",))
def test_a_pointer_8_bytes_into_a_16_byte_line(which):
    """K = 8, one channel, an even voxel count: the 16-byte route, which one pointer that starts 8 bytes into a line must turn off"""
    import torch
    from fmri_hip._lib import lib
    K, nvox = 8, 257 * 3 + 1
    stack, want = _case("smooth", K, nvox, 1)
    if which == "stack":
        room = torch.full((K * nvox + 8,), SENTINEL, dtype=torch.float64, device="cuda")
        d_stack = room[1:1 + K * nvox].view(K, nvox)
        d_stack.copy_(_dev(stack))
    else:
        d_stack = _dev(stack)
    assert (d_stack.data_ptr() % 16 == 8) == (which == "stack")
    bufs = {name: torch.full((nvox + 8,), SENTINEL, dtype=torch.float64, device="cuda") for name in NAMES}
    off = {name: 1 if name == which else 0 for name in NAMES}
    outs = [bufs[name][off[name]:off[name] + nvox] for name in NAMES]
    assert all((o.data_ptr() % 16 == 8) == (name == which) for o, name in zip(outs, NAMES))
    cnt = torch.empty((1, 2 * K + 1), dtype=torch.int64, device="cuda")
    assert _raw(lib(), d_stack, K, nvox, 1, 0.5, outs, cnt) == 0
    got = dict(zip(NAMES, outs), counts=cnt)
    _same(got, want, which)
    for name in NAMES:
        whole = bufs[name].cpu().numpy()
        assert np.all(whole[:off[name]] == SENTINEL) and np.all(whole[off[name] + nvox:] == SENTINEL), (which, name)


@pytest.mark.parametrize("K,C,nvox", [(3, 1, 2 * 524288 + 2 * 256 * 3 + 2), (3, 1, 2 * 524288 + 2 * 256 * 3 + 3), (3, 3, 524288 + 77),
                                      (17, 1, 131072 + 77), (33, 1, 65536 + 77)])
def test_the_grid_stride_loop_runs_more_than_once(ops, K, C, nvox):
    """A launch starts at most 1,024 workgroups of 256 threads = 262,144 threads (K <= 16: four workgroups per CU).  One channel, even
    voxel count: two voxels per thread, 524,288 per sweep, so 1,050,114 voxels take two sweeps and a third, partial one; the odd count
    takes the one-voxel route (five sweeps).  Three channels: a thread per voxel, 524,365 voxels in two sweeps and 77 voxels of a third.
    17 to 32 variants start two workgroups per CU (131,072 threads), 33 to 64 one (65,536): 77 voxels more than that each."""
    stack, want = _case("dyadic", K, nvox, C)
    assert nvox > 65536 * (4 if K <= 16 else (2 if K <= 32 else 1)) * (2 if C == 1 and nvox % 2 == 0 else 1)
    got = ops.tta_agreement_f64(_dev(stack), 0.5, channels=C)
    _same(got, want, (C, nvox))


def test_past_two_to_the_31_elements(ops):
    """K * nvox just above 2^31: the 64-bit index forms, checked on the device against the median kernel and torch's own sums"""
    import torch
    K, nvox = 64, 2 ** 25 + 4096
    assert K * nvox > 2 ** 31
    g = torch.Generator(device="cuda").manual_seed(11)
    stack = torch.rand((K, nvox), generator=g, dtype=torch.float64, device="cuda")
    thr = 0.5
    got = ops.tta_agreement_f64(stack, thr, maps=())
    assert set(got) == {"median", "counts"}
    med = ops.median_stack_f64(stack)
    assert torch.equal(got["median"], med)
    above = stack > thr
    M = med > thr
    want = torch.cat([M.sum().reshape(1), above.sum(dim=1), (above & M).sum(dim=1)]).reshape(1, 2 * K + 1)
    assert torch.equal(got["counts"], want)
    assert 0.1 * nvox < int(want[0, 0]) < 0.9 * nvox and 0.4 * nvox < int(want[0, K]) < 0.6 * nvox    # the far end of the stack counts


def test_the_call_zeroes_the_counts():
    import torch
    from fmri_hip._lib import lib
    K, nvox, C = 9, 40 * 27 * 9, 3
    stack, want = _case("dyadic", K, nvox, C)
    d_stack = _dev(stack)
    med = torch.empty(stack.shape[1:], dtype=torch.float64, device="cuda")
    cnt = torch.full((C, 2 * K + 1), 123456789, dtype=torch.int64, device="cuda")
    for _ in range(2):                                        # the second call finds the first one's sums in the buffer
        assert _raw(lib(), d_stack, K, nvox, C, 0.5, [med, None, None, None, None], cnt) == 0
        assert np.array_equal(cnt.cpu().numpy(), want["counts"])


@pytest.mark.parametrize("C", [1, 3])
def test_footprint(C):
    import torch
    from fmri_hip._lib import lib
    from footprint import audit
    K, nvox = 9, 40 * 27 * 9
    stack, want = _case("smooth", K, nvox, C)
    fill = _dev(stack)

    def run(alloc):
        d_stack = alloc.input(fill, name="stack")
        outs = [alloc.output(stack.shape[1:], torch.float64, offset16=(name == "variance"), name=name) for name in NAMES]
        cnt = alloc.output((C, 2 * K + 1), torch.int64, name="counts")
        assert _raw(lib(), d_stack, K, nvox, C, 0.5, outs, cnt) == 0
        return dict(zip(NAMES, outs), counts=cnt)

    plain, _ = audit(run)
    _same(plain, want, C)


def test_refusals_leave_the_outputs_untouched(ops):
    import torch
    from fmri_hip._lib import lib
    L = lib()
    K, nvox = 4, 100
    stack = torch.rand((K, nvox), dtype=torch.float64, device="cuda")
    outs = [torch.full((nvox,), SENTINEL, dtype=torch.float64, device="cuda") for _ in NAMES]
    cnt = torch.full((1, 2 * K + 1), -7, dtype=torch.int64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    f = L.fmri_tta_agreement_f64
    sp, o, c = stack.data_ptr(), [t.data_ptr() for t in outs], cnt.data_ptr()
    assert f(0, K, nvox, 1, 0.5, *o, c, s) == E_SHAPE
    assert f(sp, K, nvox, 1, 0.5, 0, *o[1:], c, s) == E_SHAPE
    assert f(sp, 0, nvox, 1, 0.5, *o, c, s) == E_SHAPE
    assert f(sp, 65, nvox, 1, 0.5, *o, c, s) == E_SHAPE
    assert f(sp, K, 0, 1, 0.5, *o, c, s) == E_SHAPE
    assert f(sp, K, -nvox, 1, 0.5, *o, c, s) == E_SHAPE
    assert f(sp, K, nvox, 0, 0.5, *o, c, s) == E_SHAPE
    assert f(sp, K, nvox // 20, 17, 0.5, *o, c, s) == E_SHAPE
    assert f(sp, K, nvox, 1, 0.5, sp, *o[1:], c, s) == E_SHAPE                       # the median on top of the stack
    assert f(sp, K, nvox, 1, 0.5, o[0], o[1], sp + 8 * nvox * (K - 1), o[3], o[4], c, s) == E_SHAPE    # a map on its last variant
    assert f(sp, K, nvox, 1, 0.5, *o, sp + 8 * nvox, s) == E_SHAPE                   # the counts inside it
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in outs) and bool((cnt == -7).all())
    for bad in (torch.zeros((65, 10), dtype=torch.float64, device="cuda"), torch.zeros((2, 10), dtype=torch.float32, device="cuda")):
        with pytest.raises(ValueError):
            ops.tta_agreement_f64(bad)
    with pytest.raises(ValueError):
        ops.tta_agreement_f64(stack, channels=17)
    with pytest.raises(ValueError):
        ops.tta_agreement_f64(stack, channels=3)              # the last extent is not 3
    with pytest.raises(ValueError):
        ops.tta_agreement_f64(stack, maps=("median",))
    with pytest.raises(RuntimeError):
        ops.tta_agreement_f64(stack.cpu())


# ------------------------------------------------------------------------------------------------------------------------------ flows
# tests/test_gpu_tta_resident.py, measured on the MI355X: the resident route repeats its bits in the 3-D flows (one tile group per launch)
# and two runs of a 2-D flow differ by at most 2^-54 per variant, which a median of 8 carries over and rounds once more
ROUTE_ATOL = 2 * 5.551e-17
MEDIAN_ATOL = ROUTE_ATOL + 2.0 ** -53


def _cfg(patch):
    return {"patch_shape": list(patch[:2]), "patch_depth": patch[2]}


@pytest.fixture(scope="module")
def net3d():
    import os
    os.environ["FMRI_DTYPE"] = "bf16"
    import fetal_net.model as fmodel
    patch = (16, 32, 32)
    return fmodel.unet_model_3d(input_shape=(1,) + patch, depth=3, n_base_filters=32), patch


@pytest.fixture(scope="module")
def net2d():
    import fetal_net.model as fmodel
    patch = (32, 32, 5)
    return fmodel.unet_model_2d(input_shape=patch, depth=2, n_base_filters=8, n_labels=3), patch


def _agreement_is_restatement_of(agreed, stack, threshold, C):
    want = R.agreement(np.asarray(stack), threshold, C)
    for name in ("median", "mean", "variance", "disagreement"):
        assert np.asarray(getattr(agreed, name)).tobytes() == want[name].tobytes(), name
    assert float(np.abs(agreed.entropy - want["entropy"]).max()) <= ENTROPY_ATOL
    assert np.array_equal(agreed.counts, want["counts"])
    dice, est, cv = R.scores(want["counts"])
    np.testing.assert_allclose(agreed.variant_dice, dice, rtol=0, atol=2.0 ** -51)
    np.testing.assert_allclose(agreed.estimated_dice, est, rtol=0, atol=2.0 ** -50)
    assert np.all((agreed.estimated_dice >= 0.0) & (agreed.estimated_dice <= 1.0))


def test_stage_infer_3d(net3d):
    from fetal_net.pipeline import Stage
    model, patch = net3d
    vol = np.random.RandomState(21).randn(24, 27, 40)
    stage = Stage(model, _cfg(patch), augment="flip", overlap=0.5)
    assert stage._resident_refusal(vol) is None
    kept, agreed = stage.infer(vol, keep_variants=True, agreement=True)
    assert kept.shape == (8, 24, 27, 40) and agreed.counts.shape == (1, 17)
    _agreement_is_restatement_of(agreed, kept, 0.5, 1)
    assert agreed.variance.max() > 0.0                        # the flips are real variants
    pred, again = stage.infer(vol, agreement=True)
    assert pred.tobytes() == stage.infer(vol).tobytes() == again.median.tobytes() == agreed.median.tobytes()
    assert np.array_equal(again.counts, agreed.counts)
    with pytest.raises(ValueError):
        Stage(model, _cfg(patch), overlap=0.5).infer(vol, agreement=True)


def test_stage_infer_2d_three_labels(net2d):
    from fetal_net.pipeline import Stage
    model, patch = net2d
    vol = np.random.RandomState(6).randn(40, 27, 9) * 50 + 100
    stage = Stage(model, _cfg(patch), augment="flip", overlap=0.5, threshold=0.4)
    kept, agreed = stage.infer(vol, keep_variants=True, agreement=True)
    assert kept.shape == (8, 40, 27, 9, 3) and agreed.counts.shape == (3, 17) and agreed.variant_dice.shape == (8, 3)
    _agreement_is_restatement_of(agreed, kept, 0.4, 3)
    pred, _ = stage.infer(vol, agreement=True)
    np.testing.assert_allclose(pred, stage.infer(vol), rtol=0, atol=MEDIAN_ATOL)


def test_predict_volume_return_agreement(net3d):
    import torch
    from scipy import ndimage
    from fetal_net import pipeline
    from fetal_net.prediction import TTAAgreement
    model, patch = net3d
    vol = ndimage.gaussian_filter(np.random.RandomState(9).randn(40, 64, 48), 2.0) * 400 + 300
    kw = dict(overlap_factor=0.5, xy_scale=0.5, augment="flip")
    plain = pipeline.predict_volume(vol, model, _cfg(patch), **kw)
    out = pipeline.predict_volume(vol, model, _cfg(patch), return_agreement=True, **kw)
    assert set(plain) == {"data", "prediction"} and set(out) == {"data", "prediction", "agreement"}
    assert out["data"].tobytes() == plain["data"].tobytes()
    # the zoom back is linear interpolation: a convex combination carries a sup-norm difference over, its own rounding adds 4 * 2^-53
    np.testing.assert_allclose(out["prediction"], plain["prediction"], rtol=0, atol=MEDIAN_ATOL + 4 * 2.0 ** -53)
    a = out["agreement"]
    assert isinstance(a, TTAAgreement) and a.counts.shape == (1, 17)
    for name in NAMES:
        m = getattr(a, name)
        assert isinstance(m, np.ndarray) and m.shape == vol.shape, name
    assert a.median.tobytes() == out["prediction"].tobytes()
    assert 0.0 <= a.estimated_dice[0] <= 1.0 and a.variant_dice.shape == (8, 1)
    assert a.counts[0, 0] <= 26 * 38 * 54                     # counted on the grid the model saw: zoomed to half in-plane, with its border
    dev = pipeline.predict_volume(torch.from_numpy(vol).cuda(), model, _cfg(patch), return_agreement=True, **kw)
    for name in NAMES:
        m = getattr(dev["agreement"], name)
        assert torch.is_tensor(m) and m.is_cuda and m.dtype == torch.float64 and tuple(m.shape) == vol.shape, name
    assert torch.is_tensor(dev["prediction"]) and isinstance(dev["agreement"].counts, np.ndarray)
    assert np.array_equal(dev["agreement"].counts, a.counts)


def test_tta_agreement_of_predict_flips(net3d):
    import torch
    from fetal_net import prediction as P
    model, patch = net3d
    vol = np.random.RandomState(21).randn(1, 24, 27, 40)
    flips = P.predict_flips(vol, model, 0.5, _cfg(patch))
    assert isinstance(flips, list) and len(flips) == 8 and isinstance(flips[0], np.ndarray)
    _agreement_is_restatement_of(P.tta_agreement(flips), np.stack(flips), 0.5, 1)
    _agreement_is_restatement_of(P.tta_agreement(flips, device=False), np.stack(flips), 0.5, 1)
    dev = P.predict_flips(torch.from_numpy(vol).cuda(), model, 0.5, _cfg(patch))
    assert all(torch.is_tensor(d) for d in dev)
    agreed = P.tta_agreement(dev)
    assert all(torch.is_tensor(getattr(agreed, name)) for name in NAMES)
    want = R.agreement(np.stack([d.cpu().numpy() for d in dev]), 0.5, 1)
    assert agreed.median.cpu().numpy().tobytes() == want["median"].tobytes()
    assert agreed.variance.cpu().numpy().tobytes() == want["variance"].tobytes()
    assert np.array_equal(agreed.counts, want["counts"])
    with pytest.raises(ValueError):
        P.tta_agreement(dev, device=False)
