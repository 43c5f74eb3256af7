"""Several labels on the device: the four label kernels bit for bit against numpy, fmri_label_sums against float64 sums,
the generator's expanded targets, n_labels = 3 models against the oracle with their label-wise Dice metrics, the label map straight from the
overlap-add, and per-label scores.  Host-side twins: tests/test_host_multilabel.py."""
import ctypes
import gzip
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NS = (5 * 7 * 11, 64 * 64 * 20 + 3)          # a tail no vector width divides; several workgroups
LS = (1, 2, 3, 5, 8, 9, 32)


@pytest.fixture(scope="module")
def ops():
    from fmri_hip import ops as o
    return o


def _values(L):
    """L distinct label values in no order"""
    return [int(v) for v in np.random.RandomState(100 + L).permutation(np.arange(1, 256))[:L]]


_MAPS = {}


def _maps(n, L):
    """two label maps of n bytes (made once per (n, L)): bytes from the labels except the last one (absent from both maps, L > 1), 0, and
    two bytes that are no label"""
    if (n, L) not in _MAPS:
        vals = _values(L)
        others = [v for v in range(1, 256) if v not in vals][:2]
        pool = np.array((vals[:-1] if L > 1 else vals) + [0, 0] + others, dtype=np.uint8)
        rs = np.random.RandomState(n % 1000 + L)
        t = pool[rs.randint(len(pool), size=n)]
        p = np.where(rs.rand(n) < 0.6, t, pool[rs.randint(len(pool), size=n)]).astype(np.uint8)
        for a in (t, p):
            a.setflags(write=False)
        _MAPS[(n, L)] = (vals, t, p)
    return _MAPS[(n, L)]


# ------------------------------------------------------------------------------------------------ kernels, exact
@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("n", NS)
def test_labels_expand_exact(ops, n, L):
    vals, lab, _ = _maps(n, L)
    ref = (lab[:, None] == np.array(vals, np.uint8)[None, :]).astype(np.uint8)
    assert L == 1 or not ref[:, -1].any()                       # the absent label's channel stays empty
    assert (ref.sum(axis=1) == 0).sum() > (lab == 0).sum()      # bytes that are no label give zero rows, like the background
    d = torch.from_numpy(lab.copy()).cuda()
    out = ops.labels_expand_u8(d, vals)
    assert out.shape == (n, L) and out.dtype == torch.uint8
    assert np.array_equal(out.cpu().numpy(), ref)
    # an output that starts on an odd address: no wide store is aligned there
    buf = torch.full((n * L + 2,), 7, dtype=torch.uint8, device="cuda")
    ops.labels_expand_u8(d, vals, out=buf[1:1 + n * L])
    got = buf.cpu().numpy()
    assert got[0] == 7 and got[-1] == 7 and np.array_equal(got[1:-1].reshape(n, L), ref)


@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("n", NS)
def test_label_counts_exact(ops, n, L):
    vals, t, p = _maps(n, L)
    ref = [(int((t == v).sum()), int((p == v).sum()), int(((t == v) & (p == v)).sum())) for v in vals]
    assert L == 1 or ref[-1] == (0, 0, 0)
    dt, dp = torch.from_numpy(t.copy()).cuda(), torch.from_numpy(p.copy()).cuda()
    assert ops.label_counts_u8(dt.reshape(1, 1, n), dp.reshape(1, 1, n), vals) == ref
    # from an odd address: the one-byte path
    ref1 = [(int((t[1:] == v).sum()), int((p[1:] == v).sum()), int(((t[1:] == v) & (p[1:] == v)).sum())) for v in vals]
    assert ops.label_counts_u8(dt[1:].reshape(1, 1, n - 1), dp[1:].reshape(1, 1, n - 1), vals) == ref1


@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("n", NS)
def test_tile_finalize_labels_exact(ops, n, L):
    """cnt in 0..4 with zeros; acc = q * cnt with q from {1/4, 1/2, 3/4, 1}: acc / cnt is exact, ties and maxima AT the threshold are common"""
    vals = _values(L)
    rs = np.random.RandomState(n % 1000 + 7 * L)
    cnt = rs.randint(0, 5, size=n).astype(np.int32)
    q = rs.randint(1, 5, size=(n, L)) / 4.0
    q[0::3] = rs.randint(1, 3, size=q[0::3].shape) / 4.0          # a third of the voxels: nothing above the threshold, mostly a maximum AT it
    q[1::3] = 0.25                                                # a third: everything below
    acc = q * cnt[:, None]
    thr = 0.5
    live = cnt > 0
    qq = np.where(live[:, None], acc / np.maximum(cnt, 1)[:, None], 0.0)
    if L == 1:
        ref = np.where(qq[:, 0] > thr, vals[0], 0)
    else:
        k = np.argmax(qq, axis=1)
        ref = np.where(qq.max(axis=1) < thr, 0, np.array(vals)[k])
        assert ((qq == qq.max(axis=1, keepdims=True)).sum(axis=1) > 1)[live].any()              # ties
    assert (qq.max(axis=1) == thr)[live].any()                                                   # at the threshold
    ref = np.where(live, ref, 0).astype(np.uint8)
    out = torch.full((n,), 255, dtype=torch.uint8, device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    ops.tile_finalize_labels(torch.from_numpy(acc).cuda(), torch.from_numpy(cnt).cuda(), out, bad, thr, vals)
    assert np.array_equal(out.cpu().numpy(), ref)
    assert int(bad.item()) == int((~live).sum()) > 0


def test_label_kernels_refuse_bad_values():
    """FMRI_E_SHAPE (-1) for L = 0, L = 33, a value twice and a zero value, on each of the three entry points; nothing is launched"""
    from fmri_hip._lib import lib
    from fmri_hip.ops import _s
    L_ = lib()
    n = 64
    lab = torch.zeros(n, dtype=torch.uint8, device="cuda")
    out = torch.full((n * 33,), 9, dtype=torch.uint8, device="cuda")
    acc = torch.zeros(n * 33, dtype=torch.float64, device="cuda")
    cnt = torch.ones(n, dtype=torch.int32, device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    counts = torch.full((99,), 5, dtype=torch.int64, device="cuda")

    def arr(*v):
        return (ctypes.c_uint8 * len(v))(*v)

    cases = [(arr(*range(1, 34)), 0), (arr(*range(1, 34)), 33), (arr(3, 5, 3), 3), (arr(3, 0, 5), 3)]
    for vals, L in cases:
        assert L_.fmri_labels_expand_u8(lab.data_ptr(), n, vals, L, out.data_ptr(), _s()) == -1
        assert L_.fmri_tile_finalize_labels(acc.data_ptr(), cnt.data_ptr(), out.data_ptr(), bad.data_ptr(), n, L, 0.5, vals, _s()) == -1
        assert L_.fmri_label_counts_u8(lab.data_ptr(), lab.data_ptr(), n, vals, L, counts.data_ptr(), _s()) == -1
    assert L_.fmri_label_sums(acc.data_ptr(), lab.data_ptr(), n, 0, acc.data_ptr(), _s()) == -1
    assert L_.fmri_label_sums(acc.data_ptr(), lab.data_ptr(), n, 33, acc.data_ptr(), _s()) == -1
    torch.cuda.synchronize()
    assert bool((out == 9).all()) and bool((counts == 5).all()) and int(bad.item()) == 0


# ------------------------------------------------------------------------------------------------ fmri_label_sums
def _sums_case():
    nvox, L = 2 * 16 * 16 * 16, 3
    g = torch.Generator().manual_seed(5)
    probs = torch.rand(nvox * L, generator=g)
    y = (torch.rand(nvox * L, generator=g) > 0.7).to(torch.uint8)
    p64, y64 = probs.numpy().astype(np.float64).reshape(nvox, L), y.numpy().astype(np.float64).reshape(nvox, L)
    ref = np.stack([(y64 * p64).sum(axis=0), y64.sum(axis=0), p64.sum(axis=0)], axis=1)          # [L][3]
    return nvox, L, probs.cuda(), y.cuda(), ref


def test_label_sums_against_float64(ops):
    """numpy float64 sums of the device's own fp32 probabilities; every term is non-negative, so any summation order of nvox terms stays
    within nvox * 2^-53 relative of the exact sum, and numpy's pairwise sum does too: the bound is for the difference of two such sums"""
    nvox, L, probs, y, ref = _sums_case()
    out = torch.full((3 * L + 2,), float("nan"), dtype=torch.float64, device="cuda")
    ops.label_sums(probs, y, L, out[:3 * L])
    got = out.cpu().numpy()
    assert np.isnan(got[-2:]).all()                                  # overwritten, and nothing behind them
    rel = np.abs(got[:3 * L].reshape(L, 3) - ref) / ref
    print("label sums: max relative error %.3e (bound %.3e)" % (rel.max(), nvox * 2.0 ** -53))
    assert rel.max() <= nvox * 2.0 ** -53


def test_label_sums_repeat_bit_for_bit_under_a_deterministic_registration(ops):
    """the workgroups' sums meet as 2^-20 fixed-point integers: two runs give the same bits; against float64 each of the at most
    nvox * L / 2048 + L workgroups rounds its sum once (half a unit of 2^-20)"""
    from gpu_util import assert_same
    nvox, L, probs, y, ref = _sums_case()
    grad, shadow = torch.zeros(64, device="cuda"), torch.zeros(64, dtype=torch.int64, device="cuda")
    ops.set_deterministic(grad, shadow)
    try:
        runs = []
        for _ in range(2):
            out = torch.full((3 * L,), float("nan"), dtype=torch.float64, device="cuda")
            ops.label_sums(probs, y, L, out)
            torch.cuda.synchronize()
            runs.append(out)
    finally:
        ops.set_deterministic(None, None)
    assert_same(runs[1], runs[0], "label sums, second run")
    groups = nvox * L // 2048 + 1 + L
    err = np.abs(runs[0].cpu().numpy().reshape(L, 3) - ref)
    assert (err <= groups * 2.0 ** -21 + ref * nvox * 2.0 ** -53).all()


# ------------------------------------------------------------------------------------------------ generator
class _Root:
    pass


class _File:
    def __init__(self, vols, truths):
        self.root = _Root()
        self.root.data, self.root.truth, self.root.mask = vols, truths, []


def _volumes(shape=(24, 24, 12), n=3, seed=0):
    """seeded volumes with a label map over {0, 1, 2, 4}: three blobs in a background"""
    rs = np.random.RandomState(seed)
    vols, truths = [], []
    X, Y, Z = shape
    for _ in range(n):
        vols.append(rs.randn(*shape).astype(np.float32) * 50 + 100)
        t = np.zeros(shape, np.uint8)
        for v in (1, 2, 4):
            c = [rs.randint(s // 4, 3 * s // 4) for s in shape]
            r = [max(2, s // 4) for s in shape]
            t[max(c[0] - r[0], 0):c[0] + r[0], max(c[1] - r[1], 0):c[1] + r[1], max(c[2] - r[2], 0):c[2] + r[2]] = v
        truths.append(t)
    return vols, truths


AUG = {"flip": [0.5, 0.5, 0.5], "rotate": (0, 0, 90), "elastic_transform": {"alpha": 5, "sigma": 4}}
LABELS = (1, 2, 4)


def _batches(n_labels, is3d, batched, n_batches=2, **kw):
    from fetal_net.device_generator import device_data_generator
    vols, truths = _volumes()
    np.random.seed(17)
    random.seed(17)
    shape = dict(patch_shape=(16, 16, 8), truth_index=0, truth_size=8) if is3d else dict(patch_shape=(16, 16, 5), truth_index=2, truth_size=1)
    g = device_data_generator(_File(vols, truths), [0, 1, 2], batch_size=4, n_labels=n_labels, labels=LABELS if n_labels > 1 else None,
                              augment=AUG, skip_blank=True, categorical=False, is3d=is3d, shuffle_index_list=False, noise_seed=3,
                              batched=batched, **dict(shape, **kw))
    out = []
    for _ in range(n_batches):
        x, y = next(g)
        out.append((x.cpu().numpy(), y.cpu().numpy(), y))
    return out


@pytest.mark.parametrize("is3d", [False, True], ids=["2d", "3d"])
def test_generator_expands_the_label_patches(is3d):
    """same seeds: x is the single-label generator's bit for bit, y the numpy expansion of its y; batched and patch by patch agree.  On a
    tree without the feature n_labels is ignored and y comes out as the raw map in the single-label shape: this is the test that fails there."""
    one = _batches(1, is3d, True)
    seen = set()
    for batched in (True, False):
        many = _batches(3, is3d, batched)
        for (x1, y1, _), (x3, y3, y3_dev) in zip(one, many):
            assert x3.tobytes() == x1.tobytes() and x3.shape == x1.shape
            if is3d:
                assert y1.shape == (4, 1, 16, 16, 8) and y3.shape == (4, 3, 16, 16, 8)
                ref = np.stack([y1[:, 0] == v for v in LABELS], axis=1).astype(np.uint8)
                # a permuted view of the channels-last buffer: the model's permute(0, 2, 3, 4, 1).contiguous() copies nothing
                back = y3_dev.permute(0, 2, 3, 4, 1)
                assert back.is_contiguous() and back.contiguous().data_ptr() == y3_dev.data_ptr()
            else:
                assert y1.shape == (4, 16, 16, 1) and y3.shape == (4, 16, 16, 3)
                ref = np.stack([y1[..., 0] == v for v in LABELS], axis=-1).astype(np.uint8)
            assert y3.dtype == np.uint8 and np.array_equal(y3, ref)
            seen |= set(np.unique(y1).tolist())
    assert seen >= {0, 1, 2, 4}                                  # every label came by


def test_generator_keeps_a_patch_of_foreign_labels_and_expands_it_to_zeros():
    """skip_blank decides on the raw map: a patch that holds only label 3 - not among `labels` - is kept, and its target is all zero"""
    from fetal_net.device_generator import device_data_generator
    vol = np.random.RandomState(1).randn(24, 24, 12).astype(np.float32)
    truth = np.full((24, 24, 12), 3, np.uint8)
    kw = dict(batch_size=2, augment=None, patch_shape=(16, 16, 5), truth_index=2, truth_size=1, skip_blank=True, categorical=False, is3d=False,
              shuffle_index_list=False)
    np.random.seed(2)
    _, y1 = next(device_data_generator(_File([vol], [truth]), [0], n_labels=1, **kw))
    np.random.seed(2)
    _, y3 = next(device_data_generator(_File([vol], [truth]), [0], n_labels=3, labels=LABELS, **kw))
    assert set(np.unique(y1.cpu().numpy()).tolist()) == {0, 3} or set(np.unique(y1.cpu().numpy()).tolist()) == {3}
    assert y3.shape == (2, 16, 16, 3) and not bool(y3.any())


def test_get_multi_class_labels_device_form_equals_the_numpy_form():
    from fetal_net.device_generator import get_multi_class_labels
    _, truths = _volumes()
    data = np.stack(truths)[:, None]                                       # (3, 1, 24, 24, 12)
    ref = get_multi_class_labels(data, 3, labels=(4, 1, 2))
    got = get_multi_class_labels(torch.from_numpy(data).cuda(), 3, labels=(4, 1, 2))
    assert got.is_cuda and got.dtype == torch.int8 and tuple(got.shape) == ref.shape
    assert np.array_equal(got.cpu().numpy(), ref)


# ------------------------------------------------------------------------------------------------ models
def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def _l2(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / (np.linalg.norm(b) + 1e-30))


def _generator_batch(patch, is3d, shape):
    """one batch (x, y) of CUDA tensors from the multi-label generator at the model's input size"""
    from fetal_net.device_generator import device_data_generator
    vols, truths = _volumes(shape, n=2, seed=4)
    np.random.seed(23)
    random.seed(23)
    kw = dict(truth_index=0, truth_size=patch[2]) if is3d else dict(truth_index=2, truth_size=1)
    return next(device_data_generator(_File(vols, truths), [0, 1], batch_size=2 if is3d else 4, n_labels=3, labels=LABELS, augment=AUG,
                                      patch_shape=patch, skip_blank=True, categorical=False, is3d=is3d, shuffle_index_list=False, **kw))


def _label_dice(eng, y, n_labels):
    """(2 I + 1) / (Sy + Sp + 1) per label in float64 from the probabilities the step left on the device"""
    p = eng.probs.reshape(-1, n_labels).double().cpu().numpy()
    t = (y.permute(0, 2, 3, 4, 1) if y.dim() == 5 else y).reshape(-1, n_labels).double().cpu().numpy()
    return [(2 * (t[:, i] * p[:, i]).sum() + 1) / (t[:, i].sum() + p[:, i].sum() + 1) for i in range(n_labels)]


def _check_label_logs(model, logs, eng, y):
    names = ["label_%d_dice_coef" % i for i in range(3)]
    assert model.metrics_names[-3:] == names and len(logs) == len(model.metrics_names)
    got = dict(zip(model.metrics_names, logs))
    want = _label_dice(eng, y, 3)
    for i, name in enumerate(names):
        print("%s: %.9f (numpy %.9f)" % (name, got[name], want[i]))
        assert got[name] == pytest.approx(want[i], rel=1e-6)            # as test_sigmoid_dice_fwd_bwd checks Dice (tests/test_gpu_ops.py)
    assert len({round(v, 6) for v in want}) == 3                        # three different labels, three different values
    return got


def _unet3d(dtype, monkeypatch, W=None):
    import fetal_net.model as fmodel
    from oracle import unet_oracle as O
    monkeypatch.setenv("FMRI_DTYPE", dtype)
    kw = dict(input_shape=(1, 16, 16, 16), depth=2, n_base_filters=8, n_labels=3)
    model = fmodel.unet_model_3d(include_label_wise_dice_coefficients=True, initial_learning_rate=1e-3, **kw)
    assert not getattr(model, "_graph_engine", False)                   # the hand-scheduled engine
    spec = O.Spec(**kw)
    W = spec.init_weights(31) if W is None else W
    model.set_weights_dict(W)
    return model, spec, W


def test_unet3d_three_labels_against_the_oracle(monkeypatch):
    """unet_model_3d, n_labels = 3, on the hand-scheduled engine: one train_on_batch on generator output.  Tolerances of the single-label twin
    test_cfg1_fp32_forward_backward_adam: logits 1e-3 relative (tests/test_gpu_engine.py:55), loss 1e-4 absolute (:57, :76), every gradient
    2e-3 relative (:66-67)."""
    from oracle import unet_oracle as O
    model, spec, W = _unet3d("fp32", monkeypatch)
    x, y = _generator_batch((16, 16, 16), True, (24, 24, 24))
    assert tuple(y.shape) == (2, 3, 16, 16, 16)
    ref = O.loss_and_grads(spec, W, x.cpu().numpy(), y.cpu().numpy(), dtype=torch.float64)
    logs = model.train_on_batch(x, y)
    eng = model.engine(2)
    logits = eng.logits.cpu().numpy().reshape(2, 16, 16, 16, 3).transpose(0, 4, 1, 2, 3)
    assert _rel(logits, ref["logits"]) <= 1e-3
    assert abs(logs[0] - ref["loss"]) <= 1e-4
    for name, L in eng.layout.items():
        gk = ref["grads"][name + "/kernel"]
        if L["kind"] == "conv":
            mine = eng.w_view(name, eng.G).cpu().numpy().reshape(3, 3, 3, L["cout"], L["cin"]).transpose(0, 1, 2, 4, 3)
        else:
            mine = eng.w_view(name, eng.G).cpu().numpy().T.reshape(gk.shape)
        assert _rel(mine, gk) <= 2e-3, name
        assert _rel(eng.b_view(name, eng.G).cpu().numpy(), ref["grads"][name + "/bias"]) <= 2e-3, name + " bias"
    _check_label_logs(model, logs, eng, y)
    # evaluation reads the same names through the same read-back
    assert len(model.test_on_batch(x, y)) == len(model.metrics_names)


def test_unet3d_three_labels_bf16_label_dice_close_to_fp32(monkeypatch):
    """the same model and batch in bf16: finite, and every label-wise Dice within the bf16 logit tolerance of its fp32 run - 1.3e-2, the bar
    of test_bf16_matches_fp32_engine_on_gpu (tests/test_gpu_engine.py:142)"""
    x, y = _generator_batch((16, 16, 16), True, (24, 24, 24))
    m32, _, W = _unet3d("fp32", monkeypatch)
    l32 = dict(zip(m32.metrics_names, m32.train_on_batch(x, y)))
    m16, _, _ = _unet3d("bf16", monkeypatch, W)
    logs = m16.train_on_batch(x, y)
    assert m16.engine(2).dtype == torch.bfloat16 and np.isfinite(logs).all()
    l16 = _check_label_logs(m16, logs, m16.engine(2), y)
    for i in range(3):
        k = "label_%d_dice_coef" % i
        print("%s: bf16 %.6f fp32 %.6f" % (k, l16[k], l32[k]))
        assert abs(l16[k] - l32[k]) <= 1.3e-2


def test_isensee3d_three_labels_against_the_oracle(monkeypatch):
    """isensee2017_model_3d, n_labels = 3, on the layer-graph engine with fixed dropout masks.  Tolerances of the single-label twin
    test_isensee_graph_engine_fp32_vs_oracle: logits 1e-3 relative (tests/test_gpu_engine.py:408), Dice (the loss) 1e-4 absolute (:409),
    every gradient 5e-3 in relative L2 (:416, :422)."""
    import fetal_net.model as fmodel
    from oracle import isensee_oracle as I
    monkeypatch.setenv("FMRI_DTYPE", "fp32")
    N, sp = 2, (16, 16, 16)
    kw = dict(input_shape=(1,) + sp, depth=3, n_base_filters=8, n_segmentation_levels=2, dropout_rate=0.3, n_labels=3)
    model = fmodel.isensee2017_model_3d(include_label_wise_dice_coefficients=True, **kw)
    spec = I.IsenseeSpec(**kw)
    W = spec.init_weights(21)
    r2 = np.random.RandomState(5)
    for k in W:
        if k.endswith(("/bias", "/beta")):
            W[k] = (r2.randn(*W[k].shape) * 0.05).astype(np.float32)
        if k.endswith("/gamma"):
            W[k] = (1.0 + r2.randn(*W[k].shape) * 0.1).astype(np.float32)
    model.set_weights_dict(W)
    rs = np.random.RandomState(8)
    masks = {lv: ((rs.rand(N, spec.levels[lv]["filters"]) < 0.7).astype(np.float64) / 0.7) for lv in range(3)}
    x, y = _generator_batch(sp, True, (24, 24, 24))
    ref = I.loss_and_grads(spec, W, x.cpu().numpy(), y.cpu().numpy(), dropout_masks=masks)
    eng = model.engine(N)
    eng.set_dropout_masks({"spatial_dropout3d_%d" % (lv + 1): torch.tensor(masks[lv], dtype=torch.float32).cuda() for lv in range(3)})
    logs = model.train_on_batch(x, y)
    assert model.engine(N) is eng
    logits = eng.logits.cpu().numpy().reshape(N, *sp, 3).transpose(0, 4, 1, 2, 3)
    assert _rel(logits, ref["logits"]) <= 1e-3
    assert abs(logs[0] - ref["loss"]) <= 1e-4
    for name, L in eng.layout.items():
        if L["kind"] == "conv":
            mine = eng.w_view(name, eng.G).cpu().numpy().reshape((L["k"],) * 3 + (L["cout"], L["cin"])).transpose(0, 1, 2, 4, 3)
            assert _l2(mine, ref["grads"][name + "/kernel"]) <= 5e-3, name
        else:
            for key in ("gamma", "beta"):
                assert _l2(eng._v(name, key, eng.G).cpu().numpy(), ref["grads"][name + "/" + key]) <= 5e-3, (name, key)
    _check_label_logs(model, logs, eng, y)


def test_unet2d_three_labels_against_the_oracle(monkeypatch):
    """unet_model_2d, n_labels = 3.  Tolerances of the fp32 row of the single-label twin test_unet2d_fp32_and_bf16_vs_oracle
    (tests/test_gpu_engine.py:162): logits 1e-5 relative (:179), Dice (the loss) 1e-7 absolute (:180), every kernel gradient 1e-5 in relative
    L2 (:190-191)."""
    import fetal_net.model as fmodel
    from oracle import unet_oracle as O
    monkeypatch.setenv("FMRI_DTYPE", "fp32")
    kw = dict(input_shape=(32, 32, 5), depth=2, n_base_filters=8, n_labels=3)
    model = fmodel.unet_model_2d(include_label_wise_dice_coefficients=True, initial_learning_rate=1e-3, **kw)
    spec = O.Spec(ndim=2, **kw)
    W = spec.init_weights(11)
    model.set_weights_dict(W)
    x, y = _generator_batch((32, 32, 5), False, (40, 40, 12))
    assert tuple(x.shape) == (4, 32, 32, 5) and tuple(y.shape) == (4, 32, 32, 3)
    ref = O.loss_and_grads(spec, W, x.cpu().numpy(), y.cpu().numpy(), dtype=torch.float64)
    logs = model.train_on_batch(x, y)
    eng = model.engine(4)
    logits = eng.logits.cpu().numpy().reshape(ref["logits"].shape)
    print("unet2d x3: logits rel %.3e, loss abs %.3e" % (_rel(logits, ref["logits"]), abs(logs[0] - ref["loss"])))
    assert _rel(logits, ref["logits"]) <= 1e-5
    assert abs(logs[0] - ref["loss"]) <= 1e-7
    for name, L in eng.layout.items():
        gk = ref["grads"][name + "/kernel"]
        if L["kind"] == "conv":
            mine = eng.w_view(name, eng.G).cpu().numpy().reshape(3, 3, 3, L["cout"], L["cin"]).transpose(0, 1, 2, 4, 3)[1]
        else:
            mine = eng.w_view(name, eng.G).cpu().numpy().T.reshape(gk.shape)
        print("unet2d x3: %s grad l2 rel %.3e" % (name, _l2(mine, gk)))
        assert _l2(mine, gk) <= 1e-5, name
    _check_label_logs(model, logs, eng, y)


def test_fit_generator_and_prefetch_with_several_labels(tmp_path, monkeypatch):
    """the expanded targets through the generator's producer thread (same batches as without it) and through fit_generator /
    evaluate_generator: history, CSV log and evaluation all carry the label-wise names"""
    import fetal_net.model as fmodel
    from fetal_net.device_generator import device_data_generator
    from fetal_net.engine_model import CSVLogger
    monkeypatch.setenv("FMRI_DTYPE", "fp32")
    vols, truths = _volumes((40, 40, 12), n=2, seed=4)

    def gen(prefetch):
        np.random.seed(29)
        random.seed(29)
        return device_data_generator(_File(vols, truths), [0, 1], batch_size=4, n_labels=3, labels=LABELS, augment=AUG, patch_shape=(32, 32, 5),
                                     truth_index=2, truth_size=1, skip_blank=True, categorical=False, is3d=False, shuffle_index_list=False,
                                     prefetch=prefetch)

    plain = [next(g) for g in [gen(0)] for _ in range(2)]
    ahead = gen(1)
    threaded = [next(ahead) for _ in range(2)]
    ahead.close()
    for (x0, y0), (x1, y1) in zip(plain, threaded):
        assert torch.equal(x0, x1) and torch.equal(y0, y1) and tuple(y1.shape) == (4, 32, 32, 3)
    model = fmodel.unet_model_2d(input_shape=(32, 32, 5), depth=2, n_base_filters=8, n_labels=3, include_label_wise_dice_coefficients=True,
                                 initial_learning_rate=1e-3)
    log = str(tmp_path / "training.log")
    h = model.fit_generator(gen(0), steps_per_epoch=3, epochs=2, verbose=0, validation_data=gen(0), validation_steps=2,
                            callbacks=[CSVLogger(log)]).history
    names = ["label_%d_dice_coef" % i for i in range(3)]
    for k in names + ["val_" + n for n in names]:
        assert len(h[k]) == 2 and all(0.0 < v < 1.0 for v in h[k]), k
    assert all(n in open(log).readline() for n in names)
    out = model.evaluate_generator(gen(0), steps=2)
    assert len(out) == len(model.metrics_names) and all(np.isfinite(out))


def test_label_wise_flag_round_trips_through_a_checkpoint(tmp_path, monkeypatch):
    from fetal_net.training import load_old_model
    model, _, _ = _unet3d("fp32", monkeypatch)
    path = str(tmp_path / "m.h5")
    model.save(path)
    again = load_old_model(path)
    assert again.metrics_names == model.metrics_names and again.metrics_names[-1] == "label_2_dice_coef"
    assert again._builder_kwargs["include_label_wise_dice_coefficients"] is True


# ------------------------------------------------------------------------------------------------ prediction
def _prediction_model(is3d, monkeypatch):
    import fetal_net.model as fmodel
    from oracle import unet_oracle as O
    monkeypatch.setenv("FMRI_DTYPE", "fp32")
    if is3d:
        kw = dict(input_shape=(1, 16, 16, 8), depth=2, n_base_filters=8, n_labels=3)
        model, spec, patch = fmodel.unet_model_3d(**kw), O.Spec(**kw), (16, 16, 8)
    else:
        kw = dict(input_shape=(16, 16, 5), depth=2, n_base_filters=8, n_labels=3)
        model, spec, patch = fmodel.unet_model_2d(**kw), O.Spec(ndim=2, **kw), (16, 16, 5)
    W = spec.init_weights(13)
    last = spec.final["name"] + "/kernel"                   # wider logits: every label and the background occur in the map
    W[last] = W[last] * 8
    model.set_weights_dict(W)
    return model, patch


@pytest.mark.parametrize("is3d", [True, False], ids=["3d", "2d"])
def test_patch_wise_label_map_equals_the_labels_of_the_prediction(is3d, monkeypatch):
    """exactly: the same accumulators, the same float64 division, then the same comparisons - with the default graph path on"""
    from fetal_net.prediction import get_prediction_labels, patch_wise_label_map, patch_wise_prediction
    assert os.environ.get("FMRI_HIPGRAPH", "1") == "1"
    model, patch = _prediction_model(is3d, monkeypatch)
    data = np.random.RandomState(6).randn(1, 20, 20, 12)
    labels = (4, 1, 9)
    pred = patch_wise_prediction(model=model, data=data, patch_shape=patch, overlap_factor=0.5)
    assert pred.shape == (20, 20, 12, 3)
    for thr in (0.5, float(np.median(pred.max(axis=-1)))):
        want = get_prediction_labels(np.moveaxis(pred, -1, 0)[np.newaxis], threshold=thr, labels=labels)[0]
        got = patch_wise_label_map(model=model, data=data, patch_shape=patch, overlap_factor=0.5, threshold=thr, labels=labels)
        assert got.shape == (20, 20, 12) and got.dtype == np.uint8
        assert np.array_equal(got, want)
    assert set(np.unique(want).tolist()) == {0, 1, 4, 9}        # background and every label: the comparison is not trivial
    # a foreign model object leaves the device path: the labels of its host-tiled prediction

    class Host:
        output_shape = model.output_shape
        _input_layout = model._input_layout                  # (a 2-D output (N, X, Y, 3) alone would pass for a 3-D one)

        def predict(self, x):
            return model.predict(np.asarray(x))

    host = patch_wise_label_map(model=Host(), data=data, patch_shape=patch, overlap_factor=0.5, labels=labels)
    assert host.dtype == np.uint8 and (host != patch_wise_label_map(model=model, data=data, patch_shape=patch, overlap_factor=0.5,
                                                                    labels=labels)).mean() < 0.01


def test_run_validation_case_writes_the_label_map_beside_the_unchanged_files(tmp_path, monkeypatch):
    from fetal_net.prediction import prediction_to_image, run_validation_case
    from fetal_net.utils.nifti import load_nifti
    model, patch = _prediction_model(True, monkeypatch)
    rs = np.random.RandomState(4)

    class DataFile:
        root = _Root()

    DataFile.root.data = [rs.randn(20, 20, 12)]
    DataFile.root.truth = [(rs.rand(20, 20, 12) > 0.7).astype(np.uint8)]
    plain, with_map = str(tmp_path / "plain"), str(tmp_path / "labels")
    run_validation_case(0, plain, model, DataFile, ["volume"], patch_shape=patch, overlap_factor=0.5)
    fn = run_validation_case(0, with_map, model, DataFile, ["volume"], patch_shape=patch, overlap_factor=0.5, output_label_map=True,
                             labels=(4, 1, 9))
    assert os.path.basename(fn) == "prediction.nii.gz"
    assert sorted(os.listdir(plain)) == ["data_volume.nii.gz", "prediction.nii.gz", "truth.nii.gz"]
    assert sorted(os.listdir(with_map)) == ["data_volume.nii.gz", "prediction.nii.gz", "prediction_labels.nii.gz", "truth.nii.gz"]
    for f in os.listdir(plain):
        # the NIfTI bytes; the gzip container around them carries the time of writing
        assert gzip.open(os.path.join(plain, f)).read() == gzip.open(os.path.join(with_map, f)).read(), f
    pred = load_nifti(fn)
    lab = load_nifti(os.path.join(with_map, "prediction_labels.nii.gz"))
    assert np.issubdtype(lab.dtype, np.integer) and lab.shape == (20, 20, 12)
    assert np.array_equal(lab, prediction_to_image(np.moveaxis(pred, -1, 0)[np.newaxis], label_map=True, labels=(4, 1, 9)))


# ------------------------------------------------------------------------------------------------ evaluation
def _two_maps():
    rs = np.random.RandomState(0)
    t = np.zeros((24, 24, 12), np.uint8)
    t[3:12, 4:14, 2:8] = 1
    t[13:21, 5:17, 3:10] = 2
    t[5:10, 16:22, 4:9] = 4
    p = np.roll(t, (1, -1, 1), axis=(0, 1, 2))
    p[rs.rand(24, 24, 12) > 0.97] = 1
    p[p == 4] = 0                                       # label 4 is absent from the prediction: NaN / inf rules
    return t, p


@pytest.mark.parametrize("spacing", [None, (0.4, 0.4, 3.0)], ids=["unit", "anisotropic"])
def test_evaluate_case_labels_device_against_host(spacing):
    """bounds of tests/test_gpu_evaluate.py (its module docstring and check_metrics): counts, hd and hd95 identical at unit spacing; otherwise
    hd rtol 1e-15, hd95 rtol 2e-15; assd rtol 1e-15 + 2 n u with n the larger surface count"""
    from scipy import ndimage
    from fetal_net import evaluate as E
    t, p = _two_maps()
    labels = (2, 4, 1)
    got = E.evaluate_case_labels(t, p, labels, spacing=spacing, device=True)
    host = E.evaluate_case_labels(t, p, labels, spacing=spacing, device=False)
    assert list(got) == list(host) == list(labels)
    structure = ndimage.generate_binary_structure(3, 1)
    for v in labels:
        g, h = got[v], host[v]
        for k in ("dice", "vod", "volume_truth", "volume_prediction", "volume_difference", "sensitivity", "precision"):
            assert g[k] == h[k] or (np.isnan(g[k]) and np.isnan(h[k])), (v, k, g[k], h[k])
        if v == 4:
            assert g["dice"] == 0.0 and np.isnan(g["precision"]) and all(np.isnan(g[k]) and np.isnan(h[k]) for k in ("hd", "hd95", "assd"))
            continue
        assert h["hd"] > 0 and h["assd"] > 0
        n = max(int(E._border(t == v, structure).sum()), int(E._border(p == v, structure).sum()))
        if spacing is None:
            assert g["hd"] == h["hd"] and g["hd95"] == h["hd95"], v
        else:
            np.testing.assert_allclose(g["hd"], h["hd"], rtol=1e-15, atol=0)
            np.testing.assert_allclose(g["hd95"], h["hd95"], rtol=2e-15, atol=0)
        np.testing.assert_allclose(g["assd"], h["assd"], rtol=1e-15 + 2 * n * 2.0 ** -53, atol=0)
