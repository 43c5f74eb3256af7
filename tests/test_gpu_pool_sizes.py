"""-m gpu: max-pooling / nearest up-sampling with per-axis factors (csrc/pointwise.hip: fmri_maxpool3d_fwd / _bwd,
fmri_upsample_nearest_fwd / _bwd) and the models that use them - unet_model_3d / unet_model_2d with a pool size other than all 2s,
unet_model_2d with SpatialDropout2D - on the layer-graph engine.

Kernel level: exact against numpy restatements (windows flattened in (d, h, w) scan order; np.argmax returns the first maximum); the
fixed-window instantiations, pool (2, 2, 2) / planar (1, 2, 2), reproduce the recorded bits of the 2x entries they replaced
(tests/golden/pool_2x_digests.json), and (1, 2, 2) equals the run-time window (2, 2, 1) on rotated axes bit for bit.
Model level: a torch-CPU float64 restatement written here (F.conv, F.max_pool(pool), F.interpolate(scale_factor=pool, 'nearest'), fixed
dropout masks, autograd) with the bounds of test_gpu_engine.py::test_isensee_graph_engine_fp32_vs_oracle: logits 1e-3 relative, Dice 1e-4,
gradients 5e-3 relative L2."""
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from gpu_util import assert_same               # noqa: E402
import make_pool_2x_fixture as FX              # noqa: E402  (the inputs of the recorded digests, and how a tensor is hashed)

pytestmark = pytest.mark.gpu

DT = [torch.float32, torch.bfloat16]
POOLS = [(2, 2, 1), (1, 2, 2), (2, 1, 2), (3, 2, 1), (4, 1, 2)]
CHANNELS = [3, 8, 40]                  # scalar path, one 8-wide vector, five vectors per voxel
E_SHAPE = -1                           # FMRI_E_SHAPE (include/fmri_hip.h)


def _ops():
    from fmri_hip import ops
    return ops


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dtype).cuda()


def _host(t):
    torch.cuda.synchronize()
    return t.float().cpu().numpy()


def _dyadic(rs, shape, lo=-8, hi=8):
    """small integers / 8: exact in bf16, and so is any sum of up to 64 of them"""
    return rs.randint(lo, hi + 1, size=shape).astype(np.float32) / 8.0


def _windows(x, pool):
    """[N][D][H][W][C] -> [N][Do][Ho][Wo][pd*ph*pw][C], each window flattened in (d, h, w) scan order"""
    N, D, H, W, C = x.shape
    pd, ph, pw = pool
    w = x.reshape(N, D // pd, pd, H // ph, ph, W // pw, pw, C).transpose(0, 1, 3, 5, 2, 4, 6, 7)
    return w.reshape(N, D // pd, H // ph, W // pw, pd * ph * pw, C)


def _unwindows(w, pool, shape):
    N, D, H, W, C = shape
    pd, ph, pw = pool
    return w.reshape(N, D // pd, H // ph, W // pw, pd, ph, pw, C).transpose(0, 1, 4, 2, 5, 3, 6, 7).reshape(shape)


def _ref_maxpool_bwd(x, dy, pool, add=None, relu_mask=False):
    win = _windows(x, pool)
    first = np.argmax(win, axis=4)                                       # first occurrence of the maximum
    hot = (np.arange(win.shape[4])[None, None, None, None, :, None] == first[:, :, :, :, None, :])
    dx = _unwindows(np.where(hot, dy[:, :, :, :, None, :], np.float32(0)), pool, x.shape)
    if add is not None:
        dx = dx + add
    if relu_mask:
        dx = np.where(x > 0, dx, np.float32(0))
    return dx.astype(np.float32)


ADDS = ((0, 0), (16, 8), (7, 3))      # (channels beyond C, offset) of the wider tensor: own tensor | vector-aligned slice | slice that drops the vector width


def _check_maxpool(shape, pool, dtype, seed, adds=ADDS, relu_masks=(False, True)):
    ops = _ops()
    N, D, H, W, C = shape
    pd, ph, pw = pool
    rs = np.random.RandomState(seed)
    x = np.maximum(_dyadic(rs, shape), 0)                                 # post-ReLU: half the entries are zero, ties in most windows
    oshape = (N, D // pd, H // ph, W // pw, C)
    dy = _dyadic(rs, oshape)
    xd, dyd = _dev(x, dtype), _dev(dy, dtype)
    y = torch.full(oshape, float("nan"), dtype=dtype, device="cuda")
    ops.maxpool_fwd(xd, y, pool=pool)
    np.testing.assert_array_equal(_host(y), _windows(x, pool).max(axis=4))
    for extra, add_off in adds:                                           # the skip gradient `add`: none, or a channel slice of a wider tensor
        add_ld = C + extra if extra else 0
        add = _dyadic(rs, (N, D, H, W, add_ld)) if add_ld else None
        addd = _dev(add, dtype) if add_ld else None
        for relu_mask in relu_masks:
            dx = torch.full(shape, float("nan"), dtype=dtype, device="cuda")
            ops.maxpool_bwd(xd, dyd, dx, add=addd, add_off=add_off, relu_mask=relu_mask, pool=pool)
            ref = _ref_maxpool_bwd(x, dy, pool, add[..., add_off:add_off + C] if add_ld else None, relu_mask)
            np.testing.assert_array_equal(_host(dx), ref, err_msg="pool %s add (%d, %d) relu_mask %s" % (pool, add_ld, add_off, relu_mask))


def _check_upsample(shape, pool, dtype, seed, slices=ADDS):
    """shape = the LOW-resolution tensor"""
    ops = _ops()
    N, D, H, W, C = shape
    pd, ph, pw = pool
    rs = np.random.RandomState(seed)
    x = _dyadic(rs, shape)
    fine = (N, D * pd, H * ph, W * pw)
    up = x.repeat(pd, axis=1).repeat(ph, axis=2).repeat(pw, axis=3)
    xd = _dev(x, dtype)
    for extra, off in slices:
        ld = C + extra
        y = torch.full(fine + (ld,), -3.0, dtype=dtype, device="cuda")
        ops.upsample_fwd(xd, y, y_off=off, pool=pool)
        ref = np.full(fine + (ld,), -3.0, np.float32)
        ref[..., off:off + C] = up
        np.testing.assert_array_equal(_host(y), ref, err_msg="pool %s ld %d off %d" % (pool, ld, off))       # and nothing outside the slice
        dy = _dyadic(rs, fine + (ld,))
        dyd = _dev(dy, dtype)
        summed = _windows(np.ascontiguousarray(dy[..., off:off + C]), pool).sum(axis=4)                      # dyadic: exact in any order
        for masked in (False, True):
            dx = torch.full(shape, float("nan"), dtype=dtype, device="cuda")
            ops.upsample_bwd(dyd, dx, dy_off=off, xmask=xd if masked else None, pool=pool)
            ref = np.where(x > 0, summed, np.float32(0)) if masked else summed
            np.testing.assert_array_equal(_host(dx), ref, err_msg="pool %s ld %d off %d xmask %s" % (pool, ld, off, masked))


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("pool", POOLS)
def test_maxpool_forward_backward_exact(pool, C, dtype):
    """two windows per axis, N = 2: the pooled tensor, and the gradient routed to the FIRST maximum of every window with the fused skip
    gradient (add_ld > C, add_off > 0) and ReLU mask"""
    _check_maxpool((2, 2 * pool[0], 2 * pool[1], 2 * pool[2], C), pool, dtype, seed=11)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("pool", POOLS)
def test_upsample_forward_backward_exact(pool, C, dtype):
    """forward into a channel slice of a wider tensor (y_ld > C, y_off > 0), backward with and without xmask"""
    _check_upsample((2, 2, 2, 2, C), pool, dtype, seed=12)


# 2 x 32 x 64 x 64 x 32 at 8 channels per thread is 262,144 windows-times-vectors for the pooling kernels: every thread of the capped grid
# (4,096 workgroups of 256 = 1,048,576 threads) runs its loop once.  The same volume with 33 channels (no vector: one thread per channel)
# is 2,162,688: the grid-stride loop wraps twice.  Both run.
@pytest.mark.parametrize("C,dtype", [(32, torch.bfloat16), (33, torch.float32)])
def test_grid_stride_loop_wraps(C, dtype):
    _check_maxpool((2, 32, 64, 64, C), (2, 2, 1), dtype, seed=13, adds=ADDS[1:2] if C == 32 else ADDS[2:], relu_masks=(True,))
    _check_upsample((2, 16, 32, 64, C), (2, 2, 1), dtype, seed=14, slices=ADDS[1:2] if C == 32 else ADDS[2:])


def _recorded():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pool_2x_digests.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("planar", [False, True])
def test_all_twos_equals_the_2x_kernels_bit_for_bit(planar, C, dtype):
    """pool=None and the explicit (2, 2, 2) - planar: (1, 2, 2) - give, output for output, the sha256 that the retired 2x entries gave on
    the same non-dyadic inputs (tests/golden/pool_2x_digests.json, recorded by make_pool_2x_fixture.py on the last commit that had them):
    forward, backward with skip gradient and ReLU mask and without both, both up-sampling directions through a channel slice"""
    recorded, key = _recorded(), FX.case_key(planar, C, dtype)
    for pool in (None, (1, 2, 2) if planar else (2, 2, 2)):
        got = FX.pool_outputs(_ops(), planar, C, dtype, pool=pool)
        assert len(got) == 6
        for name, t in got.items():
            assert FX.digest(t) == recorded["%s/%s" % (key, name)], (key, name, pool)


def test_adam_step_equals_the_recorded_bits():
    """three fmri_adam_step steps on 4,099 elements (quads and a 3-element tail), grad_scale 0.5: p, m and v hash to what the stand-alone
    Adam kernel gave before it became an instantiation of the optimizer template (same fixture)"""
    recorded = _recorded()
    got = FX.adam_outputs(_ops().adam_step)
    assert sorted(got) == ["m", "p", "v"]
    for name, t in got.items():
        assert FX.digest(t) == recorded["adam/%s" % name], name


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("vol", [(1, 5, 6, 4), (2, 4, 6, 4)])
def test_fixed_122_equals_run_time_221_on_permuted_axes(vol, C, dtype):
    """the one place where a fixed and the run-time instantiation meet: window (1, 2, 2) on x against window (2, 2, 1) on x with its axes
    rotated (d, h, w) -> (h, w, d).  Both walk the same voxels in the same order, so every result agrees bit for bit after rotating back:
    forward, backward with skip gradient and ReLU mask, both up-sampling directions through a channel slice, with xmask"""
    ops = _ops()
    fine, low, wide = vol + (C,), (vol[0], vol[1], vol[2] // 2, vol[3] // 2, C), vol + (C + FX.WIDE,)
    rot = lambda t: t.permute(0, 2, 3, 1, 4).contiguous()
    back = lambda t: t.permute(0, 3, 1, 2, 4).contiguous()
    new = lambda ref: torch.zeros_like(ref)
    x = torch.relu(FX.formula(fine, 1, dtype))
    dy, add = FX.formula(low, 2, dtype), FX.formula(wide, 3, dtype)
    xr, dyr, addr = rot(x), rot(dy), rot(add)
    a, b = dict(planar=True, pool=(1, 2, 2)), dict(pool=(2, 2, 1))
    pairs = {
        "maxpool fwd": (ops.maxpool_fwd(x, new(dy), **a), ops.maxpool_fwd(xr, new(dyr), **b)),
        "maxpool bwd + add + mask": (ops.maxpool_bwd(x, dy, new(x), add=add, add_off=FX.OFF, relu_mask=True, **a),
                                     ops.maxpool_bwd(xr, dyr, new(xr), add=addr, add_off=FX.OFF, relu_mask=True, **b)),
        "upsample fwd": (ops.upsample_fwd(dy, new(add), y_off=FX.OFF, **a), ops.upsample_fwd(dyr, new(addr), y_off=FX.OFF, **b)),
        "upsample bwd + xmask": (ops.upsample_bwd(add, new(dy), dy_off=FX.OFF, xmask=dy, **a),
                                 ops.upsample_bwd(addr, new(dyr), dy_off=FX.OFF, xmask=dyr, **b)),
        "upsample bwd": (ops.upsample_bwd(add, new(dy), dy_off=FX.OFF, **a), ops.upsample_bwd(addr, new(dyr), dy_off=FX.OFF, **b)),
    }
    torch.cuda.synchronize()
    for what, (fixed, run_time) in pairs.items():
        assert float(fixed.float().abs().max()) > 0, what
        assert_same(back(run_time), fixed, what)


def test_shape_errors_are_return_codes():
    """FMRI_E_SHAPE before anything is launched: factor 0, factor 5, pool (1, 1, 1), a dimension that its factor does not divide, a channel
    slice that does not fit"""
    from fmri_hip._lib import F32, lib
    L = lib()
    x = torch.zeros((1, 4, 4, 4, 8), dtype=torch.float32, device="cuda")
    y = torch.zeros((1, 8, 8, 8, 8), dtype=torch.float32, device="cuda")          # large enough for every well-formed call below
    p = lambda t: t.data_ptr()
    s = torch.cuda.current_stream().cuda_stream
    for pool in ((0, 2, 2), (2, 5, 2), (2, 2, -1), (1, 1, 1)):
        assert L.fmri_maxpool3d_fwd(p(x), p(y), 1, 4, 4, 4, 8, *pool, F32, s) == E_SHAPE, pool
        assert L.fmri_maxpool3d_bwd(p(x), p(y), 0, 0, 0, p(y), 1, 4, 4, 4, 8, *pool, 0, F32, s) == E_SHAPE, pool
        assert L.fmri_upsample_nearest_fwd(p(x), p(y), 8, 0, 1, 2, 2, 2, 8, *pool, F32, s) == E_SHAPE, pool
        assert L.fmri_upsample_nearest_bwd(p(y), 8, 0, 0, p(x), 1, 2, 2, 2, 8, *pool, F32, s) == E_SHAPE, pool
    for pool in ((3, 2, 2), (2, 3, 1), (1, 2, 3)):                               # 4 is no multiple of 3
        assert L.fmri_maxpool3d_fwd(p(x), p(y), 1, 4, 4, 4, 8, *pool, F32, s) == E_SHAPE, pool
        assert L.fmri_maxpool3d_bwd(p(x), p(y), 0, 0, 0, p(y), 1, 4, 4, 4, 8, *pool, 0, F32, s) == E_SHAPE, pool
    assert L.fmri_upsample_nearest_fwd(p(x), p(y), 8, 1, 1, 2, 2, 2, 8, 2, 2, 1, F32, s) == E_SHAPE       # y_ld < y_off + C
    assert L.fmri_upsample_nearest_bwd(p(y), 8, 1, 0, p(x), 1, 2, 2, 2, 8, 2, 2, 1, F32, s) == E_SHAPE    # dy_ld < dy_off + C
    assert L.fmri_maxpool3d_bwd(p(x), p(y), p(y), 8, 1, p(y), 1, 4, 4, 4, 8, 2, 2, 1, 0, F32, s) == E_SHAPE   # add_ld < add_off + C
    assert L.fmri_maxpool3d_fwd(p(x), p(y), 1, 4, 4, 4, 8, 2, 2, 1, F32, s) == 0                            # and a well-formed call is accepted
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ models against the float64 restatement
def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def _restatement(spec, W, x, y, pool, masks=None):
    """unet_model_3d / unet_model_2d in torch-CPU float64 with MaxPooling(pool) / UpSampling(pool) and fixed SpatialDropout2D masks
    ({layer name: [N, C]}, already scaled by 1 / (1 - p)); the layer walk is oracle.unet_oracle.forward's.
    -> dict(logits, dice, grads{name: ndarray in Keras layout})"""
    from oracle import unet_oracle as O
    nd = spec.ndim
    Wt = O.to_torch(W, torch.float64, requires_grad=True)
    h = torch.tensor(np.asarray(x), dtype=torch.float64)
    yt = torch.tensor(np.asarray(y), dtype=torch.float64)
    if nd == 2:
        h = h.permute(0, 3, 1, 2)
    conv = F.conv3d if nd == 3 else F.conv2d
    pool_fn = F.max_pool3d if nd == 3 else F.max_pool2d
    drop_no = [0]

    def block(h, b, dropout_behind=False):
        k = Wt[b["name"] + "/kernel"]
        h = conv(h, k.permute(*((4, 3, 0, 1, 2) if nd == 3 else (3, 2, 0, 1))), Wt[b["name"] + "/bias"], padding=1)
        if b.get("bn"):
            h = O._batchnorm_train(h, Wt[b["bn"] + "/gamma"], Wt[b["bn"] + "/beta"])
        h = F.relu(h)
        if dropout_behind and masks is not None:
            drop_no[0] += 1
            m = torch.tensor(np.asarray(masks["spatial_dropout2d_%d" % drop_no[0]]), dtype=torch.float64)
            h = h * m.reshape(m.shape + (1,) * nd)
        return h

    skips = []
    for ld, lv in enumerate(spec.enc):
        h = block(h, lv[0], dropout_behind=True)
        h = block(h, lv[1])
        skips.append(h)
        if ld < spec.depth - 1:
            h = pool_fn(h, pool)
    for dlv in spec.dec:
        h = F.interpolate(h, scale_factor=tuple(float(p) for p in pool), mode="nearest")
        h = torch.cat([h, skips[dlv["level"]]], dim=1)
        h = block(h, dlv["blocks"][0], dropout_behind=True)
        h = block(h, dlv["blocks"][1])
    f = spec.final
    k = Wt[f["name"] + "/kernel"]
    logits = conv(h, k.permute(*((4, 3, 0, 1, 2) if nd == 3 else (3, 2, 0, 1))), Wt[f["name"] + "/bias"])
    if nd == 2:
        logits = logits.permute(0, 2, 3, 1)
    dice = O.dice_coefficient_t(yt, torch.sigmoid(logits))
    (-dice).backward()
    return dict(logits=logits.detach().numpy(), dice=float(dice.detach()), grads={k: v.grad.numpy().copy() for k, v in Wt.items()})


def _weights(spec, seed):
    W = spec.init_weights(seed)
    r2 = np.random.RandomState(5)
    for k in W:
        if k.endswith(("/bias", "/beta")):
            W[k] = (r2.randn(*W[k].shape) * 0.05).astype(np.float32)
        if k.endswith("/gamma"):
            W[k] = (1.0 + r2.randn(*W[k].shape) * 0.1).astype(np.float32)
    return W


def _compare(eng, ref, xd, yd):
    """logits 1e-3 relative, Dice 1e-4, every kernel / bias / gamma / beta gradient 5e-3 relative L2"""
    eng.forward(xd)
    sums = eng.loss_forward(yd)
    eng.backward(yd)
    torch.cuda.synchronize()
    logits = eng.logits.cpu().numpy().reshape(ref["logits"].shape)
    e = _rel(logits, ref["logits"])
    d = abs(eng.metrics_from_sums(sums.cpu().numpy())["dice_coefficient"] - ref["dice"])
    print("logits rel %.3e, dice abs %.3e" % (e, d))
    assert e <= 1e-3
    assert d <= 1e-4
    assert len(eng.layout) * 2 == len(ref["grads"])
    worst = 0.0
    for name, L in eng.layout.items():
        if L["kind"] == "conv":
            g = eng.w_view(name, eng.G).cpu().numpy().reshape((L["k"],) * 3 + (L["cout"], L["cin"])).transpose(0, 1, 2, 4, 3)
            if eng.nd == 2:
                if L["k"] == 3:
                    assert float(np.abs(g[0]).max()) == 0.0 and float(np.abs(g[2]).max()) == 0.0, name     # the dead kd planes of a 2-D filter
                g = g[L["k"] // 2]
            pairs = (("kernel", g), ("bias", eng._v(name, "b", eng.G).cpu().numpy()))
        else:
            pairs = tuple((key, eng._v(name, key, eng.G).cpu().numpy()) for key in ("gamma", "beta"))
        for key, mine in pairs:
            gk = ref["grads"][name + "/" + key]
            assert mine.shape == gk.shape and np.isfinite(mine).all(), (name, key)
            if key == "bias" and float(np.abs(gk).max()) < 1e-9:
                continue                      # the bias of a conv in front of a normalisation: exactly zero gradient, only noise to compare
            e = np.linalg.norm(mine - gk) / (np.linalg.norm(gk) + 1e-30)
            worst = max(worst, e)
            assert e <= 5e-3, (name, key, e)
    print("worst gradient rel L2 %.3e" % worst)


KW3 = dict(input_shape=(1, 16, 16, 4), pool_size=(2, 2, 1), depth=3, n_base_filters=4)


def _setup3(batch_normalization, dtype=torch.float32, kw=KW3):
    import fetal_net.model as fmodel
    from fmri_hip.graph_engine import LayerGraphEngine
    from oracle import unet_oracle as O
    N, sp = 2, kw["input_shape"][1:]
    model = fmodel.unet_model_3d(batch_normalization=batch_normalization, **kw)
    assert model._unsupported is None and model._graph_engine
    spec = O.Spec(kw["input_shape"], depth=3, n_base_filters=4, batch_normalization=batch_normalization)
    W = _weights(spec, 21)
    x, y = O.synthetic_batch((N, 1) + sp)
    eng = LayerGraphEngine(model.layers, N, dtype=dtype)
    eng.load_keras_weights(W)
    xd = torch.from_numpy(x).cuda().reshape(N, *sp, 1).to(dtype).contiguous()
    yd = torch.from_numpy(y).cuda().reshape(-1).contiguous()
    return model, spec, W, x, y, eng, xd, yd


@pytest.mark.parametrize("batch_normalization", [False, True])
def test_unet3d_anisotropic_pool_fp32_vs_restatement(batch_normalization):
    model, spec, W, x, y, eng, xd, yd = _setup3(batch_normalization)
    pooled = [o for o in eng.ops if o["kind"] in ("maxpool", "upsample")]
    assert len(pooled) == 4 and all(o["pool"] == (2, 2, 1) for o in pooled)
    assert eng.T["max_pooling3d_2"].shape[1:4] == (4, 4, 4)                      # Z is never pooled
    _compare(eng, _restatement(spec, W, x, y, (2, 2, 1)), xd, yd)


@pytest.mark.parametrize("pool", [(2, 2), (2, 1)])
def test_unet2d_dropout_and_asymmetric_pool_fp32_vs_restatement(pool):
    import fetal_net.model as fmodel
    from fmri_hip.graph_engine import LayerGraphEngine
    from oracle import unet_oracle as O
    N, X, Y, C = 2, 16, 16, 5
    model = fmodel.unet_model_2d(input_shape=(X, Y, C), depth=3, n_base_filters=4, dropout_rate=0.2, pool_size=pool)
    assert model._unsupported is None and model._graph_engine
    spec = O.Spec((X, Y, C), ndim=2, depth=3, n_base_filters=4, dropout_rate=0.2)
    W = _weights(spec, 23)
    rs = np.random.RandomState(12)
    x = rs.randn(N, X, Y, C).astype(np.float32)
    y = (rs.rand(N, X, Y, 1) > 0.7).astype(np.uint8)
    drops = [l for l in model.layers if l.class_name == "SpatialDropout2D"]
    assert [l.name for l in drops] == ["spatial_dropout2d_%d" % (i + 1) for i in range(5)]
    masks = {l.name: (rs.rand(N, l.output_shape[1]) < 0.8).astype(np.float64) / 0.8 for l in drops}
    assert any((m == 0).any() for m in masks.values())                           # something is dropped
    eng = LayerGraphEngine(model.layers, N, dtype=torch.float32)
    assert eng.planar
    for o in eng.ops:
        if o["kind"] in ("maxpool", "upsample"):
            assert o["pool"] == (None if pool == (2, 2) else pool)                 # all 2s: None, the fixed-window kernels
    eng.load_keras_weights(W)
    eng.set_dropout_masks({k: torch.tensor(v, dtype=torch.float32).cuda() for k, v in masks.items()})
    xd = torch.from_numpy(x).cuda().unsqueeze(0).contiguous()
    yd = torch.from_numpy(y).cuda().reshape(-1).contiguous()
    _compare(eng, _restatement(spec, W, x, y, pool, masks), xd, yd)


# ------------------------------------------------------------------------------------------------ public surface
class _Proxy:
    """not a fetal_net Model: patch_wise_prediction tiles on the host and calls .predict"""

    def __init__(self, model):
        self.model, self.output_shape = model, model.output_shape

    def predict(self, x):
        return self.model.predict(x)


@pytest.mark.parametrize("which", ["unet3d_pool221", "unet2d_dropout"])
def test_public_surface(which, monkeypatch):
    import fetal_net.model as fmodel
    import fetal_net.prediction as P
    rs = np.random.RandomState(3)
    N = 2
    if which == "unet3d_pool221":
        model = fmodel.unet_model_3d(initial_learning_rate=5e-3, compute_dtype="fp32", **KW3)
        x = rs.randn(N, 1, 16, 16, 4).astype(np.float32)
        y = (x > 0.3).astype(np.uint8)
        patch, out_shape = (16, 16, 4), (N, 1, 16, 16, 4)
    else:
        model = fmodel.unet_model_2d(input_shape=(16, 16, 5), depth=3, n_base_filters=4, dropout_rate=0.2, initial_learning_rate=5e-3,
                                     compute_dtype="fp32")
        x = rs.randn(N, 16, 16, 5).astype(np.float32)
        y = (x[..., 2:3] > 0.3).astype(np.uint8)
        patch, out_shape = (16, 16, 5), (N, 16, 16, 1)
    p0 = model.predict(x)
    assert p0.shape == out_shape and np.isfinite(p0).all() and 0.0 <= p0.min() and p0.max() <= 1.0
    torch.manual_seed(0)                                  # the dropout masks are drawn with torch's device generator
    losses = [model.train_on_batch(x, y)[0] for _ in range(20)]
    assert min(losses[-5:]) < losses[0], losses
    a, b = model.predict(x), model.predict(x)
    np.testing.assert_array_equal(a, b)                   # dropout is the identity at inference
    assert float(np.abs(a - p0).max()) > 1e-4             # and the training steps moved the weights
    t = model.test_on_batch(x, y)
    assert np.isfinite(t).all()
    np.testing.assert_allclose(model.test_on_batch(x, y), t, rtol=1e-9, atol=0)       # no dropout in evaluation either (the metric sums are fp64 atomics)

    class NoHostTiles:
        def __init__(self, *a, **k):
            raise AssertionError("the device tile loop was not taken")

    vol = rs.randn(1, 24, 24, 8)
    with monkeypatch.context() as mp:
        mp.setattr(P, "ThreadedGenerator", NoHostTiles)
        dev = P.patch_wise_prediction(model, vol, patch, overlap_factor=0.5)
    assert model.__dict__.get("_tile_state") is not None
    host = P.patch_wise_prediction(_Proxy(model), vol, patch, overlap_factor=0.5)
    assert dev.shape == host.shape == (24, 24, 8, 1)
    np.testing.assert_allclose(dev, host, rtol=0, atol=2e-6)


# ------------------------------------------------------------------------------------------------ bf16, channel-padded
# profiles/r06_pool_sizes_timing.log, line "bf16 padded vs fp32 logits, pool (2, 2, 2)": unet_model_3d(input_shape=(1, 16, 16, 16), depth=3,
# n_base_filters=4) on the layer-graph engine of the parent commit, bf16 (channel-padded) against fp32 with the weights and the batch of
# this test's recipe: max |logits_bf16 - logits_fp32| / max |logits_fp32| = 7.495e-3.  The bound is twice that: the anisotropic model differs only
# in how many voxels its deeper levels keep, the factor covers the seed-to-seed spread.
BF16_LOGITS_REL_222 = 7.495e-3


def test_unet3d_anisotropic_pool_bf16_padded_engine():
    _, _, _, _, _, ef, xf, yd = _setup3(False, torch.float32)
    _, _, _, _, _, eb, xb, _ = _setup3(False, torch.bfloat16)
    assert eb.pad and not ef.pad
    for e, xd in ((ef, xf), (eb, xb)):
        e.forward(xd)
        e.loss_forward(yd)
        e.backward(yd)
    torch.cuda.synchronize()
    # the padding never leaks: exactly zero in every tensor, in every tensor's gradient and in the padded weight-gradient images
    padded = [name for name, t in eb.T.items() if t.shape[-1] > eb.clog[name]]
    assert {"max_pooling3d_1", "max_pooling3d_2", "up_sampling3d_2"} <= set(padded)      # 8, 16 and 16 channels in 32 (up_sampling3d_1 has 32)
    assert eb._has_grad == set(eb.T)
    for name in padded:
        assert float(eb.T[name][..., eb.clog[name]:].float().abs().max()) == 0.0, name
        assert float(eb.Gt[name][..., eb.clog[name]:].float().abs().max()) == 0.0, name
    for name, dw in eb.dWp.items():
        L = eb.layout[name]
        live = torch.zeros(dw.shape[1:], dtype=torch.bool, device="cuda")
        live[:L["cout"], eb.cin_map[name]] = True
        assert float(dw[:, ~live].abs().max()) == 0.0 and float(eb.dbp[name][L["cout"]:].abs().max()) == 0.0, name
        assert float(dw[:, live].abs().max()) > 0.0, name
    lf, lb = ef.logits.cpu().numpy(), eb.logits.cpu().numpy()
    err = float(np.abs(lb - lf).max() / np.abs(lf).max())
    print("bf16 padded vs fp32 logits, pool (2, 2, 1): %.3e" % err)
    assert err <= 2 * BF16_LOGITS_REL_222
