"""norm_net_model on the GPU: the frozen pass of UNetEngine (input gradient, nothing of the engine moves), the linear head of the
layer-graph engine, the chain of the two against the composed oracles (isensee_oracle's logits are unet_oracle's input; torch autograd
gives every gradient), and the model surface (builder, checkpoints, train_model, patch_wise_prediction).

Bars: `gpu_util.bar`, each <= 2x the value measured on MI355X with FMRI_MEASURE=1 (profiles/r07_norm_net_bars.json).
"""
import glob
import os

import numpy as np
import pytest
import torch

from gpu_util import assert_same, bar, f64

pytestmark = pytest.mark.gpu

KW_NORM = dict(n_base_filters=4, depth=3, dropout_rate=0, n_segmentation_levels=2)


def _l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))


def _grad_bars(tag, G, ref, rel_limit, zero_limit):
    """every parameter gradient against fp64 autograd, relative L2 per tensor.  The bias of a convolution in front of an
    InstanceNormalization cancels in the normalisation: its true gradient is zero (autograd: below 1e-9 of the kernel's), so there the
    engine's value is measured against the same layer's kernel gradient instead"""
    for k, g in ref.items():
        gk = np.linalg.norm(ref[k.rsplit("/", 1)[0] + "/kernel"]) if k.endswith("/bias") else 0.0
        if k.endswith("/bias") and np.linalg.norm(g) < 1e-9 * gk:
            bar(tag + ".zero_bias_grad_l2_rel_to_kernel", float(np.linalg.norm(G[k]) / gk), zero_limit)
        else:
            bar(tag + ".grad_l2_rel", _l2(G[k], g), rel_limit)


def _perturb(W, seed=11):
    """biases, gamma and beta off their initial 0 / 1 so that their gradients and the normalisation's affine part are exercised"""
    rs = np.random.RandomState(seed)
    for k in W:
        if k.endswith(("/bias", "/beta")):
            W[k] = (0.1 * rs.randn(*W[k].shape)).astype(np.float32)
        elif k.endswith("/gamma"):
            W[k] = (1.0 + 0.1 * rs.randn(*W[k].shape)).astype(np.float32)
    return W


def _unet_engine(sp, base, dtype, bn=False, N=2, **kw):
    from fmri_hip.engine import UNetEngine, UNetPlan
    return UNetEngine(UNetPlan(1, sp, depth=2, n_base_filters=base, norm="batch" if bn else None), N, dtype=dtype, **kw)


def _dev(x, y, dtype):
    N, sp = x.shape[0], x.shape[2:]
    return (torch.from_numpy(x).cuda().to(dtype).reshape(N, *sp, 1).contiguous(), torch.from_numpy(y).cuda().reshape(-1).contiguous())


# ------------------------------------------------------------------------------------------------------------------ UNetEngine, frozen pass
@pytest.mark.parametrize("bn", [False, True], ids=["plain", "bn"])
def test_unet_engine_input_gradient_fp32_and_frozen_pass(bn):
    from oracle import unet_oracle as O
    sp, N = (16, 16, 8), 2
    spec = O.Spec((1,) + sp, depth=2, n_base_filters=8, batch_normalization=bn)
    W = _perturb(spec.init_weights(4))
    x, y = O.synthetic_batch((N, 1) + sp)
    Wt = O.to_torch(W, torch.float64)
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    (-O.dice_coefficient_t(torch.tensor(y, dtype=torch.float64), O.forward(spec, Wt, xt)[1])).backward()
    ref = xt.grad.permute(0, 2, 3, 4, 1).numpy()
    eng = _unet_engine(sp, 8, torch.float32, bn, N, input_grad=True)
    assert eng.route["first_dgrad"] == "generic"          # fp32: fmri_conv3d_dgrad on the engine's own [27][Cin][Cout] image
    eng.load_keras_weights(W)
    xd, yd = _dev(x, y, torch.float32)
    # an optimizer step first, so that M, V and t are not trivially zero (lr 0: the weights stay the oracle's)
    eng.train_step(xd, yd, 0.0)
    torch.cuda.synchronize()
    keep = [t.clone() for t in (eng.P, eng.M, eng.V)] + [eng.moving[k].clone() for k in sorted(eng.moving)]
    t0 = eng.t
    for _ in range(2):
        eng.forward(xd, update_moving=False)
        eng.loss_forward(yd)
        eng.backward(yd, params=False)
    torch.cuda.synchronize()
    got = eng.input_gradient()
    assert got.dtype == torch.float32 and tuple(got.shape) == (N,) + sp + (1,)
    bar("unet_fp32%s.input_grad_l2_rel" % ("_bn" if bn else ""), _l2(got.cpu().numpy(), ref), 1.8e-6 if bn else 1e-6)            # measured 9.3e-7 / 5.1e-7
    now = [eng.P, eng.M, eng.V] + [eng.moving[k] for k in sorted(eng.moving)]
    assert eng.t == t0 and len(now) == (9 if bn else 3)          # P, M, V and the moving statistics of the six normalised blocks
    for a, b in zip(keep, now):
        assert_same(b, a, "frozen pass moved engine state")


def test_unet_engine_default_flags_leave_the_parameter_gradients_alone(monkeypatch):
    """an ordinary backward of an engine built with input_grad=True gives the bits of one built without.  Compared under
    FMRI_DETERMINISTIC=1: the default mode adds workgroup partial sums with float atomics, whose order - and with it the last bit - differs
    between two runs of one and the same engine."""
    from oracle import unet_oracle as O
    monkeypatch.setenv("FMRI_DETERMINISTIC", "1")
    sp, N = (16, 16, 8), 2
    W = _perturb(O.Spec((1,) + sp, depth=2, n_base_filters=8).init_weights(4))
    x, y = O.synthetic_batch((N, 1) + sp)
    xd, yd = _dev(x, y, torch.float32)
    out = []
    for ig in (False, True):
        eng = _unet_engine(sp, 8, torch.float32, False, N, input_grad=ig)
        assert eng.deterministic
        eng.load_keras_weights(W)
        eng.forward(xd)
        eng.loss_forward(yd)
        eng.backward(yd)
        torch.cuda.synchronize()
        out.append(eng.G.clone())
        eng.close()
    assert float(out[0].abs().max()) > 0
    assert_same(out[1], out[0], "parameter gradients with input_grad=True")


def test_unet_engine_input_gradient_bf16_on_the_first_layer_kernel():
    from oracle import unet_oracle as O
    sp, N = (8, 16, 32), 2
    W = _perturb(O.Spec((1,) + sp, depth=2, n_base_filters=32).init_weights(4))
    x, y = O.synthetic_batch((N, 1) + sp)
    got = {}
    for dtype in (torch.float32, torch.bfloat16):
        eng = _unet_engine(sp, 32, dtype, False, N, input_grad=True)
        assert eng.route["first_dgrad"] == ("first" if dtype == torch.bfloat16 else "generic")
        eng.load_keras_weights(W)
        xd, yd = _dev(x, y, dtype)
        eng.forward(xd, update_moving=False)
        eng.loss_forward(yd)
        eng.backward(yd, params=False)
        torch.cuda.synchronize()
        got[dtype] = eng.input_gradient().cpu().numpy()
    assert np.isfinite(got[torch.bfloat16]).all()
    bar("unet_bf16.input_grad_l2_rel_vs_fp32", _l2(got[torch.bfloat16], got[torch.float32]), 0.18)      # measured 0.093


# ------------------------------------------------------------------------------------------------------------------ linear head
def test_linear_head_predict_and_outside_gradient_vs_oracle():
    import fetal_net.model as fmodel
    from oracle import isensee_oracle as IO, unet_oracle as O
    sp, N = (16, 16, 16), 2
    model = fmodel.isensee2017_model_3d((1,) + sp, activation_name=None, compute_dtype="fp32", **KW_NORM)
    assert model._unsupported is None
    spec = IO.IsenseeSpec((1,) + sp, 4, 3, 0, 2)
    W = _perturb(spec.init_weights(5))
    model.set_weights_dict(W)
    x, _ = O.synthetic_batch((N, 1) + sp)
    Wt = O.to_torch(W, torch.float64, requires_grad=True)
    logits = IO.forward(spec, Wt, torch.tensor(x, dtype=torch.float64))[0]
    p = model.predict(x)
    assert p.shape == (N, 1) + sp
    bar("linear_head.predict_max_rel", float(np.abs(p - logits.detach().numpy()).max() / logits.detach().abs().max()), 1.9e-6)     # measured 9.4e-7
    g = np.random.RandomState(2).randn(N, *sp, 1).astype(np.float32)
    (logits * torch.tensor(g, dtype=torch.float64).permute(0, 4, 1, 2, 3)).sum().backward()
    eng = model.engine(N)
    assert eng.linear
    eng.forward(model._to_device_x(x))
    eng.backward(eng._dummy_y, dprobs=torch.from_numpy(g).cuda(), seg_loss=False)
    torch.cuda.synchronize()
    G = eng.flat_to_keras(eng.G.cpu().numpy())
    _grad_bars("linear_head", G, {k: v.grad.numpy() for k, v in Wt.items()}, 6.7e-6, 2.4e-7)       # measured 3.4e-6, 1.2e-7
    with pytest.raises(NotImplementedError):
        eng.backward(eng._dummy_y, dprobs=torch.from_numpy(g).cuda(), seg_loss=True)
    with pytest.raises(NotImplementedError):
        model.train_on_batch(x, np.zeros((N, 1) + sp, np.uint8))


# ------------------------------------------------------------------------------------------------------------------ the chain
def _chain(sp, seg_base, dtype, lr=5e-4, seg_seed=4, norm_seed=5):
    import fetal_net.model as fmodel
    from oracle import isensee_oracle as IO, unet_oracle as O
    seg = fmodel.unet_model_3d((1,) + sp, depth=2, n_base_filters=seg_base, compute_dtype=dtype)
    sspec = O.Spec((1,) + sp, depth=2, n_base_filters=seg_base)
    Ws = _perturb(sspec.init_weights(seg_seed))
    seg.set_weights_dict(Ws)
    model = fmodel.norm_net_model((1,) + sp, old_model_path=seg, initial_learning_rate=lr, compute_dtype=dtype, **KW_NORM)
    nspec = IO.IsenseeSpec((1,) + sp, 4, 3, 0, 2)
    Wn = _perturb(nspec.init_weights(norm_seed))
    model.set_weights_dict(Wn)
    return model, seg, (nspec, Wn, sspec, Ws)


def _chain_oracle(oracle, x, y):
    from oracle import isensee_oracle as IO, unet_oracle as O
    nspec, Wn, sspec, Ws = oracle
    Wt = O.to_torch(Wn, torch.float64, requires_grad=True)
    mid = IO.forward(nspec, Wt, torch.tensor(x, dtype=torch.float64))[0]
    probs = O.forward(sspec, O.to_torch(Ws, torch.float64), mid)[1]
    yt = torch.tensor(y, dtype=torch.float64)
    dice = O.dice_coefficient_t(yt, probs)
    (-dice).backward()
    p, t = probs.detach().numpy(), y.astype(np.float64)
    inter = ((p > 0.5) * t).sum()
    vod = (inter + 1.0) / ((p > 0.5).sum() + t.sum() - inter + 1.0)
    return dict(loss=-float(dice.detach()), acc=float(((p > 0.5) == (t > 0.5)).mean()), vod=float(vod), probs=p,
                grads={k: v.grad.numpy() for k, v in Wt.items()})


def test_chain_fp32_vs_composed_oracle_and_frozen_segmenter():
    from oracle import unet_oracle as O
    sp, N = (16, 16, 16), 2
    model, seg, oracle = _chain(sp, 8, "fp32", lr=0.0)
    assert type(model).__name__ == "NormNetModel" and model.name == "NormNetModel" and model.seg_net is seg
    assert model.metrics_names == ["loss", "binary_accuracy", "vod_coefficient"]
    x, y = O.synthetic_batch((N, 1) + sp)
    ref = _chain_oracle(oracle, x, y)
    out = dict(zip(model.metrics_names, model.train_on_batch(x, y)))            # lr 0: the gradients stay inspectable
    bar("chain_fp32.loss_rel", abs(out["loss"] - ref["loss"]) / abs(ref["loss"]), 3.5e-9)       # measured 1.8e-9
    # thresholded metrics: a probability within fp32 rounding of 0.5 may fall on the other side - at most one voxel of the 8192
    # (measured: none), which moves the accuracy by 1 / 8192 and the overlap ratio by less than 1 / (its union of ~2500 voxels)
    bar("chain_fp32.binary_accuracy_abs", abs(out["binary_accuracy"] - ref["acc"]), 1.0 / 8192 + 1e-12)
    bar("chain_fp32.vod_abs", abs(out["vod_coefficient"] - ref["vod"]), 5e-4)
    eng = model._engine
    assert eng.seg.route["first_dgrad"] == "generic"
    G = eng.flat_to_keras(eng.G.cpu().numpy())
    _grad_bars("chain_fp32", G, ref["grads"], 3.8e-6, 6.6e-7)            # measured 1.9e-6, 3.3e-7 (the combined-model test sits at 2.5e-6)
    bar("chain_fp32.predict_max_abs", float(np.abs(model.predict(x) - ref["probs"]).max()), 5e-7)      # measured 2.5e-7
    # a real learning rate: the segmenter stays put bit for bit, the norm net moves and the loss on this batch falls
    keep = [t.clone() for t in (eng.seg.P, eng.seg.M, eng.seg.V)]
    Pn = eng.norm.P.clone()
    model.optimizer.lr = 2e-3
    losses = [model.train_on_batch(x, y)[0] for _ in range(20)]
    torch.cuda.synchronize()
    for a, b in zip(keep, (eng.seg.P, eng.seg.M, eng.seg.V)):
        assert_same(b, a, "the frozen segmenter moved")
    assert eng.seg.t == 0 and eng.norm.t == 21
    assert not torch.equal(Pn, eng.norm.P)
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses[::5]


def test_chain_bf16_takes_the_first_layer_kernel():
    from oracle import unet_oracle as O
    sp, N = (8, 16, 32), 2
    x, y = O.synthetic_batch((N, 1) + sp)
    loss = {}
    for dtype in ("fp32", "bf16"):
        model, seg, _ = _chain(sp, 32, dtype, lr=0.0)
        loss[dtype] = [model.train_on_batch(x, y)[0] for _ in range(2)]
        assert model._engine.seg.route["first_dgrad"] == ("first" if dtype == "bf16" else "generic")
        assert model._engine.norm.dtype == model._engine.seg.dtype == (torch.bfloat16 if dtype == "bf16" else torch.float32)
    assert np.isfinite(loss["bf16"]).all()
    bar("chain_bf16.loss_abs_vs_fp32", max(abs(a - b) for a, b in zip(loss["bf16"], loss["fp32"])), 6e-6)       # measured 3.0e-6


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_chain_through_a_layer_graph_segmenter(dtype):
    """the frozen segmenter on the other engine (LayerGraphEngine built with input_grad=True; bf16: its input is channel-padded)"""
    import fetal_net.model as fmodel
    from oracle import isensee_oracle as IO, unet_oracle as O
    sp, N = (16, 16, 16), 2
    seg = fmodel.isensee2017_model_3d((1,) + sp, compute_dtype=dtype, **KW_NORM)
    spec = IO.IsenseeSpec((1,) + sp, 4, 3, 0, 2)
    Ws, Wn = _perturb(spec.init_weights(4)), _perturb(spec.init_weights(5))
    seg.set_weights_dict(Ws)
    model = fmodel.norm_net_model((1,) + sp, old_model_path=seg, initial_learning_rate=2e-3, compute_dtype=dtype, **KW_NORM)
    model.set_weights_dict(Wn)
    x, y = O.synthetic_batch((N, 1) + sp)
    mid = IO.forward(spec, O.to_torch(Wn, torch.float64), torch.tensor(x, dtype=torch.float64))[0]
    probs = IO.forward(spec, O.to_torch(Ws, torch.float64), mid)[1]
    ref = -float(O.dice_coefficient_t(torch.tensor(y, dtype=torch.float64), probs))
    losses = [model.train_on_batch(x, y)[0] for _ in range(10)]
    eng = model._engine
    assert type(eng.seg).__name__ == "LayerGraphEngine" and eng.seg.input_grad
    bar("chain_graph_seg_%s.first_loss_rel" % dtype, abs(losses[0] - ref) / abs(ref), 2.4e-9 if dtype == "fp32" else 1.1e-3)      # measured 1.2e-9 / 5.9e-4
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses
    assert eng.seg.t == 0 and eng.norm.t == 10
    torch.cuda.synchronize()
    assert_same(eng.seg.P.cpu(), torch.from_numpy(eng.seg.keras_to_flat(Ws)), "the frozen segmenter moved")


# ------------------------------------------------------------------------------------------------------------------ surface
def _gen(shape, seed):
    from oracle.unet_oracle import synthetic_batch
    k = 0
    while True:
        x, y = synthetic_batch(shape, seed_x=seed + k % 2, seed_y=seed + 100 + k % 2)
        yield x.astype(np.float64), y
        k += 1


def test_surface_config_checkpoints_train_model(tmp_path, monkeypatch):
    monkeypatch.setenv("FMRI_DTYPE", "fp32")
    import fetal_net.model as fmodel
    from fetal_net.training import _model_from_config, load_old_model, train_model
    assert callable(fmodel.norm_net_model)
    sp, N = (16, 16, 16), 2
    seg = fmodel.unet_model_3d((1,) + sp, depth=2, n_base_filters=8)
    seg_path = str(tmp_path / "seg.h5")
    seg.save(seg_path)
    # the driver's call: the reference defaults (depth 5, 3 segmentation levels) at the smallest input they accept
    config = dict(model_name="norm_net_model", input_shape=(1,) + sp, initial_learning_rate=1e-3, dropout_rate=0.0,
                  loss="dice_coefficient_loss", old_model=seg_path, weight_mask=None)
    big = _model_from_config(config)
    assert type(big).__name__ == "NormNetModel" and big.norm_net.count_params() > 0 and big.seg_net.count_params() == seg.count_params()
    model = fmodel.norm_net_model((1,) + sp, old_model_path=seg_path, initial_learning_rate=1e-3, **KW_NORM)
    x0 = next(_gen((N, 1) + sp, 1))[0]
    model_file = str(tmp_path / "norm_net")
    hist = train_model(model, model_file, _gen((N, 1) + sp, 1), _gen((N, 1) + sp, 50), steps_per_epoch=2, validation_steps=1,
                       initial_learning_rate=1e-3, n_epochs=2, output_folder=str(tmp_path))
    h = hist.history
    assert len(h["loss"]) == 2 and all(np.isfinite(v).all() for v in h.values())
    assert set(h) >= {"loss", "binary_accuracy", "vod_coefficient", "val_loss"}
    ckpts = sorted(glob.glob(model_file + "*.h5"), key=os.path.getmtime)
    assert ckpts
    path = str(tmp_path / "chain.h5")
    model.save(path)
    p = model.predict(x0)
    twin = load_old_model(path)
    assert type(twin).__name__ == "NormNetModel" and twin._builder_kwargs["old_model_path"] == seg_path
    np.testing.assert_array_equal(twin.predict(x0), p)
    assert twin._engine.norm.t == model._engine.norm.t == 4
    # a chain built on a Model instance cannot name its segmenter in a checkpoint
    inst = fmodel.norm_net_model((1,) + sp, old_model_path=seg, **KW_NORM)
    with pytest.raises(ValueError, match="path"):
        inst.save(str(tmp_path / "no.h5"))


def test_patch_wise_prediction_device_loop_equals_host_loop():
    import fetal_net.model as fmodel
    from fetal_net.prediction import patch_wise_prediction
    patch = (16, 16, 16)
    seg = fmodel.unet_model_3d((1,) + patch, depth=2, n_base_filters=8, compute_dtype="fp32")
    model = fmodel.norm_net_model((1,) + patch, old_model_path=seg, compute_dtype="fp32", **KW_NORM)

    class Proxy:                                   # not a fetal_net Model: patch_wise_prediction tiles on the host and calls .predict
        output_shape = model.output_shape
        input_shape = model.input_shape

        @staticmethod
        def predict(x):
            return model.predict(x)

    vol = np.random.RandomState(3).randn(1, 16, 32, 64)
    dev = patch_wise_prediction(model, vol, patch, overlap_factor=0.5, batch_size=4)
    host = patch_wise_prediction(Proxy(), vol, patch, overlap_factor=0.5, batch_size=4)
    assert dev.shape == host.shape == (16, 32, 64, 1) and np.isfinite(dev).all()
    # the same fp32 probabilities summed in float64 either way: what remains is the rounding of that overlap-add and of the engine's
    # instance-normalisation sums, which depend on how the tiles are grouped into batches (measured 1.2e-7)
    bar("chain.tile_loop_vs_host_max_abs", float(np.abs(dev - host).max()), 2.4e-7)
