"""FMRI_DETERMINISTIC=1 beyond the plain U-Net step: the ordered normalisation statistics and the transposed-conv weight gradient at op
level, then whole training steps of the normalised / transposed-conv U-Nets (UNetEngine), of the layer-graph engine (Isensee 3-D and 2-D,
U-Net with per-axis pool sizes) and of the norm_net_model chain.

"Same bits" is `gpu_util.assert_same` on the raw tensors.  An engine test builds its engine twice from the same Keras weights (close() in
between: one deterministic-gradient registration per process), runs three full steps on one batch and compares logits, metric sums, the
gradient buffer after each backward, and P, M, V and the moving statistics after each optimizer step.  The accuracy checks reuse the bars
of the existing default-mode tests of the same op / configuration (tests/test_gpu_ops.py, tests/test_gpu_engine.py) unchanged.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gpu_util import assert_close, assert_same, f64, rnd, to_ncdhw, to_ndhwc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the GPU box"
    from fmri_hip import ops as o
    return o


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def _perturb(W, seed=5):
    """biases, gamma and beta off their initial 0 / 1 (the perturbation of tests/test_gpu_engine.py)"""
    rs = np.random.RandomState(seed)
    for k in W:
        if k.endswith(("/bias", "/beta")):
            W[k] = (rs.randn(*W[k].shape) * 0.05).astype(np.float32)
        if k.endswith("/gamma"):
            W[k] = (1.0 + rs.randn(*W[k].shape) * 0.1).astype(np.float32)
    return W


# ================================================================================================ 1. ordered statistics at op level
def _ramp(N, sp, C, dtype, A=1e3):
    """a linear ramp from -A to +A over the voxel index plus small noise: the workgroups' partial sums are large and all different, their
    total nearly cancels - the arrival order of fp64 atomics shows in the last bits of such a sum"""
    V = int(np.prod(sp))
    g = torch.Generator().manual_seed(7)
    ramp = torch.linspace(-A, A, V, dtype=torch.float64).reshape(1, V, 1)
    x = ramp * (1.0 + 0.05 * torch.arange(C, dtype=torch.float64).reshape(1, 1, C)) + 0.5 * torch.randn(N, V, C, generator=g, dtype=torch.float64)
    return x.reshape((N,) + tuple(sp) + (C,)).to(dtype).cuda()


@pytest.mark.parametrize("mode", ["batch", "instance"])
@pytest.mark.parametrize("dtype,C", [(torch.bfloat16, 8), (torch.float32, 8), (torch.float32, 12)], ids=["bf16_c8_vector", "fp32_c8", "fp32_c12"])
def test_ordered_norm_statistics_repeat_bit_for_bit_and_match_fp64(ops, dtype, C, mode):
    """fmri_norm_act_fwd, fmri_norm_act_bwd_x and fmri_norm_act_bwd under ops.set_deterministic: ten repeats give the same bits in stats, y,
    dx, dgamma and dbeta, and the results stand under the bars tests/test_gpu_ops.py::test_norm_act_fwd_bwd sets for the default kernels
    (against torch-CPU fp64).  bf16 with C = 8 takes the 16-byte-load reduction kernels, fp32 the scalar ones."""
    from oracle import unet_oracle as O
    N, sp, act, alpha = 2, (16, 16, 16), 2, 0.3
    per = mode == "instance"
    G, V = (N if per else 1), int(np.prod(sp))
    rows = ops.norm_det_workspace_bytes(N, V, C, per) // (16 * C)            # slab rows = workgroups of one reduction launch
    assert rows // G > 1, "one workgroup per (group, channel) sum: the test would show nothing"
    x = _ramp(N, sp, C, dtype)
    dy = rnd((N,) + sp + (C,), 83, dtype)
    gamma = rnd((C,), 81, torch.float32) * 0.5 + 1.0
    beta = rnd((C,), 82, torch.float32) * 0.2
    grad, shadow = torch.zeros(64, device="cuda"), torch.zeros(64, dtype=torch.int64, device="cuda")     # (registration only: dgamma / dbeta are plain stores)
    scratch = torch.empty(ops.norm_det_workspace_bytes(N, V, C, per) // 8, dtype=torch.float64, device="cuda")
    ws = torch.zeros((G, C, 2), dtype=torch.float64, device="cuda")
    runs = []
    ops.set_deterministic(grad, shadow, scratch)
    try:
        for _ in range(10):
            stats, y = torch.zeros((G, C, 3), device="cuda"), torch.empty_like(x)
            ops.norm_act_fwd(x, gamma, beta, y, stats, ws, per, eps=1e-3, eps_on_std=per, act=act, alpha=alpha)
            out = [stats, y]
            for yy, bb in ((None, beta), (y, None)):                       # the form that recomputes the sign from x, and the one that reads y
                dx, dg, db = torch.empty_like(x), torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
                ops.norm_act_bwd(x, yy, dy, gamma, stats, dx, dg, db, ws, per, act=act, alpha=alpha, beta=bb)
                out += [dx, dg, db]
            torch.cuda.synchronize()
            runs.append(out)
            assert float(ws.abs().max()) == 0.0                             # the last reader leaves the accumulators zero, as in default mode
    finally:
        ops.set_deterministic(None, None)
    names = ("stats", "y", "dx (from x)", "dgamma (from x)", "dbeta (from x)", "dx (from y)", "dgamma (from y)", "dbeta (from y)")
    for k, r in enumerate(runs[1:]):
        for name, a, b in zip(names, r, runs[0]):
            assert_same(a, b, "%s, repeat %d" % (name, k + 1))
    # accuracy: the bars of test_norm_act_fwd_bwd
    stats, y, dx, dg, db = runs[0][:5]
    xr = to_ncdhw(f64(x)).requires_grad_(True)
    gr, br = f64(gamma).requires_grad_(True), f64(beta).requires_grad_(True)
    z = O._instancenorm(xr, gr, br) if per else O._batchnorm_train(xr, gr, br)
    yr = F.leaky_relu(z, alpha)
    tol = (1e-4, 1e-5) if dtype == torch.float32 else (5e-3, 2e-4)
    tolb = (2e-4, 2e-5) if dtype == torch.float32 else (6e-3, 2e-3)
    assert_close(y, to_ndhwc(yr.detach()), *tol, what="ordered norm fwd")
    yr.backward(to_ncdhw(f64(dy)))
    assert_close(runs[0][5], to_ndhwc(xr.grad), *tolb, what="ordered norm dx")
    assert_close(runs[0][6], gr.grad, *tolb, what="ordered norm dgamma")
    assert_close(runs[0][7], br.grad, *tolb, what="ordered norm dbeta")
    assert torch.equal(dx, runs[0][5])                                       # (as in default mode: both forms of the backward, the same bits)


def test_norm_ops_refuse_a_registration_without_scratch(ops):
    """deterministic mode never returns to the atomics silently: no slab, or one too small, is an error of the entry point"""
    from fmri_hip._lib import FmriError
    x = rnd((2, 4, 4, 4, 8), 1, torch.float32)
    gamma, beta = torch.ones(8, device="cuda"), torch.zeros(8, device="cuda")
    stats, ws = torch.zeros((1, 8, 3), device="cuda"), torch.zeros((1, 8, 2), dtype=torch.float64, device="cuda")
    grad, shadow = torch.zeros(64, device="cuda"), torch.zeros(64, dtype=torch.int64, device="cuda")
    for scratch in (None, torch.empty(2, dtype=torch.float64, device="cuda")):
        ops.set_deterministic(grad, shadow, scratch)
        try:
            with pytest.raises(FmriError):
                ops.norm_act_fwd(x, gamma, beta, torch.empty_like(x), stats, ws, 0)
        finally:
            ops.set_deterministic(None, None)
    ops.norm_act_fwd(x, gamma, beta, torch.empty_like(x), stats, ws, 0)      # default mode again
    torch.cuda.synchronize()


# ================================================================================================ 2. transposed-conv weight gradient
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_deconv_weight_gradient_repeats_bit_for_bit(ops, dtype):
    """fmri_deconv3d_k2s2_bwd with dw / db inside a registered gradient buffer (16 voxel ranges meet in every element): ten repeats, the
    same bits; and the default mode's result within the bars of tests/test_gpu_ops.py::test_deconv_k2s2_fwd_bwd"""
    N, D, H, W, Cin, Cout = 2, 3, 4, 5, 12, 8
    x = torch.relu(rnd((N, D, H, W, Cin), 90, dtype))
    w = rnd((8, Cout, Cin), 91, dtype, scale=0.3)
    dy = rnd((N, 2 * D, 2 * H, 2 * W, Cout + 4), 93, dtype)
    nw = 8 * Cout * Cin
    grad = torch.zeros(nw + Cout, device="cuda")
    shadow = torch.zeros(nw + Cout, dtype=torch.int64, device="cuda")
    dx = torch.empty_like(x)

    def run():
        grad.zero_()
        ops.deconv_bwd(x, w, dy, dx, grad[:nw].view(8, Cout, Cin), grad[nw:], dy_off=4, xmask=x)

    runs = []
    ops.set_deterministic(grad, shadow)
    try:
        for _ in range(10):
            run()
            ops.deterministic_finish(grad, shadow)
            torch.cuda.synchronize()
            runs.append(grad.clone())
            assert int(shadow.abs().max()) == 0
    finally:
        ops.set_deterministic(None, None)
    assert float(runs[0].abs().max()) > 0
    for k, r in enumerate(runs[1:]):
        assert_same(r, runs[0], "deterministic deconv dw / db, repeat %d" % (k + 1))
    run()
    torch.cuda.synchronize()
    tolw = (1e-4, 1e-5) if dtype == torch.float32 else (2e-5, 2e-5)
    assert_close(runs[0][:nw], grad[:nw], *tolw, what="deterministic deconv dw against default mode")
    assert_close(runs[0][nw:], grad[nw:], *tolw, what="deterministic deconv db against default mode")


def test_weighted_dice_group_sums_repeat_bit_for_bit(ops):
    """fmri_weighted_dice_fwd while a registration is on: one workgroup per sample, so no two workgroups meet in a group's fp64 sums (default
    mode: 16 at this size).  Ten repeats, the same bits; against the default mode the sums differ by the order of 65,536 fp64 additions of
    the same terms at most: n x 2^-53 = 7.3e-12 relative, bar 1e-11."""
    N, vox, L = 2, 64 * 64 * 16, 2
    g = torch.Generator().manual_seed(3)
    probs = torch.rand(N * vox * L, generator=g).cuda()
    y = (torch.rand(N * vox * L, generator=g) > 0.7).to(torch.uint8).cuda()
    grad, shadow = torch.zeros(64, device="cuda"), torch.zeros(64, dtype=torch.int64, device="cuda")

    def run():
        gs, sums = torch.empty(3 * N * L, dtype=torch.float64, device="cuda"), torch.zeros(16, dtype=torch.float64, device="cuda")
        ops.weighted_dice_fwd(probs, y, gs, sums, N, L)
        torch.cuda.synchronize()
        return gs, sums

    ops.set_deterministic(grad, shadow)
    try:
        runs = [run() for _ in range(10)]
    finally:
        ops.set_deterministic(None, None)
    for k, (gs, sums) in enumerate(runs[1:]):
        assert_same(gs, runs[0][0], "group sums, repeat %d" % (k + 1))
        assert_same(sums, runs[0][1], "loss sums, repeat %d" % (k + 1))
    gs, sums = run()
    assert float(sums[11]) == N * L
    assert float(((runs[0][0] - gs).abs() / gs.abs()).max()) <= 1e-11 and abs(float(runs[0][1][10] - sums[10])) <= 1e-11 * float(sums[10])


# ================================================================================================ engines: three reproducible steps
def _three_steps(eng, xd, yd, lr=1e-3, pad_check=False):
    """[(step, tensor name, copy)] of three full steps on one batch"""
    snaps = []
    for step in (1, 2, 3):
        eng.forward(xd)
        sums = eng.loss_forward(yd)
        eng.backward(yd)
        if pad_check:
            _padding_gradients_are_zero(eng)
        snaps += [(step, "logits", eng.logits.clone()), (step, "sums", sums.clone()), (step, "G", eng.G.clone())]
        eng.adam_step(lr)
        snaps += [(step, n, getattr(eng, n).clone()) for n in ("P", "M", "V")]
        snaps += [(step, "moving " + k, v.clone()) for k, v in sorted(getattr(eng, "moving", {}).items())]
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t.double()).all()) for _, _, t in snaps)
    get = lambda step, name: [t for s_, n, t in snaps if s_ == step and n == name][0]
    assert float(get(1, "G").abs().max()) > 0 and not torch.equal(get(1, "P"), get(2, "P"))          # gradients flow, the weights move
    return snaps


def _same_snaps(a, b, what):
    assert [(s_, n) for s_, n, _ in a] == [(s_, n) for s_, n, _ in b]
    for (step, name, ta), (_, _, tb) in zip(a, b):
        assert_same(ta, tb, "%s: %s of step %d" % (what, name, step))


def _padding_gradients_are_zero(eng):
    """channel-padded engine: the padding channels of every gradient image stay exactly zero"""
    for name, L in eng.layout.items():
        if L["kind"] == "conv":
            dw, db = eng.dWp[name], eng.dbp[name]
            mask = torch.ones(dw.shape[2], dtype=torch.bool, device=dw.device)
            mask[eng.cin_map[name]] = False
            assert float(dw[:, L["cout"]:, :].abs().max() if dw.shape[1] > L["cout"] else 0.0) == 0.0, name
            assert float(dw[:, :, mask].abs().max() if bool(mask.any()) else 0.0) == 0.0, name
            assert float(db[L["cout"]:].abs().max() if db.numel() > L["cout"] else 0.0) == 0.0, name
        elif L["kind"] == "norm":
            for t in (eng.dgp[name], eng.dbetap[name]):
                assert float(t[L["c"]:].abs().max() if t.numel() > L["c"] else 0.0) == 0.0, name


UNET_VARIANTS = [("batch", False), ("batch", True), ("instance", False), ("instance", True), (None, True)]


def _unet_twice(plan_kw, N, dtype, x, y, monkeypatch, seed=4):
    from fmri_hip.engine import UNetEngine, UNetPlan
    monkeypatch.setenv("FMRI_DETERMINISTIC", "1")
    W, out = None, []
    for _ in range(2):
        eng = UNetEngine(UNetPlan(**plan_kw), N, dtype=dtype, seed=seed)
        try:
            assert eng.deterministic and not eng.upcat_wgrad and not any(eng.route["upcat_wgrad"].values())
            assert not any(eng.route["stats"].values()) and not any(eng.route["dz"].values())          # the separate, ordered reductions
            assert all(v in ("deconv", "upcat", "upsample") for v in eng.route["up"].values()), eng.route["up"]
            if W is None:
                W = _perturb(eng.export_keras_weights())
            eng.load_keras_weights(W)
            out.append(_three_steps(eng, x, y))
        finally:
            eng.close()
    return out


@pytest.mark.parametrize("norm,deconv", UNET_VARIANTS)
@pytest.mark.parametrize("dtype,base,sp", [(torch.float32, 8, (16, 16, 8)), (torch.bfloat16, 32, (8, 16, 32))], ids=["fp32", "bf16"])
def test_unet_engine_steps_are_reproducible(monkeypatch, dtype, base, sp, norm, deconv):
    """unet_model_3d with batch / instance normalisation and / or Deconvolution3D under FMRI_DETERMINISTIC=1 (the parent commit refused these
    at construction).  bf16 at 32 base filters reaches the MFMA routes."""
    from oracle import unet_oracle as O
    N = 2
    x, y = O.synthetic_batch((N, 1) + sp)
    xd = torch.from_numpy(x).cuda().to(dtype).reshape(N, *sp, 1).contiguous()
    yd = torch.from_numpy(y).cuda().reshape(-1).contiguous()
    a, b = _unet_twice(dict(in_channels=1, spatial=sp, depth=2, n_base_filters=base, norm=norm, deconvolution=deconv), N, dtype, xd, yd, monkeypatch)
    _same_snaps(b, a, "unet %s %s" % (norm, "deconv" if deconv else "upsampling"))


def test_unet2d_engine_with_batch_norm_is_reproducible(monkeypatch):
    rs = np.random.RandomState(3)
    N, X, Y, C = 4, 32, 32, 3
    xd = torch.from_numpy(rs.randn(1, N, X, Y, C).astype(np.float32)).cuda()
    yd = torch.from_numpy((rs.rand(N * X * Y) > 0.7).astype(np.uint8)).cuda()
    a, b = _unet_twice(dict(in_channels=C, spatial=(X, Y), depth=2, n_base_filters=8, ndim=2, norm="batch"), N, torch.float32, xd, yd, monkeypatch)
    _same_snaps(b, a, "unet 2-D batch norm")


def test_unet_engine_refuses_a_final_conv_on_the_generic_kernel(monkeypatch):
    from fmri_hip.engine import UNetEngine, UNetPlan
    monkeypatch.setenv("FMRI_DETERMINISTIC", "1")
    with pytest.raises(NotImplementedError, match="1x1x1"):
        UNetEngine(UNetPlan(1, (8, 8, 8), depth=2, n_base_filters=12), 1, dtype=torch.float32)


# ------------------------------------------------------------------------------------------------ layer-graph engine
def _isensee3d(base, sp, N):
    import fetal_net.model as fmodel
    from oracle import isensee_oracle as I, unet_oracle as O
    kw = dict(input_shape=(1,) + sp, depth=3, n_base_filters=base, n_segmentation_levels=2, dropout_rate=0.3)
    model, spec = fmodel.isensee2017_model_3d(**kw), I.IsenseeSpec(**kw)
    x, y = O.synthetic_batch((N, 1) + sp)
    rs = np.random.RandomState(8)
    masks = {lv: ((rs.rand(N, spec.levels[lv]["filters"]) < 0.7).astype(np.float64) / 0.7) for lv in range(3)}
    return model, spec, x, y, masks


def _graph_twice(layers, N, dtype, W, masks, xd, yd, monkeypatch, pad_check=False):
    from fmri_hip.graph_engine import LayerGraphEngine
    monkeypatch.setenv("FMRI_DETERMINISTIC", "1")
    out = []
    for _ in range(2):
        eng = LayerGraphEngine(layers, N, dtype=dtype)
        try:
            assert eng.deterministic
            assert not eng.Ws2 and not any(Wu["wgrad"] for Wu in eng.Wup.values())                     # no parity-form weight gradient
            eng.load_keras_weights(W)
            if masks is not None:
                eng.set_dropout_masks(masks)
            out.append(_three_steps(eng, xd, yd, pad_check=pad_check and eng.pad))
        finally:
            eng.close()
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16_padded"])
def test_isensee_graph_engine_steps_are_reproducible(monkeypatch, dtype):
    """isensee2017_model_3d (instance normalisation, stride-2 convolutions, up-sampling convolutions, residual adds, fixed dropout masks) on
    the layer-graph engine; bf16: the channel-padded engine, whose weight-gradient kernels write the padded images the shadow covers"""
    N, sp = 2, (16, 32, 32)
    model, spec, x, y, masks = _isensee3d(8, sp, N)
    W = _perturb(spec.init_weights(31))
    dm = {"spatial_dropout3d_%d" % (lv + 1): torch.tensor(masks[lv], dtype=torch.float32).cuda() for lv in range(3)}
    xd = torch.from_numpy(x).cuda().reshape(N, *sp, 1).to(dtype).contiguous()
    yd = torch.from_numpy(y).cuda().reshape(-1).contiguous()
    a, b = _graph_twice(model.layers, N, dtype, W, dm, xd, yd, monkeypatch, pad_check=True)
    _same_snaps(b, a, "isensee 3-D")


def test_isensee2d_graph_engine_steps_are_reproducible(monkeypatch):
    import fetal_net.model as fmodel
    from oracle import isensee_oracle as I
    N, X, Y, C = 4, 32, 32, 3
    kw = dict(input_shape=(X, Y, C), depth=3, n_base_filters=4, n_segmentation_levels=2, dropout_rate=0.3, summation=True)
    model, spec = fmodel.isensee2017_model(**kw), I.IsenseeSpec(ndim=2, **kw)
    rs = np.random.RandomState(12)
    xd = torch.from_numpy(rs.randn(N, X, Y, C).astype(np.float32)).cuda().unsqueeze(0).contiguous()
    yd = torch.from_numpy((rs.rand(N, X, Y, 1) > 0.7).astype(np.uint8)).cuda().reshape(-1).contiguous()
    dm = {"spatial_dropout2d_%d" % (lv + 1): torch.tensor((rs.rand(N, spec.levels[lv]["filters"]) < 0.7) / 0.7, dtype=torch.float32).cuda()
          for lv in range(3)}
    a, b = _graph_twice(model.layers, N, torch.float32, _perturb(spec.init_weights(23)), dm, xd, yd, monkeypatch)
    _same_snaps(b, a, "isensee 2-D")


def test_unet_with_per_axis_pool_sizes_is_reproducible(monkeypatch):
    import fetal_net.model as fmodel
    from fmri_hip.graph_engine import LayerGraphEngine
    sp, N = (16, 16, 4), 2
    model = fmodel.unet_model_3d(input_shape=(1,) + sp, pool_size=(2, 2, 1), depth=3, n_base_filters=4, batch_normalization=True)
    assert getattr(model, "_graph_engine", False)
    probe = LayerGraphEngine(model.layers, N, dtype=torch.float32)           # default mode: only to draw a set of Keras weights
    W = _perturb(probe.export_keras_weights())
    rs = np.random.RandomState(2)
    xd = torch.from_numpy(rs.randn(N, *sp, 1).astype(np.float32)).cuda()
    yd = torch.from_numpy((rs.rand(N * int(np.prod(sp))) > 0.7).astype(np.uint8)).cuda()
    a, b = _graph_twice(model.layers, N, torch.float32, W, None, xd, yd, monkeypatch)
    _same_snaps(b, a, "unet pool (2, 2, 1)")


def test_graph_engine_refuses_what_it_cannot_reproduce(monkeypatch):
    """a deterministic layer-graph engine is reproducible or refuses at construction, naming what is in the way"""
    import fetal_net.model as fmodel
    from fmri_hip.graph_engine import LayerGraphEngine
    monkeypatch.setenv("FMRI_DETERMINISTIC", "1")
    disc = fmodel.discriminator_image_3d(input_shape=(2, 16, 16, 16), n_base_filters=4, depth=2, dropout_rate=0.0)
    with pytest.raises(NotImplementedError, match="Dense"):
        LayerGraphEngine(disc.layers, 2, dtype=torch.float32, input_grad=True)
    seg = fmodel.isensee2017_model_3d(input_shape=(1, 16, 16, 16), depth=3, n_base_filters=4, n_segmentation_levels=2)
    with pytest.raises(NotImplementedError, match="dist_ctx"):
        LayerGraphEngine(seg.layers, 2, dtype=torch.float32, dist_ctx=object())
    eng = LayerGraphEngine(seg.layers, 2, dtype=torch.float32)               # neither refusal left a registration behind
    assert eng.deterministic
    eng.close()


# ------------------------------------------------------------------------------------------------ the chain
KW_NORM = dict(n_base_filters=4, depth=3, dropout_rate=0, n_segmentation_levels=2)


def _chain_run(dtype, sp, seg_base, x, y, bn):
    import fetal_net.model as fmodel
    seg = fmodel.unet_model_3d((1,) + sp, depth=2, n_base_filters=seg_base, compute_dtype=dtype, batch_normalization=bn)
    model = fmodel.norm_net_model((1,) + sp, old_model_path=seg, initial_learning_rate=2e-3, compute_dtype=dtype, **KW_NORM)
    eng = model.engine(x.shape[0])
    try:
        assert eng.deterministic and eng.norm.deterministic and eng.seg.deterministic
        assert eng.seg.frozen and not hasattr(eng.seg, "G64") and eng.norm.G64.numel() == (eng.norm.Gp if eng.norm.pad else eng.norm.G).numel()
        torch.manual_seed(0)
        keep = [t.clone() for t in (eng.seg.P, eng.seg.M, eng.seg.V)] + [v.clone() for _, v in sorted(eng.seg.moving.items())]
        losses, snaps = [], []
        for _ in range(3):
            losses.append(model.train_on_batch(x, y)[0])
            snaps += [t.clone() for t in (eng.seg.logits, eng.seg.sums, eng.seg.input_gradient(), eng.norm.G, eng.norm.P, eng.norm.M, eng.norm.V)]
        torch.cuda.synchronize()
        now = [eng.seg.P, eng.seg.M, eng.seg.V] + [v for _, v in sorted(eng.seg.moving.items())]
        assert len(now) == (9 if bn else 3)
        for a, b in zip(keep, now):
            assert_same(b, a, "the frozen segmenter moved")
        assert eng.seg.t == 0 and eng.norm.t == 3 and np.isfinite(losses).all() and float(eng.norm.G.abs().max()) > 0
        return losses, snaps
    finally:
        eng.close()


@pytest.mark.parametrize("dtype,sp,seg_base", [("fp32", (16, 16, 16), 8), ("bf16", (8, 16, 32), 32)], ids=["fp32", "bf16"])
def test_chain_steps_are_reproducible_and_the_segmenter_stays_put(monkeypatch, dtype, sp, seg_base):
    """norm_net_model under FMRI_DETERMINISTIC=1: the trainable network in front holds the one registration, the frozen (batch-normalised)
    segmenter takes none and still sums its statistics in block order; three steps of two builds give the same bits"""
    from oracle import unet_oracle as O
    monkeypatch.setenv("FMRI_DETERMINISTIC", "1")
    x, y = O.synthetic_batch((2, 1) + sp)
    a = _chain_run(dtype, sp, seg_base, x, y, bn=True)
    b = _chain_run(dtype, sp, seg_base, x, y, bn=True)
    assert a[0] == b[0], (a[0], b[0])
    for k, (ta, tb) in enumerate(zip(a[1], b[1])):
        assert_same(tb, ta, "chain %s: tensor %d of step %d" % (dtype, k % 7, k // 7 + 1))


# ================================================================================================ 6. agreement with the default mode's bars
def test_deterministic_unet_engine_meets_the_default_modes_oracle_bars(monkeypatch):
    """the comparison of tests/test_gpu_engine.py::test_unet3d_norm_and_deconv_variants_fp32[batch-True] (logits, Dice, every gradient
    against the fp64 oracle, that test's bars) on the deterministic engine"""
    from fmri_hip.engine import UNetEngine, UNetPlan
    from oracle import unet_oracle as O
    monkeypatch.setenv("FMRI_DETERMINISTIC", "1")
    norm, deconv = "batch", True
    spatial, N = (8, 16, 16), 2
    spec = O.Spec((1,) + spatial, depth=2, n_base_filters=8, deconvolution=deconv, batch_normalization=True)
    x, y = O.synthetic_batch((N, 1) + spatial)
    for seed in range(21, 40):                             # (a weight seed without ReLU ties, as in that test)
        W = spec.init_weights(seed)
        rs = np.random.RandomState(5)
        for k in W:
            if k.endswith(("/bias", "/beta")):
                W[k] = (rs.randn(*W[k].shape) * 0.05).astype(np.float32)
            if k.endswith("/gamma"):
                W[k] = (1.0 + rs.randn(*W[k].shape) * 0.1).astype(np.float32)
        _, _, inter = O.forward(spec, O.to_torch(W, torch.float64), torch.tensor(x, dtype=torch.float64), return_intermediates=True)
        if min(float(v.abs().min()) for k, v in inter.items() if k.endswith("/z")) > 2e-5:
            break
    ref = O.loss_and_grads(spec, W, x, y, dtype=torch.float64)
    eng = UNetEngine(UNetPlan(1, spatial, depth=2, n_base_filters=8, norm=norm, deconvolution=deconv), N, dtype=torch.float32)
    try:
        assert eng.deterministic
        eng.load_keras_weights(W)
        xd = torch.from_numpy(x).cuda().reshape(N, *spatial, 1).contiguous()
        yd = torch.from_numpy(y).cuda().reshape(-1).contiguous()
        eng.forward(xd)
        sums = eng.loss_forward(yd)
        eng.backward(yd)
        torch.cuda.synchronize()
        assert _rel(eng.logits.cpu().numpy().reshape(ref["logits"].shape), ref["logits"]) <= 1e-3
        assert abs(eng.metrics_from_sums(sums.cpu().numpy())["dice_coefficient"] - ref["dice"]) <= 1e-4
        for name, L in eng.layout.items():
            gk = ref["grads"][name + "/kernel"]
            if L["kind"] == "conv":
                mine = eng.w_view(name, eng.G).cpu().numpy().reshape(3, 3, 3, L["cout"], L["cin"]).transpose(0, 1, 2, 4, 3)
            elif L["kind"] == "deconv":
                mine = eng.w_view(name, eng.G).cpu().numpy().reshape(2, 2, 2, L["cout"], L["cin"])
            else:
                mine = eng.w_view(name, eng.G).cpu().numpy().T.reshape(gk.shape)
            assert _rel(mine, gk) <= 3e-3, name
            if not L.get("norm"):
                assert _rel(eng.b_view(name, eng.G).cpu().numpy(), ref["grads"][name + "/bias"]) <= 3e-3, name + " bias"
            else:
                assert float(np.abs(eng.b_view(name, eng.G).cpu().numpy()).max()) <= 1e-6 * float(np.abs(gk).max() + 1)
                assert _rel(eng.gb_view(name, "gamma", eng.G).cpu().numpy(), ref["grads"][L["norm"] + "/gamma"]) <= 3e-3, name + " gamma"
                assert _rel(eng.gb_view(name, "beta", eng.G).cpu().numpy(), ref["grads"][L["norm"] + "/beta"]) <= 3e-3, name + " beta"
    finally:
        eng.close()


def test_deterministic_graph_engine_meets_the_default_modes_oracle_bars(monkeypatch):
    """the comparison of tests/test_gpu_engine.py::test_isensee_graph_engine_fp32_vs_oracle (its model, weights, masks and bars) on the
    deterministic engine"""
    from fmri_hip.graph_engine import LayerGraphEngine
    from oracle import isensee_oracle as I
    monkeypatch.setenv("FMRI_DETERMINISTIC", "1")
    N, sp = 2, (16, 16, 16)
    model, spec, x, y, masks = _isensee3d(4, sp, N)
    W = _perturb(spec.init_weights(21))
    ref = I.loss_and_grads(spec, W, x, y, dropout_masks=masks)
    eng = LayerGraphEngine(model.layers, N, dtype=torch.float32)
    try:
        assert eng.deterministic
        eng.load_keras_weights(W)
        eng.set_dropout_masks({"spatial_dropout3d_%d" % (lv + 1): torch.tensor(masks[lv], dtype=torch.float32).cuda() for lv in range(3)})
        xd = torch.from_numpy(x).cuda().reshape(N, *sp, 1).contiguous()
        yd = torch.from_numpy(y).cuda().reshape(-1).contiguous()
        eng.forward(xd)
        sums = eng.loss_forward(yd)
        eng.backward(yd)
        torch.cuda.synchronize()
        logits = eng.logits.cpu().numpy().reshape(ref["logits"].shape)
        assert _rel(logits, ref["logits"]) <= 1e-3
        assert abs(eng.metrics_from_sums(sums.cpu().numpy())["dice_coefficient"] - ref["dice"]) <= 1e-4
        for name, L in eng.layout.items():
            if L["kind"] == "conv":
                mine = eng.w_view(name, eng.G).cpu().numpy().reshape((L["k"],) * 3 + (L["cout"], L["cin"])).transpose(0, 1, 2, 4, 3)
                gk = ref["grads"][name + "/kernel"]
                e = np.linalg.norm(mine - gk) / (np.linalg.norm(gk) + 1e-30)
                assert e <= 5e-3, (name, e)
            else:
                for key in ("gamma", "beta"):
                    gk = ref["grads"][name + "/" + key]
                    e = np.linalg.norm(eng._v(name, key, eng.G).cpu().numpy() - gk) / (np.linalg.norm(gk) + 1e-30)
                    assert e <= 5e-3, (name, key, e)
    finally:
        eng.close()
