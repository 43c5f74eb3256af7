"""Keras SGD / RMSprop / AMSGrad step kernels, gradient clipping and the ordered sum of squares on the GPU, against the float64
restatement of tests/optimizer_restatement.py (Keras 2.2.4 as published; parity-unpinned, see there), then through both engines, the
norm-net chain and the two checkpoint containers.

Bounds (rounding counts, u = 2^-24; every fp32 operation is correctly rounded, an FMA only removes a rounding):

  slot   s' = a*s + b*h:   |dev - ref| <= 16 u (|a*s| + |b*h|).  The longest chain is RMSprop's / Adam's v under a norm clip:
         grad_scale * G (1), * clipnorm (2), / norm (3), squared (4), 1 - rho in fp32 (5), (1 - rho) * g^2 (6 - g^2 carries the
         gradient's three roundings twice: 9 in all), rho * a (1), the sum (1): every term's relative error stays below 9 u to first
         order, rounded up to 16.
  param  p' = p + D with the reference increment D formed in float64 from the DEVICE's new slots (which are checked on their own, so
         that a cancellation inside a slot cannot leak into this bound): |dev - ref| <= u |p'| + 8 u |D|.  D = -lr * g / (sqrt(a) + eps)
         takes the gradient's three roundings, lr * g (4), the square root (5), + eps (6), the division (7) - at most 8; Adam's
         -lr_t * m / (sqrt(v) + eps) takes 4; SGD's D = v takes none; the final p + D is the u |p'|.  Nesterov's D = momentum * v - lr * g
         is a difference whose terms cancel where momentum and gradient oppose: no fp32 evaluation is accurate relative to |D| there,
         so the kernel forms this one increment in float64 from the stored v and rounds once - u |p'| covers it.
  sumsq  |dev - ref| <= 32 * 2^-53 * sum g^2 against math.fsum of the exact float64 squares: the form of the fmri_moments_f64 bound
         (Neumaier pairs from the lane's loop to the last combine: the error is a few 2^-53 of the sum whatever n is).
"""
import functools
import math

import numpy as np
import pytest
import torch

import optimizer_restatement as R

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 4, 5, 1023, 1025, 2097159]      # the last: one float4 past 2048 * 256 * 4 - a second grid-stride round and the scalar tail
STEPS = 3

# (kind, hyper-parameters): lr and the rest are no float32 numbers, so the rounding of the hyper-parameters is exercised
CONFIGS = {
    "sgd": ("sgd", dict(lr=0.013, momentum=0.0, nesterov=False)),
    "sgd_momentum": ("sgd", dict(lr=0.013, momentum=0.9, nesterov=False)),
    "sgd_nesterov": ("sgd", dict(lr=0.013, momentum=0.9, nesterov=True)),
    "rmsprop": ("rmsprop", dict(lr=0.0011, rho=0.9, eps=1e-7)),
    "amsgrad": ("adam", dict(lr=0.0013, beta_1=0.9, beta_2=0.999, eps=1e-7)),
}


@functools.lru_cache(maxsize=None)
def _inputs(n):
    """p and the three gradients of a size, drawn once and never written (float32, host).  Step 3's gradient is step 1's with its first
    half shrunk a thousandfold: there Adam's v falls and AMSGrad's max keeps the old vhat."""
    rs = np.random.RandomState(1000 + n % 977)
    p = rs.randn(n).astype(np.float32)
    g = [rs.randn(n).astype(np.float32) for _ in range(2)]
    g3 = g[0].copy()
    g3[:(n + 1) // 2] *= np.float32(1e-3)
    for a in [p] + g + [g3]:
        a.setflags(write=False)
    return p, g + [g3]


def _cuda(a):
    return torch.from_numpy(np.array(a)).cuda()             # (a copy: the shared inputs are read-only)


def _host(t):
    return t.detach().cpu().numpy().copy()


def _assert_within(name, dev, ref, bound):
    dev, ref = np.asarray(dev, np.float64), np.asarray(ref, np.float64)
    err = np.abs(dev - ref)
    worst = int(np.argmax(err - bound))
    print("%s: max err / bound = %.3f" % (name, float(np.max(err / np.maximum(bound, 1e-300)))))
    assert np.all(np.isfinite(dev)), name
    assert np.all(err <= bound), "%s: |dev - ref| = %.3e > %.3e at %d (dev %r, ref %r)" % (name, err[worst], bound[worst], worst,
                                                                                         dev[worst], ref[worst])


def _check_step(kind, hp, k, before, after, G, grad_scale, norm, clipnorm, clipvalue):
    """one step of `kind` against the restatement: `before` / `after` = host copies of (p, slots...) around the launch"""
    g = R.gradient(G, grad_scale, norm, clipnorm, clipvalue)
    if kind == "sgd":
        (p0, m0), (p1, m1) = before, after
        v, a_s, b_h = R.sgd_slot(g, m0, hp["lr"], hp["momentum"])
        _assert_within("sgd moment", m1, v, R.slot_bound(a_s, b_h))
        delta = R.sgd_increment(g, m1, hp["lr"], hp["momentum"], hp["nesterov"])
    elif kind == "rmsprop":
        (p0, a0), (p1, a1) = before, after
        a, a_s, b_h = R.rmsprop_slot(g, a0, hp["rho"])
        _assert_within("rmsprop accumulator", a1, a, R.slot_bound(a_s, b_h))
        delta = R.rmsprop_increment(g, a1, hp["lr"], hp["eps"])
    else:
        (p0, m0, v0, h0), (p1, m1, v1, h1) = before, after
        (m, ma, mb), (v, va, vb) = R.adam_slots(g, m0, v0, hp["beta_1"], hp["beta_2"])
        _assert_within("adam m", m1, m, R.slot_bound(ma, mb))
        _assert_within("adam v", v1, v, R.slot_bound(va, vb))
        assert np.array_equal(h1, np.maximum(h0, v1)), "vhat is not max(vhat, v) of the device's v"
        delta = R.adam_increment(m1, h1, R.adam_lr_t(hp["lr"], hp["beta_1"], hp["beta_2"], k), hp["eps"])
    p_ref = np.asarray(p0, np.float64) + delta
    _assert_within("%s parameter" % kind, p1, p_ref, R.param_bound(p_ref, delta))


def _launch(kind, hp, k, bufs, g, grad_scale, gnorm, clipnorm, clipvalue):
    from fmri_hip import ops
    clip = dict(grad_scale=grad_scale, gnorm=gnorm, clipnorm=clipnorm, clipvalue=clipvalue)
    if kind == "sgd":
        ops.sgd_step(bufs[0], g, bufs[1], hp["lr"], hp["momentum"], hp["nesterov"], **clip)
    elif kind == "rmsprop":
        ops.rmsprop_step(bufs[0], g, bufs[1], hp["lr"], hp["rho"], hp["eps"], **clip)
    else:
        ops.adam_step_ex(bufs[0], g, bufs[1], bufs[2], bufs[3], R.adam_lr_t(hp["lr"], hp["beta_1"], hp["beta_2"], k), hp["beta_1"],
                         hp["beta_2"], hp["eps"], **clip)


def _run(config, n, grad_scale=1.0, clipnorm=0.0, clipvalue=0.0):
    """three consecutive steps from zero slots; every step is checked from the device's own state in front of it.  -> the norms read"""
    from fmri_hip import ops
    kind, hp = CONFIGS[config]
    p, gs = _inputs(n)
    bufs = [_cuda(p)] + [torch.zeros(n, dtype=torch.float32, device="cuda") for _ in range({"sgd": 1, "rmsprop": 1, "adam": 3}[kind])]
    work, out = ops.grad_sumsq_workspace("cuda")
    norms = []
    for k in range(1, STEPS + 1):
        g = _cuda(gs[k - 1])
        before = [_host(t) for t in bufs]
        gnorm = ops.grad_sumsq(g, grad_scale, work, out) if clipnorm > 0 else None
        _launch(kind, hp, k, bufs, g, grad_scale, gnorm, clipnorm, clipvalue)
        torch.cuda.synchronize()
        norm = float(np.float32(out[1].item())) if clipnorm > 0 else None          # the float the kernel made of the device's norm
        norms.append(norm)
        assert np.array_equal(_host(g), gs[k - 1]), "the gradient buffer was written"
        _check_step(kind, hp, k, before, [_host(t) for t in bufs], gs[k - 1], grad_scale, norm, clipnorm, clipvalue)
    if config == "amsgrad":
        m, v, h = (_host(t) for t in bufs[1:])
        assert np.any(h > v), "step 3 was meant to leave part of vhat above v"
    return norms


# ------------------------------------------------------------------------------------------------------------------ 1. step kernels
@pytest.mark.parametrize("grad_scale", [1.0, 0.25])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_step_kernels_three_steps(config, n, grad_scale):
    _run(config, n, grad_scale)


@functools.lru_cache(maxsize=None)
def _true_norm(n, grad_scale=1.0):
    return math.sqrt(math.fsum(float(np.float32(grad_scale) * x) ** 2 for x in _inputs(n)[1][0].tolist()))


@pytest.mark.parametrize("n", [5, 1025, 2097159])
@pytest.mark.parametrize("config", sorted(CONFIGS))
@pytest.mark.parametrize("variant", ["clipvalue", "clipnorm_above", "clipnorm_below", "both"])
def test_step_kernels_clipping(config, n, variant):
    """clipnorm half the first gradient's norm (it clips: norm >= clipnorm) and four times it (it does not); clipvalue 0.3 cuts the
    tails of a unit normal, and still cuts after a norm clip to a per-element scale of about 0.5"""
    norm1 = _true_norm(n)
    clipnorm = dict(clipvalue=0.0, clipnorm_above=0.5 * norm1, clipnorm_below=4.0 * norm1, both=0.5 * norm1)[variant]
    clipvalue = 0.3 if variant in ("clipvalue", "both") else 0.0
    norms = _run(config, n, 1.0, clipnorm=clipnorm, clipvalue=clipvalue)
    if variant in ("clipnorm_above", "both"):
        assert norms[0] >= np.float32(clipnorm)
    if variant == "clipnorm_below":
        assert all(v < np.float32(clipnorm) for v in norms)


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_zero_gradient_with_clipnorm_changes_nothing(config):
    """norm 0 < clipnorm: nothing is clipped and nothing divided by the norm - the parameters keep their bits, the slots stay 0"""
    from fmri_hip import ops
    n = 1025
    kind, hp = CONFIGS[config]
    p = _inputs(n)[0]
    bufs = [_cuda(p)] + [torch.zeros(n, dtype=torch.float32, device="cuda") for _ in range({"sgd": 1, "rmsprop": 1, "adam": 3}[kind])]
    g = torch.zeros(n, dtype=torch.float32, device="cuda")
    work, out = ops.grad_sumsq_workspace("cuda")
    for k in (1, 2):
        _launch(kind, hp, k, bufs, g, 1.0, ops.grad_sumsq(g, 1.0, work, out), 1.0, 0.0)
    torch.cuda.synchronize()
    assert out.tolist() == [0.0, 0.0]
    assert np.array_equal(_host(bufs[0]).view(np.uint32), p.view(np.uint32))
    for t in bufs[1:]:
        assert np.all(_host(t) == 0.0)


# ------------------------------------------------------------------------------------------------------------------ 2. the existing Adam
def test_adam_step_ex_without_options_gives_adam_steps_bits():
    from fmri_hip import ops
    n = 2097159
    p, gs = _inputs(n)
    rs = np.random.RandomState(5)
    m0, v0 = rs.randn(n).astype(np.float32) * 0.1, (rs.randn(n).astype(np.float32) * 0.1) ** 2
    a = [_cuda(p), _cuda(m0), _cuda(v0)]
    b = [_cuda(p), _cuda(m0), _cuda(v0)]
    for k, scale in ((1, 1.0), (2, 0.25)):
        g = _cuda(gs[k - 1])
        lr_t = R.adam_lr_t(1e-3, 0.9, 0.999, k)
        ops.adam_step(a[0], g, a[1], a[2], lr_t, 0.9, 0.999, 1e-7, scale)
        ops.adam_step_ex(b[0], g, b[1], b[2], None, lr_t, 0.9, 0.999, 1e-7, scale)
    torch.cuda.synchronize()
    for name, x, y in zip("pmv", a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), name


# ------------------------------------------------------------------------------------------------------------------ 3. sum of squares
def _sumsq_data(kind, n):
    rs = np.random.RandomState(77 + n % 911)
    if kind == "decades":
        return (rs.randn(n) * 10.0 ** rs.uniform(-3, 3, n)).astype(np.float32)
    if kind == "spike":
        g = rs.randn(n).astype(np.float32)
        g[n // 2] = np.float32(1e18)
        return g
    return np.zeros(n, np.float32)


@pytest.mark.parametrize("grad_scale", [1.0, 0.3])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 32771, 2097159])
@pytest.mark.parametrize("kind", ["decades", "spike", "zeros"])
def test_grad_sumsq_against_fsum(kind, n, grad_scale):
    from fmri_hip import ops
    g = _sumsq_data(kind, n)
    scaled = (np.float32(grad_scale) * g).astype(np.float32).astype(np.float64)          # float(grad_scale * g_i), then exact squares
    ref = math.fsum((scaled * scaled).tolist())
    gd = _cuda(g)
    work, out = ops.grad_sumsq_workspace("cuda")
    got = []
    side = torch.cuda.Stream()
    for rep in range(6):                                    # five repeats on the current stream, then one on a second stream
        work.fill_(float("nan"))                            # "any contents"
        out.fill_(-1.0)
        if rep == 5:
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                ops.grad_sumsq(gd, grad_scale, work, out)
            side.synchronize()
        else:
            ops.grad_sumsq(gd, grad_scale, work, out)
        torch.cuda.synchronize()
        got.append(out.cpu().numpy().copy())
    s, r = float(got[0][0]), float(got[0][1])
    print("sumsq %s n=%d: |dev - ref| / (2^-53 ref) = %.2f" % (kind, n, abs(s - ref) / (2.0 ** -53 * ref) if ref else 0.0))
    assert abs(s - ref) <= 32 * 2.0 ** -53 * ref
    assert r == math.sqrt(s)
    for other in got[1:]:
        assert np.array_equal(other.view(np.uint64), got[0].view(np.uint64)), "the sum's bits differ between runs / streams"


# ------------------------------------------------------------------------------------------------------------------ 4. refusals
def test_refusals_launch_nothing():
    from fmri_hip import ops
    from fmri_hip._lib import lib
    L = lib()
    SHAPE, ALIGN = -1, -2
    n = 1024
    keep = np.arange(n + 4, dtype=np.float32) + 1.0
    bufs = [_cuda(keep) for _ in range(5)]                  # p, g, m, v, vhat
    work, out = ops.grad_sumsq_workspace("cuda")
    out.fill_(7.0)
    p, g, m, v, h = (t.data_ptr() for t in bufs)
    s = torch.cuda.current_stream().cuda_stream
    calls = {
        "sgd": lambda n_, p_, g_: L.fmri_sgd_step(p_, g_, m, n_, 0.1, 0.9, 1, 1.0, None, 0.0, 0.0, s),
        "rmsprop": lambda n_, p_, g_: L.fmri_rmsprop_step(p_, g_, v, n_, 0.1, 0.9, 1e-7, 1.0, None, 0.0, 0.0, s),
        "adam_ex": lambda n_, p_, g_: L.fmri_adam_step_ex(p_, g_, m, v, h, n_, 0.1, 0.9, 0.999, 1e-7, 1.0, None, 0.0, 0.0, s),
        "sumsq": lambda n_, p_, g_: L.fmri_grad_sumsq(g_, n_, 1.0, work.data_ptr(), out.data_ptr(), s),
    }
    for name, call in calls.items():
        assert call(0, p, g) == SHAPE, name
        assert call(n, p, g + 4) == ALIGN, name              # the view [1:] of the gradient: off the 16-byte rule by one float
        if name != "sumsq":
            assert call(n, p + 4, g) == ALIGN, name
    assert L.fmri_sgd_step(p, g, m, n, 0.1, 0.9, 1, 1.0, out.data_ptr() + 4, 1.0, 0.0, s) == ALIGN      # the norm: 8-byte rule
    # a missing buffer (a caller that drops SGD's moments at momentum 0, say) is refused, not launched on; only AMSGrad's vhat may be NULL
    assert L.fmri_sgd_step(p, g, None, n, 0.1, 0.0, 0, 1.0, None, 0.0, 0.0, s) == SHAPE
    assert L.fmri_sgd_step(None, g, m, n, 0.1, 0.9, 0, 1.0, None, 0.0, 0.0, s) == SHAPE
    assert L.fmri_rmsprop_step(p, g, None, n, 0.1, 0.9, 1e-7, 1.0, None, 0.0, 0.0, s) == SHAPE
    assert L.fmri_rmsprop_step(p, None, v, n, 0.1, 0.9, 1e-7, 1.0, None, 0.0, 0.0, s) == SHAPE
    assert L.fmri_adam_step(p, g, None, v, n, 0.1, 0.9, 0.999, 1e-7, 1.0, s) == SHAPE
    assert L.fmri_adam_step_ex(p, g, m, None, h, n, 0.1, 0.9, 0.999, 1e-7, 1.0, None, 0.0, 0.0, s) == SHAPE
    torch.cuda.synchronize()
    for t in bufs:
        assert np.array_equal(_host(t), keep)
    assert out.tolist() == [7.0, 7.0]


# ------------------------------------------------------------------------------------------------------------------ 5. engines
def _unet_model(**kw):
    import fetal_net.model as fmodel
    return fmodel.unet_model_3d(input_shape=(1, 16, 16, 16), depth=2, n_base_filters=8, **kw), (2, 1, 16, 16, 16)


def _isensee_model(**kw):
    import fetal_net.model as fmodel
    return fmodel.isensee2017_model_3d(input_shape=(1, 16, 32, 32), depth=3, n_base_filters=8, **kw), (2, 1, 16, 32, 32)


def _batch(shape, seed=3):
    from oracle.unet_oracle import synthetic_batch
    x, y = synthetic_batch(shape, seed_x=seed, seed_y=seed + 100)
    return x.astype(np.float32), y


def _engine_of(model, shape, optimizer):
    model.compile(optimizer=optimizer, loss=model.loss, metrics=model.metrics)
    eng = model.engine(shape[0])
    x, y = _batch(shape)
    return eng, model._to_device_x(x), model._to_device_y(y)


def _backward(eng, xd, yd):
    eng.forward(xd)
    eng.loss_forward(yd)
    eng.backward(yd)
    torch.cuda.synchronize()


def _slot_buffers(eng, kind):
    return {"sgd": [eng.M], "rmsprop": [eng.V], "adam": [eng.M, eng.V, eng.Vhat]}[kind]


def _make_optimizer(name, clipnorm=None):
    from fetal_net import optimizers as opt
    if name == "sgd":
        return opt.SGD(lr=0.013, momentum=0.9, nesterov=True), "sgd", dict(lr=0.013, momentum=0.9, nesterov=True)
    if name == "rmsprop":
        return opt.RMSprop(), "rmsprop", dict(lr=0.001, rho=0.9, eps=1e-7)
    return (opt.Adam(amsgrad=True, clipnorm=clipnorm), "adam", dict(lr=0.001, beta_1=0.9, beta_2=0.999, eps=1e-7))


ENGINES = {"unet_fp32": (_unet_model, "fp32"), "isensee_bf16": (_isensee_model, "bf16")}


@pytest.mark.parametrize("optimizer", ["sgd", "rmsprop", "amsgrad_clipnorm"])
@pytest.mark.parametrize("engine", sorted(ENGINES))
def test_engines_step_as_the_restatement(engine, optimizer, monkeypatch):
    build, dtype = ENGINES[engine]
    monkeypatch.setenv("FMRI_DTYPE", dtype)
    model, shape = build()
    clipnorm = None
    if optimizer == "amsgrad_clipnorm":
        # c from the first step's norm, so that step 1 clips: a backward pass under the builder's optimizer gives that norm
        eng, xd, yd = _engine_of(model, shape, model.optimizer)
        _backward(eng, xd, yd)
        clipnorm = 0.5 * float(torch.linalg.vector_norm(eng.G.double()).item())
    opt, kind, hp = _make_optimizer(optimizer.split("_")[0], clipnorm)
    eng, xd, yd = _engine_of(model, shape, opt)
    assert eng.opt["kind"] == kind and (eng.Vhat is not None) == (kind == "adam") and (eng._gnorm is not None) == (clipnorm is not None)
    logits0 = None
    for k in range(1, STEPS + 1):
        _backward(eng, xd, yd)
        if logits0 is None:
            logits0 = eng.logits.float().clone()
        G = _host(eng.G)
        before = [_host(eng.P)] + [_host(t) for t in _slot_buffers(eng, kind)]
        eng.optimizer_step(opt.lr)
        torch.cuda.synchronize()
        assert eng.t == k
        norm = None
        if clipnorm is not None:
            norm = float(np.float32(eng._gnorm[1].item()))
            # padding, moving statistics and whatever else the flat layout holds add nothing: the norm over the whole buffer is the
            # norm over the trainable weights
            trainable = eng.flat_to_keras(G, moving=False)
            ref = math.sqrt(math.fsum(float(v) ** 2 for a in trainable.values() for v in np.asarray(a, np.float64).ravel().tolist()))
            assert abs(eng._gnorm[1].item() - ref) <= 1e-6 * ref
            if k == 1:
                assert norm >= np.float32(clipnorm)
        after = [_host(eng.P)] + [_host(t) for t in _slot_buffers(eng, kind)]
        _check_step(kind, hp, k, before, after, G, 1.0, norm, clipnorm or 0.0, 0.0)
    eng.forward(xd)
    torch.cuda.synchronize()
    assert not torch.equal(eng.logits.float(), logits0), "the weight copies were not refreshed: the forward pass did not move"


@pytest.mark.parametrize("engine", sorted(ENGINES))
def test_gradient_outside_the_trainable_weights_is_exactly_zero(engine, monkeypatch):
    """what fmri_grad_sumsq over the whole flat G relies on: channel padding, moving statistics and alignment holes carry exact zeros"""
    build, dtype = ENGINES[engine]
    monkeypatch.setenv("FMRI_DTYPE", dtype)
    model, shape = build()
    eng, xd, yd = _engine_of(model, shape, _make_optimizer("sgd")[0])
    for _ in range(2):
        _backward(eng, xd, yd)
        eng.optimizer_step(0.01)
    _backward(eng, xd, yd)
    G = _host(eng.G)
    ones = eng.flat_to_keras(np.ones(eng.n_flat, np.float32), moving=False)
    covered = eng.keras_to_flat(dict(eng.flat_to_keras(np.zeros(eng.n_flat, np.float32)), **ones)) != 0       # the trainable positions
    assert covered.sum() == sum(np.asarray(a).size for a in ones.values())
    assert np.count_nonzero(G[covered]) > 0.5 * covered.sum()
    assert np.all(G[~covered] == 0.0)


def test_adam_beta_2_and_epsilon_reach_the_kernel(monkeypatch):
    from fetal_net import optimizers as opt
    monkeypatch.setenv("FMRI_DTYPE", "fp32")
    model, shape = _unet_model()
    o = opt.Adam(lr=0.002, beta_2=0.99, epsilon=1e-3)
    eng, xd, yd = _engine_of(model, shape, o)
    hp = dict(lr=0.002, beta_1=0.9, beta_2=0.99, eps=1e-3)
    for k in (1, 2):
        _backward(eng, xd, yd)
        G, before = _host(eng.G), [_host(eng.P), _host(eng.M), _host(eng.V)]
        eng.optimizer_step(o.lr)
        torch.cuda.synchronize()
        after = [_host(eng.P), _host(eng.M), _host(eng.V)]
        assert eng.Vhat is None
        # without AMSGrad the denominator is v itself: the restatement's vhat slot is the device's v
        _check_step("adam", hp, k, before + [np.zeros_like(after[2])], after + [after[2]], G, 1.0, None, 0.0, 0.0)
        # and the defaults would have stepped elsewhere, by far more than the bound
        d_default = R.adam_increment(after[1], after[2], R.adam_lr_t(0.002, 0.9, 0.999, k), 1e-7)
        d_here = R.adam_increment(after[1], after[2], R.adam_lr_t(0.002, 0.9, 0.99, k), 1e-3)
        assert np.max(np.abs(d_default - d_here)) > 1e3 * R.U * np.max(np.abs(d_here))


def test_norm_net_chain_steps_rmsprop_and_leaves_the_segmenter():
    import fetal_net.model as fmodel
    from fetal_net.optimizers import RMSprop
    seg, shape = _unet_model()
    model = fmodel.norm_net_model(input_shape=shape[1:], n_base_filters=4, depth=3, dropout_rate=0, n_segmentation_levels=2,
                                  optimizer=RMSprop, old_model_path=seg)
    assert type(model.optimizer) is RMSprop and type(model.norm_net.optimizer) is RMSprop
    x, y = _batch(shape)
    eng = model.engine(shape[0])
    assert eng.opt["kind"] == "rmsprop" and eng.norm.opt["kind"] == "rmsprop"
    seg_p, norm_p = eng.seg.P.clone(), eng.norm.P.clone()
    model.train_on_batch(x, y)
    torch.cuda.synchronize()
    assert torch.equal(eng.seg.P.view(torch.int32), seg_p.view(torch.int32)) and eng.seg.t == 0
    assert not torch.equal(eng.norm.P, norm_p) and eng.norm.t == 1
    assert float(eng.norm.V.abs().max()) > 0 and float(eng.norm.M.abs().max()) == 0          # RMSprop's accumulators live in V


# ------------------------------------------------------------------------------------------------------------------ 6. checkpoints
def _ckpt_optimizer(name):
    from fetal_net import optimizers as opt
    return {"sgd": lambda: opt.SGD(lr=0.01, momentum=0.9, nesterov=True, decay=1e-3),
            "rmsprop": lambda: opt.RMSprop(lr=0.002, rho=0.8, epsilon=1e-6, decay=1e-3),
            "adam": lambda: opt.Adam(lr=0.002, beta_2=0.99, amsgrad=True, clipnorm=0.5, clipvalue=0.25)}[name]()


def _containers():
    """the HDF5 container where libhdf5 loads, the npz container everywhere"""
    from fetal_net.utils import hdf5
    return ["h5", "npz"] if hdf5.available() else ["npz"]


@pytest.mark.parametrize("container", _containers())
@pytest.mark.parametrize("name", ["sgd", "rmsprop", "adam"])
def test_checkpoint_round_trip(name, container, tmp_path, monkeypatch):
    from fetal_net.training import load_old_model
    from fetal_net.utils import hdf5
    monkeypatch.setenv("FMRI_DTYPE", "fp32")
    monkeypatch.setenv("FMRI_CHECKPOINT_FORMAT", container)
    model, shape = _unet_model()
    model.compile(optimizer=_ckpt_optimizer(name), loss=model.loss, metrics=model.metrics)
    x, y = _batch(shape)
    for _ in range(2):
        model.train_on_batch(x, y)
    path = str(tmp_path / "ckpt.h5")
    model.save(path)
    assert hdf5.is_hdf5(path) == (container == "h5")
    saved = model.get_optimizer_slots()
    again = load_old_model(path)
    assert type(again.optimizer) is type(model.optimizer)
    assert again.optimizer.keras_config() == model.optimizer.keras_config()
    pending = again.get_optimizer_slots()
    assert pending["class_name"] == saved["class_name"] == type(model.optimizer).__name__
    assert pending["iterations"] == (0 if name == "rmsprop" else 2)          # Keras' RMSprop.weights carries no iteration count
    assert list(pending["slots"]) == list(saved["slots"]) == {"sgd": ["moments"], "rmsprop": ["accumulators"], "adam": ["m", "v", "vhat"]}[name]
    for slot in saved["slots"]:
        for k, a in saved["slots"][slot].items():
            assert np.array_equal(np.asarray(pending["slots"][slot][k]).view(np.uint32), np.asarray(a, np.float32).view(np.uint32)), (slot, k)
    # the same gradient in both engines, one step: the same parameter bits
    e1, e2 = model.engine(shape[0]), again.engine(shape[0])
    assert e2.t == pending["iterations"] and e2.opt == e1.opt
    if name == "rmsprop":
        e2.t = e1.t                      # (decay reads the count, which an RMSprop checkpoint does not carry)
    for a, b in zip(_slot_buffers(e1, e1.opt["kind"]) + [e1.P], _slot_buffers(e2, e2.opt["kind"]) + [e2.P]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    _backward(e1, model._to_device_x(x), model._to_device_y(y))
    e2.G.copy_(e1.G)
    e1.optimizer_step(model.optimizer.lr)
    e2.optimizer_step(again.optimizer.lr)
    torch.cuda.synchronize()
    assert torch.equal(e1.P.view(torch.int32), e2.P.view(torch.int32))
