"""Op tests at the sizes the models run (the size-dependent branches of the kernels that test_gpu_ops.py only meets at toy shapes):
the first-layer kernels' RELU = false instantiations and the 3-channel 3-D form, the normalisation passes (reduction chunking, grid-stride
apply loops whose cached per-(instance, channel) coefficients are reused and cross instance boundaries, the scalar paths of bf16 channel
counts that are not a power-of-two multiple of 8, the *_pre entry points, inference statistics, the moving averages, constant channels,
offset data) and the k2s2 transposed / direct convolutions at Cin 64-512 (thread blocks that loop over input-channel blocks, fewer
output voxels than the weight gradient's splits, channel slices of a wider gradient, optional outputs).

References: fp64.  The convolutions' on the CPU (torch, <= 16 threads); the normalisation's element-wise fp64 restatement runs with torch
on the device (plain torch tensor ops in float64 - none of this project's kernels), which keeps 30 M-element cases within a few seconds.
Bars follow the rule of test_gpu_ops.py: |got - ref| <= atol * max|ref| + rtol * |ref|, each pair <= 2x the error measured on MI355X with
FMRI_MEASURE=1 (gpu_util records, per check, the fraction of the bar the worst element used), or exact where the arithmetic allows.
"""
import os

import pytest
import torch
import torch.nn.functional as F

import gpu_util
from gpu_util import assert_close, f64, rnd, to_ncdhw, to_ndhwc

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the GPU box"
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    from fmri_hip import ops as o
    return o


def _dy4(g, shape, lo, hi, div):
    return torch.randint(lo, hi + 1, shape, generator=g).float() / div


# ------------------------------------------------------------------------------------------------ first layer, small shapes
# (C0, Cout, N, D, H, W, planar): every channel count of FMRI_FIRST_DISPATCH, 3-D 1-4 and 2-D 1-7
FIRST_SMALL = [(c, 32 if c % 2 else 64, 1, 4, 16, 32, False) for c in (1, 2, 3, 4)] + \
              [(c, 64 if c % 2 else 32, 1, 4, 16, 64, True) for c in (1, 2, 3, 4, 5, 6, 7)]


@pytest.mark.parametrize("case", FIRST_SMALL, ids=lambda c: "%s_c%d_o%d" % ("2d" if c[6] else "3d", c[0], c[1]))
def test_first_layer_without_relu_is_exact_on_dyadic_data(ops, case):
    """the RELU = false instantiation of k_conv_first_fwd (no activation: the first conv of a normalised block; LeakyReLU) against the
    generic kernels on dyadic data: every product and partial sum exact in fp32, alpha = 0.25 exact, one bf16 rounding - bit for bit"""
    from fmri_hip._lib import ACT_LEAKY, ACT_NONE, ACT_RELU, IMPL_GENERIC, IMPL_MFMA
    C0, Cout, N, D, H, W, planar = case
    g = torch.Generator().manual_seed(C0 * 10 + Cout + planar)
    x = _dy4(g, (N, D, H, W, C0), -4, 4, 4.0).to(BF).cuda()
    w = _dy4(g, (27, Cout, C0), -2, 2, 8.0).to(BF).cuda()
    bias = _dy4(g, (Cout,), -4, 4, 4.0).cuda()
    for act, alpha in ((ACT_NONE, 0.0), (ACT_LEAKY, 0.25), (ACT_RELU, 0.0)):
        out = []
        for impl in (IMPL_MFMA, IMPL_GENERIC):
            y = torch.full((N, D, H, W, Cout), float("nan"), dtype=BF, device="cuda")
            ops.conv3d_fwd(x, None, w, bias, y, act=act, alpha=alpha, impl=impl, planar=planar)
            out.append(y.float().cpu())
        assert torch.equal(out[0], out[1]), "act %d: %d outputs differ" % (act, int((out[0] != out[1]).sum()))
        assert not bool(torch.isnan(out[0]).any())


FIRST_TOL = {"fwd": (5e-3, 1e-4),              # measured 0.75 of the bar (the bf16 rounding)
             "dw": (1.7e-7, 1.7e-7)}           # 0.52 (dw and db: fp32 sums of exact bf16 products)


@pytest.mark.parametrize("case", FIRST_SMALL, ids=lambda c: "%s_c%d_o%d" % ("2d" if c[6] else "3d", c[0], c[1]))
def test_first_layer_leaky_and_3_channel_vs_fp64(ops, case):
    """LeakyReLU(0.01) through the RELU = false kernels, and the weight gradient of every channel count (the 3-channel 3-D form has no
    other reference test), against fp64"""
    from fmri_hip._lib import ACT_LEAKY, IMPL_MFMA
    C0, Cout, N, D, H, W, planar = case
    x = rnd((N, D, H, W, C0), 600 + C0, BF)
    w = rnd((27, Cout, C0), 610 + C0, BF, scale=0.2)
    if planar:
        w[:9] = 0
        w[18:] = 0
    bias = rnd((Cout,), 620 + C0, torch.float32)
    y = torch.full((N, D, H, W, Cout), float("nan"), dtype=BF, device="cuda")
    ops.conv3d_fwd(x, None, w, bias, y, act=ACT_LEAKY, alpha=0.01, impl=IMPL_MFMA, planar=planar)
    dy = rnd((N, D, H, W, Cout), 630 + C0, BF)
    dw = torch.zeros((27, Cout, C0), device="cuda")
    db = torch.zeros(Cout, device="cuda")
    ops.conv3d_wgrad(x, None, dy, dw, db, impl=IMPL_MFMA, planar=planar)
    torch.cuda.synchronize()
    xr = to_ncdhw(f64(x))
    wk = f64(w).reshape(3, 3, 3, Cout, C0).permute(3, 4, 0, 1, 2).contiguous().requires_grad_(True)
    pre = F.conv3d(xr, wk, f64(bias), padding=1)
    assert_close(y, to_ndhwc(F.leaky_relu(pre.detach(), 0.01)), *FIRST_TOL["fwd"], what="first leaky fwd")
    pre.backward(to_ncdhw(f64(dy)))
    refg = wk.grad.permute(2, 3, 4, 0, 1).reshape(27, Cout, C0)
    if planar:
        refg[:9] = 0
        refg[18:] = 0
    assert_close(dw, refg, *FIRST_TOL["dw"], what="first dw")
    assert_close(db, f64(dy).sum(dim=(0, 1, 2, 3)), *FIRST_TOL["dw"], what="first db")


# ------------------------------------------------------------------------------------------------ normalisation
EPS = 1e-3
ALPHA = 0.2
NORM_SHAPES = [
    # N, D, H, W, C
    (2, 64, 128, 128, 16),     # Isensee level 0: the apply loops stride over 4 M items with 1 M threads and cross the sample boundary
    (2, 32, 64, 64, 32),       # level 1
    (4, 8, 16, 16, 256),       # level 4
    (3, 17, 33, 29, 32),       # odd extents: V = 16,269 is no multiple of the reduction chunk
    (2, 16, 32, 32, 48),       # C / 8 = 6: scalar reduction and non-sample-local apply in bf16; fp32: a stride that is no multiple of C / 8
    (2, 4, 8, 8, 1024),        # C / 8 = 128 > 64: the scalar paths in bf16
]
# (rtol, atol) per dtype.  fp32: the inputs are exact, what remains is the fp32 arithmetic of the statistics and the apply pass; bf16:
# plus one rounding of the stored output (2^-8 relative).  Comment: the largest fraction of the bar any element used on MI355X (and where).
NORM_TOL = {
    "fwd": {torch.float32: (3.7e-6, 3.7e-7),       # 0.51 (offset-8 data, instance; zero-mean data 0.035)
            torch.bfloat16: (5e-3, 2e-4)},         # 0.72 (the bf16 rounding)
    "dx": {torch.float32: (2.6e-7, 2.6e-8),        # 0.50
           torch.bfloat16: (5.4e-3, 1.8e-3)},      # 0.50
    "dparam": {torch.float32: (6.9e-6, 6.9e-7),    # 0.50 (dgamma)
               torch.bfloat16: (1.3e-6, 1.3e-7)},  # 0.51 (fp32 sums of the stored bf16 values)
}


# the constant-channel test: z = fma(b, gamma / s, beta - b gamma / s) is off by the rounding of |b gamma / s| (s = eps for instance norm,
# so up to ~5,000 here) rather than of |z|, and dgamma sums dz * x - mean * dz over the channel in fp32 partial sums (the bf16 path):
# both carry the constant's magnitude, hence bars of their own
CONST_TOL = {
    "fwd": {torch.float32: (2.7e-4, 2.7e-5),       # 0.50 (instance norm)
            torch.bfloat16: (5e-3, 2e-4)},         # 0.72
    "dx": {torch.float32: (2.3e-7, 2.3e-8),        # 0.51
           torch.bfloat16: (4.9e-3, 1.6e-3)},      # 0.51
    "dparam": {torch.float32: (7.5e-6, 7.5e-7),    # 0.50
               torch.bfloat16: (9.5e-4, 9.5e-5)},  # 0.50 (dgamma of the constant channels, instance norm)
}


def _act(z, act):
    return F.relu(z) if act == 1 else (F.leaky_relu(z, ALPHA) if act == 2 else z)


class NormRef:
    """fp64 normalisation of x [N, V, C] (float64, on the device): batch statistics over all N x V voxels per channel (eps inside the
    square root), or instance statistics per (sample, channel) with keras-contrib's (x - mean) / (sigma + eps)"""

    def __init__(self, x, gamma, beta, per):
        N, V, C = x.shape
        self.per, self.shape = per, x.shape
        xg = x if per else x.reshape(1, N * V, C)
        x0 = xg[:, :1]
        self.mean = x0 + (xg - x0).mean(1, keepdim=True)              # (shifted: exactly the value of a constant channel, sigma exactly 0)
        var = ((xg - self.mean) ** 2).mean(1, keepdim=True)
        self.sigma = var.sqrt()
        self.s = self.sigma + EPS if per else (var + EPS).sqrt()
        self.xhat = (xg - self.mean) / self.s
        self.gamma, self.beta = gamma, beta
        self.z = (self.xhat * gamma + beta).reshape(N, V, C)

    def bwd(self, dz):
        """dz = dy * act'(z): dx = gamma / s * (dz - mean dz - xhat * mean(dz * xhat) * s / sigma) (batch norm: s / sigma = 1; a constant
        channel, sigma = 0, has xhat = 0 and no sigma term), dgamma = sum dz * xhat, dbeta = sum dz"""
        N, V, C = self.shape
        d = dz if self.per else dz.reshape(1, N * V, C)
        m1 = d.mean(1, keepdim=True)
        m2 = (d * self.xhat).mean(1, keepdim=True)
        ratio = torch.where(self.sigma > 0, self.s / self.sigma, torch.zeros_like(self.s)) if self.per else torch.ones_like(self.s)
        dx = self.gamma / self.s * (d - m1 - self.xhat * m2 * ratio)
        return dx.reshape(N, V, C), (d * self.xhat).sum(dim=(0, 1)), d.sum(dim=(0, 1))


def _dz(dy, y, act):
    """dy * act'(z), the sign of z taken from the kernel's own stored output (fp32 and fp64 z can straddle 0 for the odd one of 30 M
    elements; the forward output itself is checked against fp64)"""
    dyd = dy.double()
    if act == 0:
        return dyd
    return torch.where(y > 0, dyd, dyd * (0.0 if act == 1 else ALPHA))


def _dev_close(got, ref, rtol, atol, what):
    """gpu_util.assert_close with its arithmetic on the device (tensors of 30 M elements)"""
    got, ref = got.reshape(ref.shape).double(), ref.double()
    scale = float(ref.abs().max()) + 1e-30
    err = (got - ref).abs()
    tol = atol * scale + rtol * ref.abs()
    if os.environ.get("FMRI_MEASURE", "0") == "1":
        gpu_util._record(what, rtol, atol, float((err / tol).max()))
        return
    bad = ~(err <= tol)                    # (NaN fails)
    if bool(bad.any()):
        idx = torch.nonzero(bad)[:5].tolist()
        raise AssertionError("%s: %d/%d elements off; max err %.3e (scale %.3e); first idx %s got %s ref %s" % (
            what, int(bad.sum()), bad.numel(), float(err.max()), scale, idx,
            [float(got[tuple(i)]) for i in idx], [float(ref[tuple(i)]) for i in idx]))


def _close(got, ref, kind, dtype, what):
    _dev_close(got, ref, *NORM_TOL[kind][dtype], what="%s %s %s" % (what, kind, "f32" if dtype == torch.float32 else "bf16"))


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("mode", ["batch", "instance"])
@pytest.mark.parametrize("shape", NORM_SHAPES, ids=lambda s: "N%d_%dx%dx%d_c%d" % s)
def test_norm_at_model_sizes_vs_fp64(ops, shape, mode, dtype):
    """fmri_norm_act_fwd, fmri_norm_act_bwd (reads y), fmri_norm_act_bwd_x (recomputes the sign from x) for ReLU, LeakyReLU and no
    activation, and fmri_norm_act_fwd_pre / fmri_norm_act_bwd_pre fed with fp64 sums, all on ONE scratch ws that every call must leave
    zero (a call that left sums behind would corrupt the statistics of the next)"""
    N, D, H, W, C = shape
    per = mode == "instance"
    G = N if per else 1
    V = D * H * W
    x = rnd(shape, 700 + C, dtype, scale=1.5) + 0.3
    gamma = rnd((C,), 701, torch.float32) * 0.5 + 1.0
    beta = rnd((C,), 702, torch.float32) * 0.2
    dy = rnd(shape, 703 + C, dtype)
    ref = NormRef(x.double().reshape(N, V, C), gamma.double(), beta.double(), per)
    ws = torch.zeros((G, C, 2), dtype=torch.float64, device="cuda")
    stats = torch.zeros((G, C, 3), device="cuda")
    y, dx, dx2 = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    for act in (1, 2, 0):
        y.fill_(float("nan"))
        ops.norm_act_fwd(x, gamma, beta, y, stats, ws, per, eps=EPS, eps_on_std=per, act=act, alpha=ALPHA)
        torch.cuda.synchronize()
        assert float(ws.abs().max()) == 0.0, "fwd left sums in ws"
        _close(y, _act(ref.z, act), "fwd", dtype, "norm %s act %d" % (mode, act))
        rdx, rdg, rdb = ref.bwd(_dz(dy.reshape(N, V, C), y.reshape(N, V, C), act))
        dg, db = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
        ops.norm_act_bwd(x, y, dy, gamma, stats, dx, dg, db, ws, per, act=act, alpha=ALPHA)
        torch.cuda.synchronize()
        assert float(ws.abs().max()) == 0.0, "bwd left sums in ws"
        _close(dx, rdx, "dx", dtype, "norm %s act %d" % (mode, act))
        _close(dg, rdg, "dparam", dtype, "norm dgamma")
        _close(db, rdb, "dparam", dtype, "norm dbeta")
        dg2, db2 = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
        ops.norm_act_bwd(x, None, dy, gamma, stats, dx2, dg2, db2, ws, per, act=act, alpha=ALPHA, beta=beta)
        torch.cuda.synchronize()
        assert float(ws.abs().max()) == 0.0, "bwd_x left sums in ws"
        _close(dx2, rdx, "dx", dtype, "norm from x %s act %d" % (mode, act))
        _close(dg2, rdg, "dparam", dtype, "norm from x dgamma")
        _close(db2, rdb, "dparam", dtype, "norm from x dbeta")
    # a second forward on the same ws: the statistics of a fresh ws (the last call above left it zero)
    stats2 = torch.zeros_like(stats)
    ops.norm_act_fwd(x, gamma, beta, y, stats2, ws, per, eps=EPS, eps_on_std=per, act=0)
    ops.norm_act_fwd(x, gamma, beta, y, stats2, ws, per, eps=EPS, eps_on_std=per, act=0)
    torch.cuda.synchronize()
    _dev_close(stats2, stats, 2.0 ** -23, 0.0, what="norm stats on a reused ws")     # (fp64 atomics in another order: <= 1 fp32 ulp)
    # the *_pre forms, fed with fp64 sums of the stored values
    xg = x.double().reshape(G, -1, C)
    ws_pre = torch.stack([xg.sum(1), (xg * xg).sum(1)], dim=-1).contiguous()
    y.fill_(float("nan"))
    stats_pre = torch.zeros_like(stats)
    ops.norm_act_fwd_pre(x, gamma, beta, y, stats_pre, ws_pre, per, eps=EPS, eps_on_std=per, act=2, alpha=ALPHA)
    torch.cuda.synchronize()
    assert float(ws_pre.abs().max()) == 0.0
    _close(y, _act(ref.z, 2), "fwd", dtype, "norm pre %s" % mode)
    dyg = dy.double().reshape(G, -1, C)
    ws_pre = torch.stack([dyg.sum(1), (dyg * xg).sum(1)], dim=-1).contiguous()          # dz := dy, {sum dz, sum dz * x}
    dg, db = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
    ops.norm_act_bwd_pre(x, dy, gamma, stats_pre, dx, dg, db, ws_pre, per)
    torch.cuda.synchronize()
    assert float(ws_pre.abs().max()) == 0.0
    rdx, rdg, rdb = ref.bwd(dy.double().reshape(N, V, C))
    _close(dx, rdx, "dx", dtype, "norm pre %s" % mode)
    _close(dg, rdg, "dparam", dtype, "norm pre dgamma")
    _close(db, rdb, "dparam", dtype, "norm pre dbeta")


def _norm_lane_terms(V, N, per, C, dtype):
    """the most values one lane of the reduction pass sums in fp32: the chunk of norm_vchunk (norm_deconv.hip) over the voxel lanes of
    the kernel that takes the shape (k_norm_reduce_v: 256 / (C / 8) lanes; k_norm_reduce: 4)"""
    total = V if per else V * N
    c = -(-V // 512) if per else -(-(V * N) // 1024)
    c = max(c, -(-65536 // C))
    if -(-total // c) * (N if per else 1) < 256:
        c = -(-(total * (N if per else 1)) // 256)
        c = min(max(-(-c // 64) * 64, 64), 4096)
    else:
        c = min(max(-(-c // 256) * 256, 512), 4096)
    cg = C // 8
    vec = dtype == BF and C % 8 == 0 and 1 <= cg <= 64 and (cg & (cg - 1)) == 0
    return -(-c // (256 // cg if vec else 4))


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("mode", ["batch", "instance"])
@pytest.mark.parametrize("offset", [8.0, 64.0])
def test_norm_of_offset_data(ops, offset, mode, dtype):
    """x = offset + N(0, 1): the variance comes from E[x^2] - mean^2 of fp32 partial sums.  At mean / std ~ 8 the normal bars hold.
    At ~ 64 they need not, and the bound follows from the arithmetic: a lane adds n values (n from the chunking, _norm_lane_terms) in
    fp32, so each partial sum of x and x^2 is off by at most (n - 1) u times the sum of the magnitudes (u = 2^-24); the lanes meet in fp64.
    Hence |d mean| <= n u E|x| and |d var| <= n u (E[x^2] + 2 |mean| E|x|) per (group, channel).  The normalised value z = gamma (x - mean)
    / s + beta then moves by at most |gamma| (|d mean| / s + |x - mean| / s * ds / s), with ds / s = |d var| / (2 (var + eps)) (batch)
    or |d var| / (2 sigma (sigma + eps)) (instance); the fp32 apply (z = fma(x, sc, sh), sc = gamma / s and sh = beta - mean sc, each
    rounded) adds 3 u (|x sc| + |sh|) + u |z|, and a bf16 store 2^-8 |z|.  ReLU and LeakyReLU do not enlarge a difference.  Each output
    element must lie within that bound of the fp64 value (x offset by 64 is stored as it is, bf16 included: the reference sees the same
    values)."""
    N, D, H, W, C = 2, 32, 64, 64, 32
    per = mode == "instance"
    G = N if per else 1
    V = D * H * W
    x = rnd((N, D, H, W, C), 710, dtype) + offset
    gamma = rnd((C,), 711, torch.float32) * 0.5 + 1.0
    beta = rnd((C,), 712, torch.float32) * 0.2
    ref = NormRef(x.double().reshape(N, V, C), gamma.double(), beta.double(), per)
    ws = torch.zeros((G, C, 2), dtype=torch.float64, device="cuda")
    stats = torch.zeros((G, C, 3), device="cuda")
    y = torch.empty_like(x)
    ops.norm_act_fwd(x, gamma, beta, y, stats, ws, per, eps=EPS, eps_on_std=per, act=2, alpha=ALPHA)
    torch.cuda.synchronize()
    zr = _act(ref.z, 2)
    if offset <= 8.0:
        _close(y, zr, "fwd", dtype, "norm offset %g %s" % (offset, mode))
        return
    u = 2.0 ** -24
    n = _norm_lane_terms(V, N, per, C, dtype)
    xg = x.double().reshape(G, -1, C)
    dmean = n * u * xg.abs().mean(1, keepdim=True) + u * ref.mean.abs()            # (+ the fp32 rounding of the stored mean)
    dvar = n * u * ((xg * xg).mean(1, keepdim=True) + 2 * ref.mean.abs() * xg.abs().mean(1, keepdim=True))
    var = ref.sigma ** 2
    rel_s = (dvar / (2 * (var + EPS)) if not per else dvar / (2 * ref.sigma * (ref.sigma + EPS))) + u           # (+ the rounding of 1/s)
    g64 = gamma.double()
    sc = (g64 / ref.s).abs()
    sh = (beta.double() - ref.mean * g64 / ref.s).abs()
    xc = (xg - ref.mean).abs()
    z = ref.z.reshape(G, -1, C).abs()
    bound = g64.abs() * (dmean / ref.s + xc / ref.s * rel_s) + 3 * u * (xg.abs() * sc + sh) + u * z
    if dtype == BF:
        bound = bound + 2.0 ** -8 * (z + bound)
    err = (y.double().reshape(G, -1, C) - zr.reshape(G, -1, C)).abs()
    gpu_util.bar("norm offset 64 %s %s: worst error / derived bound" % (mode, "f32" if dtype == torch.float32 else "bf16"), float((err / bound).max()), 1.0)


@pytest.mark.parametrize("mode", ["batch", "instance"])
@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", [(2, 32, 64, 64, 32), (3, 17, 33, 29, 32)], ids=lambda s: "N%d_%dx%dx%d_c%d" % s)
def test_norm_constant_channel(ops, shape, mode, dtype):
    """an all-background patch makes the first conv's output its bias: a channel with one value everywhere.  sigma = 0: the forward gives
    act(beta) (xhat = 0), and the backward is finite and has no sigma term - dx = gamma / s * (dz - mean dz) with s = eps (instance norm,
    1/sigma := 0) or sqrt(eps) (batch norm) - while the other channels are unaffected"""
    N, D, H, W, C = shape
    per = mode == "instance"
    G = N if per else 1
    V = D * H * W
    x = rnd((N, D, H, W, C), 720, dtype, scale=1.5)
    consts = torch.tensor([0.30078125, -1.7109375, 3.140625, 0.0123291015625])        # bf16 values (up to 8 significant bits)
    for k, b in enumerate(consts.tolist()):
        x[..., 3 * k] = b
    gamma = rnd((C,), 721, torch.float32) * 0.5 + 1.0
    beta = rnd((C,), 722, torch.float32) * 0.2
    dy = rnd((N, D, H, W, C), 723, dtype)
    ref = NormRef(x.double().reshape(N, V, C), gamma.double(), beta.double(), per)
    assert float(ref.sigma[..., 0:12:3].abs().max()) == 0.0
    ws = torch.zeros((G, C, 2), dtype=torch.float64, device="cuda")
    stats = torch.zeros((G, C, 3), device="cuda")
    y, dx = torch.empty_like(x), torch.empty_like(x)
    for act in (1, 2, 0):
        ops.norm_act_fwd(x, gamma, beta, y, stats, ws, per, eps=EPS, eps_on_std=per, act=act, alpha=ALPHA)
        dg, db = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
        ops.norm_act_bwd(x, None, dy, gamma, stats, dx, dg, db, ws, per, act=act, alpha=ALPHA, beta=beta)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(dx.float()).all()) and bool(torch.isfinite(dg).all())
        _dev_close(y, _act(ref.z, act), *CONST_TOL["fwd"][dtype], what="norm const %s fwd %s" % (mode, "f32" if dtype == torch.float32 else "bf16"))
        yc = y[..., 0:12:3].double()
        assert float((yc - _act(beta.double()[0:12:3], act)).abs().max()) <= 2.0 ** -8 * float(beta.abs().max()), "act(beta)"
        rdx, rdg, rdb = ref.bwd(_dz(dy.reshape(N, V, C), y.reshape(N, V, C), act))
        _dev_close(dx, rdx, *CONST_TOL["dx"][dtype], what="norm const %s dx %s" % (mode, "f32" if dtype == torch.float32 else "bf16"))
        _dev_close(dg, rdg, *CONST_TOL["dparam"][dtype], what="norm const %s dgamma %s" % (mode, "f32" if dtype == torch.float32 else "bf16"))
        _dev_close(db, rdb, *CONST_TOL["dparam"][dtype], what="norm const %s dbeta %s" % (mode, "f32" if dtype == torch.float32 else "bf16"))


MOVING_TOL = (6.1e-8, 6.1e-8)          # measured 0.50 of the bar (about one fp32 ulp)


def test_norm_moving_update_and_inference(ops):
    """fmri_norm_moving_update against the Keras 2.2 update (momentum 0.99, variance x M / (M - 1 - eps)) from the fp64 batch statistics,
    and the inference form (per_instance < 0: the given statistics, no reduction; ws is not touched) against fp64"""
    N, D, H, W, C = 2, 32, 64, 64, 48
    M = N * D * H * W
    x = rnd((N, D, H, W, C), 730, torch.float32, scale=1.5) + 0.3
    gamma = rnd((C,), 731, torch.float32) * 0.5 + 1.0
    beta = rnd((C,), 732, torch.float32) * 0.2
    ws = torch.zeros((1, C, 2), dtype=torch.float64, device="cuda")
    stats = torch.zeros((1, C, 3), device="cuda")
    y = torch.empty_like(x)
    ops.norm_act_fwd(x, gamma, beta, y, stats, ws, 0, eps=EPS, eps_on_std=False, act=1)
    mm = rnd((C,), 733, torch.float32) * 0.1
    mv = rnd((C,), 734, torch.float32).abs() + 0.5
    mm0, mv0 = mm.double(), mv.double()
    ops.norm_moving_update(stats, mm, mv, M, momentum=0.99, eps=EPS)
    torch.cuda.synchronize()
    xd = x.double().reshape(-1, C)
    mean, var = xd.mean(0), xd.var(0, unbiased=False)
    _dev_close(mm, 0.99 * mm0 + 0.01 * mean, *MOVING_TOL, what="moving mean")
    _dev_close(mv, 0.99 * mv0 + 0.01 * var * M / (M - 1 - EPS), *MOVING_TOL, what="moving variance")
    for dtype in (torch.float32, BF):
        xi = x.to(dtype)
        st = torch.stack([mm, torch.rsqrt(mv + EPS), torch.rsqrt(mv + EPS)], dim=-1).reshape(1, C, 3).contiguous()
        ws_i = torch.zeros((1, C, 2), dtype=torch.float64, device="cuda")
        for act in (1, 2, 0):
            yi = torch.full_like(xi, float("nan"))
            ops.norm_act_fwd(xi, gamma, beta, yi, st, ws_i, -1, eps=EPS, act=act, alpha=ALPHA)
            torch.cuda.synchronize()
            assert float(ws_i.abs().max()) == 0.0
            zr = (xi.double() - mm.double()) / (mv.double() + EPS).sqrt() * gamma.double() + beta.double()
            _close(yi, _act(zr, act), "fwd", dtype, "norm inference act %d" % act)


# ------------------------------------------------------------------------------------------------ k2s2 transposed conv
DECONV_CASES = [
    # N, D, H, W (input), Cin, Cout, planar, dy_ld - Cout, dy_off
    (2, 8, 16, 16, 64, 32, False, 0, 0),
    (1, 4, 8, 8, 128, 64, False, 16, 8),
    (2, 2, 4, 4, 256, 128, False, 32, 32),
    (1, 1, 2, 2, 512, 256, False, 5, 3),        # 4 input voxels < 16 splits; 512 channels: two 256-wide blocks
    (1, 8, 32, 32, 64, 32, True, 32, 0),
    (1, 4, 16, 16, 256, 64, True, 0, 0),
    (1, 3, 2, 2, 512, 128, True, 64, 64),
]


# measured use of each bar on MI355X in the comments (f32 / bf16)
DECONV_TOL = {
    "fwd": {torch.float32: (1e-6, 1e-6), torch.bfloat16: (5e-3, 1e-4)},         # 0.53 / 0.75
    "dx": {torch.float32: (1e-5, 1e-6), torch.bfloat16: (5e-3, 1e-4)},          # 0.55 / 0.75
    "dw": {torch.float32: (5.3e-6, 5.3e-7), torch.bfloat16: (4.5e-7, 4.5e-7)},  # 0.51 / 0.51 (dw and db)
}


def _deconv_ref(x, w, b, planar):
    """y[n, 2i + a, co] = b[co] + sum_ci x[n, i, ci] w[a][co][ci] in fp64 (taps a = ad*4 + ah*2 + aw; planar: ad = 0, D unchanged)"""
    N, D, H, W, Cin = x.shape
    Cout = w.shape[1]
    if planar:
        t = torch.einsum("ndhwc,aoc->ndhwao", x, w[:4]).reshape(N, D, H, W, 2, 2, Cout)
        return (t.permute(0, 1, 2, 4, 3, 5, 6).reshape(N, D, 2 * H, 2 * W, Cout) + b).contiguous()
    t = torch.einsum("ndhwc,aoc->ndhwao", x, w).reshape(N, D, H, W, 2, 2, 2, Cout)
    return (t.permute(0, 1, 4, 2, 5, 3, 6, 7).reshape(N, 2 * D, 2 * H, 2 * W, Cout) + b).contiguous()


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", DECONV_CASES, ids=lambda c: "%s_N%d_%dx%dx%d_%d_%d" % (("2d" if c[6] else "3d",) + c[:6]))
def test_deconv_k2s2_at_model_sizes(ops, case, dtype):
    N, D, H, W, Cin, Cout, planar, extra, off = case
    nt = 4 if planar else 8
    D2 = D if planar else 2 * D
    x = torch.relu(rnd((N, D, H, W, Cin), 800 + Cin, dtype))
    w = rnd((8, Cout, Cin), 801 + Cin, dtype, scale=Cin ** -0.5)
    b = rnd((Cout,), 802, torch.float32)
    y = torch.full((N, D2, 2 * H, 2 * W, Cout), float("nan"), dtype=dtype, device="cuda")
    ops.deconv_fwd(x, w, b, y, planar=planar)
    xr, wr = f64(x), f64(w)
    ref = _deconv_ref(xr, wr, f64(b), planar)
    torch.cuda.synchronize()
    assert_close(y, ref, *DECONV_TOL["fwd"][dtype], what="deconv fwd")
    dyfull = rnd((N, D2, 2 * H, 2 * W, Cout + extra), 803 + Cin, dtype)
    g = f64(dyfull)[..., off:off + Cout]
    if planar:
        gg = g.reshape(N, D, H, 2, W, 2, Cout).permute(0, 1, 2, 4, 3, 5, 6).reshape(N, D, H, W, 4, Cout)
    else:
        gg = g.reshape(N, D, 2, H, 2, W, 2, Cout).permute(0, 1, 3, 5, 2, 4, 6, 7).reshape(N, D, H, W, 8, Cout)
    rdx = torch.einsum("ndhwao,aoc->ndhwc", gg, wr[:nt])
    rdw = torch.einsum("ndhwao,ndhwc->aoc", gg, xr)
    rdb = g.sum(dim=(0, 1, 2, 3))
    tolx, tolw = DECONV_TOL["dx"][dtype], DECONV_TOL["dw"][dtype]
    xmask = rnd((N, D, H, W, Cin), 804, dtype)
    dx = torch.full_like(x, float("nan"))
    dw = torch.zeros((8, Cout, Cin), device="cuda")
    db = torch.zeros(Cout, device="cuda")
    ops.deconv_bwd(x, w, dyfull, dx, dw, db, dy_off=off, xmask=xmask, planar=planar)
    torch.cuda.synchronize()
    assert_close(dx, rdx * (f64(xmask) > 0), *tolx, what="deconv dx")
    assert_close(dw[:nt], rdw, *tolw, what="deconv dw")
    if planar:
        assert float(dw[nt:].abs().max()) == 0.0
    assert_close(db, rdb, *tolw, what="deconv db")
    # optional pieces: no mask, no input gradient, no weight gradient
    dx1 = torch.full_like(x, float("nan"))
    ops.deconv_bwd(x, w, dyfull, dx1, None, None, dy_off=off, planar=planar)
    dw2, db2 = torch.zeros_like(dw), torch.zeros_like(db)
    ops.deconv_bwd(x, w, dyfull, None, dw2, db2, dy_off=off, planar=planar)
    torch.cuda.synchronize()
    assert_close(dx1, rdx, *tolx, what="deconv dx")
    assert_close(dw2[:nt], rdw, *tolw, what="deconv dw")
    assert_close(db2, rdb, *tolw, what="deconv db")


# ------------------------------------------------------------------------------------------------ direct convolutions
DIRECT_CASES = [
    # planar, k, s, N, D, H, W, Cin, Cout
    (False, 3, 2, 2, 9, 10, 11, 64, 128),
    (False, 3, 2, 1, 4, 4, 6, 128, 256),        # 2 x 2 x 3 = 12 output voxels < 32 splits
    (False, 3, 2, 1, 3, 3, 3, 512, 64),         # 8 output voxels; 512 channels: two 256-wide blocks
    (False, 1, 1, 2, 5, 6, 7, 256, 128),
    (False, 1, 1, 1, 2, 3, 3, 512, 256),        # 18 voxels < 32 splits
    (True, 3, 2, 1, 3, 17, 16, 64, 32),
    (True, 3, 2, 1, 2, 5, 6, 256, 64),          # 2 x 3 x 3 = 18 output voxels
    (True, 1, 1, 1, 2, 9, 8, 512, 128),
    (True, 1, 1, 1, 4, 16, 16, 128, 32),
]


DIRECT_TOL = {
    "fwd": {torch.float32: (2e-6, 2e-6), torch.bfloat16: (5e-3, 1e-4)},         # 0.69 / 0.74
    "dx": {torch.float32: (1e-5, 1e-6), torch.bfloat16: (5e-3, 1e-4)},          # 0.55 / 0.75
    "dw": {torch.float32: (2.6e-6, 2.6e-7), torch.bfloat16: (2.7e-7, 2.7e-7)},  # 0.51 / 0.51 (dw and db)
}


def _same_pads(dims, k, s):
    """F.pad order (last axis first) of TensorFlow 'same' padding: (w_before, w_after, h_before, h_after, ...)"""
    pads = []
    for n in reversed(dims):
        tot = max((-(-n // s) - 1) * s + k - n, 0)
        pads += [tot // 2, tot - tot // 2]
    return pads


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", DIRECT_CASES, ids=lambda c: "%s_k%d_s%d_N%d_%dx%dx%d_%d_%d" % (("2d" if c[0] else "3d",) + c[1:]))
def test_conv_direct_at_model_sizes(ops, case, dtype):
    planar, k, s, N, D, H, W, Cin, Cout = case
    x = rnd((N, D, H, W, Cin), 900 + Cin, dtype)
    w = rnd((k ** 3, Cout, Cin), 901 + Cin, dtype, scale=(Cin * k * k) ** -0.5)
    b = rnd((Cout,), 902, torch.float32)
    od = ([D] if planar else [-(-D // s)]) + [-(-H // s), -(-W // s)]
    y = torch.full((N, *od, Cout), float("nan"), dtype=dtype, device="cuda")
    ops.conv_direct_fwd(x, w, b, y, k, s, act=0, planar=planar)
    xr = f64(x).requires_grad_(True)
    wr = f64(w).requires_grad_(True)
    if planar:
        c = k // 2
        wk = wr[c * k * k:(c + 1) * k * k].reshape(k, k, Cout, Cin).permute(2, 3, 0, 1)
        xin = F.pad(xr.reshape(N * D, H, W, Cin).permute(0, 3, 1, 2), _same_pads((H, W), k, s))
        yr = F.conv2d(xin, wk, f64(b), stride=s).permute(0, 2, 3, 1).reshape(N, *od, Cout)
    else:
        wk = wr.reshape(k, k, k, Cout, Cin).permute(3, 4, 0, 1, 2)
        yr = to_ndhwc(F.conv3d(F.pad(to_ncdhw(xr), _same_pads((D, H, W), k, s)), wk, f64(b), stride=s))
    torch.cuda.synchronize()
    assert_close(y, yr.detach(), *DIRECT_TOL["fwd"][dtype], what="direct fwd")
    dy = rnd(tuple(y.shape), 903 + Cin, dtype)
    yr.backward(f64(dy))
    tolx, tolw = DIRECT_TOL["dx"][dtype], DIRECT_TOL["dw"][dtype]
    dx = torch.full_like(x, float("nan"))
    dw = torch.zeros((k ** 3, Cout, Cin), device="cuda")
    db = torch.zeros(Cout, device="cuda")
    ops.conv_direct_bwd(x, w, dy, dx, dw, db, k, s, planar=planar)
    dx1 = torch.full_like(x, float("nan"))
    ops.conv_direct_bwd(x, w, dy, dx1, None, None, k, s, planar=planar)
    dw2, db2 = torch.zeros_like(dw), torch.zeros_like(db)
    ops.conv_direct_bwd(x, w, dy, None, dw2, db2, k, s, planar=planar)
    torch.cuda.synchronize()
    rdb = f64(dy).sum(dim=(0, 1, 2, 3))
    for gx, gw, gb in ((dx, dw, db), (dx1, None, None), (None, dw2, db2)):
        if gx is not None:
            assert_close(gx, xr.grad, *tolx, what="direct dx")
        if gw is not None:
            assert_close(gw, wr.grad, *tolw, what="direct dw")
            assert_close(gb, rdb, *tolw, what="direct db")
