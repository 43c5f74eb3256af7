"""Op tests of the grid-stride kernels at the sizes the models run and at their edges: pooling / up-sampling, the final 1x1x1 convolution,
sigmoid + Dice and the loss table, Adam, the element-wise helpers, the discriminator's helpers, the sliding-window tiles and the
deterministic mode at op level.  All of these kernels are a grid-stride loop behind grid_for(total, 256, cap): the toy sizes of
test_gpu_ops.py / test_gpu_losses.py / test_gpu_adversarial.py never make a thread add its stride to an index, never reach the tail of a
vector body, never give the last trip a partial wave.  Each family here has a case at or above the size of a 4 x 64x128x128 batch, a case
whose element count is no multiple of the launch's thread count nor of the vector width, and its edges.

References: fp64 restatements written here with plain torch tensor ops (on the device for the large cases - none of this project's
kernels and none of the engine's Python), oracle/metrics_oracle.py and oracle.unet_oracle.KerasAdam on the CPU where the size allows.
Bars follow the rule of test_gpu_ops.py: |got - ref| <= atol * max|ref| + rtol * |ref|, a NaN fails; each pair <= 2x the error measured
on MI355X with FMRI_MEASURE=1 (profiles/r06_tolerance_use_pointwise.json: per check, the fraction of its bar the worst element used),
exact (bit for bit) wherever the arithmetic is a copy, a maximum, one fp32 operation rounded once, or an integer count.
"""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gpu_util import assert_close, assert_same, dev_close, drnd, rnd

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
F32 = torch.float32
E_SHAPE, E_ALIGN, E_DTYPE = -1, -2, -5          # include/fmri_hip.h


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the GPU box"
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    from fmri_hip import ops as o
    from fmri_hip import _lib
    L = _lib.lib()
    assert (L.fmri_error_string(E_SHAPE), L.fmri_error_string(E_ALIGN), L.fmri_error_string(E_DTYPE)) == (
        b"unsupported shape", b"misaligned pointer", b"unsupported dtype")
    return o


def _lib():
    from fmri_hip import _lib as l
    return l.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _tn(dtype):
    return "f32" if dtype == F32 else "bf16"


# (rtol, atol) per check; comment: the largest fraction of the bar any element used on MI355X (FMRI_MEASURE=1)
TOL = {
    "conv1x1 fwd": (3.6e-7, 3.6e-7),         # 0.50 (fp32 FMA chains of C terms)
    "conv1x1 dx f32": (1.2e-7, 1.2e-7),      # 0.50
    "conv1x1 dx bf16": (8e-3, 1e-4),         # 0.47 (the bf16 rounding of the stored gradient)
    "conv1x1 dw": (3e-6, 3e-6),              # 0.47 (0.44 - 0.51 over seven runs; the scaled cases 1e3 / 1e-8 included: the fixed-point sums hold it)
    "conv1x1 db": (1e-6, 1e-6),              # 0.53 (0.25 - 0.53 over seven runs: fp32 atomics in arrival order on the LDS path)
    "probs": (9.8e-8, 9.8e-8),               # 0.50 (__expf and one division)
    # the Dice / loss sums are fp64 accumulations of fp32 terms: their relative error is the per-term error of __expf / __logf averaged
    # over the terms and does not grow with n (6.9e-8 is about one fp32 rounding)
    "sums": (6.9e-8, 0.0),                   # 0.50
    "loss value": (4.5e-7, 0.0),             # 0.50 (double dice, ratio 10: two Dice terms that partly cancel)
    "loss grad": (6.8e-6, 6.8e-7),           # 0.50
    # per-group sums of fp32 terms added in fp64, in an order that depends on the launch: any order of n positive terms is within
    # (longest chain of additions) x 2^-53 relative - 16 per thread + 6 + 2 in the workgroup + 256 atomics = 280 -> 3.2e-14 (measured 4.4e-16)
    "wdice gsums": (3.2e-14, 0.0),
    "wdice grad": (3.9e-7, 3.9e-8),          # 0.50
    # Adam: chains of <= 6 fp32 operations per element and step, three steps: within 18 roundings of 2^-24 = 1.1e-6 (asserted in the test)
    "adam p": (3.4e-7, 2.7e-9),              # 0.50 (the update's error, relative to max|p| where p itself is small)
    "adam m": (3.2e-7, 0.0),                 # 0.50
    "adam v": (6.3e-7, 0.0),                 # 0.50
    "sigmoid chain": (3.3e-7, 3.3e-8),       # 0.50
    "bce value": (1.6e-7, 0.0),              # 0.49
    "bce grad": (3.9e-7, 3.9e-8),            # 0.49
}


def _tol(name):
    return TOL[name] + (name,)


# ================================================================================================ 1. max-pool / up-sample
def _windows(x, planar):
    """[N,D,H,W,C] -> [N,Do,Ho,Wo,C,nt], the window's voxels in (d,h,w) scan order (the kernels' t = 4 dd + 2 hh + ww)"""
    N, D, H, W, C = x.shape
    if planar:
        return x.reshape(N, D, H // 2, 2, W // 2, 2, C).permute(0, 1, 2, 4, 6, 3, 5).reshape(N, D, H // 2, W // 2, C, 4)
    return x.reshape(N, D // 2, 2, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 7, 2, 4, 6).reshape(N, D // 2, H // 2, W // 2, C, 8)


def _unwindows(w, planar):
    N, Do, Ho, Wo, C, nt = w.shape
    if planar:
        return w.reshape(N, Do, Ho, Wo, C, 2, 2).permute(0, 1, 2, 5, 3, 6, 4).reshape(N, Do, 2 * Ho, 2 * Wo, C)
    return w.reshape(N, Do, Ho, Wo, C, 2, 2, 2).permute(0, 1, 5, 2, 6, 3, 7, 4).reshape(N, 2 * Do, 2 * Ho, 2 * Wo, C)


# N, D, H, W, C, planar, (add_ld, add_off) or None, relu_mask
POOL_CASES = [
    # enc0 of a 4 x 64x128x128 batch: 2,097,152 threads at width 8 against 1,048,576 launched - two full trips (N = 2 would be exactly one)
    ("enc0", 4, 64, 128, 128, 32, False, (32, 0), True),
    ("enc0_planar", 4, 32, 128, 128, 32, True, (64, 32), True),     # window 1x2x2: 2,097,152 threads as well
    ("enc0_halved", 4, 64, 128, 128, 32, False, (40, 4), True),     # add_off = 4: the launcher halves the width to 4 - 4 trips
    ("odd_c32", 3, 6, 10, 14, 32, False, (40, 4), False),
    ("odd_c12", 3, 6, 10, 14, 12, False, (12, 0), True),            # width 4; 3,780 threads: a partial last wave
    ("odd_c12_halved", 3, 6, 10, 14, 12, False, (18, 6), True),     # add_ld 18, add_off 6: width 4 -> 2
    ("odd_c6", 3, 6, 10, 14, 6, True, None, True),                  # width 2, no skip gradient
    ("odd_c5", 5, 2, 6, 22, 5, False, (7, 1), True),                # width 1
    ("odd_c5_nomask", 5, 3, 6, 22, 5, True, None, False),           # planar with an odd depth, neither skip gradient nor mask
]


def _with_dtypes(cases):
    """every case in bf16; in fp32 every case but the planar / halved-width repeats of the enc0 size (the fp32 instantiations run that size
    once, and their planar and halved-width forms at the odd shapes)"""
    both = [(c, d) for c in cases for d in (BF, F32) if d == BF or not c[0].startswith("enc0_")]
    return dict(argvalues=both, ids=["%s-%s" % (c[0], _tn(d)) for c, d in both])


@pytest.mark.parametrize("case,dtype", **_with_dtypes(POOL_CASES))
def test_maxpool_fwd_bwd_exact(ops, case, dtype):
    """forward: the window maximum, exact.  backward: the tie rule stated here - dy goes to the FIRST maximum of the window in (d,h,w) scan
    order, then the skip gradient is added (fp32, one rounding to the tensor's type), then the producer's ReLU mask zeroes what its input did
    not pass - exact as well.  The bf16 data holds windows that tie on a positive maximum (asserted), so the rule is exercised, not masked."""
    name, N, D, H, W, C, planar, add, relu = case
    x = drnd((N, D, H, W, C), 700, dtype)
    win = _windows(x, planar)
    m = win.amax(-1)
    y = torch.full(m.shape, float("nan"), dtype=dtype, device="cuda")
    ops.maxpool_fwd(x, y, planar=planar)
    assert_same(y, m, "maxpool fwd " + name)
    dy = drnd(tuple(m.shape), 701, dtype)
    a = None if add is None else drnd((N, D, H, W, add[0]), 702, dtype)
    dx = torch.full(x.shape, float("nan"), dtype=dtype, device="cuda")
    ops.maxpool_bwd(x, dy, dx, add=a, add_off=0 if add is None else add[1], relu_mask=relu, planar=planar)
    eq = win == m.unsqueeze(-1)
    if dtype == BF:
        ties = int(((eq.sum(-1) > 1) & (m > 0)).sum())
        assert ties > 0, "no window ties on a positive maximum: the tie rule is not exercised"
    first, taken = torch.zeros_like(eq), torch.zeros_like(m, dtype=torch.bool)
    for t in range(eq.shape[-1]):                     # the first maximum in scan order takes the gradient, later ties get none
        first[..., t] = eq[..., t] & ~taken
        taken |= eq[..., t]
    del eq, taken
    r = torch.where(first, dy.float().unsqueeze(-1), torch.zeros((), device="cuda"))
    del first
    if a is not None:
        r = r + _windows(a[..., add[1]:add[1] + C], planar).float()
    if relu:
        r = torch.where(win > 0, r, torch.zeros((), device="cuda"))
    assert_same(dx, _unwindows(r.to(dtype), planar), "maxpool bwd " + name)


def test_maxpool_tie_goes_to_the_first_maximum_only(ops):
    """all eight voxels of every window equal and positive: the whole gradient lands on voxel (0,0,0) of the window and nowhere else"""
    x = torch.full((2, 4, 6, 8, 8), 1.5, dtype=BF, device="cuda")
    dy = drnd((2, 2, 3, 4, 8), 705, BF)
    dx = torch.full(x.shape, float("nan"), dtype=BF, device="cuda")
    ops.maxpool_bwd(x, dy, dx, add=None, relu_mask=True)
    ref = torch.zeros_like(x)
    ref[:, ::2, ::2, ::2] = dy
    assert_same(dx, ref, "all-tie windows")


# N, D, H, W (low resolution), C, planar, ld, off, xmask
UP_CASES = [
    ("enc0", 4, 32, 64, 64, 32, False, 64, 32, True),        # into the second half of a 64-channel concat buffer: 2,097,152 threads, 2 trips
    ("enc0_planar", 4, 32, 64, 64, 32, True, 32, 0, True),
    ("enc0_halved", 2, 32, 64, 64, 32, False, 40, 4, False),  # offset 4: width 8 -> 4, 2,097,152 threads
    ("odd_c32_halved", 3, 3, 5, 7, 32, False, 44, 12, True),
    ("odd_c12", 3, 3, 5, 7, 12, False, 12, 0, True),
    ("odd_c12_halved", 3, 3, 5, 7, 12, True, 18, 2, False),   # width 4 -> 2
    ("odd_c6", 3, 3, 5, 7, 6, False, 9, 3, True),             # width 2 -> 1
    ("odd_c5", 5, 1, 3, 11, 5, True, 6, 1, False),
]
SENTINEL = -7.0


@pytest.mark.parametrize("case,dtype", **_with_dtypes(UP_CASES))
def test_upsample_fwd_bwd_exact(ops, case, dtype):
    """forward: every voxel copied to its 2x2x2 (planar: 1x2x2) children inside columns [off, off + C) of a wider destination, whose other
    columns keep a sentinel bit for bit.  backward: the children's fp32 sum in the kernel's scan order, masked by the producer's output,
    rounded once - exact."""
    name, N, D, H, W, C, planar, ld, off, use_mask = case
    x = drnd((N, D, H, W, C), 710, dtype)
    D2 = D if planar else 2 * D
    y = torch.full((N, D2, 2 * H, 2 * W, ld), SENTINEL, dtype=dtype, device="cuda")
    ops.upsample_fwd(x, y, y_off=off, planar=planar)
    ref = x.repeat_interleave(2, 2).repeat_interleave(2, 3)
    if not planar:
        ref = ref.repeat_interleave(2, 1)
    assert_same(y[..., off:off + C].contiguous(), ref, "upsample fwd " + name)
    rest = torch.cat([y[..., :off], y[..., off + C:]], -1)
    assert_same(rest, torch.full_like(rest, SENTINEL), "upsample fwd, columns outside the slice " + name)
    del y, ref, rest
    dy = drnd((N, D2, 2 * H, 2 * W, ld), 711, dtype)
    dx = torch.full(x.shape, float("nan"), dtype=dtype, device="cuda")
    ops.upsample_bwd(dy, dx, dy_off=off, xmask=x if use_mask else None, planar=planar)
    win = _windows(dy[..., off:off + C], planar).float()
    acc = torch.zeros(x.shape, device="cuda")
    for t in range(win.shape[-1]):
        acc = acc + win[..., t]
    if use_mask:
        acc = torch.where(x > 0, acc, torch.zeros((), device="cuda"))
    assert_same(dx, acc.to(dtype), "upsample bwd " + name)


def test_pool_and_upsample_refusals(ops):
    L, s = _lib(), _stream()
    x = torch.zeros((1, 2, 4, 4, 8), device="cuda")
    y = torch.zeros((1, 2, 4, 4, 8), device="cuda")
    p = x.data_ptr()
    w = (2, 2, 2)                                                                               # the fixed-window instantiations' entry
    assert L.fmri_maxpool3d_fwd(p, y.data_ptr(), 1, 2, 3, 4, 8, *w, 0, s) == E_SHAPE            # odd H
    assert L.fmri_maxpool3d_fwd(p, y.data_ptr(), 1, 3, 4, 4, 8, *w, 0, s) == E_SHAPE            # odd D, 3-D
    assert L.fmri_maxpool3d_fwd(p, y.data_ptr(), 1, 2, 4, 4, 8, *w, 7, s) == E_DTYPE
    assert L.fmri_maxpool3d_bwd(p, p, 0, 0, 0, y.data_ptr(), 1, 2, 4, 5, 8, *w, 1, 0, s) == E_SHAPE
    assert L.fmri_maxpool3d_bwd(p, p, 0, 0, 0, y.data_ptr(), 1, 2, 4, 4, 8, *w, 1, 7, s) == E_DTYPE
    assert L.fmri_upsample_nearest_fwd(p, y.data_ptr(), 8, 1, 1, 1, 2, 2, 8, *w, 0, s) == E_SHAPE  # ld < off + C
    assert L.fmri_upsample_nearest_fwd(p, y.data_ptr(), 8, 0, 1, 1, 2, 2, 8, *w, 7, s) == E_DTYPE
    assert L.fmri_upsample_nearest_bwd(p, 8, 1, 0, y.data_ptr(), 1, 1, 2, 2, 8, *w, 0, s) == E_SHAPE
    assert L.fmri_upsample_nearest_bwd(p, 8, 0, 0, y.data_ptr(), 1, 1, 2, 2, 8, *w, 7, s) == E_DTYPE
    torch.cuda.synchronize()
    assert not bool(y.any())


# ================================================================================================ 2. final 1x1x1 convolution
FULL = 4 * 64 * 128 * 128            # 4,194,304 voxels
HALF1 = 2 * 64 * 128 * 128 + 1       # 2,097,153: odd, so the last group of voxels-per-workgroup is ragged
# name, nvox, C, L, dtype, relu_mask, with dx, with db, with b, scale of dlogits
C11_CASES = [
    ("full_c64_l1", FULL, 64, 1, BF, True, True, True, True, 1.0),
    ("full_c32_l2", FULL, 32, 2, BF, True, True, True, True, 1.0),
    ("full_c64_l4_f32", FULL, 64, 4, F32, False, True, True, True, 1.0),
    # the workgroups' sums meet as 2^-40 fixed point in 64 bits (|s| < 2^23): near the top of that range and at the magnitude under Dice
    ("full_c64_large", FULL, 64, 1, BF, True, False, True, True, 1e3),       # 8,192 voxels per workgroup: |sum| ~ 1e5
    ("full_c64_tiny", FULL, 64, 1, BF, True, False, True, True, 1e-8),       # |sum| ~ 1e-6
    ("odd_c8_l4", HALF1, 8, 4, BF, True, True, False, False, 1.0),           # LPV 1
    ("odd_c16_l2", HALF1, 16, 2, F32, False, True, True, True, 1.0),         # LPV 2
    ("odd_c32_l1", HALF1, 32, 1, F32, True, None, True, True, 1.0),          # LPV 4, dx = None
    ("odd_c128_l1", HALF1, 128, 1, BF, True, True, True, False, 1.0),        # LPV 16
    ("odd_c6_l1_lds", HALF1, 6, 1, BF, True, True, True, True, 1.0),         # C % 8: the LDS kernels, width 2
    ("odd_c24_l2_lds", HALF1, 24, 2, F32, False, True, False, True, 1.0),    # C / 8 = 3 is no power of two
    ("odd_c32_l5_lds", HALF1, 32, 5, BF, True, True, True, False, 1.0),      # L > 4
]


@pytest.mark.parametrize("case", C11_CASES, ids=[c[0] for c in C11_CASES])
def test_conv1x1_fwd_bwd_vs_fp64(ops, case):
    """logits = x w^T + b, dx = dlogits w (masked by x > 0), dw = dlogits^T x, db = sum dlogits against fp64 matrix products on the device"""
    name, nvox, C, L, dtype, relu, with_dx, with_db, with_b, gscale = case
    x = drnd((nvox, C), 720, dtype)
    w = rnd((L, C), 721, F32, scale=0.2)
    b = rnd((L,), 722, F32) if with_b else None
    logits = torch.full((nvox, L), float("nan"), device="cuda")
    ops.conv1x1_fwd(x, w, b, logits)
    xd, wd = x.double(), w.double()
    ref = xd @ wd.t()
    if with_b:
        ref += b.double()
    dev_close(logits, ref, *_tol("conv1x1 fwd"))
    del ref, logits
    dl = drnd((nvox, L), 723, F32, scale=gscale)
    dx = torch.full((nvox, C), float("nan"), dtype=dtype, device="cuda") if with_dx else None
    dw = torch.zeros((L, C), device="cuda")
    db = torch.zeros(L, device="cuda") if with_db else None
    ops.conv1x1_bwd(x, w, dl, dx, dw, db, relu_mask=relu)
    dld = dl.double()
    dev_close(dw, dld.t() @ xd, *_tol("conv1x1 dw"))
    if with_db:
        dev_close(db, dld.sum(0), *_tol("conv1x1 db"))
    if with_dx:
        rdx = dld @ wd
        if relu:
            rdx = torch.where(x > 0, rdx, torch.zeros((), dtype=torch.float64, device="cuda"))
        dev_close(dx, rdx, *_tol("conv1x1 dx " + _tn(dtype)))


def test_conv1x1_refusals(ops):
    L, s = _lib(), _stream()
    t = torch.zeros(64, device="cuda")
    p = t.data_ptr()
    assert L.fmri_conv1x1_fwd(p, p, p, p, 0, 8, 1, 0, s) == E_SHAPE
    assert L.fmri_conv1x1_fwd(p, p, p, p, 4, 8, 1, 7, s) == E_DTYPE
    assert L.fmri_conv1x1_fwd(p, p, p, p, 4, 6, 1, 7, s) == E_DTYPE
    assert L.fmri_conv1x1_bwd(p, p, p, p, p, p, 4, 0, 1, 1, 0, s) == E_SHAPE
    assert L.fmri_conv1x1_bwd(p, p, p, p, p, p, 4, 8, 1, 1, 7, s) == E_DTYPE
    assert L.fmri_conv1x1_bwd(p, p, p, p, p, p, 4, 6, 1, 1, 7, s) == E_DTYPE
    torch.cuda.synchronize()
    assert not bool(t.any())


# ================================================================================================ 3. sigmoid + Dice, the loss table
N_DICE = FULL                       # 4,194,304 logits: 1,048,576 float4 items against 131,072 launched threads - 8 trips
SEED_Z = 503                        # rnd(..., scale=2.0) of this seed holds no |z| < 1e-6 (asserted): the thresholded sums are equalities
CLIP_LO, CLIP_HI = float(np.float32(1e-7)), float(np.float32(1.0) - np.float32(1e-7))      # Keras evaluates its clip in fp32
KINDS = [("dice_coefficient_loss", 0, 1.0), ("binary_crossentropy_loss", 1, 1.0), ("dice_and_xent", 2, 0.7), ("focal_loss", 3, 1.0),
         ("vod_coefficient_loss", 4, 1.0), ("double_dice_loss", 5, 10.0)]


def _labels(n, frac, seed=121):
    if frac in (0.0, 1.0):
        return torch.full((n,), int(frac), dtype=torch.uint8, device="cuda")
    return (torch.rand(n, generator=torch.Generator().manual_seed(seed)) < frac).to(torch.uint8).cuda()


def _ref_sums(z, y, w=None):
    """the 16 metric sums in fp64 from the LOGITS (float64, on the device): log p = logsigmoid(z), log(1 - p) = logsigmoid(-z)"""
    t = y.double()
    p = torch.sigmoid(z)
    lp, lq = F.logsigmoid(z), F.logsigmoid(-z)
    # Keras' clip of p to [1e-7, 1 - 1e-7] (evaluated in fp32), applied to the logarithms
    lpc = lp.clamp(math.log(CLIP_LO), math.log(CLIP_HI))
    lqc = lq.clamp(math.log1p(-CLIP_HI), math.log1p(-CLIP_LO))
    xent = -(t * lpc + (1 - t) * lqc)
    if w is not None:
        xent = w.double() * xent
    q = torch.sigmoid(-z)
    focal = -(0.5 * q * q * lp * t + 0.5 * p * p * lq * (1 - t))
    tb, pb = (t > 0.5).double(), (p > 0.5).double()
    s = torch.zeros(16, dtype=torch.float64)
    for k, v in enumerate(((t * p).sum(), t.sum(), p.sum(), (tb * pb).sum(), tb.sum(), pb.sum(), (torch.round(p) == t).double().sum(),
                           float(z.numel()), xent.sum(), focal.sum())):
        s[k] = float(v)
    return s


def _check_sums(got, ref, near_half, what):
    """[1], [4], [7] are integer counts: exact.  [3], [5], [6] threshold p at 0.5, where fp32 p and fp64 p may fall on different sides only for
    |z| < 1e-6: at most `near_half` (counted by the caller in its own input) disagreements.  The rest to the relative bar."""
    got = got.cpu()
    for k in (1, 4, 7):
        assert float(got[k]) == float(ref[k]), (what, k, float(got[k]), float(ref[k]))
    for k in (3, 5, 6):
        assert abs(float(got[k]) - float(ref[k])) <= near_half, (what, k, float(got[k]), float(ref[k]), near_half)
    for k in (0, 2, 8, 9):
        if float(ref[k]) == 0.0:
            assert float(got[k]) == 0.0, (what, k, float(got[k]))
        else:
            assert_close(got[k:k + 1], ref[k:k + 1], TOL["sums"][0], TOL["sums"][1], "sums")
    assert not bool(got[10:].any())


def _ref_loss(z, y, kind, param, w=None, smooth=1.0):
    """the loss table of reference fetal_net/metrics.py in fp64 on the logits (a scalar with a graph: autograd gives d/dlogits)"""
    t = y.double()
    p = torch.sigmoid(z)
    dice = lambda a, b: (2 * (a * b).sum() + smooth) / (a.sum() + b.sum() + smooth)
    if kind in (1, 2):
        # clip_by_value passes no gradient where it is active: the clamp of the logarithms has the same values and the same gradient
        lpc = F.logsigmoid(z).clamp(math.log(CLIP_LO), math.log(CLIP_HI))
        lqc = F.logsigmoid(-z).clamp(math.log1p(-CLIP_HI), math.log1p(-CLIP_LO))
        xe = -(t * lpc + (1 - t) * lqc)
        xent = (xe if w is None else w.double() * xe).mean()
    if kind == 0:
        return -dice(t, p)
    if kind == 1:
        return xent
    if kind == 2:
        return -dice(t, p) + param * xent
    if kind == 3:
        q = torch.sigmoid(-z)
        return -(0.5 * q * q * F.logsigmoid(z) * t).sum() - (0.5 * p * p * F.logsigmoid(-z) * (1 - t)).sum()
    if kind == 4:
        return -((t * p).sum() + smooth) / (t.sum() + p.sum() - (t * p).sum() + smooth)
    return -dice(t, p) + param * dice(1 - t, p)


def _oracle_value(name, yn, pn, param, wn=None):
    from oracle import metrics_oracle as M
    if name == "binary_crossentropy_loss":
        return M.weighted_cross_entropy_loss(yn, pn, wn)
    if name == "dice_and_xent":
        return M.dice_and_xent(yn, pn, param, wn)
    if name == "double_dice_loss":
        return M.double_dice_loss(yn, pn, param)
    return getattr(M, name)(yn, pn)


@pytest.fixture(scope="module")
def z_full():
    z = rnd((N_DICE,), SEED_Z, F32, scale=2.0)
    assert int((z.abs() < 1e-6).sum()) == 0
    return z


@pytest.mark.parametrize("frac", [0.0, 1e-4, 0.3, 1.0])
def test_sigmoid_dice_sums_at_full_size(ops, z_full, frac):
    """all ten sums of k_sigmoid_dice_fwd<4> at 4 x 64x128x128 against fp64 of the same formulas, for label fractions from none to all;
    sums[7] == n exactly; the loss values from the sums against oracle/metrics_oracle.py; probs = None gives the same sums"""
    y = _labels(N_DICE, frac)
    probs = torch.full_like(z_full, float("nan"))
    sums = torch.zeros(16, dtype=torch.float64, device="cuda")
    ops.sigmoid_dice_fwd(z_full, y, probs, sums)
    zd = z_full.double()
    ref = _ref_sums(zd, y)
    _check_sums(sums, ref, 0, "frac %g" % frac)
    assert float(sums[7]) == N_DICE
    dev_close(probs, torch.sigmoid(zd), *_tol("probs"))
    sums2 = torch.zeros(16, dtype=torch.float64, device="cuda")
    ops.sigmoid_dice_fwd(z_full, y, None, sums2)
    _check_sums(sums2, ref, 0, "probs = None, frac %g" % frac)
    yn, pn = y.cpu().numpy().astype(np.float64), torch.sigmoid(zd).cpu().numpy()
    for name, kind, param in KINDS:
        got = ops.loss_value_from_sums(sums.cpu().numpy(), kind, param)
        assert_close(torch.tensor([got]), torch.tensor([_oracle_value(name, yn, pn, param)]), TOL["loss value"][0], TOL["loss value"][1], "loss value")


@pytest.mark.parametrize("view", ["n_plus_1", "logits_4_bytes_off", "labels_1_byte_off", "probs_4_bytes_off"])
def test_sigmoid_dice_scalar_kernel_at_full_size(ops, z_full, view):
    """n % 4 != 0, or a view of logits / probs that starts 4 bytes off 16-byte alignment, or labels 1 byte off 4-byte alignment: the launcher
    must take the VEC = 1 kernel (the float4 kernel would fault or read shifted data) and the sums are those of the aligned run"""
    n = N_DICE + 1 if view == "n_plus_1" else N_DICE
    zb = torch.empty(n + 4, device="cuda")
    off = 1 if view == "logits_4_bytes_off" else 0
    z = zb[off:off + n]
    z[:N_DICE] = z_full
    z[N_DICE:] = 0.75
    yb = torch.zeros(n + 4, dtype=torch.uint8, device="cuda")
    off = 1 if view == "labels_1_byte_off" else 0
    y = yb[off:off + n]
    y[:] = _labels(n, 0.3)
    pb = torch.full((n + 4,), float("nan"), device="cuda")
    off = 1 if view == "probs_4_bytes_off" else 0
    probs = pb[off:off + n]
    assert z.is_contiguous() and y.is_contiguous() and probs.is_contiguous()
    assert {"n_plus_1": n % 4 == 1, "logits_4_bytes_off": z.data_ptr() % 16 == 4, "labels_1_byte_off": y.data_ptr() % 4 == 1,
            "probs_4_bytes_off": probs.data_ptr() % 16 == 4}[view]
    sums = torch.zeros(16, dtype=torch.float64, device="cuda")
    ops.sigmoid_dice_fwd(z, y, probs, sums)
    zd = z.double()
    _check_sums(sums, _ref_sums(zd, y), 0, view)
    dev_close(probs, torch.sigmoid(zd), *_tol("probs"))
    assert bool(torch.isnan(pb[:off]).all()) and bool(torch.isnan(pb[off + n:]).all())


def test_sigmoid_dice_planted_zero_logits_round_half_even(ops, z_full):
    """z = 0 gives p = 0.5 exactly: not above the threshold, and rintf(0.5) = 0 (Keras' round-half-even) - it counts as accurate for a
    background voxel only"""
    z = z_full[:1_000_003].clone()
    y = _labels(z.numel(), 0.3)
    at = torch.arange(0, z.numel(), 1009, device="cuda")
    z[at] = 0.0
    z[at[::3]] = -0.0
    probs = torch.empty_like(z)
    sums = torch.zeros(16, dtype=torch.float64, device="cuda")
    ops.sigmoid_dice_fwd(z, y, probs, sums)
    ref = _ref_sums(z.double(), y)
    _check_sums(sums, ref, 0, "planted zeros")
    assert bool((probs[at] == 0.5).all())
    planted_fg = int(y[at].sum())
    assert 0 < planted_fg < at.numel()
    t = y.double()
    elsewhere = torch.ones_like(t, dtype=torch.bool)
    elsewhere[at] = False
    acc_else = float(((torch.round(torch.sigmoid(z.double())) == t) & elsewhere).sum())
    assert float(sums[6]) == acc_else + (at.numel() - planted_fg)


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
def test_loss_gradients_at_full_size(ops, z_full, weighted):
    """k_sigmoid_dice_bwd and the six kinds of k_sigmoid_loss_bwd at 4 x 64x128x128 (+ 1 with the weight, so that the last trip is ragged),
    grad_scale != 1, against autograd of the fp64 formulas on the logits"""
    n = N_DICE + 1 if weighted else N_DICE
    z = torch.cat([z_full, z_full[:1]]) if weighted else z_full
    y = _labels(n, 0.3)
    w = torch.exp(-torch.rand(n, generator=torch.Generator().manual_seed(122)) * 3).cuda() if weighted else None
    probs = torch.empty_like(z)
    sums = torch.zeros(16, dtype=torch.float64, device="cuda")
    ops.sigmoid_dice_fwd(z, y, probs, sums, weight=w)
    _check_sums(sums, _ref_sums(z.double(), y, w), 0, "weighted" if weighted else "plain")
    gs = 0.5
    for name, kind, param in KINDS:
        if weighted and kind not in (1, 2):
            continue
        dl = torch.full_like(z, float("nan"))
        ops.sigmoid_loss_bwd(probs, y, sums, dl, kind, param, grad_scale=gs, weight=w)
        zd = z.double().requires_grad_(True)
        _ref_loss(zd, y, kind, param, w).backward()
        dev_close(dl, zd.grad * gs, *_tol("loss grad"))
        if kind == 0:
            dl2 = torch.full_like(z, float("nan"))
            ops.sigmoid_dice_bwd(probs, y, sums, dl2, grad_scale=gs)
            dev_close(dl2, zd.grad * gs, *_tol("loss grad"))
    if weighted:
        yn, pn, wn = y.cpu().numpy().astype(np.float64), torch.sigmoid(z.double()).cpu().numpy(), w.double().cpu().numpy()
        for name, kind, param in KINDS[1:3]:
            got = ops.loss_value_from_sums(sums.cpu().numpy(), kind, param)
            assert_close(torch.tensor([got]), torch.tensor([_oracle_value(name, yn, pn, param, wn)]), TOL["loss value"][0], TOL["loss value"][1],
                         "loss value")


SATURATED = (17.0, 30.0, 88.0, 100.0)


def _saturated_logits():
    """N(0, 2^2) with 4 x 2 x 2 x 40 = 640 voxels at +-17, +-30, +-88, +-100 on both label values: fp32 sigmoid is exactly 1.0f from 17 upward
    (and a subnormal at -88, 0 at -100)"""
    n = 262_144
    z = rnd((n,), 130, F32, scale=2.0)
    y = _labels(n, 0.3, seed=131)
    pos = 0
    for mag in SATURATED:
        for sign in (1.0, -1.0):
            for label in (0, 1):
                at = torch.arange(pos, n, n // 40, device="cuda")[:40]
                z[at] = sign * mag
                y[at] = label
                pos += 13
    return z, y


@pytest.mark.parametrize("name,kind,param", KINDS, ids=[k[0] for k in KINDS])
def test_losses_at_saturated_logits(ops, name, kind, param):
    """value and gradient of every loss stay finite at confident logits and agree with the fp64 formula evaluated on the LOGITS.  Focal loss
    (kind 3) was NaN here before this test: with p = 1.0f and t = 0 the backward pass multiplied dL/dp = -inf by p (1 - p) = 0, and the forward
    pass added -0.5 p^2 log(0) = +inf (on MI355X, before the fix: sums[9] = inf and 200 non-finite values in dlogits - the 160 background
    voxels with p = 1.0f and the 40 foreground voxels with p = 0).  The cross-entropy kinds pass no gradient where Keras' clip is active."""
    z, y = _saturated_logits()
    probs = torch.empty_like(z)
    sums = torch.zeros(16, dtype=torch.float64, device="cuda")
    ops.sigmoid_dice_fwd(z, y, probs, sums)
    assert int((probs == 1.0).sum()) >= 160 and int((probs == 0.0).sum()) >= 40
    dl = torch.full_like(z, float("nan"))
    ops.sigmoid_loss_bwd(probs, y, sums, dl, kind, param)
    torch.cuda.synchronize()
    print("saturated %s: sums[8] %r sums[9] %r, non-finite dlogits %d" % (name, float(sums[8]), float(sums[9]), int((~torch.isfinite(dl)).sum())))
    assert bool(torch.isfinite(sums).all()) and bool(torch.isfinite(dl).all())
    _check_sums(sums, _ref_sums(z.double(), y), int((z.abs() < 1e-6).sum()), "saturated")
    zd = z.double().requires_grad_(True)
    L = _ref_loss(zd, y, kind, param)
    L.backward()
    assert_close(torch.tensor([ops.loss_value_from_sums(sums.cpu().numpy(), kind, param)]), L.detach().cpu().reshape(1),
                 TOL["loss value"][0], TOL["loss value"][1], "loss value")
    dev_close(dl, zd.grad, *_tol("loss grad"))
    if kind == 3:
        # the exact gradient at a confidently wrong voxel tends to -+1/2: it is not small
        wrong = ((z >= 17) & (y == 0)) | ((z <= -17) & (y == 1))
        assert int(wrong.sum()) == 320 and float(dl[wrong].abs().min()) > 0.49


@pytest.mark.parametrize("L", [1, 3])
def test_weighted_dice_at_full_size(ops, L):
    """fmri_weighted_dice_fwd / _bwd with 4 samples of 1,048,577 voxels (the 256-workgroup cap of the sums binds from 1,048,576; odd, so the
    last trip is ragged), one group without any label voxel, against fp64 per-group sums and autograd of -mean_g dice_g on the probabilities"""
    nsamples, vox = 4, 1_048_577
    n = nsamples * vox * L
    probs = torch.sigmoid(rnd((n,), 140 + L, F32, scale=2.0))
    y = _labels(n, 0.3, seed=141).reshape(nsamples, vox, L)
    y[2, :, L - 1] = 0
    y = y.reshape(-1).contiguous()
    gsums = torch.full((nsamples * L, 3), float("nan"), dtype=torch.float64, device="cuda")
    sums = torch.zeros(16, dtype=torch.float64, device="cuda")
    ops.weighted_dice_fwd(probs, y, gsums, sums, nsamples, L)
    pd = probs.double().requires_grad_(True)
    p3, t3 = pd.reshape(nsamples, vox, L), y.double().reshape(nsamples, vox, L)
    I, Sy, Sp = (p3 * t3).sum(1), t3.sum(1), p3.sum(1)
    ref_g = torch.stack([I, Sy, Sp], -1).reshape(-1, 3).detach()
    assert float(ref_g[2 * L + L - 1, 1]) == 0.0
    assert_same(gsums[:, 1].contiguous(), ref_g[:, 1].contiguous(), "weighted dice label counts")
    dev_close(gsums[:, 0], ref_g[:, 0], *_tol("wdice gsums"))
    dev_close(gsums[:, 2], ref_g[:, 2], *_tol("wdice gsums"))
    smooth = 1e-5
    dice = (2 * I + smooth) / (Sy + Sp + smooth)
    assert float(sums[11]) == nsamples * L
    assert_close(sums[10:11], dice.sum().detach().reshape(1), TOL["wdice gsums"][0], 0.0, "wdice gsums")
    from oracle import metrics_oracle as M
    ref_val = M.weighted_dice_coefficient_loss(t3.permute(0, 2, 1).reshape(nsamples, L, 1, 1, vox).cpu().numpy(),
                                               p3.detach().permute(0, 2, 1).reshape(nsamples, L, 1, 1, vox).cpu().numpy())
    assert_close(torch.tensor([ops.loss_value_from_sums(sums.cpu().numpy(), ops.LOSS_WEIGHTED_DICE)]), torch.tensor([ref_val]),
                 TOL["loss value"][0], 0.0, "loss value")
    dl = torch.full_like(probs, float("nan"))
    ops.weighted_dice_bwd(probs, y, gsums, sums, dl, nsamples, L, grad_scale=2.0)
    (-dice.mean()).backward()
    dev_close(dl, 2.0 * pd.grad * (pd * (1 - pd)).detach(), *_tol("wdice grad"))


def test_loss_refusals(ops):
    L, s = _lib(), _stream()
    t = torch.zeros(64, dtype=torch.float64, device="cuda")
    p = t.data_ptr()
    assert L.fmri_sigmoid_dice_fwd(p, p, p, p, 0, s) == E_SHAPE
    assert L.fmri_sigmoid_dice_fwd_weighted(p, p, 0, p, p, 8, s) == E_SHAPE
    assert L.fmri_sigmoid_dice_bwd(p, p, p, p, 0, 1.0, 1.0, s) == E_SHAPE
    assert L.fmri_sigmoid_loss_bwd(p, p, p, p, 8, 6, 1.0, 1.0, 1.0, s) == E_SHAPE
    assert L.fmri_sigmoid_loss_bwd(p, p, p, p, 0, 0, 1.0, 1.0, 1.0, s) == E_SHAPE
    assert L.fmri_sigmoid_loss_bwd_weighted(p, p, p, p, p, 8, 3, 1.0, 1.0, 1.0, s) == E_SHAPE
    assert L.fmri_weighted_dice_fwd(p, p, p, p, 0, 8, 1, 1e-5, s) == E_SHAPE
    assert L.fmri_weighted_dice_bwd(p, p, p, p, p, 1, 0, 1, 1e-5, 1.0, s) == E_SHAPE
    torch.cuda.synchronize()
    assert not bool(t.any())


# ================================================================================================ 4. Adam
def _adam_grads(n, step):
    """sign fixed per element (no cancellation in m: the comparison is relative, element by element), |g| log-uniform in [1e-12, 1e3] - on
    both sides of eps = 1e-7 for sqrt(v) - and redrawn every step; one stretch that is exactly 0 in every step"""
    g = torch.Generator(device="cuda")
    sign = torch.where(torch.rand(n, generator=g.manual_seed(150), device="cuda") < 0.5, -1.0, 1.0)
    mag = torch.pow(10.0, torch.rand(n, generator=g.manual_seed(151 + step), device="cuda") * 15 - 12)
    out = (sign * mag).float()
    out[2_096_000:2_097_000] = 0.0
    out[n - 2] = 0.0                        # n = 16,000,003: one element of the scalar tail
    return out


@pytest.mark.parametrize("n", [16_000_003, 2_097_153])
def test_adam_three_steps_vs_keras_adam(ops, n):
    """three fmri_adam_step calls on one vector of the size of the whole parameter buffer (float4 body of 4,000,000 items over 524,288
    threads + a scalar tail of 3) and of 2,097,152 + 1 elements (tail of 1) against oracle.unet_oracle.KerasAdam in fp64: p, m and v.
    Where every gradient was exactly 0, m and v stay 0 and p does not move - bit for bit.
    p, m and v are chains of <= 6 fp32 operations per element and step, so three steps stay within ~18 roundings of 2^-24 = 1.1e-6."""
    from oracle.unet_oracle import KerasAdam
    # the C ABI takes the hyper-parameters as floats: the reference gets the values the kernel is given (1 - 0.999f differs from 0.001 by
    # 1.3e-5, which is Keras' own fp32 arithmetic and not an error of the kernel)
    lr, gs = 1e-3, 0.5
    b1, b2, eps = float(np.float32(0.9)), float(np.float32(0.999)), float(np.float32(1e-7))
    p = drnd((n,), 152, F32, scale=0.1)
    p0 = p.clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    W = {"w": p0.cpu().numpy().astype(np.float64)}
    ref = KerasAdam(W, lr, b1, b2, eps)
    zero = torch.ones(n, dtype=torch.bool, device="cuda")
    for step in range(3):
        g = _adam_grads(n, step)
        zero &= g == 0
        t = step + 1
        ops.adam_step(p, g, m, v, lr * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t), b1, b2, eps, grad_scale=gs)
        ref.step(W, {"w": g.cpu().numpy().astype(np.float64) * gs})
    nz = int(zero.sum())
    assert nz == 1001
    assert_same(p[zero], p0[zero], "adam p where g = 0")
    assert not bool(m[zero].any()) and not bool(v[zero].any())
    for what, got, want in (("adam p", p, W["w"]), ("adam m", m, ref.m["w"]), ("adam v", v, ref.v["w"])):
        assert TOL[what][0] <= 1.1e-6
        dev_close(got, torch.from_numpy(want).cuda(), *_tol(what))


def test_adam_refuses_a_misaligned_view(ops):
    """a view that starts 4 bytes off 16-byte alignment: FMRI_E_ALIGN (the float4 body would fault), p, m, v untouched"""
    from fmri_hip._lib import FmriError
    n = 1003
    bufs = [drnd((n + 1,), 160 + i, F32) for i in range(4)]
    before = [b.clone() for b in bufs]
    for k in range(4):
        args = [b[1:] if i == k else b[:n] for i, b in enumerate(bufs)]
        assert args[k].data_ptr() % 16 == 4 and args[k].is_contiguous()
        with pytest.raises(FmriError, match="misaligned pointer"):
            ops.adam_step(args[0], args[1], args[2], args[3], 1e-3)
    torch.cuda.synchronize()
    for b, b0 in zip(bufs, before):
        assert_same(b, b0, "adam buffers after a refused call")
    t = bufs[0]
    assert _lib().fmri_adam_step(t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), 0, 1e-3, 0.9, 0.999, 1e-7, 1.0, _stream()) == E_SHAPE


# ================================================================================================ 5. element-wise helpers
N_ELT = 3_000_001                   # 4,096 x 256 = 1,048,576 launched threads: three trips, the last one ragged


@pytest.mark.parametrize("dtype", [BF, F32], ids=_tn)
def test_add_channel_scale_slice_act_bwd_exact(ops, dtype):
    """one fp32 operation on the widened inputs, rounded once to the tensor's type: exact against the same statement in torch"""
    from fmri_hip._lib import ACT_LEAKY, ACT_NONE, ACT_RELU
    zero = torch.zeros((), device="cuda")
    a, b = drnd((N_ELT,), 800, dtype), drnd((N_ELT,), 801, dtype)
    y = torch.full_like(a, float("nan"))
    ops.add(a, b, y)
    assert_same(y, (a.float() + b.float()).to(dtype), "add")
    # channel_scale: N = 3 samples of V x C = 142,859 x 7 elements - the sample index changes inside every thread's stride
    N, V, C = 3, 142_859, 7
    x = drnd((N, V, C), 802, dtype)
    sc = (torch.rand(N, C, generator=torch.Generator().manual_seed(803)) > 0.3).float().cuda() / 0.7
    assert 0 < int((sc == 0).sum()) < N * C
    y = torch.full_like(x, float("nan"))
    ops.channel_scale(x, sc, y)
    assert_same(y, (x.float() * sc[:, None, :]).to(dtype), "channel_scale")
    # slice_channels: columns [5, 13) of 24, into and onto an 8-channel destination
    nvox, ld, off, Cs = 400_003, 24, 5, 8
    src = drnd((nvox, ld), 804, dtype)
    dst0 = drnd((nvox, Cs), 805, dtype)
    dst = dst0.clone()
    ops.slice_channels(src, off, dst, accumulate=False)
    assert_same(dst, src[:, off:off + Cs].contiguous(), "slice_channels")
    dst = dst0.clone()
    ops.slice_channels(src, off, dst, accumulate=True)
    assert_same(dst, (src[:, off:off + Cs].float() + dst0.float()).to(dtype), "slice_channels accumulate")
    # act_bwd: zeros and negative zeros in the stored output take the <= 0 branch; alpha = 0.25 keeps the products exact in bf16
    yv, dy = drnd((N_ELT,), 806, dtype), drnd((N_ELT,), 807, dtype)
    yv[::7] = 0.0
    yv[3::11] = -0.0
    for act, alpha, ref in ((ACT_RELU, 0.0, torch.where(yv > 0, dy.float(), zero)), (ACT_LEAKY, 0.25, torch.where(yv > 0, dy.float(), 0.25 * dy.float())),
                            (ACT_NONE, 0.0, dy.float())):
        dx = torch.full_like(dy, float("nan"))
        ops.act_bwd(yv, dy, dx, act, alpha)
        assert_same(dx, ref.to(dtype), "act_bwd %d" % act)


def _special_f32(n):
    """normal data, then fp32 bit patterns that sit on the edges of the bf16 rounding: ties to even (down and up), just above a tie, the
    largest finite values, +-inf, +-0 and subnormals (ties among them)"""
    x = drnd((n,), 810, F32)
    pats = [0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0x7F7FFFFF, 0x7F7F7FFF, 0x7F800000, 0x00000000, 0x00000001, 0x00008000, 0x00018000,
            0x00008001, 0x007FFFFF, 0x00800000]
    pats = pats + [p | 0x80000000 for p in pats]
    bits = torch.tensor([p - (1 << 32) if p >= (1 << 31) else p for p in pats], dtype=torch.int32, device="cuda")
    x[-len(pats):] = bits.view(F32)
    x[:len(pats)] = bits.view(F32)
    return x


def _bf16_rne(x):
    """fp32 -> bf16, round to nearest even, on the bits (no NaN in the input)"""
    b = x.view(torch.int32).long() & 0xFFFFFFFF
    r = (b + 0x7FFF + ((b >> 16) & 1)) >> 16
    r = torch.where(r >= 0x8000, r - 0x10000, r).to(torch.int16)
    return r.view(BF)


def test_cast_all_type_pairs_exact(ops):
    x = _special_f32(N_ELT)
    h = torch.full((N_ELT,), float("nan"), dtype=BF, device="cuda")
    ops.cast(x, h)
    want = _bf16_rne(x)
    assert_same(h, want, "cast f32 -> bf16")
    assert int(torch.isinf(h).sum()) >= 4
    back = torch.full((N_ELT,), float("nan"), device="cuda")
    ops.cast(h, back)
    assert_same(back, (want.view(torch.int16).int() << 16).view(F32), "cast bf16 -> f32")
    x2 = torch.full_like(x, float("nan"))
    ops.cast(x, x2)
    assert_same(x2, x, "cast f32 -> f32")
    h2 = torch.full_like(h, float("nan"))
    ops.cast(h, h2)
    assert_same(h2, h, "cast bf16 -> bf16")


def test_elementwise_refusals(ops):
    L, s = _lib(), _stream()
    t = torch.zeros(64, device="cuda")
    p = t.data_ptr()
    assert L.fmri_add(p, p, p, 0, 0, s) == E_SHAPE
    assert L.fmri_add(p, p, p, 8, 7, s) == E_DTYPE
    assert L.fmri_channel_scale(p, p, p, 0, 4, 2, 0, s) == E_SHAPE
    assert L.fmri_channel_scale(p, p, p, 1, 0, 2, 0, s) == E_SHAPE
    assert L.fmri_channel_scale(p, p, p, 1, 4, 2, 7, s) == E_DTYPE
    assert L.fmri_slice_channels(p, 8, 5, p, 4, 2, 0, 0, s) == E_SHAPE        # ld < off + C
    assert L.fmri_slice_channels(p, 8, 0, p, 4, 0, 0, 0, s) == E_SHAPE
    assert L.fmri_slice_channels(p, 8, 0, p, 4, 2, 0, 7, s) == E_DTYPE
    assert L.fmri_act_bwd(p, p, p, 1, 0.0, 0, 0, s) == E_SHAPE
    assert L.fmri_act_bwd(p, p, p, 1, 0.0, 8, 7, s) == E_DTYPE
    assert L.fmri_cast(p, 0, p, 1, 0, s) == E_SHAPE
    assert L.fmri_cast(p, 0, p, 7, 8, s) == E_DTYPE
    assert L.fmri_cast(p, 7, p, 0, 8, s) == E_DTYPE
    torch.cuda.synchronize()
    assert not bool(t.any())


# ================================================================================================ 6. discriminator helpers
# N, D, H, W, C, planar, dtype
AVG_CASES = [
    ("full", 4, 64, 128, 128, 32, False, BF),             # forward 2,097,152 threads at width 8 (two trips), backward 16,777,216
    ("full_planar", 4, 32, 128, 128, 32, True, BF),
    ("full_f32", 4, 64, 128, 128, 32, False, F32),
    ("odd_c12", 2, 9, 11, 15, 12, False, F32),            # odd extents: the trailing planes are not read and get a zero gradient
    ("odd_c12_planar", 2, 9, 11, 15, 12, True, BF),
    ("odd_c6", 3, 5, 10, 7, 6, False, BF),
    ("odd_c5", 3, 4, 7, 10, 5, True, F32),
]


@pytest.mark.parametrize("case", AVG_CASES, ids=[c[0] for c in AVG_CASES])
def test_avgpool_fwd_bwd_exact(ops, case):
    """forward: the window's fp32 sum in scan order times 1/8 (1/4), rounded once; backward: dy / 8 (a power of two) to every voxel of the
    window, 0 in an odd trailing plane - exact"""
    name, N, D, H, W, C, planar, dtype = case
    Do, Ho, Wo = (D if planar else D // 2), H // 2, W // 2
    x = drnd((N, D, H, W, C), 820, dtype)
    y = torch.full((N, Do, Ho, Wo, C), float("nan"), dtype=dtype, device="cuda")
    ops.avgpool_fwd(x, y, planar=planar)
    win = _windows(x[:, :D if planar else 2 * Do, :2 * Ho, :2 * Wo].contiguous(), planar).float()
    acc = torch.zeros(y.shape, device="cuda")
    for t in range(win.shape[-1]):
        acc = acc + win[..., t]
    inv = 1.0 / win.shape[-1]
    assert_same(y, (acc * inv).to(dtype), "avgpool fwd " + name)
    del win, acc
    dy = drnd(tuple(y.shape), 821, dtype)
    dx = torch.full(x.shape, float("nan"), dtype=dtype, device="cuda")
    ops.avgpool_bwd(dy, dx, planar=planar)
    g = (dy.float() * inv).to(dtype).repeat_interleave(2, 2).repeat_interleave(2, 3)
    if not planar:
        g = g.repeat_interleave(2, 1)
    ref = torch.zeros_like(dx)
    ref[:, :g.shape[1], :g.shape[2], :g.shape[3]] = g
    assert_same(dx, ref, "avgpool bwd " + name)


@pytest.mark.parametrize("N,V,C,dtype", [(2, 262_145, 32, BF), (2, 262_145, 32, F32), (3, 100_003, 12, BF), (3, 100_003, 5, F32)])
def test_global_avgpool_bwd_exact(ops, N, V, C, dtype):
    """dx[n][v][c] = dy[n][c] * (1 / V): one fp32 product, rounded once (2 x 262,145 x 32 / 8 = 2,097,160 threads: two trips and a ragged end)"""
    dy = drnd((N, C), 825, F32)
    dx = torch.full((N, V, C), float("nan"), dtype=dtype, device="cuda")
    ops.global_avgpool_bwd(dy, dx)
    inv = torch.ones((), device="cuda") / torch.tensor(float(V), device="cuda")
    assert inv.dtype == F32
    assert_same(dx, (dy * inv).to(dtype)[:, None, :].expand(N, V, C).contiguous(), "global_avgpool_bwd")


V_GAP = 32 * 64 * 128               # 262,144: a 64x128x128 patch after the discriminator's one (2,2,1) pooling - the largest its head averages


@pytest.mark.parametrize("V,dtype", [(V_GAP, F32), (V_GAP, BF), (64 * V_GAP, F32)], ids=["v262144-f32", "v262144-bf16", "v16777216-f32"])
def test_global_avgpool_fwd_long_fp32_chain(ops, V, dtype):
    """k_gap_fwd adds n = V / 4 values per lane one after the other in fp32.  With data of mean 8 the partial sums grow steadily, every add
    rounds by at most 2^-24 of the running sum, so |error| / |sum| <= n 2^-24 in the worst case; the roundings are independent and centred, so
    their sum is a random walk with sigma <= sqrt(n / 12) 2^-23 relative - the bar is 8 sigma (and never above the worst case), plus 4 roundings
    for the last three adds and the division.  Derived from the chain's length, not measured (the measured error is printed)."""
    C = 8
    x = drnd((1, V, C), 826, dtype, shift=8.0)
    y = torch.full((1, C), float("nan"), device="cuda")
    ops.global_avgpool_fwd(x, y)
    ref = x.double().mean(1)
    n = V // 4
    bound = min(n * 2.0 ** -24, 8 * math.sqrt(n / 12.0) * 2.0 ** -23) + 4 * 2.0 ** -24
    err = float(((y.double() - ref).abs() / ref.abs()).max())
    print("global_avgpool_fwd V = %d %s: relative error %.3e, bound %.3e" % (V, _tn(dtype), err, bound))
    assert err <= bound, (err, bound)


@pytest.mark.parametrize("nvox,L,ld,dtype", [(2_097_153, 1, 8, BF), (700_001, 3, 11, F32), (1_048_577, 2, 2, BF)])
@pytest.mark.parametrize("accumulate", [False, True], ids=["write", "accumulate"])
def test_sigmoid_chain_vs_fp64(ops, nvox, L, ld, dtype, accumulate):
    """dlogits (+)= scale * dprobs[:, :L] * p (1 - p), dprobs with a row pitch of ld >= L"""
    probs = torch.sigmoid(drnd((nvox, L), 830, F32, scale=2.0))
    dprobs = drnd((nvox, ld), 831, dtype)
    dl0 = drnd((nvox, L), 832, F32)
    dl = dl0.clone()
    ops.sigmoid_chain(probs, dprobs, dl, scale=0.3, accumulate=accumulate)
    pd = probs.double()
    ref = float(np.float32(0.3)) * dprobs[:, :L].double() * pd * (1 - pd)
    if accumulate:
        ref = ref + dl0.double()
    dev_close(dl, ref, *_tol("sigmoid chain"))


# nvox x ld >= 2,097,152 elements; L, C, ld, merge
DIS_IN_CASES = [(2, 3, 8, False), (1, 1, 8, False), (3, 1, 4, False), (1, 3, 8, True), (3, 1, 8, True), (2, 2, 8, True), (1, 1, 2, True)]


@pytest.mark.parametrize("x_dtype,out_dtype", [(F32, F32), (F32, BF), (BF, BF), (BF, F32)], ids=["f32-f32", "f32-bf16", "bf16-bf16", "bf16-f32"])
@pytest.mark.parametrize("L,C,ld,merge", DIS_IN_CASES, ids=["L%d_C%d_ld%d_%s" % (c[0], c[1], c[2], "merge" if c[3] else "concat") for c in DIS_IN_CASES])
def test_discriminator_input_exact(ops, L, C, ld, merge, x_dtype, out_dtype):
    """[probs, x, 0 ...] or the mul-merge maps [x * s, x * (1 - s), 0 ...] (numpy broadcast along the channel axis) over a NaN-filled
    destination: copies and single fp32 products rounded once - exact, the padding columns exactly zero"""
    nvox = 1_048_579 if ld == 2 else (524_291 if ld == 4 else 300_001)
    probs = torch.sigmoid(drnd((nvox, L), 835, F32, scale=2.0))
    x = drnd((nvox, C), 836, x_dtype)
    out = torch.full((nvox, ld), float("nan"), dtype=out_dtype, device="cuda")
    ops.discriminator_input(probs, x, out, merge=merge)
    xf = x.float()
    if merge:
        P = max(C, L)
        s_, x_ = probs.expand(nvox, P), xf.expand(nvox, P)
        parts = [x_ * s_, x_ * (1.0 - s_)]
    else:
        parts = [probs, xf]
    used = sum(p.shape[1] for p in parts)
    ref = torch.cat(parts + [torch.zeros((nvox, ld - used), device="cuda")], 1).to(out_dtype)
    assert_same(out, ref, "discriminator_input")
    assert not bool(out[:, used:].any())


def test_bce_at_saturated_logits(ops):
    """logits +-17, +-30, +-100 among ordinary ones, soft targets: the value is Keras' clipped formula (p clipped to [1e-7, 1 - 1e-7], evaluated
    in fp32 by Keras, hence the fp32 bounds), finite; the gradient is exactly 0 wherever the clip is active (tf.clip_by_value)"""
    n = 96
    z = rnd((n,), 840, F32)
    sat = torch.tensor([s * m for m in (17.0, 30.0, 100.0) for s in (1.0, -1.0)] * 4, device="cuda")
    z[:sat.numel()] = sat
    u = torch.rand(n, generator=torch.Generator().manual_seed(841)) * 0.1
    t = torch.where(torch.arange(n) % 4 < 2, 1.0 - u, u).float().cuda()
    probs = torch.full_like(z, float("nan"))
    sums = torch.zeros(4, dtype=torch.float64, device="cuda")
    ops.sigmoid_bce_fwd(z, t, probs, sums)
    p64, t64 = torch.sigmoid(z.double()), t.double()
    pc = p64.clamp(CLIP_LO, CLIP_HI)
    ref = -(t64 * torch.log(pc) + (1 - t64) * torch.log(1 - pc))
    assert bool(torch.isfinite(sums).all())
    assert_close(sums[0:1], ref.sum().reshape(1), *_tol("bce value"))
    assert_close(sums[1:2], (p64 - t64).abs().sum().reshape(1), *_tol("bce value"))
    assert float(sums[2]) == n
    dl = torch.full_like(z, float("nan"))
    ops.sigmoid_bce_bwd(probs, t, dl, 0.25)
    clipped = (p64 <= CLIP_LO) | (p64 >= CLIP_HI)
    assert int(clipped.sum()) == sat.numel()
    assert not bool(dl[clipped].any()), "gradient where the clip is active"
    dev_close(dl, torch.where(clipped, torch.zeros((), dtype=torch.float64, device="cuda"), 0.25 * (p64 - t64)), *_tol("bce grad"))


def test_discriminator_helper_refusals(ops):
    L, s = _lib(), _stream()
    t = torch.zeros(64, device="cuda")
    p = t.data_ptr()
    assert L.fmri_avgpool3d_2x_fwd(p, p, 1, 2, 1, 2, 4, 0, 0, s) == E_SHAPE
    assert L.fmri_avgpool3d_2x_fwd(p, p, 1, 2, 2, 2, 4, 7, 0, s) == E_DTYPE
    assert L.fmri_avgpool3d_2x_bwd(p, p, 1, 1, 2, 2, 4, 0, 0, s) == E_SHAPE          # 3-D with D = 1
    assert L.fmri_avgpool3d_2x_bwd(p, p, 1, 2, 2, 2, 4, 7, 0, s) == E_DTYPE
    assert L.fmri_global_avgpool_fwd(p, p, 1, 0, 4, 0, s) == E_SHAPE
    assert L.fmri_global_avgpool_fwd(p, p, 1, 2, 4, 7, s) == E_DTYPE
    assert L.fmri_global_avgpool_bwd(p, p, 0, 2, 4, 0, s) == E_SHAPE
    assert L.fmri_global_avgpool_bwd(p, p, 1, 2, 4, 7, s) == E_DTYPE
    assert L.fmri_sigmoid_chain(p, p, 1, 2, p, 4, 1.0, 0, 0, s) == E_SHAPE            # ld < n_labels
    assert L.fmri_sigmoid_chain(p, p, 2, 2, p, 4, 1.0, 0, 7, s) == E_DTYPE
    assert L.fmri_discriminator_input(p, 2, p, 3, 0, p, 4, 0, 4, 0, s) == E_SHAPE     # ld < L + C
    assert L.fmri_discriminator_input(p, 2, p, 3, 0, p, 8, 0, 4, 1, s) == E_SHAPE     # merge needs C = 1, L = 1 or C = L
    assert L.fmri_discriminator_input(p, 2, p, 3, 7, p, 8, 0, 4, 0, s) == E_DTYPE
    assert L.fmri_sigmoid_bce_fwd(p, p, p, p, 0, s) == E_SHAPE
    assert L.fmri_sigmoid_bce_bwd(p, p, p, 0, 1.0, s) == E_SHAPE
    torch.cuda.synchronize()
    assert not bool(t.any())


# ================================================================================================ 7. sliding-window tiles
VOL = (48, 40, 56)
PATCH = (32, 32, 48)                # 49,152 voxels per tile; 24 tiles = 1,179,648 elements against 1,048,576 launched threads


def _corners():
    """24 corners, outside the volume on every side in turn (negative, and with the tile's end past the volume's), x0 <= 8 so that the
    planes x >= 40 stay uncovered"""
    g = torch.Generator().manual_seed(850)
    idx = torch.stack([torch.randint(-20, 9, (24,), generator=g), torch.randint(-20, 31, (24,), generator=g), torch.randint(-30, 41, (24,), generator=g)], 1)
    idx[0] = torch.tensor([-20, -20, -30])
    idx[1] = torch.tensor([8, 30, 40])
    idx[2] = torch.tensor([0, 0, 0])
    idx[3] = torch.tensor([-5, 8, 8])
    idx[4] = torch.tensor([8, -7, 30])
    return idx.to(torch.int32)


@pytest.mark.parametrize("dtype", [F32, BF], ids=_tn)
def test_tile_gather_replicates_the_edge(ops, dtype):
    """corners outside the volume: the tile is the slice of np.pad(vol, mode="edge") - exact, one rounding for bf16 tiles"""
    vol = rnd(VOL, 851, F32)
    idx = _corners()
    tiles = torch.full((idx.shape[0],) + PATCH, float("nan"), dtype=dtype, device="cuda")
    ops.tile_gather(vol, idx.cuda(), PATCH, tiles)
    P = 64
    padded = np.pad(vol.cpu().numpy(), P, mode="edge")
    ref = np.stack([padded[P + x0:P + x0 + PATCH[0], P + y0:P + y0 + PATCH[1], P + z0:P + z0 + PATCH[2]] for x0, y0, z0 in idx.tolist()])
    assert_same(tiles.cpu(), torch.from_numpy(ref).to(dtype), "tile_gather")


@pytest.mark.parametrize("C", [1, 3])
def test_tile_scatter_and_finalize_exact(ops, C):
    """overlap-add of two batches of tiles whose corners lie outside the volume on every side: voxels outside are skipped, the sums (dyadic
    predictions: exact in any order of the atomics), the counts and the number of uncovered voxels are exact, out = acc / count bit for bit"""
    idx = _corners()
    B = idx.shape[0]
    g = torch.Generator().manual_seed(852 + C)
    acc = torch.zeros(VOL + (C,), dtype=torch.float64, device="cuda")
    cnt = torch.zeros(VOL, dtype=torch.int32, device="cuda")
    racc, rcnt = np.zeros(VOL + (C,)), np.zeros(VOL, dtype=np.int64)
    for batch in range(2):
        corners = idx if batch == 0 else idx.flip(0) + torch.tensor([0, 1, -1], dtype=torch.int32)
        pred = torch.randint(-8, 9, (B,) + PATCH + (C,), generator=g).float() / 8
        ops.tile_scatter_accumulate(pred.cuda(), corners.cuda(), PATCH, acc, cnt)
        pn = pred.numpy().astype(np.float64)
        for b, c0 in enumerate(corners.tolist()):
            lo = [max(0, c0[a]) for a in range(3)]
            hi = [min(VOL[a], c0[a] + PATCH[a]) for a in range(3)]
            if any(h <= l for l, h in zip(lo, hi)):
                continue
            dst = tuple(slice(l, h) for l, h in zip(lo, hi))
            src = tuple(slice(l - c, h - c) for l, h, c in zip(lo, hi, c0))
            racc[dst] += pn[b][src]
            rcnt[dst] += 1
    assert_same(cnt.cpu(), torch.from_numpy(rcnt).to(torch.int32), "tile counts")
    assert_same(acc.cpu(), torch.from_numpy(racc), "tile accumulator")
    out = torch.full(VOL + (C,), float("nan"), dtype=torch.float64, device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    ops.tile_finalize(acc, cnt, out, bad)
    uncovered = int((rcnt == 0).sum())
    assert uncovered >= 8 * VOL[1] * VOL[2] and int(bad) == uncovered
    assert_same(out.cpu(), torch.from_numpy(racc / np.maximum(rcnt, 1)[..., None]), "tile_finalize")


def test_tile_refusals(ops):
    L, s = _lib(), _stream()
    t = torch.zeros(64, device="cuda")
    p = t.data_ptr()
    assert L.fmri_tile_gather(p, 4, 4, 4, p, 0, 2, 2, 2, p, 0, s) == E_SHAPE
    assert L.fmri_tile_gather(p, 4, 4, 4, p, 1, 2, 2, 2, p, 7, s) == E_DTYPE
    assert L.fmri_tile_scatter_accumulate(p, p, 1, 2, 2, 2, 0, p, p, 4, 4, 4, s) == E_SHAPE
    assert L.fmri_tile_finalize(p, p, p, p, 0, 1, s) == E_SHAPE
    torch.cuda.synchronize()
    assert not bool(t.any())


# ================================================================================================ 8. deterministic mode at op level
def test_deterministic_mode_conv1x1_bwd_and_dice_sums(ops):
    """with fmri_set_deterministic on, the last layer's dw / db (a slice of the registered gradient buffer) and the metric sums are the same
    bits in two runs at full size, and agree with the default mode within its bar.  The switch is process-wide: off again in the finally."""
    C = 64
    x = drnd((FULL, C), 860, BF)
    w = rnd((1, C), 861, F32, scale=0.2)
    dl = drnd((FULL, 1), 862, F32, scale=1e-6)
    z = rnd((N_DICE,), SEED_Z, F32, scale=2.0)
    y = _labels(N_DICE, 0.3)
    grad = torch.zeros(4096, device="cuda")
    shadow = torch.zeros(4096, dtype=torch.int64, device="cuda")
    dw, db = grad[128:128 + C].view(1, C), grad[300:301]
    runs = []
    try:
        ops.set_deterministic(grad, shadow)
        for _ in range(2):
            grad.zero_()
            sums = torch.zeros(16, dtype=torch.float64, device="cuda")
            ops.conv1x1_bwd(x, w, dl, None, dw, db, relu_mask=True)
            ops.sigmoid_dice_fwd(z, y, None, sums)
            ops.deterministic_finish(grad, shadow)
            torch.cuda.synchronize()
            runs.append((grad.clone(), sums))
    finally:
        ops.set_deterministic(None, None)
    assert_same(runs[0][0], runs[1][0], "deterministic dw / db")
    assert_same(runs[0][1], runs[1][1], "deterministic sums")
    assert not bool(shadow.any())
    used = torch.zeros(4096, dtype=torch.bool, device="cuda")
    used[128:128 + C] = True
    used[300] = True
    assert not bool(runs[0][0][~used].any()) and bool(runs[0][0][used].all())
    dw2, db2 = torch.zeros((1, C), device="cuda"), torch.zeros(1, device="cuda")
    sums2 = torch.zeros(16, dtype=torch.float64, device="cuda")
    ops.conv1x1_bwd(x, w, dl, None, dw2, db2, relu_mask=True)
    ops.sigmoid_dice_fwd(z, y, None, sums2)
    dev_close(runs[0][0][128:128 + C].reshape(1, C), dw2, *_tol("conv1x1 dw"))
    dev_close(runs[0][0][300:301], db2, *_tol("conv1x1 db"))
    _check_sums(runs[0][1], sums2.cpu(), 0, "deterministic against default")
    _check_sums(runs[0][1], _ref_sums(z.double(), y), 0, "deterministic against fp64")
