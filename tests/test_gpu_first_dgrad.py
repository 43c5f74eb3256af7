"""fmri_conv3d_first_dgrad: the fp32 input gradient of the network's first convolution, at the smallest shapes where it can go wrong.

The kernel walks a 16 x 32 (h, w) column of a sample along d in chunks of planes (csrc/conv3d_first.hip): the cases cover one minimal tile
(every voxel a border voxel), two tiles per axis with two samples and two chunks along d (nothing may leak across tiles, chunks or
samples), interior tiles and an interior chunk, 64 output channels (a second 32-channel k-chunk) and every input-channel count.
Reference: the fp64 CPU convolution of dy with the tap-flipped, transposed filters - exact on dyadic data, where every product and every
partial sum fits fp32, so the kernel must give it bit for bit; on random bf16 data the bar follows the suite's rule (<= 2x the error
measured on MI355X with FMRI_MEASURE=1, profiles/r07_first_dgrad.log).
"""
import os

import pytest
import torch
import torch.nn.functional as F

from gpu_util import assert_close, assert_same, f64, rnd, to_ncdhw, to_ndhwc

pytestmark = pytest.mark.gpu

BF = torch.bfloat16

# (Cin, Cout, N, D, H, W)
CASES = [(1, 32, 1, 4, 16, 32), (1, 64, 2, 8, 32, 64), (1, 32, 1, 12, 48, 96), (2, 32, 1, 4, 16, 32), (3, 64, 1, 8, 16, 32), (4, 32, 2, 4, 32, 32)]
IDS = ["c%d_o%d_n%d_%dx%dx%d" % c for c in CASES]

# |got - ref| <= atol * max|ref| + rtol * |ref|: fp32 sums of exact bf16 products (27 * Cout terms), measured 0.52 of this bar at the worst case (c1_o64), 0.32-0.40 at the others
DGRAD_TOL = (2e-7, 2e-7)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the GPU box"
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    from fmri_hip import ops as o
    return o


def _dy4(g, shape, lo, hi, div):
    return torch.randint(lo, hi + 1, shape, generator=g).float() / div


def _ref(dy, w):
    """fp64: dx = conv(dy, tap-flipped transposed filters), 'same' padding.  dy [N,D,H,W,Cout], w [27][Cout][Cin] -> [N,D,H,W,Cin]"""
    Cout, Cin = w.shape[1], w.shape[2]
    k = f64(w).reshape(3, 3, 3, Cout, Cin).permute(4, 3, 0, 1, 2).flip(2, 3, 4).contiguous()        # (Cin, Cout, kd, kh, kw), taps mirrored
    return to_ndhwc(F.conv3d(to_ncdhw(f64(dy)), k, padding=1))


def _run(ops, dy, w, Cin):
    dx = torch.full(tuple(dy.shape[:4]) + (Cin,), float("nan"), dtype=torch.float32, device="cuda")
    ops.conv3d_first_dgrad(dy, w, dx)
    torch.cuda.synchronize()
    return dx


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_exact_on_dyadic_data_and_reproducible(ops, case):
    Cin, Cout, N, D, H, W = case
    assert ops.conv3d_first_dgrad_ok(Cin, Cout, D, H, W, BF)
    g = torch.Generator().manual_seed(Cin * 100 + Cout + D)
    dy = _dy4(g, (N, D, H, W, Cout), -4, 4, 4.0).to(BF).cuda()
    w = _dy4(g, (27, Cout, Cin), -2, 2, 8.0).to(BF).cuda()
    dx = _run(ops, dy, w, Cin)
    assert_same(dx.cpu(), _ref(dy, w).float(), "first dgrad, dyadic")
    assert_same(_run(ops, dy, w, Cin), dx, "first dgrad, second launch")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_random_bf16_vs_fp64(ops, case):
    Cin, Cout, N, D, H, W = case
    dy = rnd((N, D, H, W, Cout), 700 + Cin + Cout, BF)
    w = rnd((27, Cout, Cin), 710 + Cin + Cout, BF, scale=0.2)
    dx = _run(ops, dy, w, Cin)
    assert_close(dx, _ref(dy, w), *DGRAD_TOL, what="first dgrad %s" % (case,))


def test_matches_the_generic_input_gradient(ops):
    """the route the engine takes without this kernel - fmri_conv3d_dgrad (generic) on a [27][Cin][Cout] image - gives the same tensor up to
    its bf16 output rounding"""
    from fmri_hip._lib import IMPL_GENERIC
    Cin, Cout, N, D, H, W = 1, 32, 1, 8, 16, 32
    g = torch.Generator().manual_seed(5)
    dy = _dy4(g, (N, D, H, W, Cout), -4, 4, 4.0).to(BF).cuda()
    w = _dy4(g, (27, Cout, Cin), -2, 2, 8.0).to(BF).cuda()
    wd = w.flip(0).transpose(1, 2).contiguous()
    old = torch.empty((N, D, H, W, Cin), dtype=BF, device="cuda")
    ops.conv3d_dgrad(dy, wd, old, impl=IMPL_GENERIC)
    assert_same(_run(ops, dy, w, Cin).to(BF), old, "first dgrad vs generic")


def test_refusals(ops):
    from fmri_hip._lib import BF16, F32, lib
    L = lib()
    good = dict(Cin=1, Cout=32, D=4, H=16, W=32, dtype=BF16)
    dy = torch.zeros((1, 4, 16, 32, 32), dtype=BF, device="cuda")
    w = torch.zeros((27, 32, 1), dtype=BF, device="cuda")
    dx = torch.zeros((1, 4, 16, 32, 1), dtype=torch.float32, device="cuda")

    def call(dyp, wp, dxp, N=1, **kw):
        a = dict(good, **kw)
        return L.fmri_conv3d_first_dgrad(dyp, a["Cout"], wp, dxp, N, a["D"], a["H"], a["W"], a["Cin"], a["dtype"], None)

    assert L.fmri_conv3d_first_dgrad_ok(1, 32, 4, 16, 32, BF16) == 1
    assert call(dy.data_ptr(), w.data_ptr(), dx.data_ptr()) == 0
    for bad in (dict(dtype=F32), dict(Cout=48), dict(W=48), dict(H=8), dict(D=6), dict(Cin=5), dict(Cin=0), dict(Cout=0)):
        a = dict(good, **bad)
        assert L.fmri_conv3d_first_dgrad_ok(a["Cin"], a["Cout"], a["D"], a["H"], a["W"], a["dtype"]) == 0, bad
        assert call(dy.data_ptr(), w.data_ptr(), dx.data_ptr(), **bad) == -1, bad          # FMRI_E_SHAPE
    for ptrs in ((None, w.data_ptr(), dx.data_ptr()), (dy.data_ptr(), None, dx.data_ptr()), (dy.data_ptr(), w.data_ptr(), None)):
        assert call(*ptrs) == -1
    assert call(dy.data_ptr(), w.data_ptr(), dx.data_ptr(), N=0) == -1
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError):
        ops.conv3d_first_dgrad(dy.cpu(), w.cpu(), dx.cpu())
