"""Overlap losses on the device (DESIGN.md "Overlap losses"): fmri_boundary_sum, fmri_overlap_coeffs and fmri_overlap_loss_bwd against the
fp64 autograd restatement of the written formulas, the engines' training step with each new loss, the footprint of the three entry points.

Bars.  The kernels compute the coefficients in fp64 and the element in fp32, as the existing Dice gradient kernel does, so THAT kernel is
the yardstick: `yardstick` runs fmri_sigmoid_dice_fwd + fmri_sigmoid_loss_bwd kind 0 on the very inputs of the shape table below and
measures its gradient against fp64 autograd (relative to the gradient's max-abs) and its loss value (from the fp64 sums of fp32 products)
against the fp64 value.  E_grad / E_value are the LARGEST of these over the sixteen shapes (a single shape is no yardstick: at nvox = 1 the
Dice kernel's error can be exactly 0, which bars nothing but bit equality); the new kernels may be at most 2x that, at every shape.
Value errors are absolute: all these losses are O(1).  The entry points take alpha, beta, gamma, smooth and the boundary weight as C
floats, so the restatement is evaluated at the float-rounded parameters (r32): the loss the device computes has alpha = 0.3f.
The Dice VALUE is one division behind fp64 sums, and its measured error is 0 on most shapes and 1.7e-16 on the others, whichever way the
atomics of a run fall: below the rounding of the fp64 restatement itself.  So every value bar is 2 x E_value PLUS that rounding,
REF_ROUNDING = 8 x 2^-53: behind its sums the restatement makes about eight operations (T: five additions and products and a division;
1 - T; pow; the mean) of at most half an ulp of a number <= 1 each.
Measured on MI355X (profiles/overlap_losses.log): E_grad 1.95e-07 (the Dice kernel, L = 5, nvox = 4099), the new gradient kernel's largest
error 2.39e-07 (L = 32, nvox = 65539, label-mean focal), 0.61 of its bar; E_value 0 to 1.7e-16, the new values' largest error 2.2e-16 (one ulp).
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from footprint import audit
from gpu_util import bar

pytestmark = pytest.mark.gpu

E_SHAPE = -1
LS, NVOX = (1, 3, 5, 32), (1, 255, 4099, 65536 + 3)
ALPHA_BETA = ((0.5, 0.5), (0.3, 0.7), (0.0, 1.0))
GAMMAS = (1.0, 4.0 / 3, 2.0)
F32, F64 = torch.float32, torch.float64
REF_ROUNDING = 8 * 2.0 ** -53          # the fp64 restatement's own rounding of a loss value (module docstring)


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as g
    from fmri_hip._lib import LIB_PATH
    if not os.path.exists(LIB_PATH):
        g.build()
    from fmri_hip import ops as o
    assert torch.cuda.is_available()
    return o


def _s():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------ the fp64 restatement
def _tversky(i, sy, sp, a, b, s):
    return (i + s) / (i + a * (sp - i) + b * (sy - i) + s)


def ref_loss(p, y, kind, a, b, g, s, dist=None, bweight=0.0):
    """the loss of include/fmri_hip.h as a float64 torch expression of p [nvox, L] (y the same shape, float64)"""
    i, sy, sp = (y * p).sum(0), y.sum(0), p.sum(0)
    if kind <= 3:
        if kind < 2:
            i, sy, sp = i.sum(), sy.sum(), sp.sum()
        T = _tversky(i, sy, sp, a, b, s)
        if kind in (0, 2):
            f = -T
        else:
            u = 1.0 - T
            if float(u.min()) > 1e-7:
                f = u ** (1.0 / g)                                   # plain autograd
            else:
                # the documented clamp: the value is max(u, 0)^(1/g), the derivative is taken at max(u, 1e-7)
                slope = u.detach().clamp(min=1e-7) ** (1.0 / g - 1.0) / g
                f = u.detach().clamp(min=0.0) ** (1.0 / g) + slope * (u - u.detach())
        val = f.mean()
    else:
        syd = sy.detach()
        present = syd > 0
        w = torch.ones_like(syd)
        if bool(present.any()):
            w = torch.where(present, 1.0 / torch.where(present, syd, torch.ones_like(syd)) ** 2, torch.zeros_like(syd))
            w = torch.where(present, w, w.max())
        val = 1.0 - (2.0 * (w * i).sum() + s) / ((w * (sy + sp)).sum() + s)
    if dist is not None:
        val = val + bweight * ((1.0 - 2.0 * y) * dist * p).sum() / p.numel()
    return val


def ref_value_and_grad(p32, y8, L, fn):
    """(value, d/dlogits) in fp64 of fn(p, y) at the fp32 probabilities the kernels read: dL/dp by autograd, times p (1 - p)"""
    p = p32.detach().cpu().double().reshape(-1, L).requires_grad_(True)
    y = y8.cpu().double().reshape(-1, L)
    val = fn(p, y)
    val.backward()
    pd = p.detach()
    return float(val), (p.grad * pd * (1.0 - pd)).reshape(-1)


def r32(*v):
    """the parameters as the C ABI receives them: rounded to float"""
    out = tuple(float(np.float32(x)) for x in v)
    return out if len(out) > 1 else out[0]


def rel_err(got, ref):
    """max-abs error of a gradient relative to the reference's max-abs"""
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(ref).all())
    return float((got.detach().cpu().double().reshape(-1) - ref).abs().max()) / (float(ref.abs().max()) + 1e-300)


# ------------------------------------------------------------------------------------------------ inputs, yardstick
def _inputs(ops, L, nvox, seed=None):
    rs = np.random.RandomState(1000 * L + nvox % 1000 if seed is None else seed)
    logits = torch.from_numpy((rs.randn(nvox * L) * 2.0).astype(np.float32)).cuda()
    y = torch.from_numpy((rs.rand(nvox * L) > 0.7).astype(np.uint8)).cuda()
    return _forward(ops, logits, y, L)


def _forward(ops, logits, y, L):
    probs, sums = torch.empty_like(logits), torch.zeros(16, dtype=F64, device="cuda")
    ops.sigmoid_dice_fwd(logits, y, probs, sums)
    return dict(L=L, nvox=logits.numel() // L, logits=logits, y=y, probs=probs, sums=sums)


def _dice_errors(ops, d):
    """(gradient error, value error) of the existing Dice kernels on the inputs d"""
    dl = torch.empty_like(d["probs"])
    ops.sigmoid_loss_bwd(d["probs"], d["y"], d["sums"], dl, 0, 1.0)
    val, g = ref_value_and_grad(d["probs"], d["y"], 1, lambda p, y: -(2 * (y * p).sum() + 1) / (y.sum() + p.sum() + 1))
    return rel_err(dl, g), abs(ops.loss_value_from_sums(d["sums"].cpu().numpy(), 0) - val)


@pytest.fixture(scope="module")
def table(ops):
    """the sixteen input sets, each with probabilities and sums from fmri_sigmoid_dice_fwd, computed once"""
    return {(L, n): _inputs(ops, L, n) for L in LS for n in NVOX}


@pytest.fixture(scope="module")
def yardstick(ops, table):
    errs = {k: _dice_errors(ops, d) for k, d in table.items()}
    eg, ev = max(e[0] for e in errs.values()), max(e[1] for e in errs.values())
    print("\nyardstick (fmri_sigmoid_loss_bwd kind 0 / dice value vs fp64): E_grad %.3e  E_value %.3e" % (eg, ev))
    bar("overlap yardstick E_grad", eg, 1e-6)
    bar("overlap yardstick E_value", ev, 1e-13)
    for k in sorted(errs):
        print("  L %2d nvox %6d  grad %.3e  value %.3e" % (k + errs[k]))
    assert 0 < eg < 1e-6 and 0 <= ev < 1e-13, (eg, ev)         # sanity of the yardstick itself: fp32 element, fp64 sums
    return eg, ev


def run_overlap(ops, d, kind, a, b, g, s, dist=None, bweight=0.0, grad_scale=1.0, place=None):
    """label sums -> (boundary sum) -> coefficients -> gradient.  place: a function that re-homes a tensor (offset placements)"""
    L, nvox = d["L"], d["nvox"]
    probs, y = d["probs"], d["y"]
    dl = torch.full((nvox * L,), float("nan"), dtype=F32, device="cuda")
    if place is not None:
        probs, y, dl, dist = place(probs), place(y), place(dl), (place(dist) if dist is not None else None)
    lsums = torch.full((3 * L,), float("nan"), dtype=F64, device="cuda")
    coef = torch.full((2 * L + 2,), float("nan"), dtype=F64, device="cuda")
    ops.label_sums(probs, y, L, lsums)
    bd = None
    if dist is not None:
        bd = torch.full((1,), float("nan"), dtype=F64, device="cuda")
        ops.boundary_sum(probs, y, dist, bd)
    ops.overlap_coeffs(lsums, d["sums"], coef, L, kind, a, b, g, s, bd=bd, boundary_weight=bweight)
    ops.overlap_loss_bwd(probs, y, coef, dl, L, dist=dist, boundary_scale=bweight / nvox, grad_scale=grad_scale)
    return coef.cpu().numpy(), dl, (None if bd is None else float(bd))


def _cases():
    """every kind with every (alpha, beta) and, for the focal kinds, every gamma at least once per (alpha, beta) rotation"""
    out = []
    for kind in (0, 2):
        out += [(kind, a, b, 1.0, 1.0 if kind == 0 else 0.5) for a, b in ALPHA_BETA]
    for kind in (1, 3):
        out += [(kind, a, b, GAMMAS[(k + kind) % 3], 1.0) for k, (a, b) in enumerate(ALPHA_BETA)]
        out += [(kind, 0.3, 0.7, g, 1.0) for g in GAMMAS]
    out.append((4, 0.5, 0.5, 1.0, 1e-5))
    return list(dict.fromkeys(out))


def check_case(ops, d, yard, case, what, **kw):
    kind, (a, b, g, s) = case[0], r32(*case[1:])
    eg, ev = yard
    coef, dl, _ = run_overlap(ops, d, kind, a, b, g, s, **kw)
    gs = kw.get("grad_scale", 1.0)
    val, gref = ref_value_and_grad(d["probs"], d["y"], d["L"], lambda p, y: ref_loss(p, y, kind, a, b, g, s))
    name = "%s kind %d a %.1f b %.1f g %.2f" % (what, kind, a, b, g)
    bar("overlap grad: " + name, rel_err(dl, gs * gref), 2 * eg)
    bar("overlap value: " + name, abs(float(coef[-2]) - val), 2 * ev + REF_ROUNDING)
    assert coef[-1] == coef[-2]                                         # no boundary term


# ------------------------------------------------------------------------------------------------ kernel level
def test_the_feature_is_there(ops):
    """what fails on the parent commit: the symbols, the tokens, and compile + train_on_batch (NotImplementedError there)"""
    from fetal_net import metrics as M
    from fmri_hip._lib import lib
    for name in ("fmri_boundary_sum", "fmri_overlap_coeffs", "fmri_overlap_loss_bwd"):
        assert hasattr(lib(), name), name
    assert callable(M.tversky_loss) and callable(M.focal_tversky_loss) and callable(M.generalised_dice_loss) and callable(M.dice_and_boundary)


@pytest.mark.parametrize("nvox", NVOX)
@pytest.mark.parametrize("L", LS)
def test_value_and_gradient_against_fp64_autograd(ops, table, yardstick, L, nvox):
    """all kinds, (alpha, beta) and gamma at every shape: nvox * L % 4 != 0 takes the scalar kernel, the others the 16-byte one; L = 3, 5
    make the grid a multiple of an odd L; L = 32 is the cap"""
    for case in _cases():
        check_case(ops, table[(L, nvox)], yardstick, case, "L %d nvox %d" % (L, nvox))


def _offset(nbytes):
    def place(t):
        if t is None:
            return None
        raw = torch.empty(t.numel() * t.element_size() + 256, dtype=torch.uint8, device="cuda")
        base = (-raw.data_ptr()) % 256 + nbytes
        v = raw[base:base + t.numel() * t.element_size()].view(t.dtype)
        v.copy_(t.reshape(-1))
        assert v.data_ptr() % 256 == nbytes
        return v
    return place


@pytest.mark.parametrize("nbytes", [16, 4], ids=["16-byte offset", "4-byte offset"])
def test_offset_placements(ops, yardstick, nbytes):
    """nvox * L % 4 == 0 with every tensor 16 bytes behind a 256-byte boundary (still the 16-byte kernel: the engines' flat buffers put
    tensors there) and 4 bytes behind it (no 16-byte access possible: the scalar fallback), boundary term included at L = 1"""
    for L, nvox in ((3, 65536 + 4), (1, 4100)):
        d = _inputs(ops, L, nvox, seed=77 + L)
        for case in ((0, 0.3, 0.7, 1.0, 1.0), (3, 0.3, 0.7, 2.0, 1.0), (4, 0.5, 0.5, 1.0, 1e-5)):
            check_case(ops, d, yardstick, case, "%d-byte offset L %d" % (nbytes, L), place=_offset(nbytes), grad_scale=0.5)
    d = _inputs(ops, 1, 4100, seed=5)
    dist = torch.from_numpy(np.random.RandomState(6).rand(4100).astype(np.float32) * 7).cuda()
    _check_boundary(ops, d, dist, 0.05, yardstick, "%d-byte offset" % nbytes, place=_offset(nbytes))


def test_absent_label_and_empty_batch(ops, yardstick):
    """a label absent from the batch (GDL: it takes the largest weight among the present), and no foreground at all (GDL: weights 1)"""
    L, nvox = 3, 4099
    base = _inputs(ops, L, nvox, seed=21)
    y = base["y"].clone().reshape(nvox, L)
    y[:, 1] = 0
    absent = _forward(ops, base["logits"], y.reshape(-1).contiguous(), L)
    empty = _forward(ops, base["logits"], torch.zeros_like(base["y"]), L)
    for d, what in ((absent, "label 1 absent"), (empty, "no foreground")):
        for case in _cases():
            check_case(ops, d, yardstick, case, what)
    # the rule itself, from the coefficients: A_l = -2 w_l / den
    coef, _, _ = run_overlap(ops, absent, 4, 0.5, 0.5, 1.0, 1e-5)
    sy = absent["y"].reshape(nvox, L).double().sum(0).cpu().numpy()
    A = coef[0:2 * L:2]
    assert A[1] == pytest.approx(A[0] * max(1.0, (sy[0] / sy[2]) ** 2), rel=1e-12) and A[1] == min(A)
    coef, _, _ = run_overlap(ops, empty, 4, 0.5, 0.5, 1.0, 1e-5)
    assert coef[0] == coef[2] == coef[4] and coef[1] == coef[3] == coef[5]


def test_saturated_logits_and_the_focal_clamp(ops, yardstick):
    """logits of +-30 that agree with the labels: p = 1.0f or 9.4e-14, T within 1e-9 of 1.  Everything stays finite, and with gamma = 2 the
    derivative is the one at max(1 - T, 1e-7).  The value (1 - T)^(1/2) has the slope 1 / (2 sqrt(1 - T)) in 1 - T, so its bar is the
    bar of 1 - T times that slope."""
    eg, ev = yardstick
    a, b, g = r32(0.3, 0.7, 2.0)
    for L in (1, 3):
        nvox = 4099
        rs = np.random.RandomState(31 + L)
        y = torch.from_numpy((rs.rand(nvox * L) > 0.7).astype(np.uint8)).cuda()
        d = _forward(ops, (y.float() * 60.0 - 30.0).contiguous(), y, L)
        for kind in (1, 3):
            coef, dl, _ = run_overlap(ops, d, kind, a, b, g, 1.0)
            val, gref = ref_value_and_grad(d["probs"], d["y"], L, lambda p, y_: ref_loss(p, y_, kind, a, b, g, 1.0))
            assert 0.0 <= val < np.sqrt(1e-9) and np.isfinite(coef).all() and float(gref.abs().max()) > 0
            bar("overlap grad: clamp kind %d L %d" % (kind, L), rel_err(dl, gref), 2 * eg)
            bar("overlap value: clamp kind %d L %d" % (kind, L), abs(float(coef[-2]) - val), (2 * ev + REF_ROUNDING) / (2 * max(val, 1e-7)))
            # the clamp: dL/dSp = (1/2) (1e-7)^(-1/2) * alpha N / D^2, not the pole's value
            i, sy, sp = float(d["sums"][0]), float(d["sums"][1]), float(d["sums"][2])
            if kind == 1:
                D = i + a * (sp - i) + b * (sy - i) + 1.0
                assert coef[1] == pytest.approx(0.5 * 1e-7 ** -0.5 * a * (i + 1.0) / D ** 2, rel=1e-9)
        # saturated against the labels too (every prediction wrong), all kinds: finite value and gradient, within the bars
        wrong = _forward(ops, (30.0 - y.float() * 60.0).contiguous(), y, L)
        for case in _cases():
            check_case(ops, wrong, yardstick, case, "saturated wrong L %d" % L)


def test_tie_in_with_the_dice_kernel(ops, table, yardstick):
    """kind 0 with alpha = beta = smooth = 1/2 at L = 1 is the Dice loss: its gradient and fmri_sigmoid_loss_bwd kind 0 (smooth 1) differ by
    fp32 rounding only"""
    eg, ev = yardstick
    for nvox in NVOX:
        d = table[(1, nvox)]
        coef, dl, _ = run_overlap(ops, d, 0, 0.5, 0.5, 1.0, 0.5, grad_scale=0.25)
        old = torch.empty_like(dl)
        ops.sigmoid_loss_bwd(d["probs"], d["y"], d["sums"], old, 0, 1.0, smooth=1.0, grad_scale=0.25)
        bar("overlap tie-in grad nvox %d" % nvox, rel_err(dl, old.cpu().double()), 2 * eg)
        bar("overlap tie-in value nvox %d" % nvox, abs(float(coef[-2]) - ops.loss_value_from_sums(d["sums"].cpu().numpy(), 0)),
            2 * ev + REF_ROUNDING)


# ------------------------------------------------------------------------------------------------ boundary term
def _blobs():
    """12 x 10 x 7: two blobs and one voxel on the border"""
    t = np.zeros((12, 10, 7), np.uint8)
    t[2:5, 2:6, 1:4] = 1
    t[7:11, 5:9, 3:6] = 1
    t[0, 4, 6] = 1
    return t


def _check_boundary(ops, d, dist, bweight, yard, what, place=None):
    eg, ev = yard
    nvox, bweight = d["nvox"], r32(bweight)
    coef, dl, bd = run_overlap(ops, d, 0, 0.5, 0.5, 1.0, 0.5, dist=dist, bweight=bweight, place=place)
    d64 = dist.cpu().double().reshape(-1, 1)
    val, gref = ref_value_and_grad(d["probs"], d["y"], 1, lambda p, y: ref_loss(p, y, 0, 0.5, 0.5, 1.0, 0.5, dist=d64, bweight=bweight))
    p64, y64 = d["probs"].cpu().double(), d["y"].cpu().double()
    # Bd: an fp64 sum of fp32 products (1 - 2 y) * dist * p, each within 2^-24 of the exact product, summed in any order
    exact = ((1 - 2 * y64) * d64.reshape(-1) * p64)
    assert abs(bd - float(exact.sum())) <= float(exact.abs().sum()) * (2.0 ** -24 + nvox * 2.0 ** -53), (what, bd, float(exact.sum()))
    bar("overlap grad: boundary " + what, rel_err(dl, gref), 2 * eg)
    # value: the Dice part within the value bar, the boundary part bweight / n times the Bd bound above
    bar("overlap value: boundary " + what, abs(float(coef[-2]) - val), 2 * ev + REF_ROUNDING + bweight / nvox * float(exact.abs().sum()) * 2.0 ** -24 * 1.01)
    assert coef[-1] != coef[-2] and abs((coef[-2] - coef[-1]) - bweight * bd / nvox) <= 1e-15 * abs(coef[-2]) + 1e-18


def test_boundary_term(ops, yardstick):
    truth = torch.from_numpy(_blobs()).cuda()
    dist = ops.distance_mask_u8(truth).float().reshape(-1).contiguous()
    assert bool(torch.isfinite(dist).all()) and float(dist.min()) >= 1.0
    rs = np.random.RandomState(3)
    logits = torch.from_numpy((rs.randn(truth.numel()) * 2).astype(np.float32)).cuda()
    d = _forward(ops, logits, truth.reshape(-1).contiguous(), 1)
    _check_boundary(ops, d, dist, 0.01, yardstick, "12x10x7")
    _check_boundary(ops, d, dist, 1.0, yardstick, "12x10x7 weight 1")


def test_argument_checks(ops):
    """every refused argument: FMRI_E_SHAPE before any launch (the tensors are NaN-filled and stay so)"""
    from fmri_hip._lib import lib
    Lb, s = lib(), _s()
    n, L = 4096, 3
    pr = torch.full((n * L,), float("nan"), device="cuda")
    y = torch.zeros(n * L, dtype=torch.uint8, device="cuda")
    f = torch.full((256,), float("nan"), dtype=F64, device="cuda")
    p_, y_, f_ = pr.data_ptr(), y.data_ptr(), f.data_ptr()
    ok = dict(lsums=f_, sums=f_, bd=0, coef=f_, L=L, kind=0, alpha=0.3, beta=0.7, gamma=1.5, smooth=1.0, bw=0.0)

    def coeffs(**kw):
        a = dict(ok, **kw)
        return Lb.fmri_overlap_coeffs(a["lsums"], a["sums"], a["bd"], a["coef"], a["L"], a["kind"], a["alpha"], a["beta"], a["gamma"], a["smooth"],
                                      a["bw"], s)
    for bad in (dict(L=0), dict(L=33), dict(lsums=0), dict(sums=0), dict(coef=0), dict(kind=-1), dict(kind=5), dict(alpha=-0.1), dict(beta=-1.0),
                dict(gamma=0.99), dict(gamma=float("nan")), dict(bd=f_, L=3)):
        assert coeffs(**bad) == E_SHAPE, bad

    def bwd(probs=p_, yt=y_, dist=0, coef=f_, dl=p_, nvox=n, L_=L):
        return Lb.fmri_overlap_loss_bwd(probs, yt, dist, coef, dl, nvox, L_, 0.0, 1.0, s)
    for bad in (dict(probs=0), dict(yt=0), dict(coef=0), dict(dl=0), dict(nvox=0), dict(nvox=-4), dict(L_=0), dict(L_=33), dict(dist=p_, L_=3)):
        assert bwd(**bad) == E_SHAPE, bad
    for args in ((0, y_, p_, n, f_), (p_, 0, p_, n, f_), (p_, y_, 0, n, f_), (p_, y_, p_, 0, f_), (p_, y_, p_, n, 0)):
        assert Lb.fmri_boundary_sum(*args, s) == E_SHAPE, args
    torch.cuda.synchronize()
    assert bool(torch.isnan(pr).all()) and bool(torch.isnan(f).all())


def test_sums_repeat_bit_for_bit_under_a_deterministic_registration(ops):
    """fmri_boundary_sum meets as 2^-20 fixed point under fmri_set_deterministic, fmri_overlap_coeffs is one wave: equal bits every time"""
    n = 65536 + 3
    d = _inputs(ops, 1, n, seed=9)
    dist = torch.from_numpy(np.random.RandomState(10).rand(n).astype(np.float32) * 9).cuda()
    grad, shadow = torch.zeros(64, device="cuda"), torch.zeros(64, dtype=torch.int64, device="cuda")
    ops.set_deterministic(grad, shadow)
    try:
        outs = [run_overlap(ops, d, 1, 0.3, 0.7, 2.0, 1.0, dist=dist, bweight=0.01) for _ in range(4)]
    finally:
        ops.set_deterministic(None, None)
    for coef, dl, bd in outs[1:]:
        assert coef.tobytes() == outs[0][0].tobytes() and bd == outs[0][2] and torch.equal(dl, outs[0][1])
    ref = float(((1 - 2 * d["y"].cpu().double()) * dist.cpu().double() * d["probs"].cpu().double()).sum())
    assert outs[0][2] == pytest.approx(ref, rel=1e-6)


# ------------------------------------------------------------------------------------------------ footprint
@pytest.mark.parametrize("nvox", [4099, 4100], ids=["scalar", "vec4"])
@pytest.mark.parametrize("offset16", [False, True], ids=["aligned", "offset16"])
def test_footprint_of_the_three_entry_points(ops, offset16, nvox):
    """nvox = 4099, L = 3 (and the single-label boundary pair; 4100: the same through the 16-byte kernels): every tensor from the
    guard-band allocator; coef and the sum slots are outputs with guards on both sides"""
    L = 3
    d3, d1 = _inputs(ops, L, nvox, seed=41), _inputs(ops, 1, nvox, seed=42)
    dist0 = torch.from_numpy(np.random.RandomState(43).rand(nvox).astype(np.float32) * 5).cuda()

    def run(a):
        o = dict(offset16=offset16)
        out = {}
        for tag, d, dist_ in (("L3", d3, None), ("L1", d1, dist0)):
            Lc = d["L"]
            probs, y = a.input(d["probs"], name="probs_" + tag, **o), a.input(d["y"], name="y_" + tag, **o)
            sums = a.input(d["sums"], name="sums_" + tag, **o)
            lsums = a.output((3 * Lc,), F64, name="lsums_" + tag, **o)
            ops.label_sums(probs, y, Lc, lsums)
            bd = dist = None
            if dist_ is not None:
                dist = a.input(dist_, name="dist", **o)
                bd = a.output((1,), F64, name="bd", **o)
                ops.boundary_sum(probs, y, dist, bd)
                out["bd"] = bd
            coef = a.output((2 * Lc + 2,), F64, name="coef_" + tag, **o)
            ops.overlap_coeffs(lsums, sums, coef, Lc, 3 if Lc > 1 else 1, 0.3, 0.7, 1.5, 1.0, bd=bd, boundary_weight=0.02)
            dl = a.output((nvox * Lc,), F32, name="dlogits_" + tag, **o)
            ops.overlap_loss_bwd(probs, y, coef, dl, Lc, dist=dist, boundary_scale=0.02 / nvox)
            out.update({"lsums_" + tag: lsums, "coef_" + tag: coef, "dlogits_" + tag: dl})
        return out
    loose = ("lsums_L3", "coef_L3", "dlogits_L3", "lsums_L1", "coef_L1", "dlogits_L1", "bd")          # fp64 atomics: compared below
    r0, r1 = audit(run, loose=loose)
    for k in loose:
        a_, b_ = r0[k].double().cpu(), r1[k].double().cpu()
        assert bool(torch.isfinite(a_).all()) and float((a_ - b_).abs().max()) <= 1e-6 * float(a_.abs().max()), k


# ------------------------------------------------------------------------------------------------ both engines
def _labels_last(a):
    return np.moveaxis(np.asarray(a), 1, -1)


ENGINE_TOL = 1e-5          # two fp32 forward passes of one model (predict, then the step's own): the bar of test_gpu_model.py:220


def _losses():
    from fetal_net import metrics as M
    return [M.tversky_loss(), M.tversky_loss(0.5, 0.5, 0.5, per_label=True), M.focal_tversky_loss(), M.focal_tversky_loss(0.3, 0.7, 2.0, per_label=True),
            M.generalised_dice_loss]


def _one_step_each(model, x, y):
    for loss in _losses():
        model.compile(optimizer=model.optimizer, loss=loss, metrics=model.metrics)
        before = {k: v.copy() for k, v in model.get_weights_dict().items()}
        want = loss(_labels_last(y), _labels_last(model.predict(x)).astype(np.float64))
        got = model.train_on_batch(x, y)[0]
        assert np.isfinite(got) and abs(got - want) <= ENGINE_TOL, (loss.__name__, getattr(loss, "loss_params", None), got, want)
        after = model.get_weights_dict()
        assert any(not np.array_equal(before[k], after[k]) for k in before), loss.__name__
        assert abs(model.test_on_batch(x, y)[0] - loss(_labels_last(y), _labels_last(model.predict(x)).astype(np.float64))) <= ENGINE_TOL


def _batch(shape, L, seed):
    rs = np.random.RandomState(seed)
    x = rs.randn(2, *shape).astype(np.float32)
    y = (rs.rand(2, L, *shape[1:]) > 0.7).astype(np.uint8)
    return x, y


def test_unet_engine_trains_with_each_overlap_loss(ops):
    import fetal_net.model as fmodel
    from fetal_net import metrics as M
    shape = (1, 16, 16, 16)
    model = fmodel.unet_model_3d(shape, depth=2, n_base_filters=8, n_labels=3, compute_dtype="fp32", initial_learning_rate=1e-3)
    x, y = _batch(shape, 3, 50)
    _one_step_each(model, x, y)
    model.compile(optimizer=model.optimizer, loss=M.focal_tversky_loss(), metrics=model.metrics)
    losses = [model.train_on_batch(x, y)[0] for _ in range(20)]
    assert losses[-1] < losses[0], losses                                   # a direction check on a fixed batch, not a Dice claim


def test_layer_graph_engine_trains_with_each_overlap_loss(ops):
    import fetal_net.model as fmodel
    shape = (1, 16, 16, 16)
    model = fmodel.isensee2017_model_3d(input_shape=shape, depth=3, n_base_filters=8, n_labels=3, dropout_rate=0.0, compute_dtype="fp32")
    x, y = _batch(shape, 3, 51)
    _one_step_each(model, x, y)


def test_dice_and_boundary_on_the_mask_input_model(ops, tmp_path):
    import fetal_net.model as fmodel
    from fetal_net import metrics as M
    from fetal_net.training import load_old_model
    shape = (1, 16, 16, 16)
    model = fmodel.isensee2017_model_3d(input_shape=shape, loss_function=M.dice_and_boundary, mask_shape=shape, depth=3, n_base_filters=8,
                                        dropout_rate=0.0, compute_dtype="fp32")
    rs = np.random.RandomState(52)
    x = rs.randn(2, *shape).astype(np.float32)
    y = np.zeros((2,) + shape, np.uint8)
    y[0, 0, 3:9, 4:12, 2:7] = 1
    y[1, 0, 8:14, 1:6, 9:15] = 1
    masks = np.stack([ops.distance_mask_u8(torch.from_numpy(v[0]).cuda()).cpu().numpy() for v in y])[:, None].astype(np.float32)
    with pytest.raises(ValueError):
        model.test_on_batch(x, y)
    before = {k: v.copy() for k, v in model.get_weights_dict().items()}
    want = M.dice_and_boundary(masks, 0.01)(y, model.predict(x).astype(np.float64))
    plain = M.dice_coefficient_loss(y, model.predict(x).astype(np.float64))
    got = model.train_on_batch([x, masks], y)[0]
    assert abs(got - want) <= ENGINE_TOL and abs(want - plain) > 100 * ENGINE_TOL, (got, want, plain)
    after = model.get_weights_dict()
    assert any(not np.array_equal(before[k], after[k]) for k in before)
    path = str(tmp_path / "m-epoch01-loss0.100-acc0.900.h5")
    model.save(path)
    again = load_old_model(path)
    assert getattr(again.loss, "mask_input", False) and again.loss.boundary_weight == 0.01
    assert abs(again.test_on_batch([x, masks], y)[0] - model.test_on_batch([x, masks], y)[0]) <= ENGINE_TOL


def test_checkpoint_keeps_the_loss_and_its_parameters(ops, tmp_path):
    import fetal_net.model as fmodel
    from fetal_net import metrics as M
    from fetal_net.training import load_old_model
    shape = (1, 16, 16, 16)
    model = fmodel.unet_model_3d(shape, depth=2, n_base_filters=8, n_labels=3, compute_dtype="fp32")
    model.compile(optimizer=model.optimizer, loss=M.focal_tversky_loss(0.3, 0.7, 1.5), metrics=model.metrics)
    x, y = _batch(shape, 3, 53)
    model.train_on_batch(x, y)
    path = str(tmp_path / "m-epoch01-loss0.100-acc0.900.h5")
    model.save(path)
    again = load_old_model(path)
    assert again.loss.loss_params == dict(alpha=0.3, beta=0.7, gamma=1.5, smooth=1.0, per_label=False)
    assert abs(again.test_on_batch(x, y)[0] - model.test_on_batch(x, y)[0]) <= ENGINE_TOL
    assert np.isfinite(again.train_on_batch(x, y)[0])


def test_a_step_under_the_deterministic_switch_repeats_bit_for_bit():
    """in a fresh child process, so that the engine reads FMRI_DETERMINISTIC=1 where nothing else has touched the library"""
    env = dict(os.environ, FMRI_DETERMINISTIC="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "overlap_det_child.py")], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=240)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and "BITS EQUAL" in out, out[-3000:]
