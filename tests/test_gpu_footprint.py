"""Guard-band audit: does every kernel stay inside its buffers?  (tests/footprint.py holds the arena; DESIGN.md "Footprint audit")

Every case is one LEGAL call sequence written once as run(alloc) and executed twice: on ordinary fresh tensors (Plain) and inside an Arena -
one allocation of 0xFF bytes in which each tensor has a guard band of >= 64 KiB (>= one outermost slice) on both sides, fp32
parameter-like pointers sit at 256 k + 16 (the engines' flat-buffer alignment) and every workspace / scratch is EXACTLY as long as the
library's own size function or header says.  After the arena run: every guard byte still 0xFF, inputs bit-identical, sentinel columns of
strided slots untouched, outputs fully written, zero-on-exit workspaces zero.  A load from outside a tensor meets NaN there and not in
the plain run, so the results differ.

Comparison of the two runs - no new tolerance anywhere:
 * ordered kernels: bit for bit (footprint.assert_same = gpu_util.assert_same);
 * sums that meet in floating-point atomics (weight / bias gradients' atomic flush, the parity weight gradient's dwc scratch, fp64
   statistics of the normalisation passes and of the fused tails, the Dice / loss sums, conv1x1_bwd): BOTH runs against the same fp64
   reference under the bar of the op's existing test, quoted with file and line at each case.
The shapes are the smallest existing rows of the op tests (imported from them); the edge each family watches is named in its docstring.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from footprint import audit
from gpu_util import assert_close, f64, planar_kernel, ref_concat_input, rnd, to_ncdhw, to_ndhwc
from test_gpu_f32_mfma import WG as F32_WG
from test_gpu_first_dgrad import CASES as FIRST_DGRAD_CASES
from test_gpu_ops import CONV_CASES, NTAIL_CASES, PLANAR_CASES, PLANAR_TAIL_CASES, TAIL_CASES, UPCAT2D_CASES, UPCAT_CASES, WG_TOL

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the GPU box"
    from fmri_hip import ops as o
    return o


def _row(table, name):
    return next(c for c in table if c[0] == name)


def both_close(r0, r1, key, ref, rtol, atol, what):
    """a sum that meets in atomics: the plain and the arena result against the same reference under the existing test's bar"""
    assert_close(r0[key], ref, rtol, atol, what=what + " (plain)")
    assert_close(r1[key], ref, rtol, atol, what=what + " (arena)")


def zeros(shape, dtype=F32):
    return torch.zeros(shape, dtype=dtype, device="cuda")


# ================================================================================================ the checker itself, on device tensors
@pytest.mark.parametrize("kind,names", [("past_end", "BEHIND y_out"), ("before_start", "IN FRONT OF y_out"), ("behind_workspace", "BEHIND scratch_ws"),
                                        ("sentinel", "wide_out: sentinel column 5"), ("reads_behind_input", "total")])
def test_checker_catches_the_fake_defects_on_the_device(kind, names):
    """tests/test_host_footprint.py proves the checker on the CPU; the same fake ops (torch indexing inside the test's own allocations, no
    kernel of the library) must trip it on device memory too, or a green audit below would say nothing"""
    from test_host_footprint import _defect
    audit(_defect("none"))
    with pytest.raises(AssertionError) as e:
        audit(_defect(kind))
    assert names in str(e.value), str(e.value)


# ================================================================================================ A. 3x3x3 forward, every route
# Edge: the halo.  A tap outside the volume must come from the kernel's own zero, never from memory: in the arena the bytes in front of
# and behind src0 / src1 are NaN, and NaN * 0 is NaN.  mfma_deep_256 is an all-boundary tile with 8 channel chunks of out-of-volume halo.
FWD_ROWS = ["generic_odd_f32", "generic_dual_up_f32", "generic_bf16", "mfma_32_64", "mfma_dual_up", "mfma_deep_256", "mfma_cube_8",
            "mfma_cube_dual_up", "first_layer_4_modalities", "first_layer_32"]


def _fwd_run(ops, case, maskform=False, planar=False):
    if planar:
        name, dtype, S, H, W, C0, up0, C1, Cout, impl = case
        N, D = 1, S
        s0 = (1, S, H // 2, W // 2, C0) if up0 else (1, S, H, W, C0)
    else:
        name, dtype, N, D, H, W, C0, up0, C1, Cout, impl = case
        s0 = (N, D // 2, H // 2, W // 2, C0) if up0 else (N, D, H, W, C0)

    def run(a):
        src0 = a.input(rnd(s0, 1, dtype), name="src0")
        src1 = a.input(rnd((N, D, H, W, C1), 2, dtype), name="src1") if C1 else None
        w = a.input(rnd((27, Cout, C0 + C1), 3, dtype, scale=0.2), name="w")
        y = a.output((N, D, H, W, Cout), dtype, name="y")
        if maskform:          # the dgrad form: no bias, no activation, ReLU mask epilogue (test_gpu_ops.py:75)
            mask = a.input(rnd((N, D, H, W, Cout), 8, dtype), name="mask")
            ops.conv3d_fwd(src0, src1, w, None, y, up0=up0, act=0, mask=mask, impl=impl, planar=planar)
        else:
            bias = a.input(rnd((Cout,), 4, F32), offset16=True, name="bias")
            ops.conv3d_fwd(src0, src1, w, bias, y, up0=up0, act=1, impl=impl, planar=planar)
        return {"y": y}
    return run


@pytest.mark.parametrize("name", FWD_ROWS)
def test_a_conv3d_fwd(ops, name):
    audit(_fwd_run(ops, _row(CONV_CASES, name)))


@pytest.mark.parametrize("name", ["mfma_32_64", "generic_odd_f32"])
def test_a_conv3d_fwd_mask_no_bias(ops, name):
    audit(_fwd_run(ops, _row(CONV_CASES, name), maskform=True))


@pytest.mark.parametrize("name", ["planar_generic_dual_up_f32", "planar_mfma_32", "planar_mfma_dual_up", "planar_first_3"])
def test_a_conv3d_fwd_planar(ops, name):
    audit(_fwd_run(ops, _row(PLANAR_CASES, name), planar=True))


# ================================================================================================ B. fused tails
# Edge: the epilogue's second and third stores (pooled tile, logits row) and the statistics slot `1 + blockIdx.x` of a workspace that is
# exactly fmri_norm_tail_ws_doubles long.
def _tail_run(ops, N, D, H, W, C0, Cout, ok, planar):
    def run(a):
        x = a.input(rnd((N, D, H, W, C0), 21, BF), name="x")
        w = a.input(rnd((27, Cout, C0), 22, BF, scale=0.1), name="w")
        bias = a.input(rnd((Cout,), 23, F32, scale=0.3), offset16=True, name="bias")
        y = a.output((N, D, H, W, Cout), BF, name="y")
        pool = a.output((N, D if planar else D // 2, H // 2, W // 2, Cout), BF, name="pool")
        out = {"y": y, "pool": pool}
        if ok & 2:
            w1 = a.input(rnd((Cout,), 24, F32, scale=0.2), offset16=True, name="w1")
            b1 = a.input(rnd((1,), 25, F32), offset16=True, name="b1")
            logits = a.output((N * D * H * W,), F32, name="logits")
            ops.conv3d_fwd_tail(x, w, bias, y, pool=pool, w1=w1, b1=b1, logits=logits, act=1, planar=planar)
            out["logits"] = logits
        else:
            ops.conv3d_fwd_tail(x, w, bias, y, pool=pool, act=1, planar=planar)
        return out
    return run


@pytest.mark.parametrize("name", ["narrow_32", "few_tiles_64"])
def test_b_conv3d_fwd_tail(ops, name):
    _, N, D, H, W, C0, Cout, bits = _row(TAIL_CASES, name)
    ok = ops.conv3d_fwd_tail_ok(C0, Cout, N, D, H, W, BF)
    assert ok & 1, "fmri_conv3d_fwd_tail_ok says no to %s on this device" % name
    if name == "narrow_32":
        assert ok & 2, "fmri_conv3d_fwd_tail_ok: no logits tail for narrow_32 (three outputs wanted)"
    audit(_tail_run(ops, N, D, H, W, C0, Cout, ok, False))


def test_b_conv3d_fwd_tail_planar(ops):
    _, S, H, W, C0, Cout, act, bits = _row(PLANAR_TAIL_CASES, "narrow_32")
    ok = ops.conv3d_fwd_tail_ok(C0, Cout, 1, S, H, W, BF, planar=True)
    assert ok == 3, "fmri_conv3d_fwd_tail_planar_ok says %d for narrow_32" % ok
    audit(_tail_run(ops, 1, S, H, W, C0, Cout, ok, True))


def _stats_ref(y, G):
    """(sums, magnitudes) [G, C, 2] of a stored tensor in fp64 on the device (test_gpu_ops.py:482-484)"""
    C = y.shape[-1]
    yd = y.double().reshape(G, -1, C)
    return torch.stack([yd.sum(1), (yd * yd).sum(1)], dim=-1), torch.stack([yd.abs().sum(1), (yd * yd).sum(1)], dim=-1)


def _stats_bar(r, G, C, what):
    """the stats-tail bar of test_gpu_ops.py:485-487 (conv) and :512 (upcat): error relative to the sum of magnitudes <= 2e-6"""
    ref, scale = _stats_ref(r["y"], G)
    err = float(((r["totals"].view(G, C, 2) - ref).abs() / scale).max())
    assert err <= 2e-6, (what, err)


@pytest.mark.parametrize("per", [0, 1])
def test_b_conv3d_fwd_stats_exact_workspace(ops, per):
    N, D, H, W, Cin, Cout = NTAIL_CASES[0]
    assert ops.conv3d_fwd_ntail_ok(Cin, 0, Cout, N, D, H, W, BF), "fmri_conv3d_fwd_ntail_ok says no"
    G = N if per else 1
    nd = ops.norm_tail_ws_doubles(G, Cout)

    def run(a):
        x = a.input(rnd((N, D, H, W, Cin), 300, BF), name="x")
        w = a.input(rnd((27, Cout, Cin), 301, BF, scale=0.06), name="w")
        b = a.input(rnd((Cout,), 302, F32), offset16=True, name="bias")
        y = a.output((N, D, H, W, Cout), BF, name="y")
        # zero on entry; on exit the totals [G][Cout][2] in front hold the sums, everything behind them is zero again
        ws = a.workspace(nd * 8, zero=True, dtype=torch.float64, keep_front=G * Cout * 2 * 8, name="ws")
        ops.conv3d_fwd_stats(x, None, w, b, y, ws, per, act=0)
        return {"y": y, "totals": ws[:G * Cout * 2]}
    r0, r1 = audit(run, loose=("totals",))
    _stats_bar(r0, G, Cout, "plain")
    _stats_bar(r1, G, Cout, "arena")


@pytest.mark.parametrize("per", [0, 1])
def test_b_upcat_fwd_stats_exact_workspace(ops, per):
    N, D, H, W, C0, C1, Cout = 2, 16, 64, 64, 64, 32, 128          # test_gpu_ops.py:492
    assert ops.conv3d_upcat_ok(C0, C1, Cout, D, H, W, BF) & 1, "fmri_conv3d_upcat_ok says no"
    assert ops.conv3d_fwd_ntail_ok(C1, 0, Cout, N, D, H, W, BF), "fmri_conv3d_fwd_ntail_ok says no"
    G = N if per else 1
    nd = ops.norm_tail_ws_doubles(G, Cout)

    def run(a):
        xl = a.input(rnd((N, D // 2, H // 2, W // 2, C0), 310, BF), name="x_low")
        xs = a.input(rnd((N, D, H, W, C1), 311, BF), name="x_skip")
        w = a.input(rnd((27, Cout, C0 + C1), 312, F32, scale=0.05), offset16=True, name="w_master")
        up_f = a.output((8, 8, Cout, C0), BF, name="up_f")
        sk_f = a.output((27, Cout, C1), BF, name="sk_f")
        ops.conv3d_pack_up_weights(w, C0, C1, up_f, None, sk_f, None)
        b = a.input(rnd((Cout,), 313, F32), offset16=True, name="bias")
        y = a.output((N, D, H, W, Cout), BF, name="y")
        ws = a.workspace(nd * 8, zero=True, dtype=torch.float64, keep_front=G * Cout * 2 * 8, name="ws")
        ops.conv3d_upcat_fwd_stats(xl, xs, up_f, sk_f, b, y, ws, per, act=0)
        return {"y": y, "up_f": up_f, "sk_f": sk_f, "totals": ws[:G * Cout * 2]}
    r0, r1 = audit(run, loose=("totals",))
    _stats_bar(r0, G, Cout, "plain")
    _stats_bar(r1, G, Cout, "arena")


@pytest.mark.parametrize("mode", ["batch", "instance"])
def test_b_dgrad_norm_tail_exact_workspace(ops, mode):
    """fmri_conv3d_dgrad_norm + fmri_norm_act_bwd_pre on NTAIL_CASES[1]: dz bit for bit; the sums {sum dz, sum dz x} under the bar of
    test_gpu_ops.py:555-557 (<= 2e-6 of the sum of magnitudes); dx / dgamma / dbeta of the reader, which follow from those sums, both
    runs against the separate passes under the ReLU bar of test_gpu_ops.py:564-565 (dx 2e-4, dgamma / dbeta 1e-5, relative norms).  The
    reader leaves the whole workspace zero."""
    N, D, H, W, Cdy, Cx = NTAIL_CASES[1]
    per = mode == "instance"
    G = N if per else 1
    assert ops.conv3d_fwd_ntail_ok(Cdy, 0, Cx, N, D, H, W, BF), "fmri_conv3d_fwd_ntail_ok says no"
    nd = ops.norm_tail_ws_doubles(G, Cx)
    # the first block's forward statistics: made once, outside the audited calls
    x0 = rnd((N, D, H, W, Cx), 320, BF, scale=1.3) + 0.2
    gamma0 = rnd((Cx,), 321, F32) * 0.5 + 1.0
    beta0 = rnd((Cx,), 322, F32) * 0.3
    stats0, nss0 = zeros((G, Cx, 3)), torch.empty((G, Cx, 2), device="cuda")
    ops.norm_act_fwd(x0, gamma0, beta0, torch.empty_like(x0), stats0, zeros((G, Cx, 2), torch.float64), per, eps=1e-3, eps_on_std=per, act=1)
    ops.norm_scale_shift(stats0, gamma0, beta0, nss0)
    dy0, wd0 = rnd((N, D, H, W, Cdy), 323, BF), rnd((27, Cx, Cdy), 324, BF, scale=0.05)
    # the reference of the existing test: the separate passes fmri_conv3d_dgrad + fmri_norm_act_bwd_x on the same tensors (test_gpu_ops.py:538-542)
    g0 = torch.empty_like(x0)
    ops.conv3d_dgrad(dy0, wd0, g0)
    dx0, dg0, db0 = torch.empty_like(x0), zeros(Cx), zeros(Cx)
    ops.norm_act_bwd(x0, None, g0, gamma0, stats0, dx0, dg0, db0, zeros((G, Cx, 2), torch.float64), per, act=1, beta=beta0)

    def run(a):
        x = a.input(x0, name="x")
        dy2 = a.input(dy0, name="dy")
        wd = a.input(wd0, name="w_dgrad")
        nss = a.input(nss0, name="nss")
        gamma = a.input(gamma0, offset16=True, name="gamma")
        stats = a.input(stats0, name="stats")
        dz = a.output((N, D, H, W, Cx), BF, name="dz")
        ws = a.workspace(nd * 8, zero=True, dtype=torch.float64, name="ws")
        ops.conv3d_dgrad_norm(dy2, wd, x, nss, dz, ws, per, act=1)
        totals = ws[:G * Cx * 2].clone()
        tail_zero = (ws[G * Cx * 2:] == 0).all().reshape(1)
        dx = a.output((N, D, H, W, Cx), BF, name="dx")
        dg = a.accumulate(zeros(Cx), offset16=True, name="dgamma")
        db = a.accumulate(zeros(Cx), offset16=True, name="dbeta")
        ops.norm_act_bwd_pre(x, dz, gamma, stats, dx, dg, db, ws[:G * Cx * 2], per)
        return {"dz": dz, "totals": totals, "tail_zero": tail_zero, "dx": dx, "dgamma": dg, "dbeta": db}
    r0, r1 = audit(run, loose=("totals", "dx", "dgamma", "dbeta"))
    assert bool(r0["tail_zero"]) and bool(r1["tail_zero"]), "the per-workgroup blocks behind the totals were not folded and cleared"
    xd = x0.double().reshape(G, -1, Cx)
    for r, tag in ((r0, "plain"), (r1, "arena")):
        dzd = r["dz"].double().reshape(G, -1, Cx)
        ref = torch.stack([dzd.sum(1), (dzd * xd).sum(1)], dim=-1)
        scale = torch.stack([dzd.abs().sum(1), (dzd * xd).abs().sum(1)], dim=-1)
        assert float(((r["totals"].view(G, Cx, 2) - ref).abs() / (scale + 1e-30)).max()) <= 2e-6, tag
    rel = lambda p, q: float((p.double() - q.double()).norm() / q.double().norm())
    for r, tag in ((r0, "plain"), (r1, "arena")):
        e = (rel(r["dx"], dx0), rel(r["dgamma"], dg0), rel(r["dbeta"], db0))
        assert e[0] <= 2e-4 and e[1] <= 1e-5 and e[2] <= 1e-5, (tag, e)


# ================================================================================================ C. input gradients
# Edge: the same halo as A on dy, the packed images' tails (Cin = 192 is three 64-blocks, 5 x 7 none), fp32 master weights at 16 bytes.
@pytest.mark.parametrize("dtype,Cin,Cout,impl", [(F32, 5, 7, 1), (BF, 32, 64, 2), (BF, 64, 32, 2), (BF, 192, 64, 2)])      # test_gpu_ops.py:128
def test_c_pack_and_dgrad(ops, dtype, Cin, Cout, impl):
    N, D, H, W = 1, 4, 8, 16

    def run(a):
        wm = a.input(rnd((27, Cout, Cin), 12, F32, scale=0.2), offset16=True, name="w_master")
        wf = a.output((27, Cout, Cin), dtype, name="w_fwd")
        wd = a.output((27, Cin, Cout), dtype, name="w_dgrad")
        ops.pack_weights(wm, wf, wd)
        dy = a.input(rnd((N, D, H, W, Cout), 13, dtype), name="dy")
        mask = a.input(rnd((N, D, H, W, Cin), 14, dtype), name="mask")
        dx = a.output((N, D, H, W, Cin), dtype, name="dx")
        ops.conv3d_dgrad(dy, wd, dx, mask=mask, impl=impl)
        return {"w_fwd": wf, "w_dgrad": wd, "dx": dx}
    audit(run)


@pytest.mark.parametrize("name", ["planar_generic_f32", "planar_mfma_32"])
def test_c_planar_dgrad(ops, name):
    _, dtype, S, H, W, C0, up0, C1, Cout, impl = _row(PLANAR_CASES, name)

    def run(a):
        wm = a.input(rnd((27, Cout, C0), 3, dtype, scale=0.2).float(), offset16=True, name="w_master")
        wd = a.output((27, C0, Cout), dtype, name="w_dgrad")
        ops.pack_weights(wm, None, wd)
        dy = a.input(rnd((1, S, H, W, Cout), 12, dtype), name="dy")
        dx = a.output((1, S, H, W, C0), dtype, name="dx")
        ops.conv3d_dgrad(dy, wd, dx, impl=impl, planar=True)
        return {"w_dgrad": wd, "dx": dx}
    audit(run)


# smallest row of each kind of test_gpu_first_dgrad.py:23: one minimal tile per input-channel count 1 / 2, 64 output channels with 3, two samples with 4
@pytest.mark.parametrize("case", [c for c in FIRST_DGRAD_CASES if c in ((1, 32, 1, 4, 16, 32), (2, 32, 1, 4, 16, 32), (3, 64, 1, 8, 16, 32), (4, 32, 2, 4, 32, 32))],
                         ids=lambda c: "c%d_o%d_n%d_%dx%dx%d" % c)
def test_c_first_layer_dgrad(ops, case):
    Cin, Cout, N, D, H, W = case
    assert ops.conv3d_first_dgrad_ok(Cin, Cout, D, H, W, BF), "fmri_conv3d_first_dgrad_ok says no"

    def run(a):
        dy = a.input(rnd((N, D, H, W, Cout), 700 + Cin + Cout, BF), name="dy")
        w = a.input(rnd((27, Cout, Cin), 710 + Cin + Cout, BF, scale=0.2), name="w_fwd")
        dx = a.output((N, D, H, W, Cin), F32, name="dx")
        ops.conv3d_first_dgrad(dy, w, dx)
        return {"dx": dx}
    audit(run)


# ================================================================================================ D. weight gradients
# Edge: a dw column past dw_ld / a db lane past Cout lands in the next layer's parameters (dw, db at 16 bytes, accumulated into); the slab
# flush writes combos * nslab * ... floats into a workspace of exactly fmri_conv3d_wgrad_workspace_bytes.
def _ref_wgrad(src0, src1, up0, dy, planar=False):
    x = ref_concat_input(f64(src0), None if src1 is None else f64(src1), up0, planar)
    Cout, C = dy.shape[-1], x.shape[1]
    wk = torch.zeros((Cout, C, 3, 3, 3), dtype=torch.float64, requires_grad=True)
    F.conv3d(x, wk, None, padding=1).backward(to_ncdhw(f64(dy)))
    g = planar_kernel(wk.grad) if planar else wk.grad
    return g.permute(2, 3, 4, 0, 1).reshape(27, Cout, C), f64(dy).sum(dim=(0, 1, 2, 3))


def _wgrad_case(ops, dtype, N, D, H, W, C0, up0, C1, Cout, impl, planar, with_ws, tol, what):
    s0 = (N, D // (1 if planar else 2), H // 2, W // 2, C0) if up0 else (N, D, H, W, C0)
    t = {"src0": rnd(s0, 9, dtype), "src1": rnd((N, D, H, W, C1), 10, dtype) if C1 else None, "dy": rnd((N, D, H, W, Cout), 11, dtype),
         "dw0": rnd((27, Cout, C0 + C1), 15, F32), "db0": rnd((Cout,), 16, F32)}          # dw / db are accumulated INTO
    nws = ops.conv3d_wgrad_workspace_bytes(C0, C1, Cout, N, D, H, W, dtype, planar) if with_ws else 0
    if with_ws:
        assert nws > 0, "fmri_conv3d_wgrad_workspace_bytes: %s does not take the slab path" % what

    def run(a):
        src0 = a.input(t["src0"], name="src0")
        src1 = a.input(t["src1"], name="src1") if C1 else None
        dy = a.input(t["dy"], name="dy")
        dw = a.accumulate(t["dw0"], offset16=True, name="dw")
        db = a.accumulate(t["db0"], offset16=True, name="db")
        ws = a.workspace(nws, dtype=F32, name="slab_workspace") if with_ws else None
        ops.conv3d_wgrad(src0, src1, dy, dw, db, up0=up0, impl=impl, planar=planar, workspace=ws)
        return {"dw": dw, "db": db}
    r0, r1 = audit(run, loose=("dw", "db"))
    rdw, rdb = _ref_wgrad(t["src0"], t["src1"], up0, t["dy"], planar)
    both_close(r0, r1, "dw", rdw + f64(t["dw0"]), *tol, what=what + " dw")
    both_close(r0, r1, "db", rdb + f64(t["db0"]), *tol, what=what + " db")
    return r0, r1


def test_d_wgrad_generic_f32(ops):
    """bar: WG_TOL[fp32] (test_gpu_ops.py:21, used at :123-125)"""
    name, dtype, N, D, H, W, C0, up0, C1, Cout, impl = _row(CONV_CASES, "generic_odd_f32")
    _wgrad_case(ops, dtype, N, D, H, W, C0, up0, C1, Cout, impl, False, False, WG_TOL[dtype], name)


@pytest.mark.parametrize("name", ["mfma_32_64", "mfma_dual_up", "mfma_deep_256"])          # rows test_conv3d_wgrad does not skip (Cout % 64 == 0, W % 16 == 0)
@pytest.mark.parametrize("with_ws", [False, True], ids=["atomic_flush", "slab_flush_exact_workspace"])
def test_d_wgrad_mfma(ops, name, with_ws):
    """bars: WG_TOL[bf16] against fp64 (test_gpu_ops.py:123-125) for both flushes; the slab flush is ordered (test_gpu_ops.py:116 asserts two
    launches equal), so its dw is also the same bits in the arena as on plain tensors"""
    _, dtype, N, D, H, W, C0, up0, C1, Cout, impl = _row(CONV_CASES, name)
    r0, r1 = _wgrad_case(ops, dtype, N, D, H, W, C0, up0, C1, Cout, impl, False, with_ws, WG_TOL[dtype], name)
    if with_ws:
        from footprint import assert_same
        assert_same(r1["dw"], r0["dw"], name + " slab-flush dw")


def test_d_wgrad_slab_vs_atomic(ops):
    """the 1e-6 / 1e-6 slab-vs-atomic bar of test_gpu_ops.py:117, with the slab workspace exact and guarded"""
    _, dtype, N, D, H, W, C0, up0, C1, Cout, impl = _row(CONV_CASES, "mfma_32_64")
    nws = ops.conv3d_wgrad_workspace_bytes(C0, C1, Cout, N, D, H, W, dtype)
    assert nws > 0

    def run(a):
        src0 = a.input(rnd((N, D, H, W, C0), 9, dtype), name="src0")
        dy = a.input(rnd((N, D, H, W, Cout), 11, dtype), name="dy")
        dw_a, db_a = a.accumulate(zeros((27, Cout, C0)), offset16=True, name="dw_atomic"), a.accumulate(zeros(Cout), offset16=True, name="db_atomic")
        dw_s, db_s = a.accumulate(zeros((27, Cout, C0)), offset16=True, name="dw_slab"), a.accumulate(zeros(Cout), offset16=True, name="db_slab")
        ops.conv3d_wgrad(src0, None, dy, dw_a, db_a, impl=impl)
        ops.conv3d_wgrad(src0, None, dy, dw_s, db_s, impl=impl, workspace=a.workspace(nws, dtype=F32, name="slab_workspace"))
        return {"dw_atomic": dw_a, "dw_slab": dw_s}
    r0, r1 = audit(run, loose=("dw_atomic",))
    for r in (r0, r1):
        assert_close(r["dw_slab"], r["dw_atomic"], 1e-6, 1e-6, what="slab vs atomic")


def test_d_wgrad_f32_mfma(ops):
    """fp32 planes on the MFMA path always use the atomic flush; bar 2e-5 / 2e-5 (test_gpu_f32_mfma.py:181-182), smallest row of its WG"""
    from fmri_hip._lib import IMPL_MFMA, lib
    name, N, D, H, W, C0, C1, Cout = min(F32_WG, key=lambda c: c[1] * c[2] * c[3] * c[4] * (c[5] + c[6]) * c[7])
    assert lib().fmri_conv3d_uses_mfma(C0, C1, Cout, D, H, W, 0) & 2, "fmri_conv3d_uses_mfma says no"
    _wgrad_case(ops, F32, N, D, H, W, C0, name.startswith("fused_upsampling"), C1, Cout, IMPL_MFMA, False, False, (2e-5, 2e-5), "f32 " + name)


def test_d_wgrad_planar_mfma(ops):
    """bar: WG_TOL[bf16] (test_gpu_ops.py:323-325)"""
    name, dtype, S, H, W, C0, up0, C1, Cout, impl = _row(PLANAR_CASES, "planar_mfma")
    _wgrad_case(ops, dtype, 1, S, H, W, C0, up0, C1, Cout, impl, True, False, WG_TOL[dtype], name)


def _upcat_tensors(N, D, H, W, C0, C1, Cout, planar, seed):
    lo = (N, D, H // 2, W // 2, C0) if planar else (N, D // 2, H // 2, W // 2, C0)
    return {"x_low": rnd(lo, seed, BF), "x_skip": rnd((N, D, H, W, C1), seed + 1, BF) if C1 else None,
            "w": rnd((27, Cout, C0 + C1), seed + 2, BF, scale=0.05).float().contiguous(), "bias": rnd((Cout,), seed + 3, F32),
            "dy": rnd((N, D, H, W, Cout), seed + 4, BF), "m_low": rnd(lo, seed + 5, BF).clamp_min(0),
            "m_skip": rnd((N, D, H, W, C1), seed + 6, BF).clamp_min(0) if C1 else None}


def _upcat_dims(table, name, planar):
    if planar:
        _, S, H, W, C0, C1, Cout = _row(table, name)
        return 1, S, H, W, C0, C1, Cout
    return _row(table, name)[1:]


UPCAT_ROWS = [(UPCAT_CASES, "one_tile", False), (UPCAT_CASES, "narrow_cout", False), (UPCAT2D_CASES, "one_tile", True), (UPCAT2D_CASES, "no_skip", True)]
UPCAT_IDS = ["3d_one_tile", "3d_narrow_cout", "2d_one_tile", "2d_no_skip"]


@pytest.mark.parametrize("table,name,planar", UPCAT_ROWS, ids=UPCAT_IDS)
def test_d_upcat_wgrad_exact_scratch(ops, table, name, planar):
    """dwc_scratch of exactly 64 * Cout * C0 (planar: 16 * Cout * C0) floats, "overwritten": it starts as NaN.  Bar 4e-6 / 4e-6 against the
    fp64 autograd of the plain definition (test_gpu_ops.py:750-751, 2-D :850-852)."""
    N, D, H, W, C0, C1, Cout = _upcat_dims(table, name, planar)
    ok = ops.conv3d_upcat_ok(C0, C1, Cout, D, H, W, BF, planar=planar)
    if name == "narrow_cout":
        # Cout = 96 is no multiple of the weight-gradient kernel's 64-wide tile (test_gpu_ops.py:740, :854): the library refuses the call, and
        # a refused call must not touch anything either
        assert not ok & 2
    else:
        assert ok & 2, "fmri_conv%dd_upcat_ok: no weight-gradient route for %s" % (2 if planar else 3, name)
    t = _upcat_tensors(N, D, H, W, C0, C1, Cout, planar, 21 if planar else 1)
    dw0, db0 = rnd((27, Cout, C0 + C1), 30, F32), rnd((Cout,), 31, F32)

    def run(a):
        xl = a.input(t["x_low"], name="x_low")
        xs = a.input(t["x_skip"], name="x_skip") if C1 else None
        dy = a.input(t["dy"], name="dy")
        dw = a.accumulate(dw0, offset16=True, name="dw")
        db = a.accumulate(db0, offset16=True, name="db")
        dwc = a.workspace((16 if planar else 64) * Cout * C0 * 4, dtype=F32, name="dwc_scratch")
        if ok & 2:
            ops.conv3d_upcat_wgrad(xl, xs, dy, dw, db, dwc, planar=planar)
        else:
            with pytest.raises(RuntimeError):
                ops.conv3d_upcat_wgrad(xl, xs, dy, dw, db, dwc, planar=planar)
        return {"dw": dw, "db": db}
    r0, r1 = audit(run, loose=("dw", "db") if ok & 2 else ())
    if not ok & 2:
        return
    xl, xs = f64(t["x_low"]), (f64(t["x_skip"]) if C1 else None)
    if planar:
        up = xl[0].permute(0, 3, 1, 2).repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
        inp = up if xs is None else torch.cat([up, xs[0].permute(0, 3, 1, 2)], dim=1)
        kern = torch.zeros((Cout, C0 + C1, 3, 3), dtype=torch.float64, requires_grad=True)
        F.conv2d(inp, kern, None, padding=1).backward(f64(t["dy"])[0].permute(0, 3, 1, 2))
        ref = f64(dw0).clone()
        ref[9:18] += kern.grad.permute(2, 3, 0, 1).reshape(9, Cout, C0 + C1)          # only the centre kd plane exists
    else:
        kern = torch.zeros((Cout, C0 + C1, 3, 3, 3), dtype=torch.float64, requires_grad=True)
        F.conv3d(ref_concat_input(xl, xs, True), kern, None, padding=1).backward(to_ncdhw(f64(t["dy"])))
        ref = f64(dw0) + kern.grad.permute(2, 3, 4, 0, 1).reshape(27, Cout, C0 + C1)
    both_close(r0, r1, "dw", ref, 4e-6, 4e-6, what=name + " dw")
    both_close(r0, r1, "db", f64(db0) + f64(t["dy"]).sum(dim=(0, 1, 2, 3)), 4e-6, 4e-6, what=name + " db")


def test_d_upcat_wgrad_parts(ops):
    """fmri_conv3d_upcat_wgrad_parts: dwc [8, 8, Cout, C0] is an OUTPUT here (zeroed by the call, then summed into with atomics): every
    element written, nothing behind it.  Bar: the parity gradients against the fp64 sums they are defined as would need the fold's algebra;
    both runs are compared with each other under the 4e-6 / 4e-6 of test_gpu_ops.py:750, and dw's skip columns / db against fp64 autograd."""
    _, N, D, H, W, C0, C1, Cout = _row(UPCAT_CASES, "one_tile")
    assert ops.conv3d_upcat_ok(C0, C1, Cout, D, H, W, BF) & 2, "fmri_conv3d_upcat_ok: no weight-gradient route"
    t = _upcat_tensors(N, D, H, W, C0, C1, Cout, False, 1)

    def run(a):
        xl, xs, dy = a.input(t["x_low"], name="x_low"), a.input(t["x_skip"], name="x_skip"), a.input(t["dy"], name="dy")
        dw = a.accumulate(zeros((27, Cout, C0 + C1)), offset16=True, name="dw")
        db = a.accumulate(zeros(Cout), offset16=True, name="db")
        dwc = a.output((8, 8, Cout, C0), F32, name="dwc")
        ops.conv3d_upcat_wgrad_parts(xl, xs, dy, dw, db, dwc)
        return {"dw": dw, "db": db, "dwc": dwc}
    r0, r1 = audit(run, loose=("dw", "db", "dwc"))
    assert_close(r1["dwc"], r0["dwc"], 4e-6, 4e-6, what="dwc arena vs plain")
    kern = torch.zeros((Cout, C0 + C1, 3, 3, 3), dtype=torch.float64, requires_grad=True)
    F.conv3d(ref_concat_input(f64(t["x_low"]), f64(t["x_skip"]), True), kern, None, padding=1).backward(to_ncdhw(f64(t["dy"])))
    ref = kern.grad.permute(2, 3, 4, 0, 1).reshape(27, Cout, C0 + C1)
    for r, tag in ((r0, "plain"), (r1, "arena")):
        assert_close(r["dw"][..., C0:], ref[..., C0:], 4e-6, 4e-6, what="parts: skip columns of dw (%s)" % tag)
        assert float(r["dw"][..., :C0].abs().max()) == 0.0, "parts: the up-sampled columns of dw belong to dwc"
        assert_close(r["db"], f64(t["dy"]).sum(dim=(0, 1, 2, 3)), 4e-6, 4e-6, what="parts: db (%s)" % tag)


# ================================================================================================ E. parity and transposed forms
# Edge: 8 (4) parity classes store interleaved voxels of y; the low-resolution halo of x_low; ceil-sized outputs of strided convs; dy as a
# channel slice of a wider tensor.
@pytest.mark.parametrize("table,name,planar", UPCAT_ROWS, ids=UPCAT_IDS)
def test_e_upcat_fwd_and_dgrad(ops, table, name, planar):
    N, D, H, W, C0, C1, Cout = _upcat_dims(table, name, planar)
    assert ops.conv3d_upcat_ok(C0, C1, Cout, D, H, W, BF, planar=planar) & 1, "fmri_conv%dd_upcat_ok says no to %s" % (2 if planar else 3, name)
    t = _upcat_tensors(N, D, H, W, C0, C1, Cout, planar, 21 if planar else 1)
    n = 4 if planar else 8

    def run(a):
        w = a.input(t["w"], offset16=True, name="w_master")
        up_f, up_d = a.output((n, n, Cout, C0), BF, name="up_f"), a.output((n, n, C0, Cout), BF, name="up_d")
        sk_f = a.output((27, Cout, C1), BF, name="sk_f") if C1 else None
        sk_d = a.output((27, C1, Cout), BF, name="sk_d") if C1 else None
        ops.conv3d_pack_up_weights(w, C0, C1, up_f, up_d, sk_f, sk_d, planar=planar)
        xl = a.input(t["x_low"], name="x_low")
        xs = a.input(t["x_skip"], name="x_skip") if C1 else None
        bias = a.input(t["bias"], offset16=True, name="bias")
        y = a.output((N, D, H, W, Cout), BF, name="y")
        ops.conv3d_upcat_fwd(xl, xs, up_f, sk_f, bias, y, act=1, planar=planar)
        dy = a.input(t["dy"], name="dy")
        m_low = a.input(t["m_low"], name="m_low")
        m_skip = a.input(t["m_skip"], name="m_skip") if C1 else None
        dx_low = a.output(t["x_low"].shape, BF, name="dx_low")
        dx_skip = a.output(t["x_skip"].shape, BF, name="dx_skip") if C1 else None
        ops.conv3d_upcat_dgrad(dy, up_d, sk_d, m_low, m_skip, dx_low, dx_skip, planar=planar)
        out = {"up_f": up_f, "up_d": up_d, "y": y, "dx_low": dx_low}
        if C1:
            out.update({"sk_f": sk_f, "sk_d": sk_d, "dx_skip": dx_skip})
        return out
    audit(run)


def test_e_stride2_conv(ops):
    """test_gpu_ops.py:412, first row: the gather launch over the input, 27 of the 64 (parity, block offset) slots"""
    from fmri_hip.strided_parity import StridedParity
    N, D, H, W, Cin, Cout = 1, 16, 32, 64, 32, 64
    assert ops.conv3d_upcat_ok(Cout, 0, Cin, D, H, W, BF) & 1, "fmri_conv3d_upcat_ok says no"
    sp = StridedParity("cuda")
    w = rnd((27, Cout, Cin), 3, F32, scale=0.1)
    img = torch.zeros((8, 8, Cout, Cin), device="cuda", dtype=BF)
    sp.pack(w, img, torch.zeros((8, 8, Cin, Cout), device="cuda", dtype=BF))

    def run(a):
        x = a.input(rnd((N, D, H, W, Cin), 1, BF), name="x")
        wi = a.input(img, name="w_s2_fwd")
        b = a.input(rnd((Cout,), 4, F32), offset16=True, name="bias")
        y = a.output((N, D // 2, H // 2, W // 2, Cout), BF, name="y")
        ops.conv3d_stride2_fwd(x, wi, b, y)
        return {"y": y}
    audit(run)


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("planar", [False, True], ids=["3d", "planar"])
def test_e_deconv_k2s2(ops, dtype, planar):
    """test_gpu_ops.py:570; dy is the channel slice [4, 4 + Cout) of a wider tensor whose other columns are NaN.  dw / db: accumulated with
    atomics - bars (1e-4, 1e-5) fp32 / (2e-5, 2e-5) bf16 of test_gpu_ops.py:599-602, both runs against fp64 autograd."""
    N, D, H, W, Cin, Cout = 2, 3, 4, 5, 12, 8
    D2 = D if planar else 2 * D
    x0 = torch.relu(rnd((N, D, H, W, Cin), 90, dtype))
    w0, dy0 = rnd((8, Cout, Cin), 91, dtype, scale=0.3), rnd((N, D2, 2 * H, 2 * W, Cout + 4), 93, dtype)

    def run(a):
        x = a.input(x0, name="x")
        w = a.input(w0, name="w")
        b = a.input(rnd((Cout,), 92, F32), offset16=True, name="bias")
        y = a.output((N, D2, 2 * H, 2 * W, Cout), dtype, name="y")
        ops.deconv_fwd(x, w, b, y, planar=planar)
        dyfull = a.input(dy0, name="dy_wide")
        a.slot(dyfull[..., 4:], dyfull)
        dx = a.output((N, D, H, W, Cin), dtype, name="dx")
        dw = a.accumulate(zeros((8, Cout, Cin)), offset16=True, name="dw")
        db = a.accumulate(zeros(Cout), offset16=True, name="db")
        ops.deconv_bwd(x, w, dyfull, dx, dw, db, dy_off=4, xmask=x, planar=planar)
        return {"y": y, "dx": dx, "dw": dw, "db": db}
    r0, r1 = audit(run, loose=("dw", "db"))
    tolw = (1e-4, 1e-5) if dtype == F32 else (2e-5, 2e-5)
    # fp64 autograd of the transposed convolution, as test_gpu_ops.py:579-588, :597
    xr, wr, br = to_ncdhw(f64(x0)), f64(w0).requires_grad_(True), torch.zeros(Cout, dtype=torch.float64, requires_grad=True)
    if planar:
        kern = wr[:4].reshape(2, 2, Cout, Cin).permute(3, 2, 0, 1)
        yr = F.conv_transpose2d(xr.permute(0, 2, 1, 3, 4).reshape(N * D, Cin, H, W), kern, br, stride=2)
        yr = yr.reshape(N, D, Cout, 2 * H, 2 * W).permute(0, 2, 1, 3, 4)
    else:
        yr = F.conv_transpose3d(xr, wr.reshape(2, 2, 2, Cout, Cin).permute(4, 3, 0, 1, 2), br, stride=2)
    yr.backward(to_ncdhw(f64(dy0)[..., 4:]))
    nt = 4 if planar else 8
    for r, tag in ((r0, "plain"), (r1, "arena")):
        assert_close(r["dw"][:nt], wr.grad[:nt], *tolw, what="deconv dw (%s)" % tag)
        assert_close(r["db"], br.grad, *tolw, what="deconv db (%s)" % tag)


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("k,s,dims", [(1, 1, (3, 4, 5)), (3, 2, (4, 6, 8)), (3, 2, (5, 7, 6)), (3, 1, (3, 4, 5))])          # test_gpu_ops.py:606
def test_e_conv_direct(ops, dtype, k, s, dims):
    """odd dims with stride 2 give ceil-sized outputs.  dw / db meet in atomics: bars of test_gpu_ops.py:635-638, both runs against the fp64
    autograd of the TensorFlow-'same' convolution (test_gpu_ops.py:617-624, :633)."""
    N, Cin, Cout = 2, 6, 5
    D, H, W = dims
    od = tuple(-(-n // s) for n in dims)
    x0, w0, dy0 = rnd((N, D, H, W, Cin), 100, dtype), rnd((k ** 3, Cout, Cin), 101, dtype, scale=0.3), rnd((N,) + od + (Cout,), 103, dtype)

    def run(a):
        x = a.input(x0, name="x")
        w = a.input(w0, name="w")
        b = a.input(rnd((Cout,), 102, F32), offset16=True, name="bias")
        y = a.output((N,) + od + (Cout,), dtype, name="y")
        ops.conv_direct_fwd(x, w, b, y, k, s, act=0)
        dy = a.input(dy0, name="dy")
        dx = a.output((N, D, H, W, Cin), dtype, name="dx")
        dw = a.accumulate(zeros((k ** 3, Cout, Cin)), offset16=True, name="dw")
        db = a.accumulate(zeros(Cout), offset16=True, name="db")
        ops.conv_direct_bwd(x, w, dy, dx, dw, db, k, s)
        return {"y": y, "dx": dx, "dw": dw, "db": db}
    r0, r1 = audit(run, loose=("dw", "db"))
    tolw = (1e-4, 1e-5) if dtype == F32 else (2e-5, 2e-5)
    wr, br = f64(w0).requires_grad_(True), torch.zeros(Cout, dtype=torch.float64, requires_grad=True)
    pads = []
    for n_, o_ in zip(reversed(dims), reversed(od)):           # F.pad wants (w_before, w_after, h_before, h_after, d_before, d_after)
        tot = max((o_ - 1) * s + k - n_, 0)
        pads += [tot // 2, tot - tot // 2]
    yr = F.conv3d(F.pad(to_ncdhw(f64(x0)), pads), wr.reshape(k, k, k, Cout, Cin).permute(3, 4, 0, 1, 2), br, stride=s)
    yr.backward(to_ncdhw(f64(dy0)))
    both_close(r0, r1, "dw", wr.grad, *tolw, what="direct dw")
    both_close(r0, r1, "db", br.grad, *tolw, what="direct db")


# ================================================================================================ F. pooling and up-sampling
# Edge: pick_vec(C) chooses the vector width from C alone (C = 1, 6 scalar / 2-wide tails, 16, 64 full vectors); the `add` / `y` / `dy`
# tensors are channel slices of wider rows; odd extents leave trailing planes that the backward must zero and nothing else.
POOL_WINDOWS = [("2x2x2", None, False), ("planar_1x2x2", None, True), ("generic_2x2x1", (2, 2, 1), False)]


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("C", [1, 6, 16, 64])
@pytest.mark.parametrize("wname,pool,planar", POOL_WINDOWS, ids=[w[0] for w in POOL_WINDOWS])
def test_f_maxpool_fwd_bwd(ops, dtype, C, wname, pool, planar):
    N, D, H, W = 2, 4, 6, 8                                                   # test_gpu_ops.py:153
    pd, ph, pw = pool if pool else ((1, 2, 2) if planar else (2, 2, 2))
    with_add = wname == "2x2x2"                                               # the backward once with an `add` slice (add_ld > add_off + C)

    def run(a):
        x = a.input(torch.relu(rnd((N, D, H, W, C), 20, dtype)), name="x")
        y = a.output((N, D // pd, H // ph, W // pw, C), dtype, name="y")
        ops.maxpool_fwd(x, y, planar=planar, pool=pool)
        dy = a.input(rnd(tuple(y.shape), 21, dtype), name="dy")
        dx = a.output((N, D, H, W, C), dtype, name="dx")
        if with_add:
            add = a.input(rnd((N, D, H, W, C + 8 + 3), 22, dtype), name="add_wide")
            a.slot(add[..., 8:8 + C], add)
            ops.maxpool_bwd(x, dy, dx, add=add, add_off=8, relu_mask=True, planar=planar, pool=pool)
        else:
            ops.maxpool_bwd(x, dy, dx, relu_mask=True, planar=planar, pool=pool)
        return {"y": y, "dx": dx}
    audit(run)


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_f_upsample_column_slots(ops, dtype):
    N, D, H, W, C = 2, 2, 3, 4, 8                                             # test_gpu_ops.py:173

    def run(a):
        x = a.input(rnd((N, D, H, W, C), 30, dtype), name="x")
        y = a.output((N, 2 * D, 2 * H, 2 * W, C + 4 + 2), dtype, name="y_wide")
        a.slot(y[..., 4:4 + C], y)
        ops.upsample_fwd(x, y, y_off=4)
        dy = a.input(rnd((N, 2 * D, 2 * H, 2 * W, C + 4 + 2), 31, dtype), name="dy_wide")
        a.slot(dy[..., 4:4 + C], dy)
        dx = a.output((N, D, H, W, C), dtype, name="dx")
        ops.upsample_bwd(dy, dx, dy_off=4, xmask=x)
        return {"y": y[..., 4:4 + C], "dx": dx}
    audit(run)


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", [(1, 5, 7, 6, 3), (3, 5, 4, 3, 7)], ids=["1x5x7x6x3", "3x5x4x3x7"])          # test_gpu_adversarial.py:28, :48
def test_f_avgpool_and_global_avgpool_odd_shapes(ops, dtype, shape):
    N, D, H, W, C = shape

    def run(a):
        x = a.input(rnd(shape, 1, dtype), name="x")
        y = a.output((N, D // 2, H // 2, W // 2, C), dtype, name="y")
        ops.avgpool_fwd(x, y)
        dy = a.input(rnd(tuple(y.shape), 2, dtype), name="dy")
        dx = a.output(shape, dtype, name="dx")
        ops.avgpool_bwd(dy, dx)
        g = a.output((N, C), F32, name="gap")
        ops.global_avgpool_fwd(x, g)
        dg = a.input(rnd((N, C), 4, F32), name="dgap")
        dxg = a.output(shape, dtype, name="dx_gap")
        ops.global_avgpool_bwd(dg, dxg)
        return {"y": y, "dx": dx, "gap": g, "dx_gap": dxg}
    audit(run)


# ================================================================================================ G. normalisation
# Edge: gamma / beta / dgamma / dbeta live in the flat parameter and gradient buffers (16 bytes); ws [G][C][2] is zero on entry and must be
# zero on exit; C = 512 is 64 channel groups x 4 voxel lanes per workgroup.
def _norm_ref(x, gamma, beta, per, act, alpha, dy):
    from oracle import unet_oracle as O
    xr = to_ncdhw(f64(x)).requires_grad_(True)
    gr, br = f64(gamma).requires_grad_(True), f64(beta).requires_grad_(True)
    z = O._instancenorm(xr, gr, br) if per else O._batchnorm_train(xr, gr, br)
    yr = F.relu(z) if act == 1 else F.leaky_relu(z, alpha)
    yr.backward(to_ncdhw(f64(dy)))
    return to_ndhwc(yr.detach()), to_ndhwc(xr.grad), gr.grad, br.grad


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("mode", ["batch", "instance"])
@pytest.mark.parametrize("C", [16, 512])
def test_g_norm_act_fwd_bwd(ops, dtype, mode, C):
    """fmri_norm_act_fwd / _bwd / _bwd_x sharing one ws.  Their workgroups' fp64 partial sums meet in ws with atomics (include/fmri_hip.h,
    "Ordered normalisation statistics"), so both runs are held against the fp64 oracle under the bars of test_gpu_ops.py:390 (forward),
    :400 (dx, dgamma, dbeta) and :406-407 (the form that reads x: the same dx bits, dgamma within 1e-6)."""
    N, D, H, W = 2, 4, 6, 8                                                   # test_gpu_ops.py:374
    act, alpha = 2, 0.3
    per = mode == "instance"
    G = N if per else 1
    t = {"x": rnd((N, D, H, W, C), 80, dtype, scale=1.5) + 0.3, "gamma": rnd((C,), 81, F32) * 0.5 + 1.0, "beta": rnd((C,), 82, F32) * 0.2,
         "dy": rnd((N, D, H, W, C), 83, dtype)}

    def run(a):
        x, dy = a.input(t["x"], name="x"), a.input(t["dy"], name="dy")
        gamma, beta = a.input(t["gamma"], offset16=True, name="gamma"), a.input(t["beta"], offset16=True, name="beta")
        stats = a.output((G, C, 3), F32, name="stats")
        ws = a.workspace(G * C * 2 * 8, zero=True, dtype=torch.float64, name="ws")
        y = a.output((N, D, H, W, C), dtype, name="y")
        ops.norm_act_fwd(x, gamma, beta, y, stats, ws, per, eps=1e-3, eps_on_std=per, act=act, alpha=alpha)
        dx, dx2 = a.output((N, D, H, W, C), dtype, name="dx"), a.output((N, D, H, W, C), dtype, name="dx_from_x")
        dg, db = a.accumulate(zeros(C), offset16=True, name="dgamma"), a.accumulate(zeros(C), offset16=True, name="dbeta")
        dg2, db2 = a.accumulate(zeros(C), offset16=True, name="dgamma_from_x"), a.accumulate(zeros(C), offset16=True, name="dbeta_from_x")
        ops.norm_act_bwd(x, y, dy, gamma, stats, dx, dg, db, ws, per, act=act, alpha=alpha)
        ops.norm_act_bwd(x, None, dy, gamma, stats, dx2, dg2, db2, ws, per, act=act, alpha=alpha, beta=beta)
        return {"y": y, "stats": stats, "dx": dx, "dgamma": dg, "dbeta": db, "dx_from_x": dx2, "dgamma_from_x": dg2, "dbeta_from_x": db2}
    r0, r1 = audit(run, loose=("y", "stats", "dx", "dgamma", "dbeta", "dx_from_x", "dgamma_from_x", "dbeta_from_x"))
    ry, rdx, rdg, rdb = _norm_ref(t["x"], t["gamma"], t["beta"], per, act, alpha, t["dy"])
    tol = (1e-4, 1e-5) if dtype == F32 else (5e-3, 2e-4)
    tolb = (2e-4, 2e-5) if dtype == F32 else (6e-3, 2e-3)
    both_close(r0, r1, "y", ry, *tol, what="norm fwd")
    both_close(r0, r1, "dx", rdx, *tolb, what="norm dx")
    both_close(r0, r1, "dgamma", rdg, *tolb, what="norm dgamma")
    both_close(r0, r1, "dbeta", rdb, *tolb, what="norm dbeta")
    for r in (r0, r1):
        assert torch.equal(r["dx_from_x"], r["dx"])
        assert_close(r["dgamma_from_x"], r["dgamma"], 1e-6, 1e-6, what="norm dgamma (from x)")


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("mode", ["batch", "instance"])
@pytest.mark.parametrize("C", [16, 512])
def test_g_norm_pre_forms(ops, dtype, mode, C):
    """fmri_norm_act_fwd_pre / _bwd_pre read the sums a conv tail left in ws and clear them: given the same sums they are ordered kernels
    (one reader per (group, channel)), so the arena run equals the plain run bit for bit.  The sums are put there in fp64 by the test."""
    N, D, H, W = 2, 4, 6, 8
    per = mode == "instance"
    G = N if per else 1
    x0 = rnd((N, D, H, W, C), 80, dtype, scale=1.5) + 0.3
    dz0 = rnd((N, D, H, W, C), 84, dtype)
    xd, dzd = x0.double().reshape(G, -1, C), dz0.double().reshape(G, -1, C)
    sums_f = torch.stack([xd.sum(1), (xd * xd).sum(1)], dim=-1).reshape(-1)
    sums_b = torch.stack([dzd.sum(1), (dzd * xd).sum(1)], dim=-1).reshape(-1)

    def run(a):
        x, dz = a.input(x0, name="x"), a.input(dz0, name="dz")
        gamma = a.input(rnd((C,), 81, F32) * 0.5 + 1.0, offset16=True, name="gamma")
        beta = a.input(rnd((C,), 82, F32) * 0.2, offset16=True, name="beta")
        stats = a.output((G, C, 3), F32, name="stats")
        ws = a.workspace(G * C * 2 * 8, zero=True, dtype=torch.float64, name="ws")
        y = a.output((N, D, H, W, C), dtype, name="y")
        ws.copy_(sums_f)
        ops.norm_act_fwd_pre(x, gamma, beta, y, stats, ws, per, eps=1e-3, eps_on_std=per, act=1)
        cleared = (ws == 0).all().reshape(1)
        dx = a.output((N, D, H, W, C), dtype, name="dx")
        dg, db = a.accumulate(zeros(C), offset16=True, name="dgamma"), a.accumulate(zeros(C), offset16=True, name="dbeta")
        ws.copy_(sums_b)
        ops.norm_act_bwd_pre(x, dz, gamma, stats, dx, dg, db, ws, per)
        return {"y": y, "stats": stats, "cleared_by_fwd_pre": cleared, "dx": dx, "dgamma": dg, "dbeta": db}
    r0, r1 = audit(run)
    assert bool(r0["cleared_by_fwd_pre"]) and bool(r1["cleared_by_fwd_pre"])


def test_g_norm_scale_shift_and_moving_update(ops):
    G, C = 2, 19                                                              # C no multiple of anything
    M = 4 * 6 * 8.0

    def run(a):
        st = torch.rand((G, C, 3), generator=torch.Generator().manual_seed(7)).cuda() + 0.5
        stats = a.input(st, name="stats")
        gamma = a.input(rnd((C,), 81, F32) * 0.5 + 1.0, offset16=True, name="gamma")
        beta = a.input(rnd((C,), 82, F32) * 0.2, offset16=True, name="beta")
        nss = a.output((G, C, 2), F32, name="nss")
        ops.norm_scale_shift(stats, gamma, beta, nss)
        mm = a.inout(rnd((C,), 85, F32), offset16=True, name="moving_mean")
        mv = a.inout(rnd((C,), 86, F32).abs() + 0.1, offset16=True, name="moving_var")
        ops.norm_moving_update(stats, mm, mv, M)
        return {"nss": nss, "moving_mean": mm, "moving_var": mv}
    audit(run)


# ================================================================================================ H. pointwise, losses, optimizers
# Edge: float4 / scalar tails (n = 1, 3, 4, 5, 7, 1027, 4099); an optimizer tail that steps one element too far trains the next layer's bias.
@pytest.mark.parametrize("n", [1, 7, 4099])
def test_h_add_channel_scale_cast(ops, n):
    def run(a):
        out = {}
        for dtype, tag in ((BF, "bf16"), (F32, "f32")):
            p, q = a.input(rnd((n,), 110, dtype), name="a_" + tag), a.input(rnd((n,), 111, dtype), name="b_" + tag)
            y = a.output((n,), dtype, name="sum_" + tag)
            ops.add(p, q, y)
            xs = a.input(rnd((1, n, 1), 112, dtype), name="x_" + tag)
            sc = a.input(rnd((1, 1), 113, F32), name="scale_" + tag)
            z = a.output((1, n, 1), dtype, name="scaled_" + tag)
            ops.channel_scale(xs, sc, z)
            out.update({"sum_" + tag: y, "scaled_" + tag: z})
        xc = a.input(rnd((2, n, 3), 114, BF), name="x_cs")                                # [N][V][C] with C = 3: scale row per sample
        sc = a.input(rnd((2, 3), 115, F32), name="scale_cs")
        zc = a.output((2, n, 3), BF, name="scaled_cs")
        ops.channel_scale(xc, sc, zc)
        src = a.input(rnd((n,), 116, F32), name="cast_src")
        d16, d32 = a.output((n,), BF, name="cast_bf16"), a.output((n,), F32, name="cast_back")
        ops.cast(src, d16)
        ops.cast(d16, d32)
        out.update({"scaled_cs": zc, "cast_bf16": d16, "cast_back": d32})
        return out
    audit(run)


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("C,L", [(64, 1), (16, 2), (6, 1)])                   # test_gpu_ops.py:189
def test_h_conv1x1(ops, dtype, C, L):
    """the final conv's w / b / dw / db at 16 bytes; 1001 voxels.  dw / db meet in atomics: bar (1e-4, 1e-5) against fp64, test_gpu_ops.py:207-208"""
    nv = 1001
    t = {"x": torch.relu(rnd((nv, C), 40, dtype)), "w": rnd((L, C), 41, F32), "dl": rnd((nv, L), 43, F32)}

    def run(a):
        x = a.input(t["x"], name="x")
        w, b = a.input(t["w"], offset16=True, name="w"), a.input(rnd((L,), 42, F32), offset16=True, name="b")
        logits = a.output((nv, L), F32, name="logits")
        ops.conv1x1_fwd(x, w, b, logits)
        dl = a.input(t["dl"], name="dlogits")
        dx = a.output((nv, C), dtype, name="dx")
        dw, db = a.accumulate(zeros((L, C)), offset16=True, name="dw"), a.accumulate(zeros(L), offset16=True, name="db")
        ops.conv1x1_bwd(x, w, dl, dx, dw, db, relu_mask=True)
        return {"logits": logits, "dx": dx, "dw": dw, "db": db}
    r0, r1 = audit(run, loose=("dw", "db"))
    both_close(r0, r1, "dw", f64(t["dl"]).T @ f64(t["x"]), 1e-4, 1e-5, what="conv1x1 dw")
    both_close(r0, r1, "db", f64(t["dl"]).sum(0), 1e-4, 1e-5, what="conv1x1 db")


def _loss_ref_grad(logits, y, kind, param, weight=None):
    """fp64 autograd of the selectable losses (test_gpu_ops.py:673-682; weighted cross-entropy :872-879)"""
    z = f64(logits).requires_grad_(True)
    p, t = torch.sigmoid(z), f64(y)
    dice = lambda a, b: (2 * (a * b).sum() + 1) / (a.sum() + b.sum() + 1)
    pc = p.clamp(1e-7, 1 - 1e-7)
    bce = -(t * torch.log(pc) + (1 - t) * torch.log(1 - pc))
    xent = (bce if weight is None else f64(weight) * bce).mean()
    L = {0: lambda: -dice(t, p), 1: lambda: xent, 2: lambda: -dice(t, p) + param * xent,
         3: lambda: -(0.5 * (1 - p) ** 2 * torch.log(p))[t == 1].sum() - (0.5 * p ** 2 * torch.log(1 - p))[t == 0].sum(),
         4: lambda: -((t * p).sum() + 1) / (t.sum() + p.sum() - (t * p).sum() + 1), 5: lambda: -dice(t, p) + param * dice(1 - t, p)}[kind]()
    L.backward()
    return z.grad, float(dice(t, p).detach())


def _loss_inputs(n, seed):
    logits = rnd((n,), seed, F32, scale=2.0)
    y = (torch.rand(n, generator=torch.Generator().manual_seed(seed + 1)) > 0.7).to(torch.uint8).cuda()
    weight = torch.exp(-torch.rand(n, generator=torch.Generator().manual_seed(seed + 2)).cuda() * 3.0)
    return logits, y, weight


@pytest.mark.parametrize("n", [4096, 4099], ids=["vector_4096", "scalar_4099"])
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
def test_h_sigmoid_dice(ops, n, weighted):
    """probs bit for bit; the 16 sums meet in fp64 atomics: Dice from them to 1e-6 relative (test_gpu_ops.py:225), the gradient that reads
    them under (1e-4, 1e-5) against fp64 autograd (test_gpu_ops.py:234; weighted: :882)"""
    logits0, y0, w0 = _loss_inputs(n, 50)

    def run(a):
        logits, y = a.input(logits0, name="logits"), a.input(y0, name="y_true")
        wgt = a.input(w0, name="weight") if weighted else None
        probs = a.output((n,), F32, name="probs")
        sums = a.accumulate(zeros(16, torch.float64), name="sums")
        ops.sigmoid_dice_fwd(logits, y, probs, sums, weight=wgt)
        dl = a.output((n,), F32, name="dlogits")
        if weighted:
            ops.sigmoid_loss_bwd(probs, y, sums, dl, 2, param=0.7, weight=wgt)
        else:
            ops.sigmoid_dice_bwd(probs, y, sums, dl)
        return {"probs": probs, "sums": sums, "dlogits": dl}
    r0, r1 = audit(run, loose=("sums", "dlogits"))
    g, dice = _loss_ref_grad(logits0, y0, 2 if weighted else 0, 0.7, w0 if weighted else None)
    both_close(r0, r1, "dlogits", g, 1e-4, 1e-5, what="dice bwd")
    for r in (r0, r1):
        s = r["sums"].cpu().numpy()
        assert (2 * s[0] + 1) / (s[1] + s[2] + 1) == pytest.approx(dice, rel=1e-6) and s[7] == n


@pytest.mark.parametrize("kind,param", [(0, 1.0), (1, 1.0), (2, 1.0), (3, 1.0), (4, 1.0), (5, 10.0)])          # test_gpu_ops.py:653
def test_h_selectable_losses(ops, kind, param):
    """n = 4099; bar (2e-4, 2e-5) against fp64 autograd, test_gpu_ops.py:683"""
    n = 4099
    logits0, y0, _ = _loss_inputs(n, 120)

    def run(a):
        logits, y = a.input(logits0, name="logits"), a.input(y0, name="y_true")
        probs = a.output((n,), F32, name="probs")
        sums = a.accumulate(zeros(16, torch.float64), name="sums")
        ops.sigmoid_dice_fwd(logits, y, probs, sums)
        dl = a.output((n,), F32, name="dlogits")
        ops.sigmoid_loss_bwd(probs, y, sums, dl, kind, param)
        return {"probs": probs, "dlogits": dl}
    r0, r1 = audit(run, loose=("dlogits",))
    both_close(r0, r1, "dlogits", _loss_ref_grad(logits0, y0, kind, param)[0], 2e-4, 2e-5, what="loss kind %d" % kind)


def test_h_label_sums_and_weighted_dice(ops):
    """fmri_label_sums: lsums [3 L] overwritten, bound nvox * 2^-53 relative (test_gpu_multilabel.py:156-158).  fmri_weighted_dice_fwd / _bwd on
    the shape of test_gpu_losses.py:66: value within 2e-6, gradient within 2e-6 of its maximum (test_gpu_losses.py:90, :93)."""
    N, sp, L = 3, (4, 6, 5), 3
    rs = np.random.RandomState(5)
    logits = rs.randn(N, *sp, L).astype(np.float32)
    yn = (rs.rand(N, *sp, L) > 0.7).astype(np.uint8)
    yn[1] = 0
    nvox = N * sp[0] * sp[1] * sp[2]
    p0 = torch.sigmoid(torch.from_numpy(logits).cuda().reshape(-1))
    y0 = torch.from_numpy(yn).cuda().reshape(-1)

    def run(a):
        probs, y = a.input(p0, name="probs"), a.input(y0, name="y_true")
        lsums = a.output((3 * L,), torch.float64, name="lsums")
        ops.label_sums(probs, y, L, lsums)
        gs = a.output((3 * N * L,), torch.float64, name="gsums")
        sums = a.accumulate(zeros(16, torch.float64), name="sums")
        ops.weighted_dice_fwd(probs, y, gs, sums, N, L)
        dl = a.output((nvox * L,), F32, name="dlogits")
        ops.weighted_dice_bwd(probs, y, gs, sums, dl, N, L, grad_scale=1.0)
        return {"lsums": lsums, "gsums": gs, "sums": sums, "dlogits": dl}
    r0, r1 = audit(run, loose=("lsums", "gsums", "sums", "dlogits"))
    p64, y64 = p0.double().cpu().numpy().reshape(nvox, L), yn.astype(np.float64).reshape(nvox, L)
    ref = np.stack([(y64 * p64).sum(axis=0), y64.sum(axis=0), p64.sum(axis=0)], axis=1)
    pt = p0.double().cpu().reshape(N, -1, L).requires_grad_(True)
    yt = torch.from_numpy(y64).reshape(N, -1, L)
    s = 1e-5
    coef = (2.0 * ((yt * pt).sum(1) + s / 2) / (yt.sum(1) + pt.sum(1) + s)).mean()
    (-coef).backward()
    coef = coef.detach()
    g_ref = (pt.grad * pt.detach() * (1 - pt.detach())).reshape(-1).numpy()              # d/dlogits through the sigmoid
    for r, tag in ((r0, "plain"), (r1, "arena")):
        rel = np.abs(r["lsums"].cpu().numpy().reshape(L, 3) - ref) / ref
        assert rel.max() <= nvox * 2.0 ** -53, (tag, rel.max())
        got = -ops.loss_value_from_sums(r["sums"].cpu().numpy(), ops.LOSS_WEIGHTED_DICE)
        assert abs(got - float(coef)) < 2e-6, (tag, got, float(coef))
        g = r["dlogits"].cpu().numpy().astype(np.float64)
        assert np.abs(g - g_ref).max() <= 2e-6 * np.abs(g_ref).max() + 1e-12, tag


OPT_N = [1, 3, 4, 5, 1027]


def _flat(a, n, seed, name, positive=False):
    """a range of a flat fp32 buffer at a 16-byte-aligned offset: what lies behind it is the next layer's"""
    t = rnd((n,), seed, F32)
    return a.inout(t.abs() if positive else t, offset16=True, name=name)


@pytest.mark.parametrize("n", OPT_N)
def test_h_adam(ops, n):
    def run(a):
        p, m, v = _flat(a, n, 60, "p"), _flat(a, n, 61, "m"), _flat(a, n, 62, "v", positive=True)
        g = a.input(rnd((n,), 63, F32), offset16=True, name="g")
        ops.adam_step(p, g, m, v, 1e-3 * math.sqrt(1 - 0.999) / (1 - 0.9))
        return {"p": p, "m": m, "v": v}
    audit(run)


@pytest.mark.parametrize("n", OPT_N)
def test_h_adam_ex_amsgrad_clipnorm_and_grad_sumsq(ops, n):
    """fmri_grad_sumsq with a workspace of exactly fmri_grad_sumsq_workspace_bytes() ("any contents": it starts as NaN), its norm read on the
    device by the clipping AMSGrad step"""
    from fmri_hip._lib import lib
    nws = int(lib().fmri_grad_sumsq_workspace_bytes())

    def run(a):
        p, m, v, vhat = _flat(a, n, 60, "p"), _flat(a, n, 61, "m"), _flat(a, n, 62, "v", True), _flat(a, n, 64, "vhat", True)
        g = a.input(rnd((n,), 63, F32), offset16=True, name="g")
        work = a.workspace(nws, dtype=torch.float64, name="grad_sumsq_workspace")
        out = a.output((2,), torch.float64, name="sumsq_and_norm")
        ops.grad_sumsq(g, 0.5, work, out)
        ops.adam_step_ex(p, g, m, v, vhat, 1e-3, grad_scale=0.5, gnorm=out, clipnorm=0.25)
        return {"p": p, "m": m, "v": v, "vhat": vhat, "sumsq_and_norm": out}
    audit(run)


@pytest.mark.parametrize("n", OPT_N)
def test_h_sgd_and_rmsprop(ops, n):
    def run(a):
        g = a.input(rnd((n,), 63, F32), offset16=True, name="g")
        p0, m0, p1, m1, p2, m2 = _flat(a, n, 60, "p_plain"), _flat(a, n, 61, "m_plain"), _flat(a, n, 60, "p_momentum"), _flat(a, n, 61, "m_momentum"), \
            _flat(a, n, 60, "p_nesterov"), _flat(a, n, 61, "m_nesterov")
        ops.sgd_step(p0, g, m0, 1e-2)                         # momentum 0 still keeps its moment buffer (m <- v), as Keras does
        ops.sgd_step(p1, g, m1, 1e-2, momentum=0.9)
        ops.sgd_step(p2, g, m2, 1e-2, momentum=0.9, nesterov=True, clipvalue=0.5)
        p3, a3 = _flat(a, n, 60, "p_rmsprop"), _flat(a, n, 62, "a_rmsprop", True)
        ops.rmsprop_step(p3, g, a3, 1e-3)
        return {"p_plain": p0, "m_plain": m0, "p_momentum": p1, "m_momentum": m1, "p_nesterov": p2, "m_nesterov": m2, "p_rmsprop": p3, "a_rmsprop": a3}
    audit(run)


# ================================================================================================ I. tiled prediction
# Edge: an odd volume 19 x 23 x 17 with 8 x 8 x 8 patches in all eight corners (and one inside): the last row of the last patch ends on the
# volume's last element; 17 is no multiple of any store width.
VOL = (19, 23, 17)
PATCH = (8, 8, 8)


def _corners():
    idx = [[x, y, z] for x in (0, VOL[0] - PATCH[0]) for y in (0, VOL[1] - PATCH[1]) for z in (0, VOL[2] - PATCH[2])] + [[5, 7, 3]]
    return torch.tensor(idx, dtype=torch.int32).cuda()


def test_i_tile_gather_scatter_finalize(ops):
    idx0 = _corners()
    B, C = idx0.shape[0], 2

    def run(a):
        vol = a.input(rnd(VOL, 70, F32), name="volume")
        aux = a.input(rnd(VOL, 71, F32), name="aux_volume")
        idx = a.input(idx0, name="corners")
        t32, t16 = a.output((B,) + PATCH, F32, name="tiles_f32"), a.output((B,) + PATCH, BF, name="tiles_bf16")
        ops.tile_gather(vol, idx, PATCH, t32)
        ops.tile_gather(vol, idx, PATCH, t16)
        st = a.output((B, PATCH[0], PATCH[1], PATCH[2] + 3), BF, name="tiles_stacked")          # 11 channels: 2-byte stores
        ops.tile_gather_stack(vol, aux, idx, PATCH, -3, 3, st)
        pred = a.input(rnd((B,) + PATCH + (C,), 72, F32), name="pred")
        acc = a.accumulate(zeros(VOL + (C,), torch.float64), name="acc")
        cnt = a.accumulate(zeros(VOL, torch.int32), name="cnt")
        ops.tile_scatter_accumulate(pred, idx, PATCH, acc, cnt)
        out = a.output(VOL + (C,), torch.float64, name="mean")
        bad = a.accumulate(zeros(1, torch.int32), name="bad")
        ops.tile_finalize(acc, cnt, out, bad)
        return {"tiles_f32": t32, "tiles_bf16": t16, "tiles_stacked": st, "acc": acc, "cnt": cnt, "mean": out, "bad": bad}
    r0, _ = audit(run)
    assert int(r0["bad"]) > 0 and int(r0["cnt"].max()) >= 2          # the patches leave holes and overlap: both paths of the division ran


@pytest.mark.parametrize("mask", [0, 5, 7])
def test_i_pad_flip_finalize_flip_labels(ops, mask):
    lo = (2, 1, 3)
    PAD = (24, 25, 21)
    g = torch.Generator().manual_seed(9)
    cnt0 = torch.randint(0, 4, PAD, generator=g, dtype=torch.int32).cuda()
    lab0 = torch.randint(0, 6, VOL, generator=g, dtype=torch.uint8).cuda()

    def run(a):
        src = a.input(rnd(VOL, 73, F32).double(), name="volume_f64")
        dst = a.output(PAD, F32, name="padded")
        ops.volume_pad_flip(src, dst, lo, mask, -3.0)
        acc = a.input(rnd(PAD + (3,), 74, F32).double(), name="acc")
        cnt = a.input(cnt0, name="cnt")
        out = a.output(VOL + (3,), torch.float64, name="mean_window")
        bad = a.accumulate(zeros(1, torch.int32), name="bad")
        ops.tile_finalize_flip(acc, cnt, out, bad, lo, mask)
        labels = a.output(PAD, torch.uint8, name="label_map")
        bad2 = a.accumulate(zeros(1, torch.int32), name="bad_labels")
        ops.tile_finalize_labels(acc, cnt, labels, bad2, 0.1, [3, 1, 4])
        lab = a.input(lab0, name="labels_in")
        onehot = a.output(VOL + (3,), torch.uint8, name="one_hot")
        ops.labels_expand_u8(lab, [3, 1, 4], out=onehot)
        return {"padded": dst, "mean_window": out, "bad": bad, "label_map": labels, "bad_labels": bad2, "one_hot": onehot}
    audit(run)


# ================================================================================================ J. strided slots of the patch sampler
# Edge: out_ld / row strides.  The slot's sibling columns carry the sentinel and must keep it bit for bit.
def test_j_affine_sample_slot(ops):
    th = 0.3
    A = np.eye(4)
    A[:2, :2] = [[math.cos(th), -math.sin(th)], [math.sin(th), math.cos(th)]]
    A[:3, 3] = [1.5, -2.0, 0.25]                                              # part of the patch samples outside the volume (cval)
    size, ld, off = (8, 9, 5), 9, 2

    def run(a):
        vol = a.input(rnd((12, 10, 9), 4, F32), name="volume")
        lab = a.input((rnd((12, 10, 9), 5, F32) > 0).to(torch.uint8), name="label_volume")
        wide = a.output((size[0], size[1], ld), F32, name="patch_wide")
        a.slot(wide[..., off:off + size[2]], wide)
        ops.affine_sample(vol, A, (2, 1, 3), size, wide[..., off:off + size[2]], order=1, cval=-1.0, out_ld=ld)
        wl = a.output((size[0], size[1], ld), torch.uint8, name="labels_wide")
        a.slot(wl[..., off:off + size[2]], wl)
        ops.affine_sample(lab, A, (2, 1, 3), size, wl[..., off:off + size[2]], order=0, cval=0.0, out_ld=ld)
        return {"patch": wide[..., off:off + size[2]], "labels": wl[..., off:off + size[2]]}
    audit(run)


def test_j_elastic_warp_and_piecewise_affine_slots(ops):
    B, X, Y, C, ld, off = 2, 13, 11, 3, 7, 2
    d0 = rnd((B, 2, X, Y), 6, F32, scale=1.5)

    def run(a):
        srcw = a.input(rnd((B, X, Y, ld), 7, F32), name="src_wide")
        a.slot(srcw[..., off:off + C], srcw)
        d = a.input(d0, name="fields")
        outw = a.output((B, X, Y, ld), F32, name="warped_wide")
        a.slot(outw[..., off:off + C], outw)
        ops.elastic_warp_batch(srcw[..., off:off + C], d, 1, outw[..., off:off + C])
        pw = a.output((X, Y, ld), F32, name="piecewise_wide")
        a.slot(pw[..., off:off + C], pw)
        ops.piecewise_affine(srcw[0, :, :, off:off + C], [[0.5, 1.0], [0.0, Y - 2.0], [X - 1.5, 0.5], [X - 1.0, Y - 1.0]], 1, pw[..., off:off + C])
        return {"warped": outw[..., off:off + C], "piecewise": pw[..., off:off + C]}
    audit(run)


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_j_coarse_dropout_rng_batch_slot(ops, dtype):
    B, X, Y, C, ld, off = 2, 13, 11, 3, 6, 1
    x0 = rnd((B, X, Y, ld), 8, dtype)
    own = x0[..., off:off + C].float().reshape(B, -1)
    st0 = torch.stack([own.min(1).values, own.max(1).values], dim=1).contiguous()

    def run(a):
        xw = a.inout(x0, name="patches_wide")
        a.slot(xw[..., off:off + C], xw)
        stats = a.input(st0, name="stats")
        ops.coarse_dropout_rng_batch(xw[..., off:off + C], [[3, 4], [2, 2]], 0.3, stats, True, 1234, [1, 2])
        return {"patches": xw[..., off:off + C]}
    r0, _ = audit(run)
    assert not torch.equal(r0["patches"], x0[..., off:off + C]), "the dropout dropped nothing: the case exercises no store"
