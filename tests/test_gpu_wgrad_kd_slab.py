"""The kd-sharing weight-gradient kernel with the slab flush (csrc/conv3d_wgrad.hip: k_conv_wgrad_kd<false, true> + k_wgrad_reduce_kd) at the
small shapes where its unit walk takes every branch: one unit per plane, fewer units than slabs, slabs that start in the middle of a column
and end at its top, D = 8 with two columns per sample, a slab length that does not divide the unit count, one slab for the whole launch,
and a workspace too small for one slab (the per-kd route must take over).  impl = IMPL_MFMA_KD_SLAB forces the route.

Data are dyadic (k / 8, |k| <= 8): every product is a multiple of 1/64 and a gradient element sums at most 4,096 of them, each at most 1 in
size - 18 significant bits, exact in fp32 in ANY summation order.  The result must therefore equal torch.nn.grad.conv3d_weight in fp64 on
the host BIT FOR BIT; there is no tolerance on dyadic data.  Random bf16 data use the bars of tests/test_gpu_ops.py::test_conv3d_wgrad.

The route taken is proven, not assumed: the workspace is pre-filled with NaN, and the floats a call leaves finite must be exactly the
slabs x blocks x 27 x 32 x 32 the slab rule (wgrad_slab_index.h: slab_count) gives for this device - none where the call must fall back.

Every case runs in a process of its own under a time limit (a fault in one case cannot take the next ones with it); the fp64 references
are computed once per shape in the pytest process and shared by the cases of that shape."""
import functools
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

BLOCK_FLOATS = 27 * 32 * 32
# name: (N, D, H, W, C0, C1, Cout, workspace, data, mode)
#   workspace  "query": fmri_conv3d_wgrad_workspace_bytes;  ("slabs", n): exactly n slabs of partial sums;  "short": 4 bytes less than one slab
#   mode       "plain" | "repeat" (three calls, same bits; equals the per-kd slab route) | "det" (deterministic mode) | "upcat" (parity route:
#              the skip half writes columns [C0, C0 + C1) of a wider dw; FMRI_WGRAD_KD_SLAB_MIN_GFLOP=0 sends it down the route)
CASES = {
    "one_unit_per_plane_64_64": (1, 4, 8, 16, 64, 0, 64, "query", "dyadic", "plain"),
    "one_unit_per_plane_32_64": (1, 4, 8, 16, 32, 0, 64, "query", "dyadic", "plain"),
    "8x16x32_64_64": (1, 8, 16, 32, 64, 0, 64, "query", "dyadic", "plain"),
    "8x16x32_64_64_five_slabs_mid_column": (1, 8, 16, 32, 64, 0, 64, ("slabs", 5), "dyadic", "plain"),        # per = 7 of 32 units, D = 8
    "two_columns_d8_128_128": (2, 8, 16, 16, 128, 0, 128, "query", "dyadic", "plain"),
    "two_columns_d8_128_128_three_slabs": (2, 8, 16, 16, 128, 0, 128, ("slabs", 3), "dyadic", "plain"),      # per = 11: crosses columns and samples
    "256_256_queried_workspace": (1, 8, 16, 16, 256, 0, 256, "query", "dyadic", "plain"),
    "256_256_one_slab": (1, 8, 16, 16, 256, 0, 256, ("slabs", 1), "dyadic", "plain"),
    "256_256_fall_back": (1, 8, 16, 16, 256, 0, 256, "short", "dyadic", "plain"),
    "two_sources_64_64": (1, 8, 16, 32, 64, 64, 64, "query", "dyadic", "plain"),
    "upcat_skip_half_wider_dw": (1, 8, 16, 32, 64, 64, 64, ("slabs", 5), "dyadic", "upcat"),
    "random_8x16x32_64_64": (1, 8, 16, 32, 64, 0, 64, ("slabs", 5), "random", "plain"),
    "random_256_256": (1, 8, 16, 16, 256, 0, 256, "query", "random", "plain"),
    "repeat_dyadic_128_128": (2, 8, 16, 16, 128, 0, 128, ("slabs", 3), "dyadic", "repeat"),
    "repeat_random_64_64": (1, 8, 16, 32, 64, 0, 64, ("slabs", 5), "random", "repeat"),
    "deterministic_mode_64_64": (1, 8, 16, 32, 64, 0, 64, ("slabs", 5), "dyadic", "det"),
}
WG_TOL = (2e-6, 2e-6)            # tests/test_gpu_ops.py WG_TOL[bfloat16]: fp32 sums of exact bf16 products


def make_inputs(case):
    """host tensors of a case, the same in the pytest process (reference) and in the worker (device run): x0 / x1 NDHWC, dy"""
    N, D, H, W, C0, C1, Cout, _, data, mode = CASES[case]
    g = torch.Generator().manual_seed(1234 + 7 * C0 + C1 + 3 * Cout + D * H * W)
    low = mode == "upcat"

    def draw(shape):
        if data == "dyadic":
            return (torch.randint(-8, 9, shape, generator=g).to(torch.float32) / 8).to(torch.bfloat16)
        return torch.randn(*shape, generator=g).to(torch.bfloat16)
    x0 = draw((N, D // 2, H // 2, W // 2, C0) if low else (N, D, H, W, C0))
    x1 = draw((N, D, H, W, C1)) if C1 else None
    dy = draw((N, D, H, W, Cout))
    return x0, x1, dy


def _inputs_key(case):
    c = CASES[case]
    return c[:7] + (c[8], c[9] == "upcat")          # make_inputs depends on nothing else


@functools.lru_cache(maxsize=None)
def reference(key):
    """fp64 weight and bias gradient on the host, once per set of inputs: [27][Cout][Cin] and [Cout]"""
    case = next(c for c in CASES if _inputs_key(c) == key)
    N, D, H, W, C0, C1, Cout, _, _, mode = CASES[case]
    x0, x1, dy = make_inputs(case)
    a = x0.to(torch.float64).permute(0, 4, 1, 2, 3)
    if mode == "upcat":
        for ax in (2, 3, 4):
            a = torch.repeat_interleave(a, 2, dim=ax)
    if x1 is not None:
        a = torch.cat([a, x1.to(torch.float64).permute(0, 4, 1, 2, 3)], dim=1)
    g = dy.to(torch.float64).permute(0, 4, 1, 2, 3).contiguous()
    dw = torch.nn.grad.conv3d_weight(a.contiguous(), (Cout, C0 + C1, 3, 3, 3), g, padding=1)
    return dw.permute(2, 3, 4, 0, 1).reshape(27, Cout, C0 + C1).contiguous(), g.sum(dim=(0, 2, 3, 4))


def reference_of(case):
    return reference(_inputs_key(case))           # cases that differ only in workspace or mode share one reference


@pytest.mark.parametrize("case", list(CASES), ids=list(CASES))
def test_kd_slab_route(case, tmp_path):
    out = str(tmp_path / "out.pt")
    env = {k: v for k, v in os.environ.items() if not k.startswith("FMRI_WGRAD")}
    if CASES[case][9] == "upcat":
        env["FMRI_WGRAD_KD_SLAB_MIN_GFLOP"] = "0"
    p = subprocess.run([sys.executable, os.path.abspath(__file__), case, out], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=300)
    print(p.stdout)
    assert p.returncode == 0, "%s: the worker ended with %d\n%s" % (case, p.returncode, p.stdout[-4000:])
    got = torch.load(out)
    dw_ref, db_ref = reference_of(case)
    data = CASES[case][8]
    for name, g, r in (("dw", got["dw"], dw_ref), ("db", got["db"], db_ref)):
        err = float((g.to(torch.float64) - r).abs().max())
        print("%s %s: max |got - fp64| = %.3e, max |fp64| = %.3e" % (case, name, err, float(r.abs().max())))
        if data == "dyadic":
            assert torch.equal(g.to(torch.float64), r), "%s: %s differs from the fp64 gradient on dyadic data (max error %.3e)" % (case, name, err)
        else:
            tol = WG_TOL[1] * float(r.abs().max()) + WG_TOL[0] * r.abs()
            assert bool(((g.to(torch.float64) - r).abs() <= tol).all()), "%s: %s outside rtol %.0e atol %.0e (max error %.3e)" % ((case, name) + WG_TOL + (err,))


# ------------------------------------------------------------------------------------------------------------------------ the worker
def _expected_slabs(ncu, nblocks, ws_bytes, nunits):
    return max(0, min((2 * ncu) // nblocks, ws_bytes // (nblocks * BLOCK_FLOATS * 4), nunits))


def worker(case, out):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "fetal-mri-segmentation_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from fmri_hip import ops
    from fmri_hip._lib import IMPL_MFMA, IMPL_MFMA_KD_SLAB
    N, D, H, W, C0, C1, Cout, wsk, data, mode = CASES[case]
    x0, x1, dy = (None if t is None else t.cuda() for t in make_inputs(case))
    Cin = C0 + C1
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    nunits = N * D * (H // 8) * (W // 16)
    # the launch of the route: the whole call, or the skip half of the parity route (its own Cin, a wider dw)
    lC = C1 if mode == "upcat" else Cin
    nblocks = (Cout // 32) * (lC // 32)
    query = ops.conv3d_wgrad_workspace_bytes(C1, 0, Cout, N, D, H, W, torch.bfloat16) if mode == "upcat" else \
        ops.conv3d_wgrad_workspace_bytes(C0, C1, Cout, N, D, H, W, torch.bfloat16)
    assert query > 0
    ws_bytes = query if wsk == "query" else (nblocks * BLOCK_FLOATS * 4 - 4 if wsk == "short" else wsk[1] * nblocks * BLOCK_FLOATS * 4)
    nsl = _expected_slabs(ncu, nblocks, ws_bytes, nunits)
    if wsk == "short":
        assert nsl == 0
    elif wsk != "query":
        assert nsl == min(wsk[1], (2 * ncu) // nblocks), (nsl, wsk)
    print("%s: %d CUs, %d units, %d blocks, workspace %d bytes (queried %d) -> %d slabs of %d units" % (
        case, ncu, nunits, nblocks, ws_bytes, query, nsl, -(-nunits // nsl) if nsl else 0))
    ws = torch.full((ws_bytes // 4,), float("nan"), dtype=torch.float32, device="cuda")

    def check_route():
        finite = int(torch.isfinite(ws).sum())
        assert finite == nsl * nblocks * BLOCK_FLOATS, "%s: the call left %d finite floats in the workspace, the route writes %d" % (
            case, finite, nsl * nblocks * BLOCK_FLOATS)
        if nsl:
            assert bool(torch.isfinite(ws[:finite]).all()), "%s: the partial sums are not one contiguous image" % case

    def call(dw, db, impl=IMPL_MFMA_KD_SLAB, w=None):
        ops.conv3d_wgrad(x0, x1, dy, dw, db, impl=impl, workspace=ws if w is None else w)

    dw = torch.zeros((27, Cout, Cin), dtype=torch.float32, device="cuda")
    db = torch.zeros((Cout,), dtype=torch.float32, device="cuda")
    if mode == "plain":
        call(dw, db)
        torch.cuda.synchronize()
        check_route()
    elif mode == "upcat":
        dwc = torch.empty(64 * Cout * C0, dtype=torch.float32, device="cuda")
        ops.conv3d_upcat_wgrad(x0, x1, dy, dw, db, dwc, workspace=ws)
        torch.cuda.synchronize()
        check_route()
    elif mode == "repeat":
        runs = []
        for _ in range(3):
            dw.zero_()
            db.zero_()
            call(dw, db)
            torch.cuda.synchronize()
            runs.append((dw.clone(), db.clone()))
        check_route()
        for k in (1, 2):
            assert torch.equal(runs[k][0].view(torch.int32), runs[0][0].view(torch.int32)), "%s: dw of call %d differs in its bits" % (case, k + 1)
        if data == "dyadic":
            # the per-kd kernel with ITS slab flush (what IMPL_MFMA runs at this size with the queried workspace)
            w2 = torch.empty(query // 4, dtype=torch.float32, device="cuda")
            dw2, db2 = torch.zeros_like(dw), torch.zeros_like(db)
            call(dw2, db2, impl=IMPL_MFMA, w=w2)
            torch.cuda.synchronize()
            assert torch.equal(dw2.view(torch.int32), dw.view(torch.int32)) and torch.equal(db2.view(torch.int32), db.view(torch.int32)), \
                "%s: differs from the per-kd slab route" % case
            for k in (1, 2):
                assert torch.equal(runs[k][1].view(torch.int32), runs[0][1].view(torch.int32))
    elif mode == "det":
        grad = torch.zeros(27 * Cout * Cin + Cout, dtype=torch.float32, device="cuda")
        shadow = torch.zeros(grad.numel(), dtype=torch.int64, device="cuda")
        dwv, dbv = grad[:27 * Cout * Cin].view(27, Cout, Cin), grad[27 * Cout * Cin:]
        runs = []
        ops.set_deterministic(grad, shadow)
        try:
            for _ in range(3):
                grad.zero_()
                call(dwv, dbv)
                ops.deterministic_finish(grad, shadow)
                torch.cuda.synchronize()
                runs.append(grad.clone())
        finally:
            ops.set_deterministic(None, None)
        check_route()
        assert int(shadow.abs().max()) == 0
        for k in (1, 2):
            assert torch.equal(runs[k].view(torch.int32), runs[0].view(torch.int32)), "%s: call %d differs in its bits" % (case, k + 1)
        dw.copy_(dwv)
        db.copy_(dbv)
    torch.save({"dw": dw.cpu(), "db": db.cpu()}, out)


if __name__ == "__main__":
    worker(sys.argv[1], sys.argv[2])
