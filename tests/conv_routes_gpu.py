"""Runs one row of tests/conv_routes.py through the public wrapper that reaches it and states what the wrapper must return: the plain
definition of the operation on small dyadic numbers, where every product and every partial sum is exact in fp32, so the result does not
depend on the order of summation and must be met bit for bit.  Shared by tests/test_gpu_conv_routes.py and by the child processes of its
environment-switched arms (`python tests/conv_routes_gpu.py names.json out.json`: digests of the outputs, no references)."""
import hashlib
import json
import os
import sys
import zlib

import torch
import torch.nn.functional as F

import conv_routes as CR

CPU_CONV_FLOP = 12e9        # references up to this size: torch's fp32 convolution on the CPU; beyond: float64 tensor ops on the device


def conv27(x, w27, planar=False):
    """The plain definition: y[n, v, co] = sum_t sum_ci x[n, v + off(t), ci] w27[t, co, ci], off(t) = (kd - 1, kh - 1, kw - 1), zeros outside
    the volume; planar: the centre kd plane alone.  x [N, D, H, W, Cin], w27 [27, Cout, Cin] fp32 on the device -> float64 on the device.
    Small: torch's fp32 CPU convolution (tests/test_host_conv_routes.py: bit-equal to fp64 on this data); large: 27 shifted float64
    matrix products on the device (plain tensor ops, none of this project's kernels, never the device's convolution)."""
    N, D, H, W, Cin = x.shape
    Cout = w27.shape[1]
    taps = range(9, 18) if planar else range(27)
    if 2.0 * N * D * H * W * Cin * Cout * len(taps) <= CPU_CONV_FLOP:
        k = w27.cpu().reshape(3, 3, 3, Cout, Cin).permute(3, 4, 0, 1, 2).contiguous()
        if planar:
            k[:, :, 0] = 0
            k[:, :, 2] = 0
        y = F.conv3d(x.cpu().permute(0, 4, 1, 2, 3).contiguous(), k, None, padding=1)
        return y.permute(0, 2, 3, 4, 1).contiguous().to(x.device).double()
    xp = F.pad(x.double(), (0, 0, 1, 1, 1, 1, 1, 1))
    y = torch.zeros((N, D, H, W, Cout), dtype=torch.float64, device=x.device)
    for t in taps:
        kd, kh, kw = t // 9, (t // 3) % 3, t % 3
        y += xp[:, kd:kd + D, kh:kh + H, kw:kw + W] @ w27[t].double().t()
    return y


def flip_t(w27):
    """[27, Co, Ci] -> the input gradient's filters [27, Ci, Co]: dx[v] = sum_t dy[v - off(t)] w[t]"""
    return w27.flip(0).transpose(1, 2).contiguous()


def up2(x, planar):
    for ax in ((2, 3) if planar else (1, 2, 3)):
        x = torch.repeat_interleave(x, 2, dim=ax)
    return x


def sum2(x, planar):
    N, D, H, W, C = x.shape
    if planar:
        return x.reshape(N, D, H // 2, 2, W // 2, 2, C).sum(dim=(3, 5))
    return x.reshape(N, D // 2, 2, H // 2, 2, W // 2, 2, C).sum(dim=(2, 4, 6))


def max2(x, planar):
    N, D, H, W, C = x.shape
    if planar:
        return x.reshape(N, D, H // 2, 2, W // 2, 2, C).amax(dim=(3, 5))
    return x.reshape(N, D // 2, 2, H // 2, 2, W // 2, 2, C).amax(dim=(2, 4, 6))


def border_class(D, H, W, device):
    """[D, H, W] class (cd * 3 + ch) * 3 + cw, c = 0 first voxel of the axis / 1 interior / 2 last (FwdTail::bias27)"""
    c = lambda n: torch.tensor([0] + [1] * (n - 2) + [2], device=device)
    return (c(D)[:, None, None] * 3 + c(H)[None, :, None]) * 3 + c(W)[None, None, :]


class Data:
    """seeded dyadic tensors on the device: activations k/4 (|k| <= 4), weights k/8 (|k| <= 2), gradients k/2 (|k| <= 2), biases k/4"""

    def __init__(self, name):
        self.g = torch.Generator(device="cuda").manual_seed(zlib.crc32(name.encode()))

    def _r(self, shape, lo, hi, div):
        return torch.randint(lo, hi + 1, tuple(shape), generator=self.g, device="cuda", dtype=torch.int32).float() / div

    def act(self, *shape):
        return self._r(shape, -4, 4, 4.0)

    def w(self, *shape):
        return self._r(shape, -2, 2, 8.0)

    def dy(self, *shape):
        return self._r(shape, -2, 2, 2.0)

    def bias(self, *shape):
        return self._r(shape, -4, 4, 4.0)

    def w_sparse(self, Cout, Cin, nnz=8):
        """[27, Cout, Cin] with at most `nnz` non-zero weights per output channel: |conv| <= nnz * 1/4 * max|x|"""
        flat = torch.zeros((Cout, 27 * Cin), device="cuda")
        idx = torch.randint(0, 27 * Cin, (Cout, nnz), generator=self.g, device="cuda")
        val = torch.randint(0, 4, (Cout, nnz), generator=self.g, device="cuda")
        flat.scatter_(1, idx, torch.tensor([-0.25, -0.125, 0.125, 0.25], device="cuda")[val])
        return flat.view(Cout, 27, Cin).permute(1, 0, 2).contiguous()


def nan(shape, dtype):
    return torch.full(tuple(shape), float("nan"), dtype=dtype, device="cuda")


def run_row(ops, row, with_ref=True, sparse=False):
    """-> (outputs, references): two dicts name -> tensor.  Outputs are pre-filled with NaN.  sparse (the rows with normalisation sums):
    filters with <= 8 non-zero weights per output channel, so that every value summed is bounded by 3 (see sums_exact_bound)."""
    t = row.target
    N, D, H, W, C0, C1, Cout = row.shape
    dt = torch.float32 if t.f32 else torch.bfloat16
    pl = bool(t.planar)
    d = Data(t.name + ("/sparse" if sparse else ""))
    rd = lambda v: v.to(dt)
    half = (N, D if pl else D // 2, H // 2, W // 2)
    full = (N, D, H, W)
    out, ref = {}, {}
    op = t.op
    if op in ("fwd", "fwd_up", "fwd_mask", "stats"):
        up0 = op == "fwd_up"
        x0 = d.act(*(half if up0 else full), C0)
        x1 = d.act(*full, C1) if C1 else None
        w = d.w_sparse(Cout, C0 + C1) if sparse else d.w(27, Cout, C0 + C1)
        b = None if op == "fwd_mask" else d.bias(Cout)
        m = d.act(*full, Cout) if op == "fwd_mask" else None
        y = nan(full + (Cout,), dt)
        if op == "stats":
            per = 1 if N > 1 else 0
            G = N if per else 1
            ws = torch.zeros(ops.norm_tail_ws_doubles(G, Cout), dtype=torch.float64, device="cuda")
            ops.conv3d_fwd_stats(rd(x0), None if x1 is None else rd(x1), rd(w), b, y, ws, per, act=0)
            out["sums"], out["slots"] = ws[:G * Cout * 2].view(G, Cout, 2), ws[G * Cout * 2:]
        else:
            ops.conv3d_fwd(rd(x0), None if x1 is None else rd(x1), rd(w), b, y, up0=up0, act=0 if m is not None else 1,
                           mask=None if m is None else rd(m), planar=pl)
        out["y"] = y
        if with_ref:
            xin = up2(x0, pl) if up0 else x0
            pre = conv27(xin if x1 is None else torch.cat([xin, x1], dim=-1), w, pl)
            if op == "fwd_mask":
                ref["y"] = rd(torch.where(m > 0, pre, torch.zeros_like(pre)))
            elif op == "stats":
                ref["y"] = rd(pre + b.double())
                ref["sums"], ref["slots"] = sums_of(ref["y"], ref["y"], G), torch.zeros_like(out["slots"])
            else:
                ref["y"] = rd(F.relu(pre + b.double()))
    elif op in ("dgrad", "dgrad_mask", "dgrad_norm"):
        dy = d.dy(*full, C0)
        w = d.w_sparse(Cout, C0).transpose(1, 2).contiguous() if sparse else d.w(27, C0, Cout)          # the conv's filters: Cout -> C0 channels forward
        wf, wd = torch.empty((27, C0, Cout), dtype=dt, device="cuda"), torch.empty((27, Cout, C0), dtype=dt, device="cuda")
        ops.pack_weights(w, wf, wd)
        dx = nan(full + (Cout,), dt)
        m = d.act(*full, Cout) if op != "dgrad" else None
        if op == "dgrad_norm":
            per = 1 if N > 1 else 0
            G = N if per else 1
            nss = torch.stack([d._r((G, Cout), 1, 4, 4.0) * (d._r((G, Cout), 0, 1, 1.0) * 2 - 1), d.bias(G, Cout)], dim=-1).contiguous()
            ws = torch.zeros(ops.norm_tail_ws_doubles(G, Cout), dtype=torch.float64, device="cuda")
            ops.conv3d_dgrad_norm(rd(dy), wd, rd(m), nss, dx, ws, per, act=1)
            out["sums"], out["slots"] = ws[:G * Cout * 2].view(G, Cout, 2), ws[G * Cout * 2:]
        else:
            ops.conv3d_dgrad(rd(dy), wd, dx, mask=None if m is None else rd(m), planar=pl)
        out["dx"] = dx
        if with_ref:
            g = conv27(dy, flip_t(w), pl)
            if op == "dgrad":
                ref["dx"] = rd(g)
            elif op == "dgrad_mask":
                ref["dx"] = rd(torch.where(m > 0, g, torch.zeros_like(g)))
            else:
                z = m.reshape(G, -1, Cout).double() * nss[:, None, :, 0].double() + nss[:, None, :, 1].double()     # exact: no rounding to differ by
                gb = rd(g).double()                                                                                  # the staged tile is bf16
                ref["dx"] = rd(torch.where(z.reshape(gb.shape) > 0, gb, gb * 0.0))
                ref["sums"], ref["slots"] = sums_of(ref["dx"], rd(m), G), torch.zeros_like(out["slots"])
    elif op in ("tail_pool", "tail_logits", "tail_both"):
        x, w, b = d.act(*full, C0), d.w(27, Cout, C0), d.bias(Cout)
        w1, b1 = d.bias(Cout), d.bias(1)
        y = nan(full + (Cout,), dt)
        pool = nan(((N, D, H // 2, W // 2) if pl else half) + (Cout,), dt) if op != "tail_logits" else None
        lg = nan((N * D * H * W,), torch.float32) if op != "tail_pool" else None
        ops.conv3d_fwd_tail(rd(x), rd(w), b, y, pool=pool, w1=None if lg is None else w1, b1=None if lg is None else b1, logits=lg, act=1, planar=pl)
        out["y"] = y
        if pool is not None:
            out["pool"] = pool
        if lg is not None:
            out["logits"] = lg
        if with_ref:
            ref["y"] = rd(F.relu(conv27(x, w, pl) + b.double()))
            if pool is not None:
                ref["pool"] = max2(ref["y"], pl)
            if lg is not None:
                ref["logits"] = (ref["y"].double().reshape(-1, Cout) @ w1.double() + b1.double()).float()
    elif op in ("upcat", "upcat_stats", "bias27"):
        xl = d.act(*half, C0)
        xs = d.act(*full, C1) if C1 else None
        w = d.w_sparse(Cout, C0 + C1) if sparse else d.w(27, Cout, C0 + C1)
        b = d.bias(27, Cout) if op == "bias27" else d.bias(Cout)
        k = 4 if pl else 8
        up_f = torch.empty((k, k, Cout, C0), dtype=dt, device="cuda")
        sk_f = torch.empty((27, Cout, C1), dtype=dt, device="cuda") if C1 else None
        ops.conv3d_pack_up_weights(w, C0, C1, up_f, None, sk_f, None, planar=pl)
        y = nan(full + (Cout,), dt)
        if op == "upcat":
            ops.conv3d_upcat_fwd(rd(xl), None if xs is None else rd(xs), up_f, sk_f, b, y, act=1, planar=pl)
        elif op == "bias27":
            ops.conv3d_upcat_fwd_bias27(rd(xl), rd(xs), up_f, sk_f, b, y, act=1)
        else:
            per = 1 if N > 1 else 0
            G = N if per else 1
            ws = torch.zeros(ops.norm_tail_ws_doubles(G, Cout), dtype=torch.float64, device="cuda")
            ops.conv3d_upcat_fwd_stats(rd(xl), rd(xs), up_f, sk_f, b, y, ws, per, act=0)
            out["sums"], out["slots"] = ws[:G * Cout * 2].view(G, Cout, 2), ws[G * Cout * 2:]
        out["y"] = y
        if with_ref:
            part = conv27(up2(xl, pl), w[:, :, :C0].contiguous(), pl)
            if not C1:
                ref["y"] = rd(F.relu(part + b.double()))
            else:
                # two launches: the up-sampled channels' partial sum is stored in the tensor's type, the skip launch rounds its own sum + bias
                # to it as well, and the two meet in fp32 (fp32 tensors: nothing is rounded)
                bb = b.double()[border_class(D, H, W, "cuda")] if op == "bias27" else b.double()
                tot = rd(part).double() + rd(conv27(xs, w[:, :, C0:].contiguous(), pl) + bb).double()
                ref["y"] = rd(tot if op == "upcat_stats" else F.relu(tot))
                if op == "upcat_stats":
                    ref["sums"], ref["slots"] = sums_of(ref["y"], ref["y"], G), torch.zeros_like(out["slots"])
    elif op in ("upcat_dgrad", "upcat_dgrad_mask"):
        dy = d.dy(*full, Cout)
        w = d.w(27, Cout, C0 + C1)
        k = 4 if pl else 8
        up_d = torch.empty((k, k, C0, Cout), dtype=dt, device="cuda")
        sk_d = torch.empty((27, C1, Cout), dtype=dt, device="cuda") if C1 else None
        ops.conv3d_pack_up_weights(w, C0, C1, None, up_d, None, sk_d, planar=pl)
        masked = op.endswith("mask")
        ml = d.act(*half, C0) if masked else None
        ms = d.act(*full, C1) if masked and C1 else None
        dxl = nan(half + (C0,), dt)
        dxs = nan(full + (C1,), dt) if C1 else None
        ops.conv3d_upcat_dgrad(rd(dy), up_d, sk_d, None if ml is None else rd(ml), None if ms is None else rd(ms), dxl, dxs, planar=pl)
        out["dx_low"] = dxl
        if C1:
            out["dx_skip"] = dxs
        if with_ref:
            gl = sum2(conv27(dy, flip_t(w[:, :, :C0].contiguous()), pl), pl)
            ref["dx_low"] = rd(torch.where(ml > 0, gl, torch.zeros_like(gl)) if masked else gl)
            if C1:
                gs = conv27(dy, flip_t(w[:, :, C0:].contiguous()), pl)
                ref["dx_skip"] = rd(torch.where(ms > 0, gs, torch.zeros_like(gs)) if masked else gs)
    elif op == "stride2":
        from fmri_hip.strided_parity import StridedParity
        x, w, b = d.act(*full, C0), d.w(27, Cout, C0), d.bias(Cout)
        img = torch.zeros((8, 8, Cout, C0), dtype=dt, device="cuda")
        StridedParity("cuda").pack(w, img, None)
        y = nan((N, D // 2, H // 2, W // 2, Cout), dt)
        ops.conv3d_stride2_fwd(rd(x), img, b, y)
        out["y"] = y
        if with_ref:
            # TF 'same' on even dims pads one plane BEHIND the volume: out[o] = sum_t W[t] x[2o + t] = the stride-1 result at voxel 2o + 1
            ref["y"] = rd(conv27(x, w)[:, 1::2, 1::2, 1::2] + b.double())
    else:
        raise KeyError(op)
    torch.cuda.synchronize()
    return out, ref


def sums_of(v, x, G):
    """[G, C, 2] float64: {sum v, sum v * x} per (group, channel) over the stored values"""
    C = v.shape[-1]
    vd, xd = v.double().reshape(G, -1, C), x.double().reshape(G, -1, C)
    return torch.stack([vd.sum(1), (vd * xd).sum(1)], dim=-1)


def sums_exact_bound(row):
    """The largest fp32 partial sum the normalisation tails can form, in units of the smallest term, for a sparse run of the row.  A
    workgroup sums in fp32 what it stores of one (group, channel) before it adds to its fp64 slot: at most ceil(np / grid) tiles of 512
    voxels.  Sparse filters: |conv| <= 8 * 1/4 * 1 = 2 over all sources together, |bias| <= 1 -> |v| <= 3, a multiple of 1/32 below 2^2
    (7 bits: exact in bf16); v * v, and v * x with |x| <= 1 a multiple of 1/4, are multiples of 2^-10 bounded by 9.  Must stay below 2^24."""
    items = -(-row.route.np // row.route.grid)
    return items * 512 * 9 * 1024


def digest(t):
    v = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]
    return hashlib.sha256(t.contiguous().view(v).cpu().numpy().tobytes()).hexdigest()


def first_difference(got, want):
    """index tuple of the first element whose bits differ, or None (a NaN differs from everything that is not the same NaN)"""
    v = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[got.element_size()]
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, tuple(got.shape), tuple(want.shape))
    bad = got.contiguous().view(v) != want.contiguous().view(v)
    n = int(bad.sum())
    if n == 0:
        return None, 0
    flat = int(torch.nonzero(bad.reshape(-1))[0])
    import numpy as np
    return tuple(int(i) for i in np.unravel_index(flat, tuple(got.shape))), n


def ncu_of_device():
    return torch.cuda.get_device_properties(0).multi_processor_count


def main(argv):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "fetal-mri-segmentation_amd")):
        sys.path.insert(0, p)
    from fmri_hip import ops
    names = set(json.load(open(argv[1])))
    ncu = ncu_of_device()
    res = {}
    for t in CR.TARGETS:
        if t.name in names:
            row = CR.generate(t, ncu)
            out, _ = run_row(ops, row, with_ref=False)
            res[t.name] = {k: digest(v) for k, v in out.items()}
    json.dump(res, open(argv[2], "w"))
    print("DONE %d rows" % len(res))


if __name__ == "__main__":
    main(sys.argv)
