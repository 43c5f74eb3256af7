"""torch-tensor front-ends of the C ABI.  torch is plumbing only: device memory, the current HIP stream, dtypes."""
import torch

from ._lib import lib, check, F32, BF16, F64, ACT_NONE, ACT_RELU, IMPL_AUTO


def dt(t):
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    raise TypeError("unsupported dtype %s" % t.dtype)


import os as _os

_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None) if _os.environ.get("FMRI_RAW_STREAM", "1") != "0" else None
_cur_device = getattr(torch._C, "_cuda_getDevice", None)


def _s():
    """the current HIP stream of the current device as a raw handle.  torch.cuda.current_stream() costs 10-40 us of Python per call
    (device-index resolution, an is_available() probe with an environment lookup, a Stream object); an engine step makes ~100 of these
    calls and the patch sampler is launch-bound, so the two C entry points torch itself uses on its fast paths are called directly."""
    if _raw_stream is not None and _cur_device is not None:
        return _raw_stream(_cur_device())
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return 0 if t is None else t.data_ptr()


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("fmri_hip ops need device tensors (no CPU path)")
        if t is not None and not t.is_contiguous():
            raise RuntimeError("fmri_hip ops need contiguous tensors")


def conv3d_fwd(src0, src1, w, bias, y, up0=False, act=ACT_RELU, alpha=0.0, mask=None, impl=IMPL_AUTO, planar=False):
    """src0 [N,d,h,w,C0] (half-res when up0), src1 [N,D,H,W,C1] or None, w [27,Cout,C0+C1], y [N,D,H,W,Cout]."""
    _need_cuda(src0, src1, w, bias, y, mask)
    N, D, H, W, Cout = y.shape
    C0 = src0.shape[-1]
    C1 = 0 if src1 is None else src1.shape[-1]
    assert w.shape == (27, Cout, C0 + C1), (w.shape, Cout, C0, C1)
    check(lib().fmri_conv3d_fwd(_p(src0), C0, int(up0), _p(src1), C1, _p(w), _p(bias), _p(mask), _p(y), N, D, H, W, Cout,
                                act, float(alpha), dt(y), impl, int(planar), _s()), "fmri_conv3d_fwd")
    return y


def conv3d_fwd_tail_ok(C0, Cout, N, D, H, W, dtype, planar=False):
    """bit 0: the conv epilogue can also write the 2x2x2 (planar: 2x2 per slice) max-pooled tensor, bit 1: ... the logits of a final
    1x1x1 conv to one label"""
    f = lib().fmri_conv3d_fwd_tail_planar_ok if planar else lib().fmri_conv3d_fwd_tail_ok
    return int(f(C0, Cout, N, D, H, W, BF16 if dtype == torch.bfloat16 else F32))


def conv3d_fwd_tail(src0, w, bias, y, pool=None, w1=None, b1=None, logits=None, act=ACT_RELU, alpha=0.0, planar=False):
    """conv block whose epilogue also produces MaxPooling3D(2)(y) (planar: MaxPooling2D(2) of every slice) and / or the final 1x1x1 conv's
    logits (fmri_conv3d_fwd_tail / fmri_conv3d_fwd_tail_planar)"""
    _need_cuda(src0, w, bias, y, pool, w1, b1, logits)
    N, D, H, W, Cout = y.shape
    C0 = src0.shape[-1]
    assert w.shape == (27, Cout, C0)
    if pool is not None:
        assert tuple(pool.shape) == (N, D if planar else D // 2, H // 2, W // 2, Cout) and pool.dtype == y.dtype
    if logits is not None:
        assert logits.dtype == torch.float32 and logits.numel() == N * D * H * W and w1.dtype == torch.float32 and w1.numel() == Cout
    f = lib().fmri_conv3d_fwd_tail_planar if planar else lib().fmri_conv3d_fwd_tail
    check(f(_p(src0), C0, _p(w), _p(bias), _p(y), _p(pool), _p(w1), _p(b1), _p(logits), N, D, H, W, Cout, act, float(alpha), dt(y), _s()),
          "fmri_conv3d_fwd_tail_planar" if planar else "fmri_conv3d_fwd_tail")
    return y


def conv3d_dgrad(dy, w_dgrad, dx, mask=None, impl=IMPL_AUTO, planar=False):
    _need_cuda(dy, w_dgrad, dx, mask)
    N, D, H, W, Cin = dx.shape
    Cout = dy.shape[-1]
    assert w_dgrad.shape == (27, Cin, Cout)
    check(lib().fmri_conv3d_dgrad(_p(dy), Cout, _p(w_dgrad), _p(mask), _p(dx), N, D, H, W, Cin, dt(dx), impl, int(planar), _s()),
          "fmri_conv3d_dgrad")
    return dx


def conv3d_first_dgrad_ok(Cin, Cout, D, H, W, dtype):
    """does fmri_conv3d_first_dgrad take this first-layer shape? (bf16, 3-D, Cin 1..4, Cout % 32, D % 4, H % 16, W % 32)"""
    return bool(lib().fmri_conv3d_first_dgrad_ok(Cin, Cout, D, H, W, BF16 if dtype == torch.bfloat16 else F32))


def conv3d_first_dgrad(dy, w_fwd, dx):
    """dx [N,D,H,W,Cin] fp32 (overwritten) = input gradient of the first convolution from dy [N,D,H,W,Cout] bf16 and the FORWARD filter
    image w_fwd [27,Cout,Cin] bf16"""
    _need_cuda(dy, w_fwd, dx)
    N, D, H, W, Cin = dx.shape
    Cout = dy.shape[-1]
    assert tuple(dy.shape[:4]) == (N, D, H, W) and w_fwd.shape == (27, Cout, Cin) and dx.dtype == torch.float32 and w_fwd.dtype == dy.dtype
    check(lib().fmri_conv3d_first_dgrad(_p(dy), Cout, _p(w_fwd), _p(dx), N, D, H, W, Cin, dt(dy), _s()), "fmri_conv3d_first_dgrad")
    return dx


def conv3d_wgrad(src0, src1, dy, dw, db, up0=False, impl=IMPL_AUTO, planar=False, workspace=None):
    _need_cuda(src0, src1, dy, dw, db)
    N, D, H, W, Cout = dy.shape
    C0 = src0.shape[-1]
    C1 = 0 if src1 is None else src1.shape[-1]
    assert dw.dtype == torch.float32 and dw.numel() == 27 * Cout * (C0 + C1)
    check(lib().fmri_conv3d_wgrad(_p(src0), C0, int(up0), _p(src1), C1, _p(dy), _p(dw), _p(db), N, D, H, W, Cout, dt(dy),
                                  impl, int(planar), _p(workspace), 0 if workspace is None else workspace.numel() * workspace.element_size(),
                                  _s()), "fmri_conv3d_wgrad")


def pack_weights(w, w_fwd, w_dgrad):
    _need_cuda(w, w_fwd, w_dgrad)
    _, Cout, Cin = w.shape
    d = dt(w_fwd if w_fwd is not None else w_dgrad)
    check(lib().fmri_conv3d_pack_weights(_p(w), _p(w_fwd), _p(w_dgrad), Cout, Cin, d, _s()), "fmri_conv3d_pack_weights")


def pack_table(entries, device):
    """the device table of fmri_pack_weights_batched.  entries: ("plain", w, w_fwd, w_dgrad) or ("up", w, C0, C1, up_f, up_d, sk_f, sk_d, planar)
    with the tensors of pack_weights / conv3d_pack_up_weights (None = not wanted).  Returns (table int64 [n][10], n_blocks); the table holds
    raw device addresses: the tensors must stay alive and in place."""
    rows, first = [], 0
    ptr = lambda t: 0 if t is None else t.data_ptr()
    for e in entries:
        if e[0] == "plain":
            _, w, wf, wd = e
            _, Cout, Cin = w.shape
            rows.append([0, first, ptr(w), ptr(wf), ptr(wd), 0, 0, Cout, Cin, 0])
            first += 27 * ((Cout + 63) // 64) * ((Cin + 63) // 64)
        else:
            _, w, C0, C1, up_f, up_d, sk_f, sk_d, planar = e
            Cout = w.shape[1]
            rows.append([1, first, ptr(w), ptr(up_f), ptr(up_d), ptr(sk_f), ptr(sk_d), Cout, C0, C1 | (int(bool(planar)) << 32)])
            tco = (Cout + 63) // 64
            first += (16 if planar else 64) * tco * ((C0 + 63) // 64) + 27 * tco * ((C1 + 63) // 64)
    return torch.tensor(rows, dtype=torch.int64, device=device), first


def pack_weights_batched(table, n_blocks, dtype):
    """every weight image of a model in one launch (fmri_pack_weights_batched); table, n_blocks from pack_table"""
    _need_cuda(table)
    check(lib().fmri_pack_weights_batched(_p(table), table.shape[0], n_blocks, BF16 if dtype == torch.bfloat16 else F32, _s()),
          "fmri_pack_weights_batched")


def conv1x1_fwd(x, w, b, logits):
    _need_cuda(x, w, b, logits)
    C = x.shape[-1]
    L = w.shape[0]
    nvox = x.numel() // C
    check(lib().fmri_conv1x1_fwd(_p(x), _p(w), _p(b), _p(logits), nvox, C, L, dt(x), _s()), "fmri_conv1x1_fwd")
    return logits


def conv1x1_bwd(x, w, dlogits, dx, dw, db, relu_mask=True):
    _need_cuda(x, w, dlogits, dx, dw, db)
    C = x.shape[-1]
    L = w.shape[0]
    nvox = x.numel() // C
    check(lib().fmri_conv1x1_bwd(_p(x), _p(w), _p(dlogits), _p(dx), _p(dw), _p(db), nvox, C, L, int(relu_mask), dt(x), _s()),
          "fmri_conv1x1_bwd")


def sigmoid_dice_fwd(logits, y_true, probs, sums, weight=None):
    """weight (optional, fp32, one per voxel): multiplies the cross-entropy term (dice_and_xent_mask)"""
    _need_cuda(logits, y_true, probs, sums, weight)
    assert y_true.dtype == torch.uint8 and sums.dtype == torch.float64 and sums.numel() >= 16
    if weight is not None:
        assert weight.dtype == torch.float32 and weight.numel() == logits.numel()
        check(lib().fmri_sigmoid_dice_fwd_weighted(_p(logits), _p(y_true), _p(weight), _p(probs), _p(sums), logits.numel(), _s()),
              "fmri_sigmoid_dice_fwd_weighted")
        return
    check(lib().fmri_sigmoid_dice_fwd(_p(logits), _p(y_true), _p(probs), _p(sums), logits.numel(), _s()), "fmri_sigmoid_dice_fwd")


def sigmoid_dice_bwd(probs, y_true, sums, dlogits, smooth=1.0, grad_scale=1.0):
    _need_cuda(probs, y_true, sums, dlogits)
    check(lib().fmri_sigmoid_dice_bwd(_p(probs), _p(y_true), _p(sums), _p(dlogits), probs.numel(), float(smooth),
                                      float(grad_scale), _s()), "fmri_sigmoid_dice_bwd")


def _pool3(pool, planar):
    """per-axis factors (pd, ph, pw) of a layer's pool_size / size; None: all 2s; the 2-D layer of a planar tensor leaves the slice axis
    alone"""
    if pool is None:
        return (1, 2, 2) if planar else (2, 2, 2)
    pool = tuple(int(v) for v in pool)
    if len(pool) == 2:
        if not planar:
            raise ValueError("a 2-D pool size %s needs planar=True" % (pool,))
        pool = (1,) + pool
    if len(pool) != 3 or (planar and pool[0] != 1):
        raise ValueError("pool size %s (planar=%s)" % (pool, planar))
    return pool


def maxpool_fwd(x, y, planar=False, pool=None):
    """pool=(pd, ph, pw) or, planar, (ph, pw): per-axis factors 1..4; None: 2x2x2 (planar: 1x2x2)"""
    _need_cuda(x, y)
    N, D, H, W, Cc = x.shape
    pd, ph, pw = _pool3(pool, planar)
    assert tuple(y.shape) == (N, D // pd, H // ph, W // pw, Cc), (tuple(x.shape), tuple(y.shape), pool)
    check(lib().fmri_maxpool3d_fwd(_p(x), _p(y), N, D, H, W, Cc, pd, ph, pw, dt(x), _s()), "fmri_maxpool3d_fwd")
    return y


def maxpool_bwd(x, dy, dx, add=None, add_off=0, relu_mask=True, planar=False, pool=None):
    _need_cuda(x, dy, dx, add)
    N, D, H, W, Cc = x.shape
    add_ld = 0 if add is None else add.shape[-1]
    pd, ph, pw = _pool3(pool, planar)
    assert tuple(dy.shape) == (N, D // pd, H // ph, W // pw, Cc) and dx.shape == x.shape, (tuple(x.shape), tuple(dy.shape), pool)
    check(lib().fmri_maxpool3d_bwd(_p(x), _p(dy), _p(add), add_ld, add_off, _p(dx), N, D, H, W, Cc, pd, ph, pw, int(relu_mask), dt(x), _s()),
          "fmri_maxpool3d_bwd")
    return dx


def upsample_fwd(x, y, y_off=0, planar=False, pool=None):
    _need_cuda(x, y)
    N, D, H, W, Cc = x.shape
    pd, ph, pw = _pool3(pool, planar)
    assert tuple(y.shape[:-1]) == (N, D * pd, H * ph, W * pw), (tuple(x.shape), tuple(y.shape), pool)
    check(lib().fmri_upsample_nearest_fwd(_p(x), _p(y), y.shape[-1], y_off, N, D, H, W, Cc, pd, ph, pw, dt(x), _s()),
          "fmri_upsample_nearest_fwd")
    return y


def upsample_bwd(dy, dx, dy_off=0, xmask=None, planar=False, pool=None):
    _need_cuda(dy, dx, xmask)
    N, D, H, W, Cc = dx.shape
    pd, ph, pw = _pool3(pool, planar)
    assert tuple(dy.shape[:-1]) == (N, D * pd, H * ph, W * pw), (tuple(dx.shape), tuple(dy.shape), pool)
    check(lib().fmri_upsample_nearest_bwd(_p(dy), dy.shape[-1], dy_off, _p(xmask), _p(dx), N, D, H, W, Cc, pd, ph, pw, dt(dx), _s()),
          "fmri_upsample_nearest_bwd")
    return dx


def adam_step(p, g, m, v, lr_t, beta1=0.9, beta2=0.999, eps=1e-7, grad_scale=1.0):
    _need_cuda(p, g, m, v)
    check(lib().fmri_adam_step(_p(p), _p(g), _p(m), _p(v), p.numel(), float(lr_t), beta1, beta2, eps, float(grad_scale), _s()),
          "fmri_adam_step")


def grad_sumsq_workspace(device):
    """the partial-sum workspace of grad_sumsq and its two float64 results {sum of squares, norm}: allocated once by the caller"""
    return (torch.empty(lib().fmri_grad_sumsq_workspace_bytes() // 8, dtype=torch.float64, device=device),
            torch.zeros(2, dtype=torch.float64, device=device))


def grad_sumsq(g, grad_scale, work, out):
    """out[0] = sum (float(grad_scale * g_i))^2 in float64 (compensated, ordered: the same bits every run), out[1] = its square root"""
    _need_cuda(g, work, out)
    check(lib().fmri_grad_sumsq(_p(g), g.numel(), float(grad_scale), _p(work), _p(out), _s()), "fmri_grad_sumsq")
    return out


def _gnorm_ptr(gnorm):
    """device pointer to the norm (out[1] of grad_sumsq) from the 2-element result tensor, or 0"""
    return 0 if gnorm is None else gnorm.data_ptr() + 8


def sgd_step(p, g, m, lr, momentum=0.0, nesterov=False, grad_scale=1.0, gnorm=None, clipnorm=0.0, clipvalue=0.0):
    """Keras SGD on flat buffers; gnorm: the result tensor of grad_sumsq (clipnorm reads its norm on the device) or None"""
    _need_cuda(p, g, m, gnorm)
    check(lib().fmri_sgd_step(_p(p), _p(g), _p(m), p.numel(), float(lr), float(momentum), int(bool(nesterov)), float(grad_scale),
                              _gnorm_ptr(gnorm), float(clipnorm), float(clipvalue), _s()), "fmri_sgd_step")


def rmsprop_step(p, g, a, lr, rho=0.9, eps=1e-7, grad_scale=1.0, gnorm=None, clipnorm=0.0, clipvalue=0.0):
    _need_cuda(p, g, a, gnorm)
    check(lib().fmri_rmsprop_step(_p(p), _p(g), _p(a), p.numel(), float(lr), float(rho), float(eps), float(grad_scale),
                                  _gnorm_ptr(gnorm), float(clipnorm), float(clipvalue), _s()), "fmri_rmsprop_step")


def adam_step_ex(p, g, m, v, vhat, lr_t, beta1=0.9, beta2=0.999, eps=1e-7, grad_scale=1.0, gnorm=None, clipnorm=0.0, clipvalue=0.0):
    """adam_step with AMSGrad (vhat: a tensor, or None for none) and clipping"""
    _need_cuda(p, g, m, v, vhat, gnorm)
    check(lib().fmri_adam_step_ex(_p(p), _p(g), _p(m), _p(v), _p(vhat), p.numel(), float(lr_t), float(beta1), float(beta2), float(eps),
                                  float(grad_scale), _gnorm_ptr(gnorm), float(clipnorm), float(clipvalue), _s()), "fmri_adam_step_ex")


def tile_gather(vol, idx, patch, tiles):
    _need_cuda(vol, idx, tiles)
    X, Y, Z = vol.shape
    B = idx.shape[0]
    check(lib().fmri_tile_gather(_p(vol), X, Y, Z, _p(idx), B, patch[0], patch[1], patch[2], _p(tiles), dt(tiles), _s()),
          "fmri_tile_gather")
    return tiles


def tile_gather_stack(vol, aux, idx, patch, aux_dz, aux_nz, tiles):
    """tiles (..., B, px, py, pz + aux_nz): the pz slices of vol at each corner of idx, then aux_nz slices of aux starting aux_dz slices from the
    corner (fmri_tile_gather_stack; the previous-slice truth channels of reference prediction.py:98-114).  aux: fp32 (X, Y, Z) or None if aux_nz = 0"""
    _need_cuda(vol, aux, idx, tiles)
    X, Y, Z = vol.shape
    if aux_nz:
        assert aux is not None and tuple(aux.shape) == (X, Y, Z) and aux.dtype == torch.float32
    assert vol.dtype == torch.float32 and idx.dtype == torch.int32
    B = idx.shape[0]
    assert tiles.numel() == B * patch[0] * patch[1] * (patch[2] + aux_nz)
    check(lib().fmri_tile_gather_stack(_p(vol), _p(aux if aux_nz else None), X, Y, Z, _p(idx), B, patch[0], patch[1], patch[2], int(aux_dz),
                                       int(aux_nz), _p(tiles), dt(tiles), _s()), "fmri_tile_gather_stack")
    return tiles


def tile_scatter_accumulate(pred, idx, patch, acc, cnt):
    _need_cuda(pred, idx, acc, cnt)
    X, Y, Z, Cc = acc.shape
    B = idx.shape[0]
    check(lib().fmri_tile_scatter_accumulate(_p(pred), _p(idx), B, patch[0], patch[1], patch[2], Cc, _p(acc), _p(cnt), X, Y, Z,
                                             _s()), "fmri_tile_scatter_accumulate")


def tile_finalize(acc, cnt, out, bad):
    _need_cuda(acc, cnt, out, bad)
    Cc = acc.shape[-1]
    check(lib().fmri_tile_finalize(_p(acc), _p(cnt), _p(out), _p(bad), cnt.numel(), Cc, _s()), "fmri_tile_finalize")


def tile_scatter_weighted(pred, idx, patch, tables, acc, wsum):
    """acc (X, Y, Z, C) float64 += w * pred and wsum (X, Y, Z) float64 += w for every tile voxel inside the volume, w = (gx[x] * gy[y]) * gz[z]
    in float64 from the three float32 device tables `tables` of patch[0], patch[1], patch[2] entries (fmri_tile_scatter_weighted)"""
    gx, gy, gz = tables
    _need_cuda(pred, idx, gx, gy, gz, acc, wsum)
    X, Y, Z, Cc = acc.shape
    B = idx.shape[0]
    if tuple(wsum.shape) != (X, Y, Z) or [g.numel() for g in tables] != [int(v) for v in patch] or pred.numel() != B * patch[0] * patch[1] * patch[2] * Cc:
        raise ValueError("tile_scatter_weighted: pred (B, px, py, pz, C), one table entry per tile voxel and axis, wsum of acc's extent "
                         "(got pred %s, tables %s, patch %s, acc %s, wsum %s)" % (tuple(pred.shape), [g.numel() for g in tables], tuple(patch),
                                                                                  tuple(acc.shape), tuple(wsum.shape)))
    if pred.dtype != torch.float32 or idx.dtype != torch.int32 or any(g.dtype != torch.float32 for g in tables) or \
            acc.dtype != torch.float64 or wsum.dtype != torch.float64:
        raise TypeError("tile_scatter_weighted: float32 pred and tables, int32 idx, float64 acc and wsum")
    check(lib().fmri_tile_scatter_weighted(_p(pred), _p(idx), B, patch[0], patch[1], patch[2], Cc, _p(gx), _p(gy), _p(gz), _p(acc), _p(wsum),
                                           X, Y, Z, _s()), "fmri_tile_scatter_weighted")


def tile_finalize_weighted(acc, wsum, out, bad):
    """out float64 like acc = acc / wsum; bad (int32, accumulated) counts the voxels with wsum <= 0, which divide by 1 (fmri_tile_finalize_weighted)"""
    _need_cuda(acc, wsum, out, bad)
    Cc = acc.shape[-1]
    if acc.dtype != torch.float64 or wsum.dtype != torch.float64 or out.dtype != torch.float64 or bad.dtype != torch.int32:
        raise TypeError("tile_finalize_weighted: float64 acc, wsum and out, int32 bad")
    if acc.numel() != wsum.numel() * Cc or out.numel() != acc.numel():
        raise ValueError("tile_finalize_weighted: acc and out (..., C), wsum (...) (got %s, %s, %s)" % (tuple(acc.shape), tuple(out.shape), tuple(wsum.shape)))
    check(lib().fmri_tile_finalize_weighted(_p(acc), _p(wsum), _p(out), _p(bad), wsum.numel(), Cc, _s()), "fmri_tile_finalize_weighted")


def _dt_vol(t):
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.float64:
        return F64
    raise TypeError("unsupported dtype %s (float32 or float64)" % t.dtype)


def _lo3(lo):
    import ctypes
    vals = [int(v) for v in lo]
    if len(vals) != 3:
        raise ValueError("lo: one offset per axis (got %r)" % (lo,))
    return (ctypes.c_int32 * 3)(*vals)


def flip_mask_of(axes):
    """the 3-bit mask of a tuple of mirrored axes (bit k = axis k)"""
    mask = 0
    for a in axes:
        mask |= 1 << int(a)
    return mask


def volume_pad_flip(src, dst, lo=(0, 0, 0), flip_mask=0, fill=0.0):
    """dst (OX, OY, OZ) = np.pad(np.flip(src, axes of flip_mask), ..., constant_values=fill) with lo voxels in front of every axis, cut to
    dst's extent (a negative lo crops); src (X, Y, Z); each float32 or float64, converted as numpy's astype (fmri_volume_pad_flip)"""
    _need_cuda(src, dst)
    if src.dim() != 3 or dst.dim() != 3:
        raise ValueError("volume_pad_flip: 3-D volumes (got %s -> %s)" % (tuple(src.shape), tuple(dst.shape)))
    X, Y, Z = src.shape
    OX, OY, OZ = dst.shape
    with torch.cuda.device(dst.device):
        check(lib().fmri_volume_pad_flip(_p(src), _dt_vol(src), X, Y, Z, _p(dst), _dt_vol(dst), OX, OY, OZ, _lo3(lo), int(flip_mask),
                                         float(fill), _s()), "fmri_volume_pad_flip")
    return dst


def tile_finalize_flip(acc, cnt, out, bad, lo=(0, 0, 0), flip_mask=0):
    """out (X, Y, Z, C) float64 = acc / cnt (tile_finalize's division) of the window [lo, lo + (X, Y, Z)) of acc (AX, AY, AZ, C), mirrored
    along the axes of flip_mask; bad (int32, accumulated) counts the window's voxels with a zero count (fmri_tile_finalize_flip)"""
    _need_cuda(acc, cnt, out, bad)
    if acc.dim() != 4 or out.dim() != 4 or tuple(cnt.shape) != tuple(acc.shape[:3]) or out.shape[3] != acc.shape[3]:
        raise ValueError("tile_finalize_flip: acc (AX, AY, AZ, C), cnt (AX, AY, AZ), out (X, Y, Z, C) (got %s, %s, %s)" % (
            tuple(acc.shape), tuple(cnt.shape), tuple(out.shape)))
    if acc.dtype != torch.float64 or out.dtype != torch.float64 or cnt.dtype != torch.int32 or bad.dtype != torch.int32:
        raise TypeError("tile_finalize_flip: float64 acc and out, int32 cnt and bad")
    AX, AY, AZ, Cc = acc.shape
    X, Y, Z = out.shape[:3]
    with torch.cuda.device(out.device):
        check(lib().fmri_tile_finalize_flip(_p(acc), _p(cnt), AX, AY, AZ, Cc, _p(out), X, Y, Z, _lo3(lo), int(flip_mask), _p(bad), _s()),
              "fmri_tile_finalize_flip")
    return out


def tile_finalize_flip_weighted(acc, wsum, out, bad, lo=(0, 0, 0), flip_mask=0):
    """tile_finalize_flip with the float64 weight sums wsum (AX, AY, AZ) in place of the counts: out = acc / wsum of the window, mirrored; bad
    counts the window's voxels with wsum <= 0 (fmri_tile_finalize_flip_weighted)"""
    _need_cuda(acc, wsum, out, bad)
    if acc.dim() != 4 or out.dim() != 4 or tuple(wsum.shape) != tuple(acc.shape[:3]) or out.shape[3] != acc.shape[3]:
        raise ValueError("tile_finalize_flip_weighted: acc (AX, AY, AZ, C), wsum (AX, AY, AZ), out (X, Y, Z, C) (got %s, %s, %s)" % (
            tuple(acc.shape), tuple(wsum.shape), tuple(out.shape)))
    if acc.dtype != torch.float64 or out.dtype != torch.float64 or wsum.dtype != torch.float64 or bad.dtype != torch.int32:
        raise TypeError("tile_finalize_flip_weighted: float64 acc, wsum and out, int32 bad")
    AX, AY, AZ, Cc = acc.shape
    X, Y, Z = out.shape[:3]
    with torch.cuda.device(out.device):
        check(lib().fmri_tile_finalize_flip_weighted(_p(acc), _p(wsum), AX, AY, AZ, Cc, _p(out), X, Y, Z, _lo3(lo), int(flip_mask), _p(bad),
                                                     _s()), "fmri_tile_finalize_flip_weighted")
    return out


MAX_LABELS = 32


def label_values(values):
    """the label values of the multi-label kernels as the host byte array they read at enqueue: 1 to 32 distinct integers in 1..255"""
    import ctypes
    vals = [int(v) for v in values]
    if not 1 <= len(vals) <= MAX_LABELS or any(v != w or not 1 <= v <= 255 for v, w in zip(vals, values)) or len(set(vals)) != len(vals):
        raise ValueError("labels: 1 to %d distinct integers in 1..255 (got %r)" % (MAX_LABELS, list(values)))
    return (ctypes.c_uint8 * len(vals))(*vals)


def labels_expand_u8(lab, values, out=None):
    """out (*lab.shape, L) uint8, channels last = (lab == values[l]); a byte that is no label - background included - gives a zero row.
    One launch whatever lab's shape (a whole batch of label patches)."""
    vals = label_values(values)
    if out is None:
        out = torch.empty(tuple(lab.shape) + (len(vals),), dtype=torch.uint8, device=lab.device)
    _need_cuda(lab, out)
    if lab.dtype != torch.uint8 or out.dtype != torch.uint8 or out.numel() != lab.numel() * len(vals):
        raise ValueError("labels_expand_u8: uint8 label map and a uint8 output of L times its size")
    check(lib().fmri_labels_expand_u8(_p(lab), lab.numel(), vals, len(vals), _p(out), _s()), "fmri_labels_expand_u8")
    return out


def tile_finalize_labels(acc, cnt, out, bad, threshold, values):
    """out uint8 like cnt: the label map of acc / cnt (tile_finalize's division) - C == 1: values[0] where the mean > threshold; C > 1:
    values[first argmax], 0 where the maximum < threshold"""
    _need_cuda(acc, cnt, out, bad)
    vals = label_values(values)
    Cc = acc.shape[-1]
    if len(vals) != Cc or out.dtype != torch.uint8 or out.numel() != cnt.numel():
        raise ValueError("tile_finalize_labels: %d label values for %d channels, uint8 output of cnt's size" % (len(vals), Cc))
    check(lib().fmri_tile_finalize_labels(_p(acc), _p(cnt), _p(out), _p(bad), cnt.numel(), Cc, float(threshold), vals, _s()),
          "fmri_tile_finalize_labels")


def tile_finalize_labels_weighted(acc, wsum, out, bad, threshold, values):
    """tile_finalize_labels with the float64 weight sums wsum in place of the counts: the label map of acc / wsum; wsum <= 0 gives 0 and counts
    in bad (fmri_tile_finalize_labels_weighted)"""
    _need_cuda(acc, wsum, out, bad)
    vals = label_values(values)
    Cc = acc.shape[-1]
    if len(vals) != Cc or out.dtype != torch.uint8 or out.numel() != wsum.numel() or acc.numel() != wsum.numel() * Cc:
        raise ValueError("tile_finalize_labels_weighted: %d label values for %d channels, uint8 output of wsum's size" % (len(vals), Cc))
    if acc.dtype != torch.float64 or wsum.dtype != torch.float64 or bad.dtype != torch.int32:
        raise TypeError("tile_finalize_labels_weighted: float64 acc and wsum, int32 bad")
    check(lib().fmri_tile_finalize_labels_weighted(_p(acc), _p(wsum), _p(out), _p(bad), wsum.numel(), Cc, float(threshold), vals, _s()),
          "fmri_tile_finalize_labels_weighted")


def label_sums(probs, y_true, n_labels, lsums):
    """lsums float64 [3 * L] (overwritten) = per label {sum y*p, sum y, sum p} of probs fp32 / y_true uint8 [nvox * L], label = index % L"""
    _need_cuda(probs, y_true, lsums)
    n = probs.numel()
    if probs.dtype != torch.float32 or y_true.dtype != torch.uint8 or y_true.numel() != n or n % n_labels or lsums.dtype != torch.float64 \
            or lsums.numel() < 3 * n_labels:
        raise ValueError("label_sums: fp32 probs and uint8 targets of nvox * L elements, 3 * L float64 sums")
    check(lib().fmri_label_sums(_p(probs), _p(y_true), n // n_labels, n_labels, _p(lsums), _s()), "fmri_label_sums")


def cast(src, dst):
    _need_cuda(src, dst)
    check(lib().fmri_cast(_p(src), dt(src), _p(dst), dt(dst), src.numel(), _s()), "fmri_cast")
    return dst


def norm_act_fwd(x, gamma, beta, y, stats, ws, per_instance, eps=1e-3, eps_on_std=False, act=ACT_RELU, alpha=0.0):
    """x,y [N,...,C]; stats [G,C,3] fp32; ws [G,C,2] fp64 scratch"""
    _need_cuda(x, gamma, beta, y, stats, ws)
    N, Cc = x.shape[0], x.shape[-1]
    V = x.numel() // (N * Cc)
    check(lib().fmri_norm_act_fwd(_p(x), _p(gamma), _p(beta), _p(y), _p(stats), _p(ws), N, V, Cc, int(per_instance), float(eps),
                                  int(eps_on_std), act, float(alpha), dt(x), _s()), "fmri_norm_act_fwd")
    return y


def norm_act_bwd(x, y, dy, gamma, stats, dx, dgamma, dbeta, ws, per_instance, act=ACT_RELU, alpha=0.0, beta=None):
    """beta given: the sign of the block's output comes from x (recomputed exactly as the forward formed it), y is not read (may be None)"""
    _need_cuda(x, y, dy, gamma, stats, dx, dgamma, dbeta, ws, beta)
    N, Cc = x.shape[0], x.shape[-1]
    V = x.numel() // (N * Cc)
    if beta is not None:
        check(lib().fmri_norm_act_bwd_x(_p(x), _p(dy), _p(gamma), _p(beta), _p(stats), _p(dx), _p(dgamma), _p(dbeta), _p(ws), N, V, Cc,
                                        int(per_instance), act, float(alpha), dt(x), _s()), "fmri_norm_act_bwd_x")
        return dx
    check(lib().fmri_norm_act_bwd(_p(x), _p(y), _p(dy), _p(gamma), _p(stats), _p(dx), _p(dgamma), _p(dbeta), _p(ws), N, V, Cc,
                                  int(per_instance), act, float(alpha), dt(x), _s()), "fmri_norm_act_bwd")
    return dx


# ---- normalisation tails of the conv launches (include/fmri_hip.h: "Normalisation tails")
def conv3d_fwd_ntail_ok(C0, C1, Cout, N, D, H, W, dtype):
    return bool(lib().fmri_conv3d_fwd_ntail_ok(C0, C1, Cout, N, D, H, W, BF16 if dtype == torch.bfloat16 else F32))


def norm_tail_ws_doubles(G, C):
    """fp64 elements of the `ws` the tail entry points need (the totals [G,C,2] in front + one block per workgroup of the persistent launch)"""
    return int(lib().fmri_norm_tail_ws_doubles(int(G), int(C)))


def conv3d_fwd_stats(src0, src1, w, bias, y, ws, per_instance, up0=False, act=ACT_NONE, alpha=0.0):
    """conv3d_fwd whose epilogue leaves {sum y, sum y^2} per (group, channel) in front of ws (fp64, norm_tail_ws_doubles(G, Cout) elements).
    ws must be ZERO on entry (allocate it zeroed): no fmri_norm_* / *_stats call clears it in front any more - the last reader of the sums
    (norm_act_fwd_pre / norm_act_bwd_pre / the fold kernel) leaves it zero for the next call.  After a call sequence that was interrupted
    between the summing launch and its reader, zero it again before reuse."""
    _need_cuda(src0, src1, w, bias, y, ws)
    N, D, H, W, Cout = y.shape
    c0, c1 = src0.shape[-1], (0 if src1 is None else src1.shape[-1])
    check(lib().fmri_conv3d_fwd_stats(_p(src0), c0, int(up0), _p(src1), c1, _p(w), _p(bias), _p(y), N, D, H, W, Cout, act, float(alpha), _p(ws),
                                      int(per_instance), dt(y), _s()), "fmri_conv3d_fwd_stats")
    return y


def conv3d_upcat_fwd_stats(src0_low, src1, w_up_f, w_sk_f, bias, y, ws, per_instance, act=ACT_NONE, alpha=0.0):
    _need_cuda(src0_low, src1, w_up_f, w_sk_f, bias, y, ws)
    N, D, H, W, Cout = y.shape
    check(lib().fmri_conv3d_upcat_fwd_stats(_p(src0_low), src0_low.shape[-1], _p(src1), src1.shape[-1], _p(w_up_f), _p(w_sk_f), _p(bias), _p(y),
                                            N, D, H, W, Cout, act, float(alpha), _p(ws), int(per_instance), dt(y), _s()),
          "fmri_conv3d_upcat_fwd_stats")
    return y


def norm_act_fwd_pre(x, gamma, beta, y, stats, ws, per_instance, eps=1e-3, eps_on_std=False, act=ACT_RELU, alpha=0.0):
    """norm_act_fwd with the sums {sum x, sum x^2} already in ws (conv3d_fwd_stats / conv3d_upcat_fwd_stats)"""
    _need_cuda(x, gamma, beta, y, stats, ws)
    N, Cc = x.shape[0], x.shape[-1]
    V = x.numel() // (N * Cc)
    check(lib().fmri_norm_act_fwd_pre(_p(x), _p(gamma), _p(beta), _p(y), _p(stats), _p(ws), N, V, Cc, int(per_instance), float(eps),
                                      int(eps_on_std), act, float(alpha), dt(x), _s()), "fmri_norm_act_fwd_pre")
    return y


def norm_moving_update(stats, moving_mean, moving_var, M, momentum=0.99, eps=1e-3):
    """Keras BatchNormalization moving mean / variance after a training forward (one launch)"""
    _need_cuda(stats, moving_mean, moving_var)
    check(lib().fmri_norm_moving_update(_p(stats), _p(moving_mean), _p(moving_var), moving_mean.numel(), float(M), float(momentum), float(eps), _s()),
          "fmri_norm_moving_update")


def norm_scale_shift(stats, gamma, beta, nss):
    """nss [G,C,2] fp32 = {scale, shift} of the apply pass (z = fma(x, scale, shift))"""
    _need_cuda(stats, gamma, beta, nss)
    check(lib().fmri_norm_scale_shift(_p(stats), _p(gamma), _p(beta), _p(nss), stats.shape[0], stats.shape[1], _s()), "fmri_norm_scale_shift")
    return nss


def conv3d_dgrad_norm(dy, w_dgrad, x, nss, dz, ws, per_instance, act=ACT_RELU, alpha=0.0):
    """conv3d_dgrad into a normalised block: dz = dgrad * act'(z(x)), ws [G,Cin,2] = {sum dz, sum dz * x}"""
    _need_cuda(dy, w_dgrad, x, nss, dz, ws)
    N, D, H, W, Cin = dz.shape
    check(lib().fmri_conv3d_dgrad_norm(_p(dy), dy.shape[-1], _p(w_dgrad), _p(x), _p(nss), _p(dz), N, D, H, W, Cin, act, float(alpha), _p(ws),
                                       int(per_instance), dt(dz), _s()), "fmri_conv3d_dgrad_norm")
    return dz


def norm_act_bwd_pre(x, dz, gamma, stats, dx, dgamma, dbeta, ws, per_instance):
    _need_cuda(x, dz, gamma, stats, dx, dgamma, dbeta, ws)
    N, Cc = x.shape[0], x.shape[-1]
    V = x.numel() // (N * Cc)
    check(lib().fmri_norm_act_bwd_pre(_p(x), _p(dz), _p(gamma), _p(stats), _p(dx), _p(dgamma), _p(dbeta), _p(ws), N, V, Cc, int(per_instance),
                                      dt(x), _s()), "fmri_norm_act_bwd_pre")
    return dx


def deconv_fwd(x, w, b, y, planar=False):
    """x [N,D,H,W,Cin], w [8,Cout,Cin] (compute dtype), y [N,2D,2H,2W,Cout]"""
    _need_cuda(x, w, b, y)
    N, D, H, W, Cin = x.shape
    Cout = w.shape[1]
    check(lib().fmri_deconv3d_k2s2_fwd(_p(x), _p(w), _p(b), _p(y), N, D, H, W, Cin, Cout, dt(x), int(planar), _s()),
          "fmri_deconv3d_k2s2_fwd")
    return y


def deconv_bwd(x, w, dy, dx, dw, db, dy_off=0, xmask=None, planar=False):
    _need_cuda(x, w, dy, dx, dw, db, xmask)
    N, D, H, W, Cin = x.shape
    Cout = w.shape[1]
    check(lib().fmri_deconv3d_k2s2_bwd(_p(x), _p(w), _p(dy), dy.shape[-1], dy_off, _p(xmask), _p(dx), _p(dw), _p(db), N, D, H, W, Cin,
                                       Cout, dt(x), int(planar), _s()), "fmri_deconv3d_k2s2_bwd")


def conv_direct_fwd(x, w, bias, y, ksize, stride, act=ACT_NONE, alpha=0.0, planar=False):
    """x [N,D,H,W,Cin], w [k^3,Cout,Cin] (compute dtype), y [N,ceil(D/s),ceil(H/s),ceil(W/s),Cout]; planar: x [1,S,H,W,Cin] 2-D slices,
    the stride applies to H and W only"""
    _need_cuda(x, w, bias, y)
    N, D, H, W, Cin = x.shape
    Cout = w.shape[1]
    if planar:
        assert N == 1
        check(lib().fmri_conv2d_direct_fwd(_p(x), _p(w), _p(bias), _p(y), D, H, W, Cin, Cout, ksize, stride, act, float(alpha), dt(x), _s()),
              "fmri_conv2d_direct_fwd")
        return y
    check(lib().fmri_conv3d_direct_fwd(_p(x), _p(w), _p(bias), _p(y), N, D, H, W, Cin, Cout, ksize, stride, act, float(alpha), dt(x), _s()),
          "fmri_conv3d_direct_fwd")
    return y


def conv_direct_bwd(x, w, dy, dx, dw, db, ksize, stride, planar=False):
    _need_cuda(x, w, dy, dx, dw, db)
    N, D, H, W, Cin = x.shape
    Cout = w.shape[1]
    if planar:
        assert N == 1
        check(lib().fmri_conv2d_direct_bwd(_p(x), _p(w), _p(dy), _p(dx), _p(dw), _p(db), D, H, W, Cin, Cout, ksize, stride, dt(x), _s()),
              "fmri_conv2d_direct_bwd")
        return
    check(lib().fmri_conv3d_direct_bwd(_p(x), _p(w), _p(dy), _p(dx), _p(dw), _p(db), N, D, H, W, Cin, Cout, ksize, stride, dt(x), _s()),
          "fmri_conv3d_direct_bwd")


def add(a, b, y):
    _need_cuda(a, b, y)
    check(lib().fmri_add(_p(a), _p(b), _p(y), a.numel(), dt(a), _s()), "fmri_add")
    return y


def channel_scale(x, scale, y):
    """x,y [N,...,C]; scale fp32 [N,C]"""
    _need_cuda(x, scale, y)
    N, Cc = x.shape[0], x.shape[-1]
    check(lib().fmri_channel_scale(_p(x), _p(scale), _p(y), N, x.numel() // (N * Cc), Cc, dt(x), _s()), "fmri_channel_scale")
    return y


def slice_channels(src, off, dst, accumulate=False):
    """dst [...,C] (+)= src[..., off:off+C]"""
    _need_cuda(src, dst)
    Cc = dst.shape[-1]
    check(lib().fmri_slice_channels(_p(src), src.shape[-1], off, _p(dst), Cc, dst.numel() // Cc, int(accumulate), dt(dst), _s()),
          "fmri_slice_channels")
    return dst


def act_bwd(y, dy, dx, act, alpha=0.0):
    _need_cuda(y, dy, dx)
    check(lib().fmri_act_bwd(_p(y), _p(dy), _p(dx), act, float(alpha), y.numel(), dt(y), _s()), "fmri_act_bwd")
    return dx


LOSS_KINDS = {"dice_coefficient_loss": 0, "binary_crossentropy_loss": 1, "dice_and_xent": 2, "focal_loss": 3, "vod_coefficient_loss": 4,
              "double_dice_loss": 5, "weighted_dice_coefficient_loss": 6}
LOSS_WEIGHTED_DICE = 6          # not a kind of fmri_sigmoid_loss_bwd: per-(sample, label) sums, fmri_weighted_dice_fwd / _bwd
WEIGHTED_DICE_SMOOTH = 1e-5     # reference metrics.py:39
# The overlap losses of fmri_overlap_coeffs / fmri_overlap_loss_bwd (per-label sums): loss_kind = LOSS_OVERLAP + the kernels' kind 0..4
LOSS_OVERLAP = 7
LOSS_KINDS.update({"tversky_loss": 7, "focal_tversky_loss": 8, "label_tversky_loss": 9, "label_focal_tversky_loss": 10,
                   "generalised_dice_loss": 11})
GDL_SMOOTH = 1e-5
# An engine's sums tensor: the 16 metric sums, the [L][3] label sums, then (overlap losses only) the boundary sum Bd, the [L][2] coefficient
# pairs right-aligned in front of the two value slots, so that the loss value sits at ONE index whatever L is
SUMS_BD = 16 + 3 * MAX_LABELS                       # 112
SUMS_OVERLAP_VALUE = SUMS_BD + 2 + 2 * MAX_LABELS   # 178: the loss value, 179: the value without the boundary term
SUMS_TOTAL = SUMS_OVERLAP_VALUE + 2


def is_overlap_loss(kind):
    return LOSS_OVERLAP <= int(kind) < LOSS_OVERLAP + 5


def boundary_sum(probs, y_true, dist, bd):
    """bd float64 [1] (overwritten) = sum (1 - 2 y) * dist * p over the voxels of a single-label batch; dist: the fp32 distance mask"""
    _need_cuda(probs, y_true, dist, bd)
    n = probs.numel()
    if probs.dtype != torch.float32 or dist.dtype != torch.float32 or y_true.dtype != torch.uint8 or y_true.numel() != n or dist.numel() != n \
            or bd.dtype != torch.float64 or bd.numel() < 1:
        raise ValueError("boundary_sum: fp32 probs and distances, uint8 targets of one size (single label), one float64 sum")
    check(lib().fmri_boundary_sum(_p(probs), _p(y_true), _p(dist), n, _p(bd), _s()), "fmri_boundary_sum")


def overlap_coeffs(lsums, sums, coef, n_labels, kind, alpha=0.5, beta=0.5, gamma=1.0, smooth=1.0, bd=None, boundary_weight=0.0):
    """coef float64 [2 * L + 2] = the (A_l, B_l) pairs, the loss value and the value without the boundary term, from lsums [3 * L]
    (label_sums), the 16 metric sums and, for the boundary term, bd (boundary_sum): one single-wave launch (include/fmri_hip.h)"""
    _need_cuda(lsums, sums, coef, bd)
    L = int(n_labels)
    if any(t.dtype != torch.float64 for t in (lsums, sums, coef) + ((bd,) if bd is not None else ())) or lsums.numel() < 3 * L \
            or sums.numel() < 16 or coef.numel() < 2 * L + 2:
        raise ValueError("overlap_coeffs: float64 lsums [3 L], sums [16], coef [2 L + 2]")
    check(lib().fmri_overlap_coeffs(_p(lsums), _p(sums), _p(bd), _p(coef), L, int(kind), float(alpha), float(beta), float(gamma),
                                    float(smooth), float(boundary_weight), _s()), "fmri_overlap_coeffs")


def overlap_loss_bwd(probs, y_true, coef, dlogits, n_labels, dist=None, boundary_scale=0.0, grad_scale=1.0):
    """dlogits = grad_scale * (A_l y + B_l + boundary_scale * (1 - 2 y) dist) * p (1 - p), element [v * L + l]"""
    _need_cuda(probs, y_true, coef, dlogits, dist)
    L, n = int(n_labels), probs.numel()
    if probs.dtype != torch.float32 or dlogits.dtype != torch.float32 or y_true.dtype != torch.uint8 or coef.dtype != torch.float64 \
            or L < 1 or n % L or y_true.numel() != n or dlogits.numel() != n or coef.numel() < 2 * L \
            or (dist is not None and (dist.dtype != torch.float32 or dist.numel() * L != n)):
        raise ValueError("overlap_loss_bwd: fp32 probs / dlogits and uint8 targets of nvox * L elements, float64 coef [2 L], fp32 dist [nvox]")
    check(lib().fmri_overlap_loss_bwd(_p(probs), _p(y_true), _p(dist), _p(coef), _p(dlogits), n // L, L, float(boundary_scale),
                                      float(grad_scale), _s()), "fmri_overlap_loss_bwd")


def weighted_dice_fwd(probs, y_true, gsums, sums, nsamples, n_labels, smooth=WEIGHTED_DICE_SMOOTH):
    """per-(sample, label) Dice sums of probs / y_true [(n * vox + v) * L + l] into gsums [nsamples * L, 3] (float64, zeroed by the call);
    sums[10] += sum of the groups' Dice coefficients, sums[11] += group count (reference metrics.py:39-51)"""
    _need_cuda(probs, y_true, gsums, sums)
    assert y_true.dtype == torch.uint8 and gsums.dtype == torch.float64 and sums.dtype == torch.float64 and sums.numel() >= 16
    vox = probs.numel() // (nsamples * n_labels)
    assert vox * nsamples * n_labels == probs.numel() == y_true.numel() and gsums.numel() >= 3 * nsamples * n_labels
    check(lib().fmri_weighted_dice_fwd(_p(probs), _p(y_true), _p(gsums), _p(sums), nsamples, vox, n_labels, float(smooth), _s()), "fmri_weighted_dice_fwd")


def weighted_dice_bwd(probs, y_true, gsums, sums, dlogits, nsamples, n_labels, smooth=WEIGHTED_DICE_SMOOTH, grad_scale=1.0):
    _need_cuda(probs, y_true, gsums, sums, dlogits)
    vox = probs.numel() // (nsamples * n_labels)
    check(lib().fmri_weighted_dice_bwd(_p(probs), _p(y_true), _p(gsums), _p(sums), _p(dlogits), nsamples, vox, n_labels, float(smooth),
                                       float(grad_scale), _s()), "fmri_weighted_dice_bwd")


def sigmoid_loss_bwd(probs, y_true, sums, dlogits, kind, param=1.0, smooth=1.0, grad_scale=1.0, weight=None):
    _need_cuda(probs, y_true, sums, dlogits, weight)
    if weight is not None:
        check(lib().fmri_sigmoid_loss_bwd_weighted(_p(probs), _p(y_true), _p(weight), _p(sums), _p(dlogits), probs.numel(), int(kind), float(param),
                                                   float(smooth), float(grad_scale), _s()), "fmri_sigmoid_loss_bwd_weighted")
        return
    check(lib().fmri_sigmoid_loss_bwd(_p(probs), _p(y_true), _p(sums), _p(dlogits), probs.numel(), int(kind), float(param), float(smooth),
                                      float(grad_scale), _s()), "fmri_sigmoid_loss_bwd")


def loss_value_from_sums(s, kind, param=1.0, smooth=1.0):
    """host-side value of the loss `kind` from the 16 metric sums (float64); an overlap loss: the value fmri_overlap_coeffs wrote, which
    rides behind the sums (s = the engine's log_sums)"""
    if is_overlap_loss(kind):
        if len(s) <= SUMS_OVERLAP_VALUE:
            raise ValueError("an overlap loss takes its value from slot %d of the engine's log_sums(), got %d sums" % (SUMS_OVERLAP_VALUE, len(s)))
        return float(s[SUMS_OVERLAP_VALUE])
    I, Sy, Sp, n = float(s[0]), float(s[1]), float(s[2]), float(s[7])
    dice = (2 * I + smooth) / (Sy + Sp + smooth)
    if kind == 0:
        return -dice
    if kind == 1:
        return float(s[8]) / n
    if kind == 2:
        return -dice + param * float(s[8]) / n
    if kind == 3:
        return float(s[9])
    if kind == 4:
        return -(I + smooth) / (Sy + Sp - I + smooth)
    if kind == LOSS_WEIGHTED_DICE:
        return -float(s[10]) / float(s[11])          # mean over the (sample, label) groups of the (all-reduced) per-group Dice
    return -dice + param * (2 * (Sp - I) + smooth) / ((n - Sy) + Sp + smooth)


def clock_stamp(out16):
    """one {s_memtime, s_memrealtime} pair per XCD into out16 (int64[16], device) on the current stream (include/fmri_hip.h: fmri_clock_stamp)"""
    _need_cuda(out16)
    assert out16.dtype == torch.int64 and out16.numel() >= 16 and out16.is_contiguous()
    check(lib().fmri_clock_stamp(_p(out16), _s()), "fmri_clock_stamp")


def clock_ghz(stamp0, stamp1):
    """average shader clock between two stamps: median over the XCDs both stamps reached of d(memtime) / d(memrealtime) x 0.1 GHz;
    returns (GHz or None, per-XCD list)"""
    a, b = stamp0.cpu().numpy().astype("int64"), stamp1.cpu().numpy().astype("int64")
    per = []
    for x in range(8):
        dt, dr = int(b[2 * x] - a[2 * x]), int(b[2 * x + 1] - a[2 * x + 1])
        if a[2 * x + 1] != 0 and dr > 0 and dt > 0:
            per.append(dt / dr * 0.1)
    if not per:
        return None, per
    srt = sorted(per)
    return srt[len(srt) // 2], per


def set_deterministic(grad, shadow, scratch=None):
    """register (fp32 gradient buffer, zeroed int64 shadow of the same length) for bit-reproducible gradient accumulation, or (None, None)
    to switch it off (include/fmri_hip.h: fmri_set_deterministic); process-wide.  scratch: the slab of the ordered normalisation statistics
    (any contiguous device tensor of norm_det_workspace_bytes; the caller keeps it alive) - without one the normalisation entry points
    refuse to run while the registration is on"""
    if grad is None:
        check(lib().fmri_set_deterministic_scratch(0, 0), "fmri_set_deterministic_scratch")
        check(lib().fmri_set_deterministic(0, 0, 0), "fmri_set_deterministic")
        return
    _need_cuda(grad, shadow, scratch)
    assert grad.dtype == torch.float32 and shadow.dtype == torch.int64 and shadow.numel() == grad.numel() and grad.is_contiguous() and shadow.is_contiguous()
    set_deterministic_scratch(scratch)
    check(lib().fmri_set_deterministic(_p(grad), _p(shadow), grad.numel()), "fmri_set_deterministic")


def set_deterministic_scratch(scratch):
    """the slab of the ordered normalisation statistics on its own (None takes it back): a frozen network that holds no gradient
    registration of its own grows the registered engine's slab through this"""
    if scratch is None:
        check(lib().fmri_set_deterministic_scratch(0, 0), "fmri_set_deterministic_scratch")
        return
    _need_cuda(scratch)
    assert scratch.is_contiguous()
    check(lib().fmri_set_deterministic_scratch(_p(scratch), scratch.numel() * scratch.element_size()), "fmri_set_deterministic_scratch")


def norm_det_workspace_bytes(N, V, C, per_instance):
    """bytes of the deterministic scratch one norm_act_fwd / norm_act_bwd call on [N][V][C] needs"""
    return int(lib().fmri_norm_det_workspace_bytes(int(N), int(V), int(C), int(per_instance)))


def deterministic_finish(grad, shadow):
    """grad += shadow * 2^-40, shadow = 0: once per backward pass, behind every gradient kernel"""
    _need_cuda(grad, shadow)
    check(lib().fmri_deterministic_finish(_p(grad), _p(shadow), grad.numel(), _s()), "fmri_deterministic_finish")


def conv3d_wgrad_workspace_bytes(C0, C1, Cout, N, D, H, W, dtype, planar=False):
    d = BF16 if dtype == torch.bfloat16 else F32
    return int(lib().fmri_conv3d_wgrad_workspace_bytes(C0, C1, Cout, N, D, H, W, d, int(planar)))


# ---------------------------------------------------------------------------------------------- patch sampler / intensity augmentation
U8 = 2


def _dt_any(t):
    return U8 if t.dtype == torch.uint8 else dt(t)


def minmax(x, out2):
    _need_cuda(x, out2)
    check(lib().fmri_minmax(_p(x), x.numel(), dt(x), _p(out2), _s()), "fmri_minmax")
    return out2


def rescale_intensity(x, stats, contrast, lo=0.0, hi=0.0, mult=1.0):
    _need_cuda(x, stats)
    check(lib().fmri_rescale_intensity(_p(x), x.numel(), dt(x), _p(stats), 1 if contrast else 0, float(lo), float(hi), float(mult), _s()),
          "fmri_rescale_intensity")
    return x


def noise_augment(x, stats, noise, kind, sigma):
    _need_cuda(x, stats, noise)
    assert noise.dtype == torch.float32 and noise.numel() == x.numel()
    check(lib().fmri_noise_augment(_p(x), x.numel(), dt(x), _p(stats), _p(noise), int(kind), float(sigma), _s()), "fmri_noise_augment")
    return x


# ---------------------------------------------------------------------------------------------- up-sample + concat + conv, parity form
def conv3d_upcat_ok(C0, C1, Cout, D, H, W, dtype, planar=False):
    """bit 0: forward / input gradients, bit 1: weight gradient.  planar: 2-D slices [1][S][H][W][C] (D = S is not up-sampled)"""
    f = lib().fmri_conv2d_upcat_ok if planar else lib().fmri_conv3d_upcat_ok
    return int(f(C0, C1, Cout, D, H, W, BF16 if dtype == torch.bfloat16 else F32))


def conv3d_pack_up_weights(w, C0, C1, up_f=None, up_d=None, sk_f=None, sk_d=None, planar=False):
    _need_cuda(w, up_f, up_d, sk_f, sk_d)
    Cout = w.shape[1]
    ref = next(t for t in (up_f, up_d, sk_f, sk_d) if t is not None)
    f = lib().fmri_conv2d_pack_up_weights if planar else lib().fmri_conv3d_pack_up_weights
    check(f(_p(w), C0, C1, Cout, _p(up_f), _p(up_d), _p(sk_f), _p(sk_d), dt(ref), _s()), "fmri_conv%dd_pack_up_weights" % (2 if planar else 3))


def conv3d_upcat_fwd(src0_low, src1, w_up_f, w_sk_f, bias, y, act=ACT_RELU, alpha=0.0, planar=False):
    _need_cuda(src0_low, src1, w_up_f, w_sk_f, bias, y)
    N, D, H, W, Cout = y.shape
    c0, c1 = src0_low.shape[-1], (0 if src1 is None else src1.shape[-1])
    if planar:
        assert N == 1
        check(lib().fmri_conv2d_upcat_fwd(_p(src0_low), c0, _p(src1), c1, _p(w_up_f), _p(w_sk_f), _p(bias), _p(y), D, H, W, Cout, act, float(alpha),
                                          dt(y), _s()), "fmri_conv2d_upcat_fwd")
        return y
    check(lib().fmri_conv3d_upcat_fwd(_p(src0_low), c0, _p(src1), c1, _p(w_up_f), _p(w_sk_f), _p(bias), _p(y), N, D, H, W,
                                      Cout, act, float(alpha), dt(y), _s()), "fmri_conv3d_upcat_fwd")
    return y


def conv3d_upcat_dgrad(dy, w_up_d, w_sk_d, mask_low, mask_skip, dx_low, dx_skip, planar=False):
    _need_cuda(dy, w_up_d, w_sk_d, mask_low, mask_skip, dx_low, dx_skip)
    N, D, H, W, Cout = dy.shape
    c0, c1 = dx_low.shape[-1], (0 if dx_skip is None else dx_skip.shape[-1])
    if planar:
        assert N == 1
        check(lib().fmri_conv2d_upcat_dgrad(_p(dy), Cout, _p(w_up_d), _p(w_sk_d), _p(mask_low), _p(mask_skip), _p(dx_low), _p(dx_skip), D, H, W,
                                            c0, c1, dt(dy), _s()), "fmri_conv2d_upcat_dgrad")
        return
    check(lib().fmri_conv3d_upcat_dgrad(_p(dy), Cout, _p(w_up_d), _p(w_sk_d), _p(mask_low), _p(mask_skip), _p(dx_low), _p(dx_skip), N, D, H, W,
                                        c0, c1, dt(dy), _s()), "fmri_conv3d_upcat_dgrad")


def conv3d_stride2_fwd(x, w_s2_fwd, bias, y):
    """Conv3D(3x3x3, strides 2, 'same') forward: x [N,D,H,W,Cin] (even dims), w_s2_fwd [8,8,Cout,Cin] (StridedParity.pack), bias fp32 [Cout] or
    None (added in the fp32 accumulators), y [N,D/2,H/2,W/2,Cout] (fmri_conv3d_stride2_fwd)"""
    _need_cuda(x, w_s2_fwd, bias, y)
    N, D, H, W, Cin = x.shape
    Cout = y.shape[-1]
    assert tuple(y.shape) == (N, D // 2, H // 2, W // 2, Cout) and tuple(w_s2_fwd.shape) == (8, 8, Cout, Cin)
    assert bias is None or (bias.dtype == torch.float32 and bias.numel() >= Cout)
    check(lib().fmri_conv3d_stride2_fwd(_p(x), Cin, _p(w_s2_fwd), _p(bias), _p(y), N, D, H, W, Cout, dt(x), _s()), "fmri_conv3d_stride2_fwd")
    return y


def conv3d_upcat_wgrad(src0_low, src1, dy, dw, db, dwc_scratch, workspace=None, planar=False):
    _need_cuda(src0_low, src1, dy, dw, db, dwc_scratch, workspace)
    N, D, H, W, Cout = dy.shape
    C0, C1 = src0_low.shape[-1], (0 if src1 is None else src1.shape[-1])
    assert dwc_scratch.dtype == torch.float32 and dwc_scratch.numel() >= (16 if planar else 64) * Cout * C0
    nws = 0 if workspace is None else workspace.numel() * workspace.element_size()
    if planar:
        assert N == 1
        check(lib().fmri_conv2d_upcat_wgrad(_p(src0_low), C0, _p(src1), C1, _p(dy), _p(dw), _p(db), _p(dwc_scratch), D, H, W, Cout, dt(dy),
                                            _p(workspace), nws, _s()), "fmri_conv2d_upcat_wgrad")
        return
    check(lib().fmri_conv3d_upcat_wgrad(_p(src0_low), C0, _p(src1), C1, _p(dy), _p(dw), _p(db), _p(dwc_scratch), N, D, H, W, Cout, dt(dy),
                                        _p(workspace), nws, _s()),
          "fmri_conv3d_upcat_wgrad")


# ---- Deconvolution3D -> concatenate -> Conv3D folded into one parity-form convolution (fmri_hip.deconv_fold holds the weight algebra)
def conv3d_upcat_fwd_bias27(src0_low, src1, w_up_f, w_sk_f, bias27, y, act=ACT_RELU, alpha=0.0):
    """as conv3d_upcat_fwd with the effective bias per border class of the output voxel: bias27 [27, Cout] fp32"""
    _need_cuda(src0_low, src1, w_up_f, w_sk_f, bias27, y)
    N, D, H, W, Cout = y.shape
    assert bias27.dtype == torch.float32 and tuple(bias27.shape) == (27, Cout) and bias27.is_contiguous()
    check(lib().fmri_conv3d_upcat_fwd_bias27(_p(src0_low), src0_low.shape[-1], _p(src1), src1.shape[-1], _p(w_up_f), _p(w_sk_f), _p(bias27), _p(y),
                                             N, D, H, W, Cout, act, float(alpha), dt(y), _s()), "fmri_conv3d_upcat_fwd_bias27")
    return y


def conv3d_upcat_wgrad_parts(src0_low, src1, dy, dw, db, dwc, workspace=None):
    """parity-filter gradients into dwc [8, 8, Cout, C0] fp32 (zeroed by the call), skip columns of dw [27, Cout, C0 + C1] and db accumulated"""
    _need_cuda(src0_low, src1, dy, dw, db, dwc, workspace)
    N, D, H, W, Cout = dy.shape
    C0, C1 = src0_low.shape[-1], src1.shape[-1]
    assert dwc.dtype == torch.float32 and dwc.numel() >= 64 * Cout * C0 and tuple(dw.shape) == (27, Cout, C0 + C1)
    nws = 0 if workspace is None else workspace.numel() * workspace.element_size()
    check(lib().fmri_conv3d_upcat_wgrad_parts(_p(src0_low), C0, _p(src1), C1, _p(dy), _p(dw), _p(db), _p(dwc), N, D, H, W, Cout, dt(dy), _p(workspace),
                                              nws, _s()), "fmri_conv3d_upcat_wgrad_parts")


def border_class_sums(dy, out27):
    """out27 [27, C] fp32 += per-border-class sums of dy [N, D, H, W, C]; the interior class (row 13) is left untouched"""
    _need_cuda(dy, out27)
    N, D, H, W, C = dy.shape
    assert out27.dtype == torch.float32 and tuple(out27.shape) == (27, C) and out27.is_contiguous()
    check(lib().fmri_border_class_sums(_p(dy), _p(out27), N, D, H, W, C, dt(dy), _s()), "fmri_border_class_sums")
    return out27


# ---------------------------------------------------------------------------------------------------- post-processing (fetal_net.postprocess)
def _gaussian_passes(vol, sig, truncate, launch):
    """the separable passes of scipy.ndimage.gaussian_filter (order 0) over the axes of `sig`: an axis whose sigma is ~0 is skipped as
    scipy skips it, any other gets scipy's normalised weights of radius int(truncate * sd + 0.5) on the device and one
    `launch(src, dst, axis, weights, radius)`.  Two buffers ping-pong and `vol` is never written; returns the last destination, or `vol`
    itself when every axis was skipped"""
    a, b = vol, None
    with torch.cuda.device(vol.device):                       # a volume on a non-current GPU: its device's stream, its device's weights
        for axis, sd in enumerate(sig):
            if sd <= 1e-15:
                continue
            radius = int(truncate * sd + 0.5)
            w = torch.from_numpy(gaussian_kernel1d(sd, 0, radius)).to(vol.device)
            b = torch.empty_like(vol) if b is None or b is vol else b
            launch(a, b, axis, w, radius)
            a, b = b, a
    return a


def gaussian_filter_f64(vol, sigma, truncate=4.0):
    """scipy.ndimage.gaussian_filter(vol, sigma) (order 0, mode 'reflect') of a float64 device volume [X,Y,Z]: three separable passes with
    scipy's own weights and summation order - bit-identical to the host result"""
    import numpy as np
    _need_cuda(vol)
    assert vol.dtype == torch.float64 and vol.dim() == 3
    X, Y, Z = vol.shape
    sig = [float(sigma)] * 3 if np.isscalar(sigma) else [float(v) for v in sigma]
    out = _gaussian_passes(vol, sig, truncate, lambda a, b, axis, w, radius: check(
        lib().fmri_correlate1d_f64(_p(a), _p(b), X, Y, Z, axis, _p(w), radius, _s()), "fmri_correlate1d_f64"))
    return out if out is not vol else vol.clone()


def _until_stable(step, device, sweeps=16, limit=100000):
    """run `step(sweeps, changed)` until a batch of sweeps changes nothing (one 4-byte read-back per batch); the flag lives on the
    volume's device (the callers run under torch.cuda.device(volume.device), so _s() is that device's stream)"""
    changed = torch.zeros(1, dtype=torch.int32, device=device)
    done = 0
    while done < limit:
        changed.zero_()
        step(sweeps, changed)
        done += sweeps
        if int(changed.item()) == 0:
            return done
    raise RuntimeError("label propagation did not converge")


# ---- threshold, hole filling and the largest component for L <= MAX_LABELS channels at once: the masks of a voxel are the L low bits of
# one uint32 word (bit l = channel l); a single mask is L = 1
def _words(words, n_labels):
    _need_cuda(words)
    if words.dtype != torch.uint32 or words.dim() != 3 or not 1 <= int(n_labels) <= MAX_LABELS:
        raise ValueError("mask words: a uint32 volume [X,Y,Z] of 1 to %d channel bits" % MAX_LABELS)
    return tuple(words.shape) + (int(n_labels),)


def gaussian_filter_channels_f64(vol4, sigma, truncate=4.0):
    """scipy.ndimage.gaussian_filter(vol4[..., l], sigma) for every channel of a channels-last float64 device volume [X,Y,Z,L]: the
    passes of gaussian_filter_f64 (sigma per spatial axis, an axis whose sigma is ~0 skipped) without splitting the channels apart -
    bit-identical to the host result per channel"""
    import numpy as np
    _need_cuda(vol4)
    if vol4.dtype != torch.float64 or vol4.dim() != 4 or not 1 <= vol4.shape[3] <= MAX_LABELS:
        raise ValueError("gaussian_filter_channels_f64: a float64 volume [X,Y,Z,L] with 1 to %d channels" % MAX_LABELS)
    X, Y, Z, L = vol4.shape
    sig = [float(sigma)] * 3 if np.isscalar(sigma) else [float(v) for v in sigma]
    if len(sig) != 3:
        raise ValueError("gaussian_filter_channels_f64: one sigma, or one per spatial axis")
    out = _gaussian_passes(vol4, sig, truncate, lambda a, b, axis, w, radius: check(
        lib().fmri_correlate1d_cl_f64(_p(a), _p(b), X, Y, Z, L, axis, _p(w), radius, _s()), "fmri_correlate1d_cl_f64"))
    return out if out is not vol4 else vol4.clone()


def threshold_bits_f64(smoothed, thr):
    """words uint32 [X,Y,Z] of a channels-last float64 device volume [X,Y,Z,L]: bit l = smoothed[..., l] > thr"""
    _need_cuda(smoothed)
    if smoothed.dtype != torch.float64 or smoothed.dim() != 4 or not 1 <= smoothed.shape[3] <= MAX_LABELS:
        raise ValueError("threshold_bits_f64: a float64 volume [X,Y,Z,L] with 1 to %d channels" % MAX_LABELS)
    words = torch.empty(smoothed.shape[:3], dtype=torch.uint32, device=smoothed.device)
    with torch.cuda.device(smoothed.device):
        check(lib().fmri_threshold_bits_f64(_p(smoothed), _p(words), words.numel(), smoothed.shape[3], float(thr), _s()),
              "fmri_threshold_bits_f64")
    return words


def binary_fill_holes_bits(words, n_labels):
    """scipy.ndimage.binary_fill_holes (default 6-connectivity) of every channel of the mask words at once; bits n_labels..31 come out
    zero"""
    X, Y, Z, nl = _words(words, n_labels)
    reached, out = torch.empty_like(words), torch.empty_like(words)
    L = lib()
    with torch.cuda.device(words.device):
        check(L.fmri_fill_holes_bits_step(_p(words), _p(reached), 0, X, Y, Z, nl, 0, 0, 0, _s()), "fmri_fill_holes_bits_step")
        _until_stable(lambda k, ch: check(L.fmri_fill_holes_bits_step(_p(words), _p(reached), 0, X, Y, Z, nl, 1, k, _p(ch), _s()),
                                          "fmri_fill_holes_bits_step"), words.device)
        check(L.fmri_fill_holes_bits_step(_p(words), _p(reached), _p(out), X, Y, Z, nl, 2, 0, 0, _s()), "fmri_fill_holes_bits_step")
    return out


def largest_components_bits(words, n_labels):
    """every channel of the mask words reduced to its largest 6-connected component (scipy.ndimage.label + argmax of the sizes per
    channel: ties to the component scipy numbers first, an empty channel stays empty); all channels share the sweeps and the convergence
    flag; bits n_labels..31 come out zero"""
    X, Y, Z, nl = _words(words, n_labels)
    n = words.numel()
    labels = torch.empty(nl * n, dtype=torch.int32, device=words.device)
    counts = torch.empty(nl * (n + 1), dtype=torch.int32, device=words.device)
    best = torch.empty(nl, dtype=torch.int64, device=words.device)
    out = torch.empty_like(words)
    L = lib()
    with torch.cuda.device(words.device):
        check(L.fmri_largest_components_bits_step(_p(words), _p(labels), 0, 0, 0, X, Y, Z, nl, 0, 0, 0, _s()),
              "fmri_largest_components_bits_step")
        _until_stable(lambda k, ch: check(L.fmri_largest_components_bits_step(_p(words), _p(labels), 0, 0, 0, X, Y, Z, nl, 1, k, _p(ch), _s()),
                                          "fmri_largest_components_bits_step"), words.device, sweeps=8)
        check(L.fmri_largest_components_bits_step(_p(words), _p(labels), _p(counts), _p(best), _p(out), X, Y, Z, nl, 2, 0, 0, _s()),
              "fmri_largest_components_bits_step")
    return out


def label_map_from_bits(words, smoothed, values):
    """uint8 [X,Y,Z]: values[l] of the first channel l among the set bits of a voxel's word with the largest smoothed value, 0 where no
    bit is set.  smoothed: float64 [X,Y,Z,L], values: L label values (label_values' rule)"""
    vals = label_values(values)
    X, Y, Z, nl = _words(words, len(vals))
    _need_cuda(smoothed)
    if smoothed.dtype != torch.float64 or tuple(smoothed.shape) != (X, Y, Z, nl) or smoothed.device != words.device:
        raise ValueError("label_map_from_bits: a float64 volume [X,Y,Z,%d] next to the words, %d label values" % (nl, nl))
    out = torch.empty(words.shape, dtype=torch.uint8, device=words.device)
    with torch.cuda.device(words.device):
        check(lib().fmri_label_map_bits(_p(words), _p(smoothed), _p(out), words.numel(), nl, vals, _s()), "fmri_label_map_bits")
    return out


def _edt_sampling(sampling):
    import numpy as np
    if sampling is None:
        return (1.0, 1.0, 1.0)
    sp = [float(sampling)] * 3 if np.isscalar(sampling) else [float(v) for v in sampling]     # a scalar is broadcast, as scipy does
    if len(sp) != 3 or not all(v > 0 and np.isfinite(v) for v in sp):
        raise ValueError("sampling: one positive number, or one per axis of the 3-D volume (got %r)" % (sampling,))
    return tuple(sp)


def _edt(mask, sampling, two_class):
    _need_cuda(mask)
    assert mask.dtype == torch.uint8 and mask.dim() == 3
    X, Y, Z = mask.shape
    sx, sy, sz = _edt_sampling(sampling)
    out = torch.empty(mask.shape, dtype=torch.float64, device=mask.device)
    if mask.numel() == 0:
        return out
    scratch = torch.empty((3 if two_class else 1) * mask.numel(), dtype=torch.float64, device=mask.device)
    name = "fmri_edt_two_class_u8" if two_class else "fmri_edt_u8"
    with torch.cuda.device(mask.device):
        check(getattr(lib(), name)(_p(mask), _p(out), _p(scratch), X, Y, Z, sx, sy, sz, _s()), name)
    return out


def distance_transform_edt_u8(mask, sampling=None):
    """scipy.ndimage.distance_transform_edt(mask, sampling) of a uint8 device volume [X,Y,Z] (nonzero = foreground) -> float64 device
    tensor: the distance of every foreground voxel to the nearest zero voxel, 0 on zero voxels.  Identical to scipy with unit spacing,
    within a few ulp otherwise (csrc/postprocess.hip).  A volume without a zero voxel gives +inf everywhere."""
    return _edt(mask, sampling, False)


def distance_mask_u8(truth, sampling=None):
    """edt(truth) + edt(1 - truth) - the distance of every voxel to the nearest voxel of the other class, the reference's distance mask
    (fetal_net/utils/create_distance_masks.py) - with both fields carried through one set of passes.  +inf everywhere when the volume
    holds a single class."""
    return _edt(truth, sampling, True)


# ---------------------------------------------------------------------------------------------------- spline resampling, median (postprocess.hip)
def _vol_f64(vol):
    _need_cuda(vol)
    if vol.dtype != torch.float64 or vol.dim() != 3 or vol.numel() == 0:
        raise ValueError("a non-empty float64 volume [X,Y,Z] is needed (got %s %s)" % (vol.dtype, tuple(vol.shape)))


def spline_filter_f64(vol, order, axes=(0, 1, 2)):
    """scipy.ndimage.spline_filter1d(., order, axis, mode='mirror') along each of `axes` (ascending, as scipy.ndimage.spline_filter runs
    them) of a float64 device volume [X,Y,Z] -> a new tensor: the B-spline coefficients scipy interpolates with for mode='constant'.
    Orders 0 and 1 need no filter: a copy."""
    _vol_f64(vol)
    if order not in (0, 1, 2, 3):
        raise NotImplementedError("spline order %r" % (order,))
    out = vol.clone()
    if order > 1:
        X, Y, Z = out.shape
        with torch.cuda.device(out.device):
            for axis in sorted(set(int(a) for a in axes)):
                check(lib().fmri_spline_filter1d_f64(_p(out), X, Y, Z, axis, order, _s()), "fmri_spline_filter1d_f64")
    return out


def affine_transform_f64(vol, matrix, offset, output_shape, order, prefilter=True, cval=0.0, axes_orders=None):
    """scipy.ndimage.affine_transform(vol, matrix, offset, output_shape, order=order, mode='constant', cval=cval, prefilter=prefilter) of a
    float64 device volume [X,Y,Z] -> float64 device tensor of `output_shape`.  matrix: 3x3, or 3 numbers for a diagonal one; offset: one
    number or 3.  axes_orders: a spline order per axis instead of `order` for all three (rotate_f64 passes (o, o, 0)); the prefilter runs
    along the axes whose order is above 1."""
    import ctypes
    import numpy as np
    _vol_f64(vol)
    orders = [int(order)] * 3 if axes_orders is None else [int(o) for o in axes_orders]
    if len(orders) != 3 or not all(0 <= o <= 3 for o in orders):
        raise NotImplementedError("spline orders %r" % (orders,))
    if len(set(o for o in orders if o > 1)) > 1:
        raise NotImplementedError("one prefilter order per volume (got %r)" % (orders,))
    M = np.asarray(matrix, dtype=np.float64)
    if M.shape == (3,):
        M = np.diag(M)
    if M.shape != (3, 3):
        raise ValueError("matrix: 3x3 or 3 numbers")
    t = np.broadcast_to(np.asarray(offset, dtype=np.float64), (3,))
    shape = tuple(int(v) for v in output_shape)
    if len(shape) != 3 or min(shape) < 1:
        raise ValueError("output_shape: three positive extents")
    coef = vol
    if prefilter and max(orders) > 1:
        coef = spline_filter_f64(vol, max(orders), [a for a in range(3) if orders[a] > 1])
    A = (ctypes.c_double * 12)(*np.concatenate([M, t[:, None]], axis=1).ravel())
    O = (ctypes.c_int * 3)(*orders)
    out = torch.empty(shape, dtype=torch.float64, device=vol.device)
    X, Y, Z = vol.shape
    with torch.cuda.device(vol.device):
        check(lib().fmri_spline_affine_f64(_p(coef), X, Y, Z, ctypes.addressof(A), ctypes.addressof(O), _p(out), shape[0], shape[1], shape[2],
                                           float(cval), _s()), "fmri_spline_affine_f64")
    return out


def zoom_geometry(shape, factors):
    """output shape and per-axis coordinate ratio of scipy.ndimage.zoom(., factors) (grid_mode=False): m = int(round(n * f)) with Python's
    round (halves to even), ratio (n - 1) / (m - 1), 1 where m == 1.  Pure host arithmetic."""
    import numpy as np
    shape = tuple(int(n) for n in shape)
    f = [float(v) for v in np.broadcast_to(factors, (len(shape),))]
    out_shape = tuple(int(round(n * v)) for n, v in zip(shape, f))
    ratios = tuple(float(n - 1) / float(m - 1) if m > 1 else 1.0 for n, m in zip(shape, out_shape))
    return out_shape, ratios


def zoom_f64(vol, factors, order=3):
    """scipy.ndimage.zoom(vol, factors, order=order) (mode 'constant', cval 0) of a float64 device volume [X,Y,Z]: a diagonal matrix of
    the ratios and a zero offset, so the kernel forms scipy's k * ratio; prefilter along all three axes when order > 1"""
    _vol_f64(vol)
    out_shape, ratios = zoom_geometry(vol.shape, factors)
    if min(out_shape) < 1:
        raise ValueError("zoom factors %r leave no voxel of %r" % (factors, tuple(vol.shape)))
    return affine_transform_f64(vol, ratios, 0.0, out_shape, order)


def rotate_f64(vol, angle, order=3, reshape=True):
    """scipy.ndimage.rotate(vol, angle, axes=(1, 0), reshape=reshape, order=order) of a float64 device volume [n0,n1,slices]: scipy rotates
    plane by plane, i.e. prefilter along axes 0 and 1 and a single tap along the slice axis.  Matrix, output shape and offset are those
    of fetal_net.spline_rotate.rotate (ndimage.rotate's own)."""
    import math
    import numpy as np
    _vol_f64(vol)
    n0, n1, ns = (int(v) for v in vol.shape)
    a = np.deg2rad(angle)
    c, s = math.cos(a), math.sin(a)
    if angle % 360 == 0:
        c, s = 1.0, 0.0
    elif angle % 360 == 90:
        c, s = 0.0, 1.0
    elif angle % 360 == 180:
        c, s = -1.0, 0.0
    elif angle % 360 == 270:
        c, s = 0.0, -1.0
    M = np.array([[c, s], [-s, c]])
    in_shape = np.array([n0, n1])
    if reshape:
        bounds = M @ np.array([[0, 0, n0, n0], [0, n1, 0, n1]], dtype=np.float64)
        out_shape = (np.ptp(bounds, axis=1) + 0.5).astype(int)
    else:
        out_shape = in_shape
    offset = (in_shape - 1) / 2.0 - M @ ((out_shape - 1) / 2.0)
    M3 = np.eye(3)
    M3[:2, :2] = M
    return affine_transform_f64(vol, M3, [offset[0], offset[1], 0.0], (int(out_shape[0]), int(out_shape[1]), ns), order,
                                axes_orders=(order, order, 0))


def median_stack_f64(stack):
    """np.median(stack, axis=0) of a float64 device stack [K, ...], 1 <= K <= 64, finite values -> float64 device tensor"""
    _need_cuda(stack)
    if stack.dtype != torch.float64 or stack.dim() < 2 or stack.numel() == 0:
        raise ValueError("a non-empty float64 stack [K, ...] is needed (got %s %s)" % (stack.dtype, tuple(stack.shape)))
    K = int(stack.shape[0])
    out = torch.empty(stack.shape[1:], dtype=torch.float64, device=stack.device)
    with torch.cuda.device(stack.device):
        check(lib().fmri_median_stack_f64(_p(stack), K, out.numel(), _p(out), _s()), "fmri_median_stack_f64")
    return out


TTA_MAPS = ("mean", "variance", "entropy", "disagreement")


def tta_agreement_f64(stack, threshold=0.5, channels=1, maps=TTA_MAPS, counts=True):
    """What the K variants of a float64 device stack [K, ...] (channels > 1: [K, ..., channels], channels last) agree on, in one pass
    (fmri_tta_agreement_f64, include/fmri_hip.h): a dict of float64 device tensors shaped like stack[0] - 'median' (the bits of
    median_stack_f64) and every map named in `maps` - plus, with counts=True, 'counts': an int64 device tensor (channels, 2K + 1) of
    |median > t|, |v_k > t| and |v_k > t and median > t| per channel.  1 <= K <= 64, 1 <= channels <= 16, finite values."""
    _need_cuda(stack)
    if stack.dtype != torch.float64 or stack.dim() < 2 or stack.numel() == 0:
        raise ValueError("a non-empty float64 stack [K, ...] is needed (got %s %s)" % (stack.dtype, tuple(stack.shape)))
    K, C = int(stack.shape[0]), int(channels)
    if not 1 <= K <= 64:
        raise ValueError("1 to 64 variants are needed (got %d)" % K)
    if not 1 <= C <= 16 or (C > 1 and int(stack.shape[-1]) != C):
        raise ValueError("channels must be 1, or the stack's last extent and at most 16 (got %d for %s)" % (C, tuple(stack.shape)))
    maps = tuple(maps)
    unknown = [m for m in maps if m not in TTA_MAPS]
    if unknown or len(set(maps)) != len(maps):
        raise ValueError("maps must be distinct names of %s (got %r)" % (TTA_MAPS, maps))
    out = {name: torch.empty(stack.shape[1:], dtype=torch.float64, device=stack.device) for name in ("median",) + maps}
    if counts:
        out["counts"] = torch.empty((C, 2 * K + 1), dtype=torch.int64, device=stack.device)
    with torch.cuda.device(stack.device):
        check(lib().fmri_tta_agreement_f64(_p(stack), K, out["median"].numel() // C, C, float(threshold), _p(out["median"]),
                                           _p(out.get("mean")), _p(out.get("variance")), _p(out.get("entropy")),
                                           _p(out.get("disagreement")), _p(out.get("counts")), _s()), "fmri_tta_agreement_f64")
    return out


# ---------------------------------------------------------------------------------------------------- discriminator head (discriminator.hip)
# ---------------------------------------------------------------------------------------------------- intensity preparation (postprocess.hip)
MAP_WINDOW, MAP_MINMAX, MAP_ZSCORE = 0, 1, 2
_MAX_RANKS = 8


def order_stats_f64(vol, ranks):
    """(np.sort(vol, axis=None)[ranks] as a float64 numpy array, the number of NaNs in vol) of a float64 device tensor of any shape: a
    radix select on the device, all ranks in one sweep per digit; more than 8 ranks go in groups of 8.  One read-back at the end."""
    import ctypes
    import numpy as np
    _need_cuda(vol)
    if vol.dtype != torch.float64 or vol.numel() == 0:
        raise ValueError("a non-empty float64 tensor is needed (got %s %s)" % (vol.dtype, tuple(vol.shape)))
    n = vol.numel()
    ranks = [int(r) for r in np.asarray(ranks).ravel()]
    if not ranks:
        raise ValueError("no ranks")
    L = lib()
    groups = (len(ranks) + _MAX_RANKS - 1) // _MAX_RANKS
    with torch.cuda.device(vol.device):
        ws = torch.empty(L.fmri_order_stats_workspace_bytes(), dtype=torch.uint8, device=vol.device)
        out = torch.empty(groups * _MAX_RANKS, dtype=torch.float64, device=vol.device)
        nan = torch.empty(groups, dtype=torch.int64, device=vol.device)
        for g in range(groups):
            part = ranks[g * _MAX_RANKS:(g + 1) * _MAX_RANKS]
            R = (ctypes.c_int64 * len(part))(*part)
            check(L.fmri_order_stats_f64(_p(vol), n, ctypes.addressof(R), len(part), out.data_ptr() + 8 * _MAX_RANKS * g,
                                         nan.data_ptr() + 8 * g, _p(ws), _s()), "fmri_order_stats_f64")
    vals = out.cpu().numpy().reshape(groups, _MAX_RANKS)
    return np.concatenate([vals[g, :len(ranks[g * _MAX_RANKS:(g + 1) * _MAX_RANKS])] for g in range(groups)]), int(nan[0].item())


def percentile_f64(vol, qs):
    """np.percentile(vol, qs) (the default 'linear' method) of a float64 device tensor -> float64 numpy array of len(qs), or a numpy
    scalar for a scalar q: the two neighbouring order statistics of every q from ONE order_stats_f64 call, then numpy's own _lerp on the
    host in float64.  A NaN anywhere in vol gives NaN for every q, as numpy does."""
    import numpy as np
    scalar = np.ndim(qs) == 0
    q = np.atleast_1d(np.asarray(qs, dtype=np.float64))
    if not np.all((q >= 0) & (q <= 100)):
        raise ValueError("Percentiles must be in the range [0, 100]")
    n = vol.numel()
    vi = np.true_divide(q, 100) * (n - 1)                    # numpy's virtual index of method 'linear'
    lo = np.floor(vi)
    hi = np.minimum(lo + 1, n - 1)
    t = np.subtract(vi, lo)
    vals, nans = order_stats_f64(vol, np.concatenate([lo, hi]).astype(np.int64))
    if nans:
        res = np.full(q.shape, np.nan)
    else:
        a, b = vals[:q.size], vals[q.size:]
        diff = b - a
        with np.errstate(invalid="ignore", over="ignore"):
            res = a + diff * t                                   # numpy.lib._function_base_impl._lerp
            res = np.where(t >= 0.5, b - diff * (1 - t), res)
    return res[0] if scalar else res


def minmax_f64(vol):
    """(vol.min(), vol.max()) of a float64 device tensor as Python floats; NaN for both when vol holds a NaN, as numpy gives"""
    _need_cuda(vol)
    if vol.dtype != torch.float64 or vol.numel() == 0:
        raise ValueError("a non-empty float64 tensor is needed (got %s %s)" % (vol.dtype, tuple(vol.shape)))
    with torch.cuda.device(vol.device):
        out = torch.empty(2, dtype=torch.float64, device=vol.device)
        nan = torch.empty(1, dtype=torch.int64, device=vol.device)
        check(lib().fmri_minmax_f64(_p(vol), vol.numel(), _p(out), _p(nan), _s()), "fmri_minmax_f64")
    lo, hi = out.tolist()
    return (float("nan"), float("nan")) if int(nan.item()) else (lo, hi)


def moments_f64(vol):
    """(vol.mean(), vol.std(), vol.min(), vol.max()) of a float64 device tensor as Python floats, numpy's definitions (population std
    from a second pass around the mean); one call of fmri_moments_f64, one read-back.  The sums are compensated and added in an order
    fixed by the size: within a few ulp of the exact values, mean identical to numpy's where the partial sums are exact (integer
    volumes), same bits on every run.  A NaN in vol gives NaN for all four, as numpy does.  Infinities are not covered (they make the
    compensated sums NaN where numpy's mean is an infinity).  `vol` must be dense; a view may start anywhere in its storage."""
    host = moments_f64_enqueue(vol).cpu()
    if int(host[5:].view(torch.int64).item()):
        return (float("nan"),) * 4
    mean, std, lo, hi = host[:4].tolist()
    return mean, std, lo, hi


def moments_f64_enqueue(vol):
    """the launches of moments_f64 on the current stream, nothing read back -> a device tensor of 6 float64: {mean, std, min, max, sum} as
    fmri_moments_f64 leaves them (min / max over the values that are not NaN) and, in the last 8 bytes, the int64 number of NaNs"""
    _need_cuda(vol)
    if vol.dtype != torch.float64 or vol.numel() == 0 or not vol.is_contiguous():
        raise ValueError("a non-empty contiguous float64 tensor is needed (got %s %s)" % (vol.dtype, tuple(vol.shape)))
    L = lib()
    with torch.cuda.device(vol.device):
        ws = torch.empty(L.fmri_moments_workspace_bytes(), dtype=torch.uint8, device=vol.device)
        out = torch.empty(6, dtype=torch.float64, device=vol.device)
        check(L.fmri_moments_f64(_p(vol), vol.numel(), _p(out), out.data_ptr() + 40, _p(ws), _s()), "fmri_moments_f64")
    return out


def intensity_map_f64(vol, kind, p0, p1, p2=0.0, p3=0.0, out=None):
    """out = map(vol) element by element (csrc/postprocess.hip: MAP_WINDOW, MAP_MINMAX, MAP_ZSCORE); out=None: a new tensor, out=vol: in
    place"""
    _need_cuda(vol, out)
    if vol.dtype != torch.float64 or vol.numel() == 0:
        raise ValueError("a non-empty float64 tensor is needed (got %s %s)" % (vol.dtype, tuple(vol.shape)))
    if out is None:
        out = torch.empty_like(vol)
    assert out.dtype == torch.float64 and out.shape == vol.shape and out.device == vol.device
    with torch.cuda.device(vol.device):
        check(lib().fmri_intensity_map_f64(_p(vol), _p(out), vol.numel(), int(kind), float(p0), float(p1), float(p2), float(p3), _s()),
              "fmri_intensity_map_f64")
    return out


def window_intensities_f64(vol, min_percent=1, max_percent=99, out_min=0.0, out_max=255.0):
    """fetal_net.pipeline.window_intensities_data of a float64 device volume -> a new tensor"""
    _vol_f64(vol)
    lo, hi = (float(v) for v in percentile_f64(vol, [min_percent, max_percent]))
    if hi == lo:
        return torch.full_like(vol, float(out_min))
    return intensity_map_f64(vol, MAP_WINDOW, lo, hi, (out_max - out_min) / (hi - lo), out_min)


def norm_minmax_f64(vol):
    """-1 + 2 * (d - d.min()) / (d.max() - d.min()) (reference fetal_net/preprocess.py:5-6) -> a new tensor; NaN everywhere for a
    constant volume (0 / 0), as on the host"""
    _vol_f64(vol)
    mn, mx = minmax_f64(vol)
    return intensity_map_f64(vol, MAP_MINMAX, mn, mx)


def normalize_f64(vol, mean, std):
    """(vol - mean) / std (reference fetal_net/normalize.py:66-69) -> a new tensor"""
    _vol_f64(vol)
    return intensity_map_f64(vol, MAP_ZSCORE, mean, std)


def laplace_f64(vol):
    """scipy.ndimage.laplace(vol) (mode 'reflect') of a float64 device volume [X,Y,Z] -> a new tensor"""
    _vol_f64(vol)
    X, Y, Z = vol.shape
    out = torch.empty_like(vol)
    with torch.cuda.device(vol.device):
        check(lib().fmri_laplace_f64(_p(vol), _p(out), X, Y, Z, _s()), "fmri_laplace_f64")
    return out


def gaussian_kernel1d(sigma, order, radius):
    """scipy.ndimage._filters._gaussian_kernel1d for orders 0 and 1, reversed as gaussian_filter1d reverses it before it correlates"""
    import numpy as np
    if order not in (0, 1):
        raise NotImplementedError("gaussian derivative order %r" % (order,))
    sigma2 = sigma * sigma
    x = np.arange(-radius, radius + 1)
    phi_x = np.exp(-0.5 / sigma2 * x ** 2)
    phi_x = phi_x / phi_x.sum()
    if order == 0:
        return phi_x[::-1].copy()
    exponent_range = np.arange(order + 1)
    q = np.zeros(order + 1)
    q[0] = 1
    D = np.diag(exponent_range[1:], 1)
    P = np.diag(np.ones(order) / -sigma2, -1)
    q = (D + P).dot(q)
    q = (x[:, None] ** exponent_range).dot(q)
    return (q * phi_x)[::-1].copy()


def gaussian_gradient_magnitude_f64(vol, sigma, truncate=4.0):
    """scipy.ndimage.gaussian_gradient_magnitude(vol, sigma) (mode 'reflect') of a float64 device volume [X,Y,Z] -> a new tensor.
    D_a = derivative along a, smoothing along the other two, the axes in ascending order as gaussian_filter runs them; the smoothed
    prefixes are shared (g0 serves D_1 and D_2): 8 correlation passes instead of 9, then sqrt((D_0^2 + D_1^2) + D_2^2)."""
    import numpy as np
    _vol_f64(vol)
    X, Y, Z = vol.shape
    sig = [float(sigma)] * 3 if np.isscalar(sigma) else [float(v) for v in sigma]
    if len(sig) != 3:
        raise ValueError("sigma: one number, or one per axis")
    if any(sd <= 1e-15 for sd in sig):
        raise NotImplementedError("a sigma of ~0 (scipy skips that axis, its derivative included)")
    L = lib()
    with torch.cuda.device(vol.device):
        radius = [int(truncate * sd + 0.5) for sd in sig]
        w = [[torch.from_numpy(gaussian_kernel1d(sd, o, r)).to(vol.device) for o in (0, 1)] for sd, r in zip(sig, radius)]

        def run(src, axis, order):
            dst = torch.empty_like(vol)
            name = "fmri_correlate1d_asym_f64" if order else "fmri_correlate1d_f64"
            check(getattr(L, name)(_p(src), _p(dst), X, Y, Z, axis, _p(w[axis][order]), radius[axis], _s()), name)
            return dst

        d0 = run(run(run(vol, 0, 1), 1, 0), 2, 0)
        g0 = run(vol, 0, 0)
        d1 = run(run(g0, 1, 1), 2, 0)
        d2 = run(run(g0, 1, 0), 2, 1)
        del g0
        check(L.fmri_grad_magnitude_combine_f64(_p(d0), _p(d1), _p(d2), _p(d0), vol.numel(), _s()), "fmri_grad_magnitude_combine_f64")
    return d0


# ---------------------------------------------------------------------------------------------------- evaluation (postprocess.hip)
def _masks_u8(*masks):
    _need_cuda(*masks)
    for m in masks:
        if m.dtype != torch.uint8 or m.dim() != 3 or m.numel() == 0:
            raise ValueError("a non-empty uint8 volume [X,Y,Z] is needed (got %s %s)" % (m.dtype, tuple(m.shape)))
        if m.shape != masks[0].shape or m.device != masks[0].device:
            raise ValueError("the two masks differ in shape or device (%s, %s)" % (tuple(masks[0].shape), tuple(m.shape)))


def _connectivity(connectivity):
    if connectivity not in (1, 2, 3):
        raise ValueError("connectivity: 1, 2 or 3 (scipy.ndimage.generate_binary_structure(3, connectivity)), got %r" % (connectivity,))
    return int(connectivity)


def seg_counts_u8(a, b):
    """(|A|, |B|, |A n B|) as Python ints of two uint8 device volumes (nonzero = in the mask): exact integer sums"""
    _masks_u8(a, b)
    with torch.cuda.device(a.device):
        out = torch.empty(3, dtype=torch.int64, device=a.device)
        check(lib().fmri_seg_counts_u8(_p(a), _p(b), a.numel(), _p(out), _s()), "fmri_seg_counts_u8")
    return tuple(int(v) for v in out.tolist())


def label_counts_u8(truth, pred, values):
    """[(|T == v|, |P == v|, |both|) for v in values] as Python ints of two uint8 device label maps: exact, one pass for all labels"""
    _masks_u8(truth, pred)
    vals = label_values(values)
    with torch.cuda.device(truth.device):
        out = torch.empty((len(vals), 3), dtype=torch.int64, device=truth.device)
        check(lib().fmri_label_counts_u8(_p(truth), _p(pred), truth.numel(), vals, len(vals), _p(out), _s()), "fmri_label_counts_u8")
    return [tuple(int(v) for v in row) for row in out.tolist()]


def _surface(a, b, connectivity, counts):
    """enqueue the border extraction of a (and b, or None) -> their inverted borders; counts: int64 device tensor of 1 (2) entries"""
    X, Y, Z = a.shape
    inv_a = torch.empty_like(a)
    inv_b = None if b is None else torch.empty_like(b)
    check(lib().fmri_surface_u8(_p(a), _p(inv_a), _p(b), _p(inv_b), X, Y, Z, connectivity, _p(counts), _s()), "fmri_surface_u8")
    return inv_a, inv_b


def surface_u8(mask, connectivity=1):
    """(inv_border, count): inv_border is 0 on the surface voxels of a uint8 device volume and 1 elsewhere - the complement of
    mask ^ scipy.ndimage.binary_erosion(mask, generate_binary_structure(3, connectivity)), so a foreground voxel on a volume face is
    surface - which is the input distance_transform_edt_u8 turns into the distance to the nearest surface voxel; count = the number of
    surface voxels."""
    _masks_u8(mask)
    connectivity = _connectivity(connectivity)
    with torch.cuda.device(mask.device):
        count = torch.empty(1, dtype=torch.int64, device=mask.device)
        inv, _ = _surface(mask, None, connectivity, count)
    return inv, int(count.item())


def _compact(field, inv_sel, out, cursor):
    check(lib().fmri_masked_compact_f64(_p(field), _p(inv_sel), field.numel(), _p(out), out.numel(), _p(cursor), _s()),
          "fmri_masked_compact_f64")


def surface_distances_f64(result, reference, sampling=None, connectivity=1):
    """The distances from every surface voxel of `result` to the nearest surface voxel of `reference` (medpy's
    __surface_distances: distance_transform_edt(~reference_border, sampling)[result_border]) as a dense float64 device tensor, in no
    particular order.  `result` without a surface gives an empty tensor; `reference` without one gives +inf for every entry (there is
    no nearest voxel) without running the distance transform."""
    _masks_u8(result, reference)
    connectivity = _connectivity(connectivity)
    sampling = _edt_sampling(sampling)
    dev = result.device
    with torch.cuda.device(dev):
        counts = torch.empty(2, dtype=torch.int64, device=dev)
        inv_r, inv_f = _surface(result, reference, connectivity, counts)
        n_r, n_f = (int(v) for v in counts.tolist())
        if n_r == 0 or n_f == 0:
            return torch.full((n_r,), float("inf"), dtype=torch.float64, device=dev)
        field = _edt(inv_f, sampling, False)
        out = torch.empty(n_r, dtype=torch.float64, device=dev)
        cursor = torch.zeros(1, dtype=torch.int64, device=dev)
        _compact(field, inv_r, out, cursor)
    return out


_NAN = float("nan")


def _scores(a, b, sampling, connectivity, percentile, with_counts):
    _masks_u8(a, b)
    connectivity = _connectivity(connectivity)
    sampling = _edt_sampling(sampling)
    L = lib()
    dev = a.device
    n = a.numel()
    with torch.cuda.device(dev):
        ints = torch.zeros(5, dtype=torch.int64, device=dev)                # |A|, |B|, |A n B|, surface voxels of A, of B
        if with_counts:
            check(L.fmri_seg_counts_u8(_p(a), _p(b), n, _p(ints), _s()), "fmri_seg_counts_u8")
        inv_a, inv_b = _surface(a, b, connectivity, ints[3:])
        c = [int(v) for v in ints.tolist()]                                 # the one read-back in front of the distance transforms
        n_a, n_b = c[3], c[4]
        res = {"hd": _NAN, "hd95": _NAN, "assd": _NAN, "n_surface": (n_a, n_b)}
        if with_counts:
            res["counts"] = tuple(c[:3])
        if n_a == 0 or n_b == 0:                                             # an empty mask: no surface, the field would be +inf
            return res
        dist = torch.empty(n_a + n_b, dtype=torch.float64, device=dev)       # d(A -> B), then d(B -> A)
        cursor = torch.zeros(1, dtype=torch.int64, device=dev)
        stats = torch.empty(4, dtype=torch.float64, device=dev)
        ws = torch.empty(L.fmri_masked_stats_workspace_bytes(), dtype=torch.uint8, device=dev)
        for k, (sel, other) in enumerate(((inv_a, inv_b), (inv_b, inv_a))):
            field = _edt(other, sampling, False)
            check(L.fmri_masked_stats_f64(_p(field), _p(sel), n, stats.data_ptr() + 16 * k, _p(ws), _s()), "fmri_masked_stats_f64")
            _compact(field, sel, dist, cursor)
            del field
        hd95 = float(percentile_f64(dist, percentile))
        s_ab, m_ab, s_ba, m_ba = stats.tolist()
        if int(cursor.item()) != n_a + n_b:
            raise RuntimeError("the compaction kept %d distances, the surfaces hold %d" % (int(cursor.item()), n_a + n_b))
    res.update(hd=max(m_ab, m_ba), hd95=hd95, assd=(s_ab / n_a + s_ba / n_b) / 2)
    return res


def surface_metrics_u8(a, b, sampling=None, connectivity=1, percentile=95):
    """medpy.metric.binary's hd, hd95 and assd of two uint8 device volumes (nonzero = in the mask; sampling = the voxel spacing) ->
    {"hd": max(max d(A->B), max d(B->A)), "hd95": np.percentile(hstack(d(A->B), d(B->A)), percentile), "assd": mean(mean d(A->B),
    mean d(B->A)), "n_surface": (nA, nB)} with d(A->B) the distances of surface_distances_f64(a, b).  One surface launch for both
    masks, a read-back of the two counts, then per direction a distance transform, a masked sum / max and a compaction, and the radix
    select of percentile_f64 on the compacted distances.  hd and hd95 are exact functions of the distance field; the sum behind assd
    is added in a fixed order (two calls agree bit for bit).  A mask without a voxel: the three metrics are NaN and no distance
    transform runs."""
    return _scores(a, b, sampling, connectivity, percentile, False)


def segmentation_scores_u8(a, b, sampling=None, connectivity=1, percentile=95):
    """surface_metrics_u8 plus "counts": (|A|, |B|, |A n B|), the integers every overlap score is a ratio of, counted in front of the
    surface launch and read back with the surface counts (fetal_net.evaluate.evaluate_case)"""
    return _scores(a, b, sampling, connectivity, percentile, True)


def avgpool_fwd(x, y, planar=False):
    """x [N,D,H,W,C] -> y [N,D//2,H//2,W//2,C] (planar: [N,D,H//2,W//2,C]); AveragePooling3D() / AveragePooling2D()"""
    _need_cuda(x, y)
    N, D, H, W, Cc = x.shape
    assert tuple(y.shape) == (N, D if planar else D // 2, H // 2, W // 2, Cc), (x.shape, y.shape)
    check(lib().fmri_avgpool3d_2x_fwd(_p(x), _p(y), N, D, H, W, Cc, dt(x), int(planar), _s()), "fmri_avgpool3d_2x_fwd")
    return y


def avgpool_bwd(dy, dx, planar=False):
    _need_cuda(dy, dx)
    N, D, H, W, Cc = dx.shape
    assert tuple(dy.shape) == (N, D if planar else D // 2, H // 2, W // 2, Cc), (dx.shape, dy.shape)
    check(lib().fmri_avgpool3d_2x_bwd(_p(dy), _p(dx), N, D, H, W, Cc, dt(dx), int(planar), _s()), "fmri_avgpool3d_2x_bwd")
    return dx


def global_avgpool_fwd(x, y):
    """x [N, ..., C] -> y [N, C] fp32"""
    _need_cuda(x, y)
    N, Cc = x.shape[0], x.shape[-1]
    assert y.dtype == torch.float32 and tuple(y.shape) == (N, Cc)
    check(lib().fmri_global_avgpool_fwd(_p(x), _p(y), N, x.numel() // (N * Cc), Cc, dt(x), _s()), "fmri_global_avgpool_fwd")
    return y


def global_avgpool_bwd(dy, dx):
    _need_cuda(dy, dx)
    N, Cc = dx.shape[0], dx.shape[-1]
    assert dy.dtype == torch.float32 and tuple(dy.shape) == (N, Cc)
    check(lib().fmri_global_avgpool_bwd(_p(dy), _p(dx), N, dx.numel() // (N * Cc), Cc, dt(dx), _s()), "fmri_global_avgpool_bwd")
    return dx


def dense_fwd(x, w, b, y, act=ACT_NONE, alpha=0.0):
    """x [N,K] fp32, w [K,M] (Keras kernel), b [M] -> y [N,M] fp32"""
    _need_cuda(x, w, b, y)
    N, K = x.shape
    M = w.shape[1]
    assert w.shape[0] == K and tuple(y.shape) == (N, M) and all(t.dtype == torch.float32 for t in (x, w, y))
    check(lib().fmri_dense_fwd(_p(x), _p(w), _p(b), _p(y), N, K, M, act, float(alpha), _s()), "fmri_dense_fwd")
    return y


def dense_bwd(x, w, y, dy, dx, dw, db, act=ACT_NONE, alpha=0.0):
    """dw / db accumulate, dx is written; any of the three may be None"""
    _need_cuda(x, w, y, dy, dx, dw, db)
    N, K = x.shape
    M = w.shape[1]
    check(lib().fmri_dense_bwd(_p(x), _p(w), _p(y), _p(dy), _p(dx), _p(dw), _p(db), N, K, M, act, float(alpha), _s()), "fmri_dense_bwd")


def sigmoid_bce_fwd(logits, target, probs, sums):
    """sums (fp64, >= 3) += [sum of Keras binary_crossentropy terms, sum |p - t|, n]"""
    _need_cuda(logits, target, probs, sums)
    assert target.dtype == torch.float32 and logits.dtype == torch.float32 and sums.dtype == torch.float64
    check(lib().fmri_sigmoid_bce_fwd(_p(logits), _p(target), _p(probs), _p(sums), logits.numel(), _s()), "fmri_sigmoid_bce_fwd")
    return probs


def sigmoid_bce_bwd(probs, target, dlogits, scale):
    _need_cuda(probs, target, dlogits)
    check(lib().fmri_sigmoid_bce_bwd(_p(probs), _p(target), _p(dlogits), probs.numel(), float(scale), _s()), "fmri_sigmoid_bce_bwd")
    return dlogits


def sigmoid_chain(probs, dprobs, dlogits, scale=1.0, accumulate=False):
    """dlogits [nvox, L] (+)= scale * dprobs[..., :L] * p * (1 - p); dprobs [..., ld] is the discriminator's input gradient"""
    _need_cuda(probs, dprobs, dlogits)
    nvox, L = probs.shape
    ld = dprobs.shape[-1]
    assert dprobs.numel() == nvox * ld and dlogits.shape == probs.shape
    check(lib().fmri_sigmoid_chain(_p(probs), _p(dprobs), ld, L, _p(dlogits), nvox, float(scale), int(accumulate), dt(dprobs), _s()),
          "fmri_sigmoid_chain")
    return dlogits


def discriminator_input(probs, x, out, merge=False):
    """out [..., ld] = [probs, x, 0...] or, merge, the mul-merge maps [x * probs, x * (1 - probs), 0...] (train_adv.py:92-95)"""
    _need_cuda(probs, x, out)
    nvox, L = probs.shape
    Cc = x.shape[-1]
    assert x.numel() == nvox * Cc and out.numel() == nvox * out.shape[-1]
    check(lib().fmri_discriminator_input(_p(probs), L, _p(x), Cc, dt(x), _p(out), out.shape[-1], dt(out), nvox, int(merge), _s()),
          "fmri_discriminator_input")
    return out


# ---------------------------------------------------------------------------------------------------- augmenters of the skimage family
def gaussian_filter_f32(patch, sigma, truncate=4.0, mode="nearest"):
    """skimage.filters.gaussian(patch, sigma) of an fp32 device patch [X,Y,Z] (reference augment.py:113-114): scipy's weights, mode
    'nearest'; a patch with 3 planes along the last axis is not smoothed along it (skimage takes it for an RGB image).  Returns a new
    tensor (or `patch` itself when every sigma is ~0)."""
    import numpy as np
    _need_cuda(patch)
    assert patch.dtype == torch.float32 and patch.dim() == 3
    X, Y, Z = patch.shape
    if np.isscalar(sigma):
        sig = [float(sigma)] * 3
        if Z == 3:
            sig[2] = 0.0
    else:                                                 # one sigma per axis (0: the axis is left alone)
        sig = [float(v) for v in sigma]
        assert len(sig) == 3
    return _gaussian_passes(patch, sig, truncate, lambda a, b, axis, w, radius: check(
        lib().fmri_correlate1d_f32(_p(a), _p(b), X, Y, Z, axis, _p(w), radius, 1 if mode == "nearest" else 0, _s()), "fmri_correlate1d_f32"))


def elastic_ksize(sigma):
    """imgaug 0.4.0 blur.py `_compute_gaussian_blur_ksize` + the odd-size rule of `blur_gaussian_`: width of the truncated Gaussian kernel"""
    k = 3.3 * sigma if sigma < 3.0 else (2.9 * sigma if sigma < 5.0 else 2.6 * sigma)
    k = int(max(k, 5))
    return k + 1 if k % 2 == 0 else k


_ELASTIC_KERNELS = {}
ELASTIC_RNG_KMAX = 31


def _elastic_kernel(k, sigma, device):
    """the truncated, normalised Gaussian of cv2.GaussianBlur(ksize=k, sigma) as a device fp64 vector; one pageable upload (a host sync) per
    (k, sigma, device), not per patch"""
    import numpy as np
    device = torch.device(device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (k, float(sigma), device)
    wd = _ELASTIC_KERNELS.get(key)
    if wd is None:
        xs = np.arange(k, dtype=np.float64) - (k - 1) / 2.0
        w = np.exp(-(xs * xs) / (2.0 * float(sigma) ** 2))
        wd = _ELASTIC_KERNELS[key] = torch.from_numpy(w / w.sum()).to(device)
    return wd


def elastic_fields_rng(shape2d, alpha, sigma, seed, seq, device="cuda"):
    """elastic_fields with the noise drawn in the kernel, one patch (see elastic_fields_rng_batch) -> (d0, d1)"""
    d = elastic_fields_rng_batch(shape2d, [alpha], sigma, seed, [seq], device=device)
    return d[0, 0], d[0, 1]


def elastic_fields(shape2d, alpha, sigma, generator=None, noise=None):
    """-> (d0, d1): the displacement along axis 0 (imgaug's dy) and axis 1 (dx) of an X x Y image, fp32 device tensors.
    imgaug 0.4.0 ElasticTransformation._generate_shift_maps: uniform(-1, 1) noise on the image padded by the kernel width on every side
    (one draw of (2 * h_pad, w_pad): dx from the first half, dy from the second), blurred with the truncated normalised Gaussian kernel
    (cv2.GaussianBlur(ksize, sigma)), times alpha, padding cropped - the border mode never reaches the kept part.  `noise`: the draw itself
    (fp32 device tensor (2, h_pad, w_pad), block 0 = dx) instead of the device generator's (tests feed the oracle's)."""
    import numpy as np
    X, Y = int(shape2d[0]), int(shape2d[1])
    k = elastic_ksize(float(sigma))
    hp, wp = X + 2 * k, Y + 2 * k
    if noise is None:
        dev = torch.device("cuda", torch.cuda.current_device()) if generator is None else generator.device
        noise = torch.rand((2, hp, wp), device=dev, dtype=torch.float32, generator=generator) * 2 - 1
    _need_cuda(noise)
    assert tuple(noise.shape) == (2, hp, wp) and noise.dtype == torch.float32 and noise.is_contiguous()
    wd = _elastic_kernel(k, sigma, noise.device)
    a = noise
    for axis in (1, 2):
        b = torch.empty_like(a)
        check(lib().fmri_correlate1d_f32(_p(a), _p(b), 2, hp, wp, axis, _p(wd), k // 2, 0, _s()), "fmri_correlate1d_f32")
        a = b
    f = a[:, k:k + X, k:k + Y] * float(alpha)
    return f[1].contiguous(), f[0].contiguous()


def piecewise_affine_matrices(shape2d, dest_yx):
    """the two triangle maps of imgaug PiecewiseAffine(nb_rows=2, nb_cols=2): corners (0,0), (0,w), (h,0), (h,w) (y, x) moved to dest_yx (4, 2);
    triangle 0 = {p0, p2, p3}: in = d0 + (y/h)(d2 - d0) + (x/w)(d3 - d2); triangle 1 = {p0, p1, p3}: in = d0 + (x/w)(d1 - d0) + (y/h)(d3 - d1).
    -> 12 floats: per triangle (row_in = a i + b j + c), (col_in = a i + b j + c)"""
    import numpy as np
    h, w = float(shape2d[0]), float(shape2d[1])
    d = np.asarray(dest_yx, dtype=np.float64)
    out = []
    for (dy, dx) in (((d[2] - d[0]) / h, (d[3] - d[2]) / w), ((d[3] - d[1]) / h, (d[1] - d[0]) / w)):
        out += [dy[0], dx[0], d[0][0], dy[1], dx[1], d[0][1]]
    return np.asarray(out, dtype=np.float64)


def piecewise_affine(src, dest_yx, order, out):
    """out[i, j, c] = src[:, :, c] at the piecewise-affine image of (i, j) (fmri_piecewise_affine2); dest_yx: the moved corners, host (4, 2)"""
    import ctypes
    if not src.is_cuda or not out.is_cuda:
        raise RuntimeError("fmri_hip ops need device tensors (no CPU path)")
    X, Y, C = src.shape
    assert tuple(out.shape) == (X, Y, C) and out.dtype == src.dtype
    for t in (src, out):
        assert t.stride(2) == 1 and t.stride(0) == Y * t.stride(1), "rows of equal length, channels contiguous"
    m = piecewise_affine_matrices((X, Y), dest_yx)
    arr = (ctypes.c_double * 12)(*m.tolist())
    check(lib().fmri_piecewise_affine2(_p(src), _dt_any(src), X, Y, C, int(src.stride(1)), ctypes.cast(arr, ctypes.c_void_p), int(order), _p(out),
                                       int(out.stride(1)), _s()), "fmri_piecewise_affine2")
    return out


def coarse_dropout(x, keep, stats, per_channel=True):
    """in place on x (X, Y, C) fp32 / bf16 (last axis may be a view into a wider row): voxels whose cell of `keep` (uint8 (hs, ws, C) or (hs, ws, 1))
    is 0 take stats[0] (= minmax(x) before the call)"""
    _need_cuda(keep, stats)
    X, Y, C = x.shape
    hs, ws, kc = keep.shape
    assert keep.dtype == torch.uint8 and keep.is_contiguous() and kc == (C if per_channel else 1)
    assert x.stride(2) == 1 and x.stride(0) == Y * x.stride(1)
    check(lib().fmri_coarse_dropout(_p(x), dt(x), X, Y, C, int(x.stride(1)), _p(keep), hs, ws, kc, _p(stats), _s()), "fmri_coarse_dropout")
    return x


AUG_WS_INTS = 1568        # FMRI_AUG_WS_INTS
_U64 = 2 ** 64 - 1


def aug_workspace(device, batch=1):
    """(stats, ws) for the *_rng intensity steps: [batch][2] floats and the zeroed int32 workspaces they keep re-armed; one pair per stream of
    calls.  The single-patch wrappers below take row 0 of a batch-1 workspace as (stats, ws)."""
    stats = torch.zeros((batch, 2), device=device, dtype=torch.float32)
    ws = torch.zeros((batch, AUG_WS_INTS), device=device, dtype=torch.int32)
    return (stats[0], ws[0]) if batch == 1 else (stats, ws)


def _batch_geometry(xb):
    """xb: (B, ...) device tensor whose patches are dense and equally spaced -> (B, elements per patch, stride in elements)"""
    B = xb.shape[0]
    n = xb[0].numel()
    assert xb.is_cuda and xb[0].is_contiguous() and (B == 1 or xb.stride(0) >= n)
    return B, n, (xb.stride(0) if B > 1 else n)


def _seqs(seqs):
    import numpy as np
    a = np.ascontiguousarray(seqs, dtype=np.uint32)
    return a, a.ctypes.data


def minmax_ws_batch(xb, stats, ws):
    """stats[b] = {min, max} of xb[b], all patches in one launch (fmri_minmax_ws_batch)"""
    _need_cuda(stats, ws)
    B, n, stride = _batch_geometry(xb)
    check(lib().fmri_minmax_ws_batch(_p(xb), n, stride, B, dt(xb), _p(stats), _p(ws), _s()), "fmri_minmax_ws_batch")
    return stats


def rescale_intensity_ws_batch(xb, stats, ws, params):
    """params: (B, 4) rows {mode, lo, hi, mult}, mode 0 skip / 1 multiply / 2 contrast + multiply; stats[b] updated"""
    import numpy as np
    _need_cuda(stats, ws)
    B, n, stride = _batch_geometry(xb)
    a = np.ascontiguousarray(params, dtype=np.float32)
    assert a.shape == (B, 4)
    check(lib().fmri_rescale_intensity_ws_batch(_p(xb), n, stride, B, dt(xb), _p(stats), _p(ws), a.ctypes.data, _s()), "fmri_rescale_intensity_ws_batch")
    return xb


def noise_rng_batch(xb, stats, ws, kind, sigma, seed, seqs):
    """gaussian (kind 0) / speckle (1) noise in place on every patch with seqs[b] != 0, the normal draws in the kernel; stats[b] updated"""
    _need_cuda(stats, ws)
    B, n, stride = _batch_geometry(xb)
    a, ap = _seqs(seqs)
    assert a.shape == (B,)
    check(lib().fmri_noise_rng_batch(_p(xb), n, stride, B, dt(xb), _p(stats), _p(ws), int(kind), float(sigma), int(seed) & _U64, ap, _s()),
          "fmri_noise_rng_batch")
    return xb


def shot_noise_rng_batch(xb, stats, ws, seed, seqs):
    """reference augment.py:87-94 in place on every patch with seqs[b] != 0, the Poisson draws in the kernel; stats[b] updated"""
    _need_cuda(stats, ws)
    B, n, stride = _batch_geometry(xb)
    a, ap = _seqs(seqs)
    assert a.shape == (B,)
    check(lib().fmri_shot_noise_rng_batch(_p(xb), n, stride, B, dt(xb), _p(stats), _p(ws), int(seed) & _U64, ap, _s()), "fmri_shot_noise_rng_batch")
    return xb


def coarse_dropout_rng_batch(xb, grids, rate, stats, per_channel, seed, seqs):
    """coarse dropout in place on xb (B, X, Y, C); grids: (B, 2) keep-grid sizes (per slice when per_channel), drawn in the kernel"""
    import numpy as np
    _need_cuda(stats)
    B, X, Y, C = xb.shape
    assert xb.is_cuda and xb.stride(3) == 1 and xb.stride(1) == Y * xb.stride(2)
    g = np.ascontiguousarray(grids, dtype=np.int32)
    a, ap = _seqs(seqs)
    assert g.shape == (B, 2) and a.shape == (B,)
    check(lib().fmri_coarse_dropout_rng_batch(_p(xb), dt(xb), X, Y, C, int(xb.stride(2)), int(xb.stride(0)), B, g.ctypes.data, C if per_channel else 1,
                                              float(rate), _p(stats), int(seed) & _U64, ap, _s()), "fmri_coarse_dropout_rng_batch")
    return xb


def affine_sample_batch(vols, affines, corners, size, out, order, cvals, table=None, z_off=0, out_ld=None):
    """out[b] (dense (nx, ny, nz) patches, equally spaced) = vols[b] sampled at affines[b] . (corners[b] + (i, j, k), 1), order 0 (nearest) / 1
    (trilinear), cvals[b] outside the volume: the patches of a batch in one launch (fmri_affine_sample_batch).  vols: device tensors of one dtype
    (float32 or uint8), each (X, Y, Z) contiguous; affines (B, 4, 4) or (B, 3, 4), host.
    table: inter-slice motion - output slice k of patch b is displaced in-plane by row k + z_off of table[b] (device float64 (B, nz_table, 6):
    (i', j') = (m0 i + m1 j + m2, m3 i + m4 j + m5) in patch coordinates; a row outside the table is the identity) before the affine; z_off: where
    the first output slice sits among the image slices the table was drawn for.  None: the plain gather.
    out_ld: row length of out when its last axis is a view into wider rows (the previous-slice truth channels behind the image slices)"""
    import ctypes
    import numpy as np
    B = len(vols)
    nx, ny, nz = (int(v) for v in size)
    if out_ld is None:
        assert out.is_cuda and tuple(out.shape) == (B, nx, ny, nz) and out[0].is_contiguous()
        out_ld = nz
    else:
        out_ld = int(out_ld)
        assert out.is_cuda and tuple(out.shape) == (B, nx, ny, nz) and out_ld >= nz
        assert out.stride(3) == 1 and out.stride(2) == out_ld and out.stride(1) == ny * out_ld, "rows of out_ld elements, channels contiguous"
    for v in vols:
        if not v.is_cuda or not v.is_contiguous() or v.dtype != vols[0].dtype or v.dim() != 3:
            raise RuntimeError("fmri_hip ops need contiguous device volumes of one dtype")
    if table is not None and not (table.is_cuda and table.dtype == torch.float64 and table.is_contiguous() and table.dim() == 3
                                  and table.shape[0] == B and table.shape[1] >= 1 and table.shape[2] == 6):
        raise RuntimeError("slice table: a contiguous device float64 tensor (patches, rows, 6)")
    ptrs = (ctypes.c_void_p * B)(*[v.data_ptr() for v in vols])
    dims = np.ascontiguousarray([v.shape for v in vols], dtype=np.int32)
    A = np.ascontiguousarray(np.asarray(affines, dtype=np.float64)[:, :3, :4])
    cr = np.ascontiguousarray(corners, dtype=np.int32)
    cv = np.ascontiguousarray(cvals, dtype=np.float32)
    assert A.shape == (B, 3, 4) and cr.shape == (B, 3) and cv.shape == (B,)
    check(lib().fmri_affine_sample_batch(B, ctypes.cast(ptrs, ctypes.c_void_p), dims.ctypes.data, A.ctypes.data, _p(table),
                                         0 if table is None else int(table.shape[1]), int(z_off), cr.ctypes.data, cv.ctypes.data, _dt_any(vols[0]),
                                         nx, ny, nz, int(order), _p(out), _dt_any(out), out_ld, int(out.stride(0)), _s()), "fmri_affine_sample_batch")
    return out


MRI_PARAMS, MRI_TERMS = 23, (0, 4, 10, 20)        # FMRI_MRI_PARAMS; monomials of order 0 (no field) .. 3


def mri_intensity_ws_batch(xb, stats, ws, gammas, coefs, gains, vmins):
    """gamma, bias field and slice gain in place on the dense patches xb (B, X, Y, Z), one launch (fmri_mri_intensity_ws_batch).  Per patch:
    gammas[b] (0 = skip), coefs[b] (None, or the 4 / 10 / 20 coefficients of the order 1 / 2 / 3 field), gains[b] (None, or a device float32
    tensor of Z slice gains), vmins[b] (the volume's minimum, which the gains leave in place).  stats[b] = range of xb[b] before the call, updated
    for every patch that is written; a patch that skips all three is not touched."""
    import ctypes
    import numpy as np
    _need_cuda(stats, ws)
    assert xb.dim() == 4
    B, n, stride = _batch_geometry(xb)
    X, Y, Z = (int(v) for v in xb.shape[1:])
    assert len(gammas) == B and len(coefs) == B and len(gains) == B and len(vmins) == B
    a = np.zeros((B, MRI_PARAMS), dtype=np.float32)
    ptrs = (ctypes.c_void_p * B)()
    for b in range(B):
        a[b, 0], a[b, 1] = gammas[b], vmins[b]
        if coefs[b] is not None:
            c = np.asarray(coefs[b], dtype=np.float32).reshape(-1)
            assert c.size in MRI_TERMS[1:], "bias field: 4, 10 or 20 coefficients"
            a[b, 2] = c.size
            a[b, 3:3 + c.size] = c
        g = gains[b]
        if g is not None:
            if not (g.is_cuda and g.dtype == torch.float32 and g.is_contiguous() and g.numel() == Z):
                raise RuntimeError("slice gains: a contiguous device float32 tensor, one gain per slice")
            ptrs[b] = g.data_ptr()
    check(lib().fmri_mri_intensity_ws_batch(_p(xb), X, Y, Z, stride, B, dt(xb), _p(stats), _p(ws), a.ctypes.data, ctypes.cast(ptrs, ctypes.c_void_p),
                                            _s()), "fmri_mri_intensity_ws_batch")
    return xb


def elastic_fields_rng_batch(shape2d, alphas, sigma, seed, seqs, device="cuda"):
    """-> d (B, 2, X, Y) fp32: d[b, 0] = shift along axis 0, d[b, 1] along axis 1 (ops.elastic_fields' (d0, d1)), the noise drawn in the kernel
    (fmri_elastic_fields_rng_batch: one launch); seqs[b] == 0 -> zero fields.  Kernel widths above ELASTIC_RNG_KMAX (sigma >= 12) are not
    covered - callers use elastic_fields there"""
    import numpy as np
    X, Y = int(shape2d[0]), int(shape2d[1])
    k = elastic_ksize(float(sigma))
    assert k <= ELASTIC_RNG_KMAX
    wd = _elastic_kernel(k, sigma, device)
    al = np.ascontiguousarray(alphas, dtype=np.float32)
    a, ap = _seqs(seqs)
    B = al.shape[0]
    assert a.shape == (B,)
    d = torch.empty((B, 2, X, Y), device=wd.device, dtype=torch.float32)
    check(lib().fmri_elastic_fields_rng_batch(_p(d), X, Y, k, _p(wd), al.ctypes.data, int(seed) & _U64, ap, B, _s()), "fmri_elastic_fields_rng_batch")
    return d


def elastic_warp_batch(src, d, order, out):
    """out[b, i, j, c] = src[b, :, :, c] at (i - d[b, 0, i, j], j - d[b, 1, i, j]), order 0 / 1, mode 'nearest' (fmri_elastic_warp_batch); d: the
    fields of elastic_fields_rng_batch (or elastic_fields' pairs, stacked); src, out: (B, X, Y, C) float32 or uint8, patches equally spaced, the
    last axis may be a view into a wider row (stride(2) = row length)"""
    _need_cuda(d)
    B, X, Y, C = src.shape
    assert src.is_cuda and out.is_cuda and tuple(out.shape) == (B, X, Y, C) and out.dtype == src.dtype and tuple(d.shape) == (B, 2, X, Y)
    assert d.is_contiguous() and d.dtype == torch.float32
    for t in (src, out):
        assert t.stride(3) == 1 and t.stride(1) == Y * t.stride(2), "rows of equal length, channels contiguous"
    check(lib().fmri_elastic_warp_batch(_p(src), _dt_any(src), X, Y, C, int(src.stride(2)), int(src.stride(0)), _p(d), int(order), _p(out),
                                        int(out.stride(2)), int(out.stride(0)), B, _s()), "fmri_elastic_warp_batch")
    return out


# one patch = a batch of one (tests, the footprint audit)
def affine_sample(vol, affine, start, size, out, order=1, cval=0.0, out_ld=None):
    """`out` (nx, ny, nz) may be a view into a wider channels-last tensor (pass its row length as out_ld)"""
    return affine_sample_slices(vol, affine, start, size, out, None, 0, order, cval, out_ld)


def affine_sample_slices(vol, affine, start, size, out, table, z_off=0, order=1, cval=0.0, out_ld=None):
    """table: a device float64 (nz_table, 6), or None"""
    ob = out.unsqueeze(0)
    if out_ld is not None:                # rows of out_ld elements from out's first element on, whatever shape the caller's view has
        nx, ny, nz = (int(v) for v in size)
        ob = out.as_strided((1, nx, ny, nz), (nx * ny * out_ld, ny * out_ld, out_ld, 1))
    affine_sample_batch([vol], [affine], [start], size, ob, order, [cval], None if table is None else table.unsqueeze(0), z_off, out_ld)
    return out


def elastic_warp(src, d0, d1, order, out):
    """src, out: (X, Y, C) float32 or uint8, the last axis may be a view into a wider row; d0, d1 (X, Y): ops.elastic_fields' pair"""
    elastic_warp_batch(src.unsqueeze(0), torch.stack([d0, d1]).unsqueeze(0), order, out.unsqueeze(0))
    return out


def minmax_ws(x, stats, ws):
    minmax_ws_batch(x.unsqueeze(0), stats, ws)
    return stats


def rescale_intensity_ws(x, stats, ws, contrast, lo=0.0, hi=0.0, mult=1.0):
    rescale_intensity_ws_batch(x.unsqueeze(0), stats, ws, [[2 if contrast else 1, lo, hi, mult]])
    return x


def mri_intensity_ws(x, stats, ws, gamma=0.0, coef=None, gains=None, vmin=0.0):
    mri_intensity_ws_batch(x.unsqueeze(0), stats, ws, [gamma], [coef], [gains], [vmin])
    return x


def noise_rng(x, stats, ws, kind, sigma, seed, seq):
    noise_rng_batch(x.unsqueeze(0), stats, ws, kind, sigma, seed, [seq])
    return x


def shot_noise_rng(x, stats, ws, seed, seq):
    shot_noise_rng_batch(x.unsqueeze(0), stats, ws, seed, [seq])
    return x


def coarse_dropout_rng(x, grid, rate, stats, per_channel, seed, seq):
    coarse_dropout_rng_batch(x.unsqueeze(0), [[int(grid[0]), int(grid[1])]], rate, stats, per_channel, seed, [seq])
    return x


def shot_noise(x, stats, generator=None, draws_fn=None):
    """reference augment.py:87-94 in place on `x` (fp32 / bf16 device tensor); `stats` = minmax(x) taken before the call.  The Poisson
    draws come from torch's device generator (`draws_fn(rates)` overrides them: tests feed the oracle's own draws)."""
    _need_cuda(x, stats)
    n = x.numel()
    present = torch.zeros(1024, dtype=torch.int32, device=x.device)
    rates = torch.empty(n, dtype=torch.float32, device=x.device)
    L = lib()
    check(L.fmri_shot_noise_step(_p(x), n, _dt_any(x), _p(stats), _p(present), 0, 0, 0, _s()), "fmri_shot_noise_step(0)")
    check(L.fmri_shot_noise_step(_p(x), n, _dt_any(x), _p(stats), _p(present), _p(rates), 0, 1, _s()), "fmri_shot_noise_step(1)")
    draws = draws_fn(rates) if draws_fn is not None else torch.poisson(rates, generator=generator)
    draws = draws.to(torch.float32).contiguous()
    check(L.fmri_shot_noise_step(_p(x), n, _dt_any(x), _p(stats), _p(present), 0, _p(draws), 2, _s()), "fmri_shot_noise_step(2)")
    return rates
