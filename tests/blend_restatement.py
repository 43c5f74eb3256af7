"""float64 numpy restatements of the Gaussian-blending entry points - fmri_tile_scatter_weighted, fmri_tile_finalize_weighted,
fmri_tile_finalize_flip_weighted, fmri_tile_finalize_labels_weighted - and of the blended tiler as a whole, written from the formulas of
include/fmri_hip.h (not from the package's code).  The weight of a tile voxel is w = ((double)gx[x] * (double)gy[y]) * (double)gz[z] in
that order: the first product is exact, the second rounds once, so a voxel that one tile covers can be compared bit for bit."""
import numpy as np


def tables(tile, sigma_scale=0.125):
    """g_a[i] = float32(exp(-0.5 * ((i - (p_a - 1) / 2) / (sigma_scale * p_a))^2)), float64 arithmetic, rounded once"""
    out = []
    for p in tile:
        g = [np.exp(-0.5 * ((float(i) - (int(p) - 1) / 2.0) / (float(sigma_scale) * int(p))) ** 2) for i in range(int(p))]
        out.append(np.asarray(g, dtype=np.float64).astype(np.float32))
    return out


def weights(gx, gy, gz):
    gx, gy, gz = (np.asarray(g, dtype=np.float32).astype(np.float64) for g in (gx, gy, gz))
    return (gx[:, None, None] * gy[None, :, None]) * gz[None, None, :]


def tile_scatter_weighted(pred, idx, tabs, acc, wsum):
    """acc[o][c] += w * (double)pred[b][x][y][z][c], wsum[o] += w at o = idx[b] + (x, y, z), tile voxels outside the volume skipped.
    pred (B, px, py, pz, C), float32 as the entry point takes it.  ->(acc, wsum, mag, wmag, cover): the sums with the tiles added in the order of b; mag[o][c] / wmag[o]
    = the sum of |terms| that met in acc[o][c] / wsum[o] (the start value included) and cover[o] = the number of tiles on o: what the
    order-of-addition bound of a float64 sum is made of."""
    pred = np.asarray(pred)                                   # float32 for the entry point; the host route's float64 tiles are taken as they are
    acc, wsum = np.array(acc, dtype=np.float64), np.array(wsum, dtype=np.float64)
    B, px, py, pz, C = pred.shape
    X, Y, Z = wsum.shape
    assert acc.shape == (X, Y, Z, C)
    w = weights(*tabs)
    assert w.shape == (px, py, pz)
    mag, wmag = np.abs(acc), np.abs(wsum)
    cover = np.zeros((X, Y, Z), dtype=np.int64)
    for b in range(B):
        cx, cy, cz = (int(v) for v in idx[b])
        x0, y0, z0 = max(-cx, 0), max(-cy, 0), max(-cz, 0)
        x1, y1, z1 = min(px, X - cx), min(py, Y - cy), min(pz, Z - cz)
        if x1 <= x0 or y1 <= y0 or z1 <= z0:
            continue
        tile = (slice(x0, x1), slice(y0, y1), slice(z0, z1))
        vol = (slice(cx + x0, cx + x1), slice(cy + y0, cy + y1), slice(cz + z0, cz + z1))
        term = w[tile][..., None] * pred[b][tile].astype(np.float64)
        acc[vol] += term
        mag[vol] += np.abs(term)
        wsum[vol] += w[tile]
        wmag[vol] += w[tile]
        cover[vol] += 1
    return acc, wsum, mag, wmag, cover


def _divisor(wsum):
    bad = ~(wsum > 0)
    return np.where(bad, 1.0, wsum), bad


def tile_finalize_weighted(acc, wsum):
    """-> (out = acc / wsum with 1 in place of a wsum <= 0, the number of such voxels)"""
    acc, wsum = np.asarray(acc, dtype=np.float64), np.asarray(wsum, dtype=np.float64)
    d, bad = _divisor(wsum)
    return acc / d[..., None], int(bad.sum())


def tile_finalize_flip_weighted(acc, wsum, out_shape, lo, mask):
    """out[g][c] = acc[a][c] / wsum[a], a = lo + m(g), m mirroring the axes of `mask` over out's extent"""
    acc, wsum = np.asarray(acc, dtype=np.float64), np.asarray(wsum, dtype=np.float64)
    g = np.indices(tuple(out_shape))
    a = [int(lo[k]) + (out_shape[k] - 1 - g[k] if mask >> k & 1 else g[k]) for k in range(3)]
    d, bad = _divisor(wsum[a[0], a[1], a[2]])
    return acc[a[0], a[1], a[2], :] / d[..., None], int(bad.sum())


def tile_finalize_labels_weighted(acc, wsum, threshold, values):
    """q_c = acc / wsum.  C == 1: values[0] where q_0 > threshold; C > 1: values[first index of the maximum], 0 where the maximum <
    threshold; wsum <= 0: 0, counted"""
    acc, wsum = np.asarray(acc, dtype=np.float64), np.asarray(wsum, dtype=np.float64)
    C = acc.shape[-1]
    d, bad = _divisor(wsum)
    q = acc / d[..., None]
    best, k = q[..., 0].copy(), np.zeros(wsum.shape, dtype=np.int64)
    for j in range(1, C):
        better = q[..., j] > best
        best = np.where(better, q[..., j], best)
        k = np.where(better, j, k)
    keep = best > threshold if C == 1 else ~(best < threshold)
    out = np.where(keep & ~bad, np.asarray(values, dtype=np.uint8)[k], 0).astype(np.uint8)
    return out, int(bad.sum())


def blend_tiles(preds, corners, ashape, sigma_scale=0.125):
    """the blended tiler: preds (n, px, py, pz, C) at `corners` (n, 3) overlap-added into (X, Y, Z, C) = ashape and divided.
    -> (means, the largest number of tiles on one voxel)"""
    preds = np.asarray(preds)
    tabs = tables(preds.shape[1:4], sigma_scale)
    acc, wsum, _, _, cover = tile_scatter_weighted(preds, corners, tabs, np.zeros(tuple(ashape)), np.zeros(tuple(ashape[:3])))
    out, bad = tile_finalize_weighted(acc, wsum)
    assert bad == 0, "uncovered voxels"
    return out, int(cover.max())
