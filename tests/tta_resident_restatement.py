"""numpy restatements of fmri_volume_pad_flip and fmri_tile_finalize_flip, written from the index formulas of include/fmri_hip.h (not from
np.pad / np.flip: tests/test_host_tta_resident.py proves the two agree).  The GPU tests compare the kernels with these bit for bit."""
import numpy as np


def masks_axes(mask):
    return tuple(a for a in range(3) if mask >> a & 1)


def _mirror(u, n, mask):
    return [n[a] - 1 - u[a] if mask >> a & 1 else u[a] for a in range(3)]


def volume_pad_flip(src, out_shape, lo, mask, fill, dtype):
    """dst[o] = fill where u = o - lo leaves src's extent on any axis, else src[m(u)]; converted to `dtype` round-to-nearest"""
    src = np.asarray(src)
    n = src.shape
    o = np.indices(tuple(out_shape))
    u = [o[a] - int(lo[a]) for a in range(3)]
    inside = np.ones(tuple(out_shape), dtype=bool)
    for a in range(3):
        inside &= (u[a] >= 0) & (u[a] < n[a])
    m = _mirror([np.clip(u[a], 0, n[a] - 1) for a in range(3)], n, mask)
    return np.where(inside, src[m[0], m[1], m[2]].astype(dtype), np.asarray(fill, dtype=np.float64).astype(dtype))


def tile_finalize_flip(acc, cnt, out_shape, lo, mask):
    """-> (out[g][c] = acc[a][c] / (double)max-with-1-where-zero cnt[a], a = lo + m(g); the number of voxels g whose count is 0)"""
    acc, cnt = np.asarray(acc, dtype=np.float64), np.asarray(cnt)
    g = np.indices(tuple(out_shape))
    a = [int(lo[k]) + mk for k, mk in enumerate(_mirror([g[0], g[1], g[2]], out_shape, mask))]
    c = cnt[a[0], a[1], a[2]]
    bad = int((c <= 0).sum())
    return acc[a[0], a[1], a[2], :] / np.where(c <= 0, 1, c).astype(np.float64)[..., None], bad
