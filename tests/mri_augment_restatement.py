"""float64 restatement of the fetal acquisition augmenters for the tests (tests/test_gpu_mri_augment.py): the gather with a per-slice table through
scipy.ndimage.map_coordinates, and gamma / bias field / slice gain written out voxel by voxel from include/fmri_hip.h - independent of both the
kernels and the vectorised host forms in fetal_net/augment.py."""
import numpy as np
import scipy.ndimage

# Bound of the intensity kernel against the float64 restatement, relative to the range of the restated result.  Not derivable from the project:
# expf / powf / the polynomial run in fp32.  Measured on an MI355X over the cases of tests/test_gpu_mri_augment.py, the generator's patches
# included (profiles/r12_mri_augment.log: 3.8e-8 ... 8.32e-7, the largest on a generator patch under an order-3 field), and doubled - the
# project's "2x measured" rule.
MRI_INTENSITY_TOL = 2 * 8.32e-7
GATHER_ATOL = 1e-5                      # the bound tests/test_gpu_augment.py holds fmri_affine_sample_batch to


def slice_coordinates(affine, corner, size, table, z_off):
    """source coordinates (3, nx, ny, nz) of the patch: affine . (corner + (i', j', k), 1), (i', j') by table row k + z_off (identity outside)"""
    nx, ny, nz = size
    A = np.asarray(affine, dtype=np.float64)
    out = np.empty((3, nx, ny, nz))
    for k in range(nz):
        r = k + z_off
        m = np.asarray(table[r], dtype=np.float64) if 0 <= r < len(table) else np.array([1.0, 0, 0, 0, 1.0, 0])
        for i in range(nx):
            for j in range(ny):
                p = np.array([corner[0] + (m[0] * i + m[1] * j + m[2]), corner[1] + (m[3] * i + m[4] * j + m[5]), corner[2] + k, 1.0])
                out[:, i, j, k] = A[:3, :4].dot(p)
    return out


def inside(coords, shape):
    return np.all([(coords[a] >= 0) & (coords[a] <= shape[a] - 1) for a in range(3)], axis=0)


def gather_slices(vol, affine, corner, size, table, z_off, order, cval):
    """-> (patch float64, coords): map_coordinates(mode='constant') per output point inside the volume, cval outside (no interpolation beyond
    the edges: the inside-test of fmri_affine_sample_batch)"""
    c = slice_coordinates(affine, corner, size, table, z_off)
    ok = inside(c, vol.shape)
    out = np.full(tuple(size), float(cval))
    out[ok] = scipy.ndimage.map_coordinates(np.asarray(vol, dtype=np.float64), c[:, ok], order=order, mode="constant", cval=float(cval))
    return out, c


def rounding_margin(coords, shape):
    """how far the nearest-neighbour decision of any inside point is from flipping: distance to a half-integer and to the volume's faces"""
    ok = inside(coords, shape)
    half = np.abs(coords - np.floor(coords) - 0.5)[:, ok].min()
    faces = min(min(np.abs(coords[a]).min(), np.abs(coords[a] - (shape[a] - 1)).min()) for a in range(3))
    return min(half, faces)


def mri_intensity(x, gamma, coef, gains, vmin):
    """the three effects on one patch (X, Y, Z) in the kernel's order; gamma 0 / coef None / gains None skip"""
    v = np.asarray(x, dtype=np.float64).copy()
    X, Y, Z = v.shape
    lo, hi = v.min(), v.max()
    if gamma and hi > lo:
        v = ((v - lo) / (hi - lo)) ** gamma * (hi - lo) + lo
    if coef is not None:
        order = {4: 1, 10: 2, 20: 3}[len(coef)]
        terms = [(a, b, c) for a in range(order + 1) for b in range(order + 1 - a) for c in range(order + 1 - a - b)]
        at = lambda n, s: 0.0 if s == 1 else 2.0 * n / (s - 1) - 1.0
        for i in range(X):
            for j in range(Y):
                for k in range(Z):
                    xyz = (at(i, X), at(j, Y), at(k, Z))
                    p = sum(float(w) * xyz[0] ** a * xyz[1] ** b * xyz[2] ** c for w, (a, b, c) in zip(coef, terms))
                    v[i, j, k] = (v[i, j, k] - vmin) * np.exp(p) + vmin
    if gains is not None:
        for k in range(Z):
            v[:, :, k] = (v[:, :, k] - vmin) * float(gains[k]) + vmin
    return v


def relative_error(got, want):
    rng = float(want.max() - want.min())
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max()) / (rng if rng > 0 else 1.0)
