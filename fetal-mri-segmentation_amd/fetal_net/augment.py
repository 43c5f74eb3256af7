"""Host side of the augmentation path: the small amount of arithmetic that decides WHAT to sample (random draws, 4x4 affines,
permutation keys); the sampling itself runs on the MI355X (fmri_hip.ops.affine_sample & co, csrc/augment.hip).

Mirrors the names of reference fetal_net/augment.py so that callers (generator, prediction) read the same:
  scale_image / translate_image / rotate_image / flip_image / distort_image   reference augment.py:14-84, :189-212
  random draws of augment_data                                                reference augment.py:229-291 (same order, same RNGs)
  generate_permutation_keys / permute_data / reverse_permute_data             reference augment.py:380-471
  contrast_augment                                                            reference augment.py:125-128 (skimage rescale_intensity restated)
Not in the reference: draw_mri_parameters and apply_slice_motion / gamma_augment / bias_field / slice_gain, the acquisition effects of a
fetal stack of 2-D slices (the `augment` keys slice_motion, gamma, bias_field, slice_intensity).
"""
import itertools
import random

import numpy as np


# ---------------------------------------------------------------------------------------------------------- 4x4 affine algebra
def scale_image(affine, scale_factor):
    return np.diag(list(scale_factor) + [1]).dot(affine)


def translate_image(affine, translate_factor):
    out = np.copy(affine)
    out[0:3, 3] = out[0:3, 3] + np.asarray(translate_factor)
    return out


def rotate_image_axis(affine, angle, axis):
    s, c = np.sin(angle), np.cos(angle)
    r = np.eye(4)
    a, b = [(1, 2), (0, 2), (0, 1)][axis]
    r[a, a], r[b, b] = c, c
    if axis == 1:
        r[a, b], r[b, a] = s, -s
    else:
        r[a, b], r[b, a] = -s, s
    return r.dot(affine)


def rotate_image(affine, rotate_angles):
    out = np.copy(affine)
    for i, angle in enumerate(rotate_angles):
        if angle != 0:
            out = rotate_image_axis(out, angle, axis=i)
    return out


def flip_image(affine, axis):
    out = np.copy(affine)
    for ax in axis:
        out = rotate_image_axis(out, np.deg2rad(180), axis=int(ax))     # the reference "flips" by a half turn about the axis
    return out


def distort_image(data, affine, flip_axis=None, scale_factor=None, rotate_factor=None, translate_factor=None):
    """-> (data, affine'): centre the volume, flip / scale / rotate, move back, translate"""
    centre = np.array(data.shape) / 2
    affine = translate_image(affine, -centre)
    if flip_axis is not None:
        affine = flip_image(affine, flip_axis)
    if scale_factor is not None:
        affine = scale_image(affine, scale_factor)
    if rotate_factor is not None:
        affine = rotate_image(affine, rotate_factor)
    affine = translate_image(affine, +centre)
    if translate_factor is not None:
        affine = translate_image(affine, translate_factor)
    return data, affine


# ---------------------------------------------------------------------------------------------------------- random draws
def random_scale_factor(n_dim=3, mean=1, std=0.25):
    return np.random.normal(mean, std, n_dim)


def random_translate_factor(n_dim=3, min=0, max=7):
    return np.random.uniform(min, max, n_dim)


def random_rotation_angle(n_dim=3, mean=0, std=5):
    return np.random.uniform(low=mean - np.array(std), high=mean + np.array(std), size=n_dim)


def random_boolean():
    return np.random.choice([True, False])


def random_flip_dimensions(n_dim, flip_factor):
    return np.arange(n_dim)[[flip_rate > random.random() for flip_rate in flip_factor]]


def draw_augment_parameters(augment, n_dim, data_min, data_max):
    """Every random number augment_data draws before it touches the data, in its order (numpy's global generator; python's `random`
    for the flips), so that a seeded run picks the same transformation as the reference.  Draws belonging to augmenters this
    package does not apply (poisson, gaussian filter, piecewise affine, elastic, coarse dropout) are still consumed."""
    g = augment.get
    p = {}
    scale_factor = list(random_scale_factor(n_dim, std=g("scale"))) if g("scale") else [1, 1, 1]
    if g("iso_scale"):
        iso = np.random.uniform(1, g("iso_scale")["max"])
        if random_boolean():
            iso = 1 / iso
        scale_factor[0] *= iso
        scale_factor[1] *= iso
    p["scale_factor"] = scale_factor
    p["rotate_factor"] = np.deg2rad(random_rotation_angle(n_dim, std=g("rotate"))) if g("rotate") else None
    flip = g("flip")
    p["flip_axis"] = random_flip_dimensions(n_dim, flip) if (flip is not None and flip) else None
    if g("translate") is not None:
        t = random_translate_factor(n_dim, -np.array(g("translate")), np.array(g("translate")))
        t[-1] = np.floor(t[-1])                                    # whole slices only
        p["translate_factor"] = t
    else:
        p["translate_factor"] = None
    if g("contrast") is not None:
        val_range = data_max - data_min
        lo = data_min + g("contrast")["min_factor"] * np.random.uniform(-1, 1) * val_range
        hi = data_max + g("contrast")["max_factor"] * np.random.uniform(-1, 1) * val_range
        p["contrast"] = (lo, hi)
    else:
        p["contrast"] = None
    p["apply_poisson_noise"] = (g("poisson_noise") > np.random.random()) if g("poisson_noise") is not None else False
    p["apply_gaussian_noise"] = (g("gaussian_noise")["prob"] > np.random.random()) if g("gaussian_noise") is not None else False
    p["apply_speckle_noise"] = (g("speckle_noise")["prob"] > np.random.random()) if g("speckle_noise") is not None else False
    gf = g("gaussian_filter")
    if gf is not None and gf["prob"] > 0:
        p["gaussian_sigma"] = gf["max_sigma"] * np.random.random()
        p["apply_gaussian_filter"] = gf["prob"] > np.random.random()
    else:
        p["apply_gaussian_filter"], p["gaussian_sigma"] = False, None
    p["piecewise_affine_scale"] = np.random.random() * g("piecewise_affine")["scale"] if g("piecewise_affine") is not None else 0
    et = g("elastic_transform")
    p["elastic_transform_scale"] = np.random.random() * et["alpha"] if (et is not None and et["alpha"] > 0) else 0
    im = g("intensity_multiplication")
    if im is not None:
        a, b = im
        p["intensity_multiplication"] = np.random.random() * (b - a) + a
    else:
        p["intensity_multiplication"] = 1
    p["coarse_dropout"] = g("coarse_dropout") is not None
    return p


# ---------------------------------------------------------------------------------------------------------- intensity (host form, TTA)
def contrast_augment(data, min_per, max_per):
    data = np.asarray(data, dtype=np.float64)
    omin, omax = float(data.min()), float(data.max())
    out = np.clip(data, min_per, max_per)
    if min_per != max_per:
        return (out - min_per) / (max_per - min_per) * (omax - omin) + omin
    return np.clip(out, omin, omax)


# ---------------------------------------------------------------------------------------------------------- fetal MRI acquisition effects
# Not in the reference: a fetal scan is a stack of independently acquired 2-D slices, so slices are displaced against each other (the fetus
# moves between them), whole slices lose signal (spin history) and the surface coil modulates the intensity smoothly.  Four optional keys of
# the `augment` dict: slice_motion {prob, slice_prob, rotate (degrees, std), translate (voxels, std)}, gamma {prob, range (lo, hi)},
# bias_field {prob, order 1..3, coefficient}, slice_intensity {prob, slice_prob, sigma}.  The draws below are the written semantics; the device
# generator applies them with csrc/augment.hip (k_affine_sample with a slice table, k_mri_intensity_ws), the float64 forms here are their host twins.
MRI_KEYS = ("slice_motion", "gamma", "bias_field", "slice_intensity")
GAMMA_RANGE, BIAS_ORDER, BIAS_COEFFICIENT = (0.7, 1.5), 3, 0.5


def bias_monomials(order):
    """exponents (a, b, c) of x^a y^b z^c with a + b + c <= order, lexicographic: 4 / 10 / 20 terms for order 1 / 2 / 3"""
    return [(a, b, c) for a in range(order + 1) for b in range(order + 1 - a) for c in range(order + 1 - a - b)]


def draw_mri_parameters(augment, patch_shape, rng):
    """The draws of the four fetal keys for one patch, from `rng` (a numpy RandomState of the caller's: neither numpy's global state nor python's
    `random` is touched), in the order slice_motion, gamma, bias_field, slice_intensity.  Each key that is present draws its apply decision
    (prob > rng.random_sample()) and, only when it applies, its parameters.  -> dict of float64 arrays, None / 0 for what does not apply:
      slice_table (nz, 6)  rows (m0 .. m5): slice k reads (i', j') = (m0 i + m1 j + m2, m3 i + m4 j + m5), a rotation by theta_k about the
                           in-plane centre plus a shift t_k; slices not moved are exact identity rows;  slice_moved (nz,) bool
      gamma                exponent of the contrast curve (0.0: not applied)
      bias_coef            (4 | 10 | 20,) coefficients of bias_monomials(order)
      slice_gain           (nz,) gains, 1 on the slices not chosen"""
    nx, ny, nz = (int(v) for v in patch_shape)
    out = {"slice_table": None, "slice_moved": None, "gamma": 0.0, "bias_coef": None, "slice_gain": None}
    sm = augment.get("slice_motion")
    if sm is not None and sm["prob"] > rng.random_sample():
        moved = rng.random_sample(nz) < sm["slice_prob"]
        theta = np.deg2rad(rng.normal(0.0, sm["rotate"], nz))
        t = rng.normal(0.0, sm["translate"], (nz, 2))
        c0, c1 = (nx - 1) / 2.0, (ny - 1) / 2.0
        cs, sn = np.cos(theta), np.sin(theta)
        table = np.stack([cs, -sn, c0 - cs * c0 + sn * c1 + t[:, 0], sn, cs, c1 - sn * c0 - cs * c1 + t[:, 1]], axis=1)
        table[~moved] = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
        out["slice_table"], out["slice_moved"] = table, moved
    ga = augment.get("gamma")
    if ga is not None and ga["prob"] > rng.random_sample():
        lo, hi = ga.get("range", GAMMA_RANGE)
        out["gamma"] = float(rng.uniform(lo, 1.0) if rng.random_sample() < 0.5 else rng.uniform(1.0, hi))
    bf = augment.get("bias_field")
    if bf is not None and bf["prob"] > rng.random_sample():
        order, coefficient = int(bf.get("order", BIAS_ORDER)), bf.get("coefficient", BIAS_COEFFICIENT)
        if not 1 <= order <= 3:
            raise ValueError("bias_field order %r: 1, 2 or 3" % (order,))
        out["bias_coef"] = rng.uniform(-coefficient, coefficient, len(bias_monomials(order)))
    si = augment.get("slice_intensity")
    if si is not None and si["prob"] > rng.random_sample():
        chosen = rng.random_sample(nz) < si["slice_prob"]
        out["slice_gain"] = np.where(chosen, np.exp(rng.normal(0.0, si["sigma"], nz)), 1.0)
    return out


def apply_slice_motion(volume, table, order=1, cval=0.0, affine=None, corner=(0, 0, 0), size=None, z_off=0):
    """float64 host twin of the device gather: out[i, j, k] = volume at affine . (corner + (i', j', k), 1), (i', j') the in-plane map of table row
    k + z_off (a row outside the table is the identity), scipy map_coordinates(mode='constant') semantics: a point outside [0, n - 1] on any axis
    gives cval, order 0 picks floor(c + 0.5), order 1 is trilinear.  With the defaults (identity affine, the whole volume) it moves the slices of
    a patch against each other; an identity table then returns the input."""
    vol = np.asarray(volume)
    v = vol.astype(np.float64)
    nx, ny, nz = vol.shape if size is None else (int(s) for s in size)
    A = np.eye(4) if affine is None else np.asarray(affine, dtype=np.float64)
    table = np.asarray(table, dtype=np.float64)
    i, j, k = np.meshgrid(np.arange(nx, dtype=np.float64), np.arange(ny, dtype=np.float64), np.arange(nz, dtype=np.float64), indexing="ij")
    r = np.arange(nz) + int(z_off)
    m = np.tile(np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0]), (nz, 1))
    inside = (r >= 0) & (r < table.shape[0])
    m[inside] = table[r[inside]]
    ip = m[:, 0] * i + m[:, 1] * j + m[:, 2]
    jp = m[:, 3] * i + m[:, 4] * j + m[:, 5]
    p = (corner[0] + ip, corner[1] + jp, corner[2] + k)
    c = [A[a, 0] * p[0] + A[a, 1] * p[1] + A[a, 2] * p[2] + A[a, 3] for a in range(3)]
    X, Y, Z = vol.shape
    ok = (c[0] >= 0) & (c[0] <= X - 1) & (c[1] >= 0) & (c[1] <= Y - 1) & (c[2] >= 0) & (c[2] <= Z - 1)
    c = [np.where(ok, ca, 0.0) for ca in c]
    if order == 0:
        got = v[tuple(np.floor(ca + 0.5).astype(np.int64) for ca in c)]
    else:
        i0 = [np.floor(ca).astype(np.int64) for ca in c]
        f = [ca - ia for ca, ia in zip(c, i0)]
        i1 = [np.minimum(ia + 1, n - 1) for ia, n in zip(i0, (X, Y, Z))]
        along_z = lambda a, b: v[a, b, i0[2]] * (1 - f[2]) + v[a, b, i1[2]] * f[2]
        c00, c01, c10, c11 = along_z(i0[0], i0[1]), along_z(i0[0], i1[1]), along_z(i1[0], i0[1]), along_z(i1[0], i1[1])
        got = (c00 * (1 - f[1]) + c01 * f[1]) * (1 - f[0]) + (c10 * (1 - f[1]) + c11 * f[1]) * f[0]
    return np.where(ok, got, float(cval))


def gamma_augment(data, gamma):
    """contrast curve on the patch's own range: ((v - lo) / (hi - lo)) ^ gamma * (hi - lo) + lo; a constant patch is returned as it is"""
    data = np.asarray(data, dtype=np.float64)
    lo, hi = float(data.min()), float(data.max())
    if hi == lo or gamma == 0:
        return data
    return np.power(np.maximum((data - lo) / (hi - lo), 0.0), gamma) * (hi - lo) + lo


def bias_field(data, coef, vmin):
    """smooth multiplicative field on a patch (X, Y, Z): (v - vmin) * exp(P(x, y, z)) + vmin, P the polynomial with the coefficients `coef` of
    bias_monomials(order), x, y, z in [-1, 1] across the patch (an axis of length 1 sits at 0).  vmin: the volume's minimum - the background of
    z-scored data is a negative constant, and the coil scales signal, not background."""
    data = np.asarray(data, dtype=np.float64)
    coef = np.asarray(coef, dtype=np.float64).reshape(-1)
    order = {4: 1, 10: 2, 20: 3}[coef.size]
    axes = [np.linspace(-1.0, 1.0, n) if n > 1 else np.zeros(1) for n in data.shape]
    x, y, z = np.meshgrid(*axes, indexing="ij")
    p = np.zeros(data.shape)
    for w, (a, b, c) in zip(coef, bias_monomials(order)):
        p += w * x ** a * y ** b * z ** c
    return (data - vmin) * np.exp(p) + vmin


def slice_gain(data, gains, vmin):
    """per-slice gain on a patch (X, Y, Z): (v - vmin) * gains[k] + vmin on slice k"""
    data = np.asarray(data, dtype=np.float64)
    return (data - vmin) * np.asarray(gains, dtype=np.float64).reshape(1, 1, -1) + vmin


# ---------------------------------------------------------------------------------------------------------- the 48 cube isometries
def generate_permutation_keys():
    """keys ((rotate_y, rotate_z), flip_x, flip_y, flip_z, transpose); as in the reference only rotate_y and the flips act"""
    return set(itertools.product(itertools.combinations_with_replacement(range(2), 2), range(2), range(2), range(2), range(2)))


def random_permutation_key():
    return random.choice(list(generate_permutation_keys()))


def permute_data(data, key):
    """data (n_modalities, x, y, z)"""
    data = np.copy(data)
    (rotate_y, rotate_z), flip_x, flip_y, flip_z, transpose = key
    if rotate_y != 0:
        data = np.rot90(data, rotate_y, axes=(1, 2))
    if flip_x:
        data = data[:, ::-1]
    if flip_y:
        data = data[:, :, ::-1]
    if flip_z:
        data = data[:, :, :, ::-1]
    return data


def random_permutation_x_y(x_data, y_data):
    key = random_permutation_key()
    return permute_data(x_data, key), permute_data(y_data, key)


def reverse_permutation_key(key):
    return tuple(-r for r in key[0]), key[1], key[2], key[3], key[4]


def reverse_permute_data(data, key):
    (rotate_y, rotate_z), flip_x, flip_y, flip_z, transpose = reverse_permutation_key(key)
    data = np.copy(data)
    if flip_z:
        data = data[:, :, :, ::-1]
    if flip_y:
        data = data[:, :, ::-1]
    if flip_x:
        data = data[:, ::-1]
    if rotate_y != 0:
        data = np.rot90(data, rotate_y, axes=(1, 2))
    return data
