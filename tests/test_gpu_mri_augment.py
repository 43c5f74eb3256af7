"""The fetal acquisition augmenters on the device: the gather with a per-slice motion table (fmri_affine_sample_batch, table=) and the gamma / bias
field / slice gain launch (fmri_mri_intensity_ws_batch) against the float64 restatement of tests/mri_augment_restatement.py, and the device
generator with the four new `augment` keys."""
import random

import numpy as np
import pytest
import scipy.ndimage
import torch

import mri_augment_restatement as R

pytestmark = pytest.mark.gpu

IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the GPU box"
    from fmri_hip import ops as o
    return o


def _affine(shape, angles, scale, shift):
    """rotation + scale about the volume's centre, then a shift"""
    from fetal_net.augment import distort_image
    return distort_image(np.empty(shape), np.eye(4), scale_factor=scale, rotate_factor=angles, translate_factor=shift)[1]


def _table(rs, nz, moved, nx, ny, rotate=4.0, translate=1.0):
    tab = np.tile(np.array(IDENTITY), (nz, 1))
    for k in moved:
        th = np.deg2rad(rs.normal(0, rotate))
        t = rs.normal(0, translate, 2)
        c0, c1, cs, sn = (nx - 1) / 2.0, (ny - 1) / 2.0, np.cos(th), np.sin(th)
        tab[k] = (cs, -sn, c0 - cs * c0 + sn * c1 + t[0], sn, cs, c1 - sn * c0 - cs * c1 + t[1])
    return tab


@pytest.fixture(scope="module")
def volumes():
    rs = np.random.RandomState(7)
    vol = (scipy.ndimage.gaussian_filter(rs.randn(12, 11, 9), 1.0) * 4.0 + 0.2 * rs.randn(12, 11, 9)).astype(np.float32)
    lab = rs.randint(0, 3, size=(12, 11, 9)).astype(np.uint8)                    # three values, voxel noise: any wrong index shows
    return vol, lab, torch.from_numpy(vol).cuda(), torch.from_numpy(lab).cuda()


def test_gather_with_a_slice_table_equals_the_restatement(ops, volumes):
    """image trilinear to the bound of the plain gather, labels exact; two identity rows and three moved ones"""
    vol, lab, dvol, dlab = volumes
    rs = np.random.RandomState(3)
    size, corner = (8, 8, 5), (2, 1, 3)
    A = _affine(vol.shape, (0.04, -0.03, 0.2), (1.06, 0.94, 1.0), (0.3, -0.2, 0.0))
    tab = _table(rs, 5, (0, 2, 4), 8, 8)
    assert [tuple(r) == IDENTITY for r in tab] == [False, True, False, True, False]
    dtab = torch.from_numpy(tab).cuda()
    want, coords = R.gather_slices(vol, A, corner, size, tab, 0, 1, float(vol.min()))
    got = ops.affine_sample_slices(dvol, A, corner, size, torch.empty(size, device="cuda"), dtab, 0, order=1, cval=float(vol.min()))
    assert R.inside(coords, vol.shape).mean() > 0.5
    np.testing.assert_allclose(got.cpu().numpy(), want, rtol=0, atol=R.GATHER_ATOL)
    assert R.rounding_margin(coords, lab.shape) > 1e-9                          # no label decision within rounding of flipping (the seed's choice)
    want_l, _ = R.gather_slices(lab, A, corner, size, tab, 0, 0, 0.0)
    got_l = ops.affine_sample_slices(dlab, A, corner, size, torch.empty(size, device="cuda", dtype=torch.uint8), dtab, 0, order=0, cval=0.0)
    assert np.array_equal(got_l.cpu().numpy(), want_l.astype(np.uint8))
    plain = ops.affine_sample(dlab, A, corner, size, torch.empty(size, device="cuda", dtype=torch.uint8), order=0, cval=0.0)
    assert torch.equal(plain[..., [1, 3]], got_l[..., [1, 3]]) and not torch.equal(plain, got_l)      # the moved slices moved, the others did not


def _batch_case(rs, vol, lab, B, size, nzt):
    vols = [rs.randint(2) for _ in range(B)]
    affines = [_affine(vol.shape, (rs.uniform(-0.05, 0.05), rs.uniform(-0.05, 0.05), rs.uniform(-0.3, 0.3)), (rs.uniform(0.9, 1.1), rs.uniform(0.9, 1.1), 1.0),
                       (rs.uniform(-0.5, 0.5), rs.uniform(-0.5, 0.5), 0.0)) for _ in range(B)]
    corners = [(rs.randint(0, 12 - size[0] + 1), rs.randint(0, 11 - size[1] + 1), rs.randint(0, 9 - max(size[2], nzt) + 1)) for _ in range(B)]
    tabs = np.stack([_table(rs, nzt, [k for k in range(nzt) if rs.rand() < 0.6], size[0], size[1]) for _ in range(B)])
    return vols, affines, corners, tabs


@pytest.mark.parametrize("B,size,nzt,z_off,wide", [(17, (5, 4, 3), 3, 0, False),      # crosses the 16-patch chunk
                                                   (3, (6, 5, 1), 5, 2, False),       # nz = 1: the 2-D truth, under image slice 2
                                                   (2, (6, 5, 4), 5, 2, False),       # the last slice falls off the table: identity
                                                   (3, (5, 4, 2), 4, 1, True)])       # out_ld > nz: a view into wider rows
def test_gather_batch_shapes(ops, volumes, B, size, nzt, z_off, wide):
    vol, lab, dvol, dlab = volumes
    vol2 = np.ascontiguousarray(vol[::-1]) * 0.5 + 1.0
    lab2 = np.ascontiguousarray(lab[:, ::-1])
    dv, dl = [dvol, torch.from_numpy(vol2).cuda()], [dlab, torch.from_numpy(lab2).cuda()]
    rs = np.random.RandomState(100 + B + nzt)
    pick, affines, corners, tabs = _batch_case(rs, vol, lab, B, size, nzt)
    dtab = torch.from_numpy(tabs).cuda()
    cv = [float((vol, vol2)[p].min()) for p in pick]
    ld = size[2] + 3 if wide else size[2]
    for src, host, order, dtype, cvals in ((dv, (vol, vol2), 1, torch.float32, cv), (dl, (lab, lab2), 0, torch.uint8, [0.0] * B)):
        buf = torch.full((B,) + size[:2] + (ld,), 77, device="cuda", dtype=dtype)
        out = buf[..., 2:2 + size[2]] if wide else buf
        ops.affine_sample_batch([src[p] for p in pick], affines, corners, size, out, order, cvals, table=dtab, z_off=z_off, out_ld=ld if wide else None)
        got = out.cpu().numpy()
        margin = np.inf
        for b in range(B):
            want, coords = R.gather_slices(host[pick[b]], affines[b], corners[b], size, tabs[b], z_off, order, cvals[b])
            if order == 1:
                np.testing.assert_allclose(got[b], want, rtol=0, atol=R.GATHER_ATOL)
            else:
                margin = min(margin, R.rounding_margin(coords, lab.shape))
                assert np.array_equal(got[b], want.astype(np.uint8)), b
            single = ops.affine_sample_slices(src[pick[b]], affines[b], corners[b], size, torch.empty(size, device="cuda", dtype=dtype), dtab[b], z_off,
                                              order=order, cval=cvals[b])
            assert torch.equal(single, out[b])                                   # the single entry point = row b of the batch
        assert order == 1 or margin > 1e-9
        if wide:
            assert bool((buf[..., :2] == 77).all()) and bool((buf[..., 2 + size[2]:] == 77).all())     # nothing written beside the view
        if z_off + size[2] > nzt:                                                # slices past the table: the plain gather's
            plain = ops.affine_sample_batch([src[p] for p in pick], affines, corners, size, torch.empty((B,) + size, device="cuda", dtype=dtype), order, cvals)
            assert torch.equal(plain[..., nzt - z_off:], out[..., nzt - z_off:])


@pytest.mark.parametrize("order,dtype", [(1, torch.float32), (0, torch.uint8)])
def test_identity_table_is_the_plain_gather_bit_for_bit(ops, volumes, order, dtype):
    vol, lab, dvol, dlab = volumes
    rs = np.random.RandomState(5)
    B, size = 17, (6, 5, 4)
    pick, affines, corners, _ = _batch_case(rs, vol, lab, B, size, 4)
    src = [dvol if dtype == torch.float32 else dlab] * B
    cv = [float(vol.min()) if order else 0.0] * B
    ident = torch.from_numpy(np.tile(np.array(IDENTITY), (B, 4, 1))).cuda()
    a = ops.affine_sample_batch(src, affines, corners, size, torch.empty((B,) + size, device="cuda", dtype=dtype), order, cv)
    b = ops.affine_sample_batch(src, affines, corners, size, torch.empty((B,) + size, device="cuda", dtype=dtype), order, cv, table=ident)
    assert torch.equal(a, b)


@pytest.mark.parametrize("order,dtype", [(1, torch.float32), (0, torch.uint8)])
def test_identity_table_is_the_plain_gather_bit_for_bit_on_a_million_voxels(ops, order, dtype):
    """the two kernels must round every coordinate alike: a product fused differently moves the last bit of an fp64 coordinate, which shows in
    one fp32 result among ~1e5 - so 17 patches of 48 x 40 x 32 under rotations up to 40 degrees, compared on the device"""
    rs = np.random.RandomState(6)
    shape, size, B = (64, 56, 40), (48, 40, 32), 17
    vol = torch.from_numpy(rs.randn(*shape).astype(np.float32)).cuda() if order else torch.from_numpy(rs.randint(0, 3, shape).astype(np.uint8)).cuda()
    affines = [_affine(shape, (rs.uniform(-0.1, 0.1), rs.uniform(-0.1, 0.1), rs.uniform(-0.7, 0.7)), (rs.uniform(0.8, 1.2), rs.uniform(0.8, 1.2), 1.0),
                       rs.uniform(-3, 3, 3)) for _ in range(B)]
    corners = [[int(rs.randint(0, s - p + 1)) for s, p in zip(shape, size)] for _ in range(B)]
    ident = torch.from_numpy(np.tile(np.array(IDENTITY), (B, size[2], 1))).cuda()
    cv = [-4.0 if order else 0.0] * B
    a = ops.affine_sample_batch([vol] * B, affines, corners, size, torch.empty((B,) + size, device="cuda", dtype=dtype), order, cv)
    b = ops.affine_sample_batch([vol] * B, affines, corners, size, torch.empty((B,) + size, device="cuda", dtype=dtype), order, cv, table=ident)
    assert torch.equal(a, b) and float((a != cv[0]).float().mean()) > 0.5


def _ws_is_armed(ws):
    return not bool(ws.any().item())


INTENSITY_CASES = {"gamma": (True, False, False), "bias": (False, True, False), "gains": (False, False, True), "all": (True, True, True)}


@pytest.mark.parametrize("case", sorted(INTENSITY_CASES))
def test_intensity_kernel_equals_the_restatement(ops, case):
    """B = 3 patches of 7 x 6 x 5 (210 elements: no multiple of 4); patch 1 skips everything and stays bit-identical; the error is printed
    relative to the restated patch's range before it is held to R.MRI_INTENSITY_TOL"""
    use_g, use_b, use_s = INTENSITY_CASES[case]
    rs = np.random.RandomState(12)
    vmin = -1.5
    x0 = np.maximum(rs.randn(3, 7, 6, 5) * 1.2, vmin).astype(np.float32)         # z-scored data over a constant negative background
    gam = [0.75 if use_g else 0.0, 0.0, 1.4 if use_g else 0.0]
    coefs = [rs.uniform(-0.5, 0.5, 20) if use_b else None, None, rs.uniform(-0.5, 0.5, 10) if use_b else None]
    gains = [np.exp(rs.normal(0, 0.3, 5)) if use_s else None, None, np.array([1, 2.0, 1, 0.5, 1]) if use_s else None]
    x = torch.from_numpy(x0).cuda()
    stats, ws = ops.aug_workspace("cuda", 3)
    ops.minmax_ws_batch(x, stats, ws)
    before = stats.clone()
    dg = [None if g is None else torch.from_numpy(g.astype(np.float32)).cuda() for g in gains]
    ops.mri_intensity_ws_batch(x, stats, ws, gam, coefs, dg, [vmin] * 3)
    torch.cuda.synchronize()
    got = x.cpu().numpy()
    assert np.array_equal(got[1], x0[1]) and stats[1].tolist() == before[1].tolist()
    worst = 0.0
    for b in (0, 2):
        want = R.mri_intensity(x0[b], gam[b], coefs[b], None if gains[b] is None else gains[b].astype(np.float32), vmin)
        err = R.relative_error(got[b], want)
        print("mri_intensity %s patch %d: max error / range = %.3e" % (case, b, err))
        worst = max(worst, err)
        assert not np.array_equal(got[b], x0[b])
        assert stats[b].tolist() == [float(got[b].min()), float(got[b].max())]
    assert _ws_is_armed(ws)
    assert worst <= R.MRI_INTENSITY_TOL, worst
    if case == "gains":                                                          # gain 2 on one slice doubles (v - vmin) there, exactly in fp32 too
        assert np.array_equal(got[2][..., 1] - vmin, 2 * (x0[2][..., 1] - vmin)) and np.array_equal(got[2][..., [0, 2, 4]], x0[2][..., [0, 2, 4]])


def test_intensity_kernel_on_a_constant_patch(ops):
    x = torch.full((1, 7, 6, 5), 2.5, device="cuda")
    stats, ws = ops.aug_workspace("cuda", 2)
    ops.minmax_ws_batch(x, stats[:1], ws[:1])
    ops.mri_intensity_ws_batch(x, stats[:1], ws[:1], [1.3], [None], [None], [-1.0])
    assert bool((x == 2.5).all()) and stats[0].tolist() == [2.5, 2.5] and _ws_is_armed(ws)
    ops.mri_intensity_ws(x[0], stats[0], ws[0], gamma=0.8, coef=np.full(4, 0.1), gains=torch.full((5,), 1.5, device="cuda"), vmin=-1.0)
    got = x.cpu().numpy()
    assert np.isfinite(got).all() and stats[0].tolist() == [float(got.min()), float(got.max())] and _ws_is_armed(ws)
    want = R.mri_intensity(np.full((7, 6, 5), 2.5), 0.8, np.full(4, 0.1), np.full(5, 1.5), -1.0)      # gamma leaves it alone, the others act
    assert R.relative_error(got[0], want) <= R.MRI_INTENSITY_TOL


# ---------------------------------------------------------------------------------------------------------------- the generator
class _Root:
    pass


class FakeDataFile:
    def __init__(self, vols, truths, masks=None):
        self.root = _Root()
        self.root.data, self.root.truth = vols, truths
        self.root.mask = masks if masks is not None else []


BASE = {"flip": [0.5, 0.5, 0], "scale": [0.08, 0.08, 0], "rotate": [0, 0, 12], "translate": [1.5, 1.5, 1]}
KEYS = {"slice_motion": {"prob": 1, "slice_prob": 0.5, "rotate": 4.0, "translate": 1.0}, "gamma": {"prob": 1},
        "bias_field": {"prob": 1, "order": 3, "coefficient": 0.5}, "slice_intensity": {"prob": 1, "slice_prob": 0.5, "sigma": 0.2}}
PS = (8, 8, 4)


@pytest.fixture(scope="module")
def data_file():
    rs = np.random.RandomState(4)
    vols, truths = [], []
    for _ in range(3):
        v = scipy.ndimage.gaussian_filter(rs.randn(20, 18, 12), 1.2) * 4.0 + 0.2 * rs.randn(20, 18, 12)
        vols.append(v.astype(np.float32))                                        # float32: the volume minimum is the kernels' vmin exactly
        truths.append((scipy.ndimage.gaussian_filter(rs.randn(20, 18, 12), 1.5) > 0.0).astype(np.uint8))
    return FakeDataFile(vols, truths)


def _batches(df, augment, n, seed=1, **kw):         # seed 1: the first three patches lie inside the volumes, not in their padding
    from fetal_net.device_generator import device_data_generator
    np.random.seed(seed)
    random.seed(seed)
    args = dict(batch_size=3, augment=augment, patch_shape=PS, skip_blank=False, categorical=False, is3d=True, truth_index=0, truth_size=4,
                shuffle_index_list=False, noise_seed=5)
    args.update(kw)
    gen = device_data_generator(df, [0, 1, 2], **args)
    out = [next(gen) for _ in range(n)]
    torch.cuda.synchronize()
    return out


def test_generator_keys_at_prob_zero_change_nothing(data_file):
    """(a) passes without the feature by design: unknown keys are ignored there"""
    off = dict(BASE, **{k: dict(v, prob=0) for k, v in KEYS.items()})
    for (x0, y0), (x1, y1) in zip(_batches(data_file, BASE, 3), _batches(data_file, off, 3)):
        assert torch.equal(x0, x1) and torch.equal(y0, y1)


def test_generator_batched_equals_patch_by_patch_and_reproduces(data_file):
    on = dict(BASE, **KEYS)
    a, b, c = _batches(data_file, on, 2), _batches(data_file, on, 2, batched=False), _batches(data_file, on, 2)
    plain = _batches(data_file, BASE, 2)
    for (xa, ya), (xb, yb), (xc, yc), (xp, yp) in zip(a, b, c, plain):
        assert torch.equal(xa, xb) and torch.equal(ya, yb) and torch.equal(xa, xc) and torch.equal(ya, yc)
        assert not torch.equal(xa, xp) and not torch.equal(ya, yp) and bool(torch.isfinite(xa).all())


def test_generator_labels_mask_and_previous_truth_move_with_their_slice(data_file):
    """(c) 2-D flow, a 'mask volume' equal to the (padded) labels: the mask batch IS y; the previous-slice truth channel is the label slice
    prev_truth_index moved by ITS row of the table - the y of a run that asks for that slice as the truth"""
    root = data_file.root
    masks = [np.pad(t.astype(np.float32), ((3, 3), (3, 3), (5, 5))) for t in root.truth]          # samples_pad 3, then 2 slices of patch padding
    df = FakeDataFile(root.data, root.truth, masks)
    on = dict(BASE, **KEYS)
    kw = dict(is3d=False, truth_size=1, prev_truth_size=1)
    for batched in (True, False):
        ((x, m), y), = _batches(df, on, 1, truth_index=2, prev_truth_index=2, batched=batched, **kw)
        assert x.shape == (3, 8, 8, 5) and 0.02 < float(y.float().mean()) < 0.98
        assert torch.equal(m, y.float()) and torch.equal(x[..., 4:5], y.float())
        ((x1, _), y1), = _batches(df, on, 1, truth_index=2, prev_truth_index=1, batched=batched, **kw)
        ((_, _), y2), = _batches(df, on, 1, truth_index=1, prev_truth_index=1, batched=batched, **kw)
        assert torch.equal(y1, y) and torch.equal(x1[..., 4:5], y2.float()) and torch.equal(x1[..., :4], x[..., :4])
    ((_, _), yp), = _batches(df, BASE, 1, truth_index=2, prev_truth_index=2, **kw)
    assert not torch.equal(yp, y)                                                # and the labels did move


def _sampler(data_file, augment):
    from fetal_net.device_generator import DeviceDataFile, _Sampler
    ddf = DeviceDataFile(data_file, PS)
    return ddf, _Sampler(ddf, PS, augment, 0, 4, None, None, False, 5)


def _launch(sampler, seed=1):
    np.random.seed(seed)
    random.seed(seed)
    plans = [sampler.plan(i) for i in (0, 1, 2)]
    x = torch.empty((3,) + PS, device="cuda")
    y = torch.empty((3,) + PS, device="cuda", dtype=torch.uint8)
    sampler.launch(plans, x, y)
    torch.cuda.synchronize()
    return plans, x.cpu().numpy(), y.cpu().numpy()


def test_generator_batch_equals_the_host_forms_on_the_planned_draws(data_file, ops):
    """(d) the plan's numbers through fetal_net/augment.py's float64 forms: the gather of the plan's affine, corner and table within the gather's
    bound, then gamma / bias field / slice gain on that gathered patch (the device's own fp32 gather) within the intensity bound"""
    from fetal_net.augment import apply_slice_motion, bias_field, gamma_augment, slice_gain
    ddf, s_all = _sampler(data_file, dict(BASE, **KEYS))
    plans, x, _ = _launch(s_all)
    for b, q in enumerate(plans):
        r = q["mri"]
        assert r["slice_table"].shape == (4, 6) and r["gamma"] > 0 and r["bias_coef"].shape == (20,) and r["slice_gain"].shape == (4,)
        vol, vmin = ddf.data[q["index"]], ddf.min[q["index"]]
        xg = ops.affine_sample_slices(vol, q["A"], q["corner"], PS, torch.empty(PS, device="cuda"), torch.from_numpy(r["slice_table"]).cuda(), 0, order=1,
                                      cval=vmin).cpu().numpy()
        host = apply_slice_motion(vol.cpu().numpy(), r["slice_table"], order=1, cval=vmin, affine=q["A"], corner=q["corner"], size=PS)
        np.testing.assert_allclose(xg, host, rtol=0, atol=R.GATHER_ATOL)
        assert (xg != np.float32(vmin)).mean() > 0.9                              # a patch of the volume, not of its padding
        want = slice_gain(bias_field(gamma_augment(xg, r["gamma"]), r["bias_coef"], vmin), r["slice_gain"].astype(np.float32), vmin)
        err = R.relative_error(x[b], want)
        print("mri_intensity generator patch %d: max error / range = %.3e" % (b, err))
        assert err <= R.MRI_INTENSITY_TOL, err


def test_slice_motion_alone_moves_only_the_marked_slices(data_file):
    """(e) against the same seeds without the key"""
    _, s_motion = _sampler(data_file, dict(BASE, slice_motion=KEYS["slice_motion"]))
    _, s_plain = _sampler(data_file, BASE)
    plans, x, y = _launch(s_motion)
    plans_p, xp, yp = _launch(s_plain)
    moved = np.stack([q["mri"]["slice_moved"] for q in plans])
    assert all(q["mri"] is None for q in plans_p) and moved.any() and not moved.all()
    for b in range(3):
        for k in range(4):
            if not moved[b, k]:
                assert np.array_equal(y[b, :, :, k], yp[b, :, :, k]) and np.array_equal(x[b, :, :, k], xp[b, :, :, k])
    assert any(not np.array_equal(y[b, :, :, k], yp[b, :, :, k]) for b in range(3) for k in range(4) if moved[b, k])
    assert any(not np.array_equal(x[b, :, :, k], xp[b, :, :, k]) for b in range(3) for k in range(4) if moved[b, k])
