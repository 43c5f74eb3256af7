"""The device Euclidean distance transform (csrc/postprocess.hip: fmri_edt_u8, fmri_edt_two_class_u8) and what is built on it
(fetal_net.utils.create_distance_masks, DeviceDataFile(distance_masks=...)) against scipy.ndimage.distance_transform_edt.

Tolerances
  unit spacing: identical.  Every squared distance is an integer below 2^53, exact on both sides; the root is correctly rounded on both.
  other spacings: rtol 1e-15, zeros exactly where scipy has zeros.  With u = 2^-53: a term fl(fl(d * s)^2) is within 3u of the true one,
    the two additions add 2u, so either side's squared distance of any candidate is within 5u and the two minima differ by at most 10u;
    the root halves that and adds u per side: 7u = 7.8e-16.  The summation order (z, y, x here; x, y, z in scipy) is inside that bound.
  float32 masks of DeviceDataFile against scipy(...).astype(float32): rtol 2^-23 - a last-bit fp64 difference can flip the fp32 rounding.
"""
import functools
import random

import numpy as np
import pytest
import scipy.ndimage
import torch

pytestmark = pytest.mark.gpu

REF = (0.4, 0.4, 3.0)                       # the reference's voxel spacing (fetal_net/utils/create_distance_masks.py)
SKEW = (0.7, 1.3, 2.1)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the GPU box"
    from fmri_hip import ops as o
    return o


@functools.lru_cache(maxsize=None)
def random_volume(shape, density, seed=0):
    v = (np.random.RandomState(seed + 1000 * int(density * 1000) + sum(shape)).rand(*shape) < density).astype(np.uint8)
    if v.all():
        v[tuple(s // 2 for s in shape)] = 0
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def ellipsoid():
    x, y, z = np.meshgrid(np.arange(40), np.arange(48), np.arange(20), indexing="ij")
    v = (((x - 20) / 12.0) ** 2 + ((y - 22) / 15.0) ** 2 + ((z - 9) / 6.0) ** 2 < 1).astype(np.uint8)
    v.setflags(write=False)
    return v


def scipy_edt(vol, sampling):
    return scipy.ndimage.distance_transform_edt(vol, sampling=sampling)


def scipy_mask(vol, sampling):
    return scipy_edt(vol, sampling) + scipy_edt(1 - vol, sampling)


def unit(sampling):
    return sampling is None or all(float(s) == 1.0 for s in np.atleast_1d(sampling))


def check_equal(got, want, sampling, what=""):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.dtype == np.float64 and got.shape == want.shape, what
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(want > 0, np.abs(got - want) / want, np.abs(got - want))
    print("%s sampling=%s max rel err %.3e" % (what, sampling, float(np.nanmax(rel)) if rel.size else 0.0))
    if unit(sampling):
        np.testing.assert_array_equal(got, want, err_msg=what)
    else:
        np.testing.assert_array_equal(got == 0, want == 0, err_msg=what)
        np.testing.assert_allclose(got, want, rtol=1e-15, atol=0, err_msg=what)


def both_forms(ops, vol, sampling, what):
    d = torch.from_numpy(vol.copy()).cuda()
    check_equal(ops.distance_transform_edt_u8(d, sampling), scipy_edt(vol, sampling), sampling, what + " edt")
    if vol.any():                       # the two-class form needs both classes (a single class is +inf: test_degenerate_input)
        check_equal(ops.distance_mask_u8(d, sampling), scipy_mask(vol, sampling), sampling, what + " mask")


@pytest.mark.parametrize("density", [0.5, 0.97, 0.03])
@pytest.mark.parametrize("shape", [(17, 33, 9), (24, 20, 12), (1, 16, 16), (5, 1, 7)])
def test_random_volumes(ops, shape, density):
    vol = random_volume(shape, density)
    for sampling in (None, REF, SKEW):
        both_forms(ops, vol, sampling, "%s p=%s" % (shape, density))


def test_scalar_sampling_is_broadcast(ops):
    vol = random_volume((17, 33, 9), 0.5)
    d = torch.from_numpy(vol.copy()).cuda()
    check_equal(ops.distance_transform_edt_u8(d, 1.7), scipy_edt(vol, 1.7), 1.7, "scalar")
    check_equal(ops.distance_transform_edt_u8(d, 1.0), scipy_edt(vol, None), None, "scalar one")
    for bad in ((1.0, 2.0), (1.0, 0.0, 1.0), -1.0, (1.0, float("nan"), 1.0)):
        with pytest.raises(ValueError):
            ops.distance_transform_edt_u8(d, bad)


@pytest.mark.parametrize("sampling", [REF, SKEW])
def test_ellipsoid_two_class(ops, sampling):
    """the shape of real labels: one blob, long pruned walks"""
    vol = ellipsoid()
    check_equal(ops.distance_mask_u8(torch.from_numpy(vol.copy()).cuda(), sampling), scipy_mask(vol, sampling), sampling, "ellipsoid")


@pytest.mark.parametrize("density", [0.5, 0.995])
@pytest.mark.parametrize("shape", [(600, 3, 2), (3, 600, 2), (2, 3, 600)])
def test_lines_longer_than_a_workgroup(ops, shape, density):
    vol = random_volume(shape, density)
    for sampling in (None, REF):
        both_forms(ops, vol, sampling, "%s p=%s" % (shape, density))


@pytest.mark.parametrize("density", [0.5, 0.995])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_lines_past_the_lds_cap_take_the_global_pass(ops, axis, density):
    from fmri_hip._lib import lib
    cap = lib().fmri_edt_lds_max_line()
    assert cap == 1024
    shape = [2, 2, 2]
    shape[axis] = cap + 1
    vol = random_volume(tuple(shape), density)
    for sampling in (None, REF):
        both_forms(ops, vol, sampling, "%s p=%s" % (shape, density))


def test_no_pruning_possible(ops):
    """one zero in a corner of 64^3: every voxel has to look along the whole line in every pass; closed form in scipy's summation order"""
    vol = np.ones((64, 64, 64), np.uint8)
    vol[63, 63, 63] = 0
    d = np.stack(np.meshgrid(*[63.0 - np.arange(64)] * 3, indexing="ij"))
    for a, s in enumerate(REF):
        d[a] *= s
    np.multiply(d, d, d)
    want = np.sqrt(np.add.reduce(d, axis=0))
    got = ops.distance_transform_edt_u8(torch.from_numpy(vol).cuda(), REF)
    check_equal(got, want, REF, "corner zero")
    check_equal(got, scipy_edt(vol, REF), REF, "corner zero vs scipy")


def test_degenerate_input(ops):
    for shape in ((3, 4, 5), (1, 1, 1)):
        zeros = torch.zeros(shape, dtype=torch.uint8, device="cuda")
        ones = torch.ones(shape, dtype=torch.uint8, device="cuda")
        for sampling in (None, REF):
            assert torch.all(ops.distance_transform_edt_u8(zeros, sampling) == 0)
            assert torch.all(ops.distance_transform_edt_u8(ones, sampling) == float("inf"))
            # the two-class form: no voxel of the other class anywhere
            assert torch.all(ops.distance_mask_u8(zeros, sampling) == float("inf"))
            assert torch.all(ops.distance_mask_u8(ones, sampling) == float("inf"))


def test_bad_input(ops):
    for fn in (ops.distance_transform_edt_u8, ops.distance_mask_u8):
        with pytest.raises(RuntimeError):
            fn(torch.zeros(2, 3, 4, dtype=torch.uint8))
        with pytest.raises(AssertionError):
            fn(torch.zeros(2, 3, 4, device="cuda"))
        with pytest.raises(AssertionError):
            fn(torch.zeros(3, 4, dtype=torch.uint8, device="cuda"))


def test_create_distance_mask_device_equals_host():
    from fetal_net.utils.create_distance_masks import create_distance_mask
    vol = ellipsoid()
    for sampling in (REF, SKEW, (1, 1, 1)):
        host = create_distance_mask(vol, sampling, device=False)
        np.testing.assert_array_equal(host, scipy_mask(vol, sampling))
        check_equal(create_distance_mask(vol, sampling, device=True), host, sampling, "create_distance_mask")
    check_equal(create_distance_mask(vol * 3.0), create_distance_mask(vol, device=False), REF, "default sampling, float labels, device=None")


# ------------------------------------------------------------------------------------------------ masks made at load time
class _Root:
    pass


class FakeDataFile:
    def __init__(self, vols, truths, masks=None):
        self.root = _Root()
        self.root.data, self.root.truth = vols, truths
        self.root.mask = masks if masks is not None else []
        self.root.subject_ids = [("s%d" % i).encode() for i in range(len(vols))]


def synth_subjects(seed, shapes):
    """smooth random volumes; labels = the bright blobs, background on the volume's border (as fetal labels: the padding of the device
    data file then changes no distance inside the original extent)"""
    rs = np.random.RandomState(seed)
    vols, truths = [], []
    for s in shapes:
        v = scipy.ndimage.gaussian_filter(rs.randn(*s), 1.5) * 4.0
        t = (v > 0.02).astype(np.uint8)
        for a in range(3):
            edge = [slice(None)] * 3
            for side in (0, -1):
                edge[a] = side
                t[tuple(edge)] = 0
        assert t.any()
        vols.append(v + 0.3 * rs.randn(*s))
        truths.append(t)
    return vols, truths


def check_f32(got, want64, what):
    want = want64.astype(np.float32)
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.dtype == np.float32 and got.shape == want.shape, what
    np.testing.assert_array_equal(got == 0, want == 0, err_msg=what)
    np.testing.assert_allclose(got, want, rtol=2.0 ** -23, atol=0, err_msg=what)


def test_device_data_file_makes_the_masks():
    from fetal_net.device_generator import DeviceDataFile, device_data_generator
    shapes, ps, pad = [(20, 22, 9), (16, 16, 12)], (16, 16, 8), 3
    vols, truths = synth_subjects(3, shapes)
    ddf = DeviceDataFile(FakeDataFile(vols, truths), ps, samples_pad=pad, distance_masks=REF)
    plain = DeviceDataFile(FakeDataFile(vols, truths), ps, samples_pad=pad)
    assert plain.mask is None and sorted(ddf.mask) == [0, 1]
    assert ddf.nbytes() == plain.nbytes() + sum(4 * t.numel() for t in ddf.truth.values())
    for i, t in enumerate(truths):
        assert ddf.mask[i].shape == ddf.truth[i].shape and ddf.mask[i].dtype == torch.float32
        padded = ddf.truth[i].cpu().numpy()
        check_f32(ddf.mask[i], scipy_mask(padded, REF), "subject %d, padded grid" % i)
        # shift consistency: where the unpadded volume sits in the padded one, the mask is the unpadded labels' own
        off = [(p - s) // 2 for p, s in zip(padded.shape, t.shape)]
        block = tuple(slice(o, o + s) for o, s in zip(off, t.shape))
        np.testing.assert_array_equal(padded[block], t)
        assert padded.sum() == t.sum()
        check_f32(ddf.mask[i][block], scipy_mask(t, REF), "subject %d, original extent" % i)
        assert ddf.mask_for_crops(i) is ddf.mask[i]
    # True = the reference's spacing
    auto = DeviceDataFile(FakeDataFile(vols, truths), ps, samples_pad=pad, distance_masks=True)
    assert all(torch.equal(auto.mask[i], ddf.mask[i]) for i in (0, 1))

    np.random.seed(5)
    random.seed(5)
    gen = device_data_generator(FakeDataFile(vols, truths), [0, 1], batch_size=2, patch_shape=ps, augment=None, skip_blank=False,
                                categorical=False, is3d=True, truth_index=0, truth_size=ps[2], samples_pad=pad, shuffle_index_list=False,
                                distance_masks=REF)
    (x, m), y = next(gen)
    gen.close()
    assert tuple(x.shape) == (2, 1) + ps and tuple(m.shape) == tuple(y.shape) == (2, 1) + ps and m.dtype == torch.float32
    np.random.seed(5)                       # the generator's own draws: one corner per patch, subjects 0 and 1 in order
    for b in (0, 1):
        corner = [np.random.randint(low=0, high=h) for h in np.array(ddf.truth[b].shape) - np.array(ps)]
        crop = tuple(slice(c, c + p) for c, p in zip(corner, ps))
        tb = ddf.truth[b].cpu().numpy()
        yb, mb = y[b, 0].cpu().numpy(), m[b, 0].cpu().numpy()
        np.testing.assert_array_equal(yb, tb[crop])
        assert np.isfinite(mb).all()
        np.testing.assert_array_equal(mb, ddf.mask[b][crop].cpu().numpy())
        fg = scipy_edt(tb, REF)[crop]
        assert (yb == 1).any()
        check_f32(mb[yb == 1], fg[yb == 1], "patch %d" % b)

    masks = [scipy_mask(t, REF) for t in truths]
    with pytest.raises(ValueError):
        DeviceDataFile(FakeDataFile(vols, truths, masks), ps, samples_pad=pad, distance_masks=REF)
    with pytest.raises(ValueError):
        next(device_data_generator(FakeDataFile(vols, truths, masks), [0, 1], patch_shape=ps, distance_masks=True))


def test_mask_weighted_training_from_a_file_without_masks():
    """the whole chain: labels in HBM -> distance masks (device EDT) -> ([x, masks], y) batches -> the mask-weighted loss"""
    import fetal_net.model as fmodel
    from fetal_net import metrics as M
    from fetal_net.device_generator import device_data_generator
    shape = (1, 16, 16, 16)
    vols, truths = synth_subjects(7, [(14, 15, 4), (13, 14, 5)])
    np.random.seed(1)
    random.seed(1)
    gen = device_data_generator(FakeDataFile(vols, truths), [0, 1], batch_size=2, patch_shape=shape[1:], augment=None, skip_blank=True,
                                categorical=False, is3d=True, truth_index=0, truth_size=16, samples_pad=3, shuffle_index_list=False,
                                distance_masks=REF)
    model = fmodel.isensee2017_model_3d(input_shape=shape, loss_function=M.dice_and_xent_mask, mask_shape=shape, depth=3, n_base_filters=4,
                                        n_segmentation_levels=2, dropout_rate=0.0, compute_dtype="fp32")
    losses = []
    for _ in range(15):
        (x, m), y = next(gen)
        assert bool(torch.isfinite(m).all())
        losses.append(float(model.train_on_batch([x, m], y)[0]))
    gen.close()
    print("losses", losses)
    assert np.isfinite(losses).all()
    assert min(losses[-4:]) < losses[0]
