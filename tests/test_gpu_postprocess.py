"""Device post-processing (csrc/postprocess.hip) against scipy.ndimage - the reference's own implementation of
fetal_net/postprocess.py:7-19 - on seeded volumes: the gaussian bit for bit, the masks voxel for voxel; edge cases: holes touching the
border (not holes), nested holes, several components of equal size (tie -> the first in scan order), an empty mask, a full mask."""
import numpy as np
import pytest
import torch
from scipy import ndimage

pytestmark = pytest.mark.gpu


def _blobs(shape, seed, sigma=3.0, q=0.6):
    rs = np.random.RandomState(seed)
    f = ndimage.gaussian_filter(rs.randn(*shape), sigma)
    return (f > np.quantile(f, q)).astype(np.uint8)


@pytest.mark.parametrize("shape", [(40, 48, 56), (17, 33, 9), (64, 64, 64)])
def test_gaussian_filter_bit_exact(shape):
    from fmri_hip import ops
    rs = np.random.RandomState(1)
    v = rs.rand(*shape)
    for sigma in (1, 0.5, 2.3, (1.0, 0.0, 2.0)):
        got = ops.gaussian_filter_f64(torch.from_numpy(v).cuda(), sigma).cpu().numpy()
        ref = ndimage.gaussian_filter(v, sigma)
        assert np.array_equal(got, ref), (shape, sigma, float(np.abs(got - ref).max()))


def _fill_holes(mask):
    """ops.binary_fill_holes_bits at one label on a 0/1 uint8 volume: packed with numpy, bit 0 unpacked, bits 1..31 must be zero"""
    from fmri_hip import ops
    words = ops.binary_fill_holes_bits(torch.from_numpy(mask.astype(np.uint32)).cuda(), 1).cpu().numpy()
    assert not (words >> 1).any()
    return (words & 1).astype(bool)


def _largest_component(mask):
    from fmri_hip import ops
    words = ops.largest_components_bits(torch.from_numpy(mask.astype(np.uint32)).cuda(), 1).cpu().numpy()
    assert not (words >> 1).any()
    return (words & 1).astype(bool)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_fill_holes_and_largest_component_equal_scipy(seed):
    from fetal_net.postprocess import get_main_connected_component
    m = _blobs((48, 56, 40), seed)
    assert np.array_equal(_fill_holes(m), ndimage.binary_fill_holes(m))
    assert np.array_equal(_largest_component(m), get_main_connected_component(m))


def test_edge_cases():
    from fetal_net.postprocess import get_main_connected_component
    shape = (20, 24, 28)
    m = np.zeros(shape, np.uint8)
    m[4:16, 4:20, 4:24] = 1
    m[7:13, 8:16, 8:20] = 0                       # a hole ...
    m[9:11, 10:14, 10:18] = 1                     # ... with an island inside (its own component, filled along with the hole)
    m[4:16, 10:12, 0:8] = 1                       # an arm to the border
    m[10, 11, 0:12] = 0                           # a tunnel from the border into the hole: not a hole any more
    for vol in (m, np.zeros(shape, np.uint8), np.ones(shape, np.uint8)):
        assert np.array_equal(_fill_holes(vol), ndimage.binary_fill_holes(vol))
        assert np.array_equal(_largest_component(vol), get_main_connected_component(vol))
    t = np.zeros(shape, np.uint8)                 # three components of 8 voxels each: scipy's argmax takes the first in scan order
    t[10:12, 10:12, 20:22] = 1
    t[2:4, 2:4, 2:4] = 1
    t[15:17, 3:5, 7:9] = 1
    got = _largest_component(t)
    assert np.array_equal(got, get_main_connected_component(t)) and got[2, 2, 2] and got.sum() == 8
    s = np.zeros((9, 40, 40), np.uint8)           # a long snake: many propagation steps
    s[4, 2:38:4, 2:38] = 1
    s[4, 2:38, 2] = 1
    assert np.array_equal(_largest_component(s), get_main_connected_component(s))


@pytest.mark.parametrize("kw", [dict(), dict(gaussian_std=0.5), dict(fill_holes=False), dict(connected_component=False, threshold=0.4)])
def test_postprocess_prediction_device_equals_host(kw):
    """the reference entry point on a volume-sized probability map (160x256x256 = BASELINE configs[4]) - device path == scipy path"""
    from fetal_net.postprocess import postprocess_prediction
    rs = np.random.RandomState(5)
    shape = (160, 256, 256) if not kw else (64, 96, 80)
    p = ndimage.gaussian_filter(rs.rand(*shape), 2.0)
    p = (p - p.min()) / (p.max() - p.min())
    dev = postprocess_prediction(p, device=True, **kw)
    host = postprocess_prediction(p, device=False, **kw)
    assert dev.dtype == bool and dev.shape == host.shape
    assert np.array_equal(dev, host)
    assert np.array_equal(postprocess_prediction(p, **kw), host)          # the default picks the device path here and agrees


def test_single_volume_is_the_label_chain_at_one_label():
    """one channel of the smallest field of tests/test_gpu_postprocess_labels.py (its CASES[0]: 17x33x9, 5 channels, seed 0): the mask of
    postprocess_prediction is where postprocess_label_map puts its one label, and both device forms equal the host"""
    from fetal_net.postprocess import postprocess_label_map, postprocess_prediction
    rs = np.random.RandomState(0)
    field = np.stack([ndimage.gaussian_filter(rs.rand(17, 33, 9), 2.0) for _ in range(5)], axis=-1)
    field = (field - field.min()) / (field.max() - field.min())
    p = np.ascontiguousarray(field[..., 0])
    thr = float(np.quantile(ndimage.gaussian_filter(p, 1), 0.6))
    host = postprocess_prediction(p, threshold=thr, device=False)
    dev = postprocess_prediction(p, threshold=thr, device=True)
    assert dev.dtype == bool and dev.shape == p.shape and host.any() and not host.all()
    assert np.array_equal(dev, postprocess_label_map(p, threshold=thr, labels=[7], device=True) == 7)
    assert np.array_equal(dev, host)
    assert np.array_equal(postprocess_label_map(p, threshold=thr, labels=[7], device=False) == 7, host)
