"""Multi-label clean-up on the device (csrc/postprocess.hip, the *_bits kernels) against its host definition
(fetal_net.postprocess.postprocess_label_map(device=False): scipy per channel, numpy for the merge).  Every comparison is exact: the
smoothing bit for bit, masks and label maps byte for byte."""
import numpy as np
import pytest
import torch
from scipy import ndimage

pytestmark = pytest.mark.gpu

CASES = [((17, 33, 9), 5, 0), ((40, 48, 56), 3, 1), ((24, 20, 28), 32, 2)]          # shape, channels, seed


def _pack(masks):
    """[L] masks -> uint32 words, bit l = channel l"""
    words = np.zeros(masks[0].shape, np.uint32)
    for l, m in enumerate(masks):
        words |= (np.asarray(m) != 0).astype(np.uint32) << np.uint32(l)
    return words


def _unpack(words, l):
    return ((words >> np.uint32(l)) & np.uint32(1)).astype(bool)


def _dev(words):
    return torch.from_numpy(words).cuda()


@pytest.mark.parametrize("shape,n_labels", [(s, l) for s, l, _ in CASES])
def test_channels_last_gaussian_bit_exact(shape, n_labels):
    """odd sizes and L = 5 catch a wrong z stride, L = 32 the last channel"""
    from fmri_hip import ops
    v = np.random.RandomState(1).rand(*(shape + (n_labels,)))
    d = torch.from_numpy(v).cuda()
    for sigma in (1, 0.5, 2.3, (1.0, 0.0, 2.0)):
        got = ops.gaussian_filter_channels_f64(d, sigma).cpu().numpy()
        for l in range(n_labels):
            ref = ndimage.gaussian_filter(v[..., l], sigma)
            assert np.array_equal(got[..., l], ref), (shape, sigma, l, float(np.abs(got[..., l] - ref).max()))
    assert np.array_equal(d.cpu().numpy(), v)                                         # the input is never a scratch buffer


def _constructed():
    shape = (20, 24, 28)
    a = np.zeros(shape, np.uint8)
    a[4:16, 4:20, 4:24] = 1
    a[7:13, 8:16, 8:20] = 0                       # a closed hole ...
    a[9:11, 10:14, 10:18] = 1                     # ... with an island inside
    b = a.copy()
    b[4:16, 10:12, 0:8] = 1                       # an arm to the border
    b[10, 11, 0:12] = 0                           # a tunnel from the border into the hole: not a hole any more
    c = np.zeros(shape, np.uint8)
    c[8:12, 9:15, 9:19] = 1                       # sits inside (a)'s hole
    d = np.zeros(shape, np.uint8)
    e = np.zeros(shape, np.uint8)                 # three components of 8 voxels: the first in scan order wins
    e[10:12, 10:12, 20:22] = 1
    e[2:4, 2:4, 2:4] = 1
    e[15:17, 3:5, 7:9] = 1
    return [a, b, c, d, e, a.copy()]


def test_constructed_volume_device_equals_host():
    from fetal_net.postprocess import postprocess_label_map, postprocess_prediction
    chans = _constructed()
    pred = np.stack([0.1 + 0.8 * ch for ch in chans], axis=-1).astype(np.float64)
    kw = dict(gaussian_std=0.5, threshold=0.5, labels=(1, 2, 4, 7, 9, 200))
    host = postprocess_label_map(pred, device=False, **kw)
    # the host result is what the case was built for (figures from the definition, computed with scipy)
    sm = [ndimage.gaussian_filter(pred[..., l], 0.5) for l in range(6)]
    mk = [postprocess_prediction(pred[..., l], 0.5, 0.5, device=False) for l in range(6)]
    filled_only = [int((mk[l] & ~(sm[l] > 0.5)).sum()) for l in range(6)]
    assert filled_only[0] == 512 and filled_only[1] == 0                              # (a)'s hole is filled, (b)'s is open
    assert int(mk[4].sum()) == 8 and mk[4][2, 2, 2]                                   # (e) keeps the component at [2, 2, 2]
    assert int((np.sum(mk, axis=0) > 1).sum()) > 0                                    # voxels in two masks
    assert dict(zip(*[x.tolist() for x in np.unique(host, return_counts=True)])) == {0: 9500, 1: 3474, 2: 218, 4: 240, 9: 8}
    assert not (host == 200).any() and not (host == 7).any()
    dev = postprocess_label_map(pred, device=True, **kw)
    assert dev.dtype == np.uint8 and dev.shape == host.shape
    assert np.array_equal(dev, host)


@pytest.fixture(scope="module", params=CASES, ids=lambda c: "%dx%dx%dx%d" % (c[0] + (c[1],)))
def field(request):
    shape, n_labels, seed = request.param
    rs = np.random.RandomState(seed)
    p = np.stack([ndimage.gaussian_filter(rs.rand(*shape), 2.0) for _ in range(n_labels)], axis=-1)
    p = (p - p.min()) / (p.max() - p.min())
    return p


@pytest.mark.parametrize("kw", [dict(), dict(gaussian_std=0.5), dict(fill_holes=False), dict(connected_component=False)],
                         ids=["default", "std0.5", "nofill", "nocc"])
def test_random_fields_device_equals_host(field, kw):
    from fetal_net.postprocess import postprocess_label_map
    n_labels = field.shape[-1]
    sm = np.stack([ndimage.gaussian_filter(field[..., l], kw.get("gaussian_std", 1)) for l in range(n_labels)])
    thr = float(np.quantile(sm, 0.6))
    host = postprocess_label_map(field, threshold=thr, device=False, **kw)
    dev = postprocess_label_map(field, threshold=thr, device=True, **kw)
    assert np.array_equal(dev, host)
    assert int(((sm > thr).sum(0) > 1).sum()) > 100 and len(np.unique(host)) > min(n_labels, 3)      # overlapping masks, several labels


def test_fill_holes_and_components_on_packed_masks():
    """ops level: every channel of the words against scipy on that channel alone.  Three channels, so bits 3..31 must stay zero; a
    second pack puts the slow snake next to single blocks, which converge at once and must come through the extra sweeps unchanged."""
    from fmri_hip import ops
    from fetal_net.postprocess import get_main_connected_component
    a, b, _, _, e, _ = _constructed()
    shape = a.shape
    for masks in ([b, np.zeros(shape, np.uint8), np.ones(shape, np.uint8)], [a, e, b]):
        words = _pack(masks)
        noisy = words | np.uint32(0xfffffff8)                                         # unused bits set on input: ignored, zero on output
        for w in (words, noisy):
            filled = ops.binary_fill_holes_bits(_dev(w), 3).cpu().numpy()
            big = ops.largest_components_bits(_dev(w), 3).cpu().numpy()
            assert filled.dtype == np.uint32 and not (filled >> np.uint32(3)).any() and not (big >> np.uint32(3)).any()
            for l, m in enumerate(masks):
                assert np.array_equal(_unpack(filled, l), ndimage.binary_fill_holes(m)), l
                assert np.array_equal(_unpack(big, l), get_main_connected_component(m)), l
    assert _unpack(ops.largest_components_bits(_dev(_pack([a, e, b])), 3).cpu().numpy(), 1)[2, 2, 2]

    s = np.zeros((9, 40, 40), np.uint8)                                               # the long snake: many propagation steps
    s[4, 2:38:4, 2:38] = 1
    s[4, 2:38, 2] = 1
    block = np.zeros_like(s)
    block[1:4, 5:30, 5:30] = 1
    two = np.zeros_like(s)
    two[0:2, 0:3, 0:3] = 1
    two[6:9, 30:40, 30:40] = 1
    ring = np.ones_like(s)                                                            # a shell around a closed cavity with one voxel in it
    ring[1:8, 1:39, 1:39] = 0
    ring[4, 20, 20] = 1
    masks = [block, s, two, 1 - s, ring]
    words = _pack(masks)
    big = ops.largest_components_bits(_dev(words), 5).cpu().numpy()
    filled = ops.binary_fill_holes_bits(_dev(words), 5).cpu().numpy()
    for l, m in enumerate(masks):
        assert np.array_equal(_unpack(big, l), get_main_connected_component(m)), l
        assert np.array_equal(_unpack(filled, l), ndimage.binary_fill_holes(m)), l
    assert np.array_equal(_unpack(big, 0), block.astype(bool))                        # the fast channel, untouched by the snake's sweeps
    assert not (big >> np.uint32(5)).any() and not (filled >> np.uint32(5)).any()
    masks32 = [s if l == 31 else (ring if l % 2 else two) for l in range(32)]          # all 32 bits in use, the snake in the last
    w32 = _pack(masks32)
    big32 = ops.largest_components_bits(_dev(w32), 32).cpu().numpy()
    fill32 = ops.binary_fill_holes_bits(_dev(w32), 32).cpu().numpy()
    for l in (0, 1, 30, 31):
        assert np.array_equal(_unpack(big32, l), get_main_connected_component(masks32[l])), l
        assert np.array_equal(_unpack(fill32, l), ndimage.binary_fill_holes(masks32[l])), l


def test_threshold_bits_and_label_map_ops():
    from fmri_hip import ops
    rs = np.random.RandomState(7)
    for shape, n_labels in (((5, 7, 37), 5), ((6, 9, 43), 32), ((3, 4, 5), 1)):       # 37 * 7 * 5 voxels: no multiple of the 256-voxel tile
        v = rs.rand(*(shape + (n_labels,)))
        v[..., 0][v[..., 0] > 0.9] = 0.5                                              # values equal to the threshold: not above it
        d = torch.from_numpy(v).cuda()
        words = ops.threshold_bits_f64(d, 0.5)
        assert words.dtype == torch.uint32 and tuple(words.shape) == shape
        ref = _pack([v[..., l] > 0.5 for l in range(n_labels)])
        assert np.array_equal(words.cpu().numpy(), ref)
        values = list(range(200, 200 + n_labels))
        got = ops.label_map_from_bits(words, d, values).cpu().numpy()
        idx = np.argmax(np.where(v > 0.5, v, -np.inf), axis=-1)
        want = np.where((v > 0.5).any(-1), np.asarray(values, np.uint8)[idx], 0).astype(np.uint8)
        assert got.dtype == np.uint8 and np.array_equal(got, want)
    tie = np.full((2, 3, 4, 3), 0.7)
    words = _dev(np.full((2, 3, 4), 0b110, np.uint32))
    assert (ops.label_map_from_bits(words, torch.from_numpy(tie).cuda(), (5, 6, 7)).cpu().numpy() == 6).all()      # first set bit among equals


def test_ops_refuse_cpu_tensors_and_wrong_arguments():
    from fmri_hip import ops
    w = torch.zeros((2, 3, 4), dtype=torch.uint32)
    v = torch.zeros((2, 3, 4, 2), dtype=torch.float64)
    for call in (lambda: ops.gaussian_filter_channels_f64(v, 1), lambda: ops.threshold_bits_f64(v, 0.5),
                 lambda: ops.binary_fill_holes_bits(w, 2), lambda: ops.largest_components_bits(w, 2),
                 lambda: ops.label_map_from_bits(w, v, (1, 2))):
        with pytest.raises(RuntimeError):
            call()
    with pytest.raises(ValueError):
        ops.binary_fill_holes_bits(w.cuda(), 33)
    with pytest.raises(ValueError):
        ops.label_map_from_bits(w.cuda(), v.cuda(), (1, 1))
    with pytest.raises(ValueError):
        ops.label_map_from_bits(w.cuda(), v.cuda(), (1, 2, 3))


def test_device_resident_form_and_default_path():
    from fetal_net.postprocess import postprocess_label_map
    shape, n_labels, seed = CASES[0]
    rs = np.random.RandomState(seed + 10)
    p = np.stack([ndimage.gaussian_filter(rs.rand(*shape), 2.0) for _ in range(n_labels)], axis=-1)
    p = (p - p.min()) / (p.max() - p.min())
    thr = float(np.quantile(p, 0.6))
    kw = dict(threshold=thr, labels=(9, 8, 7, 6, 5))
    host = postprocess_label_map(p, device=False, **kw)
    d = torch.from_numpy(p).cuda()
    out = postprocess_label_map(d, **kw)
    assert isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == shape
    assert np.array_equal(out.cpu().numpy(), host)
    assert np.array_equal(d.cpu().numpy(), p)
    auto = postprocess_label_map(p, **kw)                                             # a float64 array: the default is the device path
    assert isinstance(auto, np.ndarray) and np.array_equal(auto, host)
    one = postprocess_label_map(d[..., 0].contiguous(), threshold=thr, labels=[3])    # three dimensions: one label
    assert np.array_equal(one.cpu().numpy(), postprocess_label_map(p[..., 0], threshold=thr, labels=[3], device=False))
