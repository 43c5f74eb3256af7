"""The volume stays on the device through tiled prediction and the eight-flip TTA.

Kernels: fmri_volume_pad_flip and fmri_tile_finalize_flip against their numpy restatements (tests/tta_resident_restatement.py, proven
against np.pad / np.flip / the crop in tests/test_host_tta_resident.py), bit for bit.

Flows: the resident route against the kept host route (`prediction._predict_flips_host`, `Stage._infer_host`, `device=False`) driving the
SAME engine model: both fill the tiler's fp32 volume with the same bytes, replay the same captured graphs over the same index list and
divide the same float64 sums, so all that is left between them is the order of the float64 atomic adds of the overlap-add."""
import ctypes

import numpy as np
import pytest

import tta_resident_restatement as R

pytestmark = pytest.mark.gpu

# Route against route.  The starting bar was the 1e-6 of tests/test_gpu_tta.py ("same bf16 network outputs; fp64 overlap-add on both
# sides").  Measured on the MI355X, five runs of this file: 0.0 in every 3-D flow (one tile group per launch, the adds of a voxel arrive in
# one order on both routes) and at most 5.551e-17 = 2^-54 in the 2-D flows (64 tiles per launch, their adds race), i.e. one unit in the
# last place of a mean below 0.5 and well inside max(cnt) * 2^-52 = 1.8e-15, the level two orders of up to 8 float64 adds can differ by.
# The bar is therefore twice the measured value.
ROUTE_ATOL = 2 * 5.551e-17
# np.median of 8 is the midpoint of the two middle values: it does not amplify a sup-norm difference, but each side rounds its own
# midpoint (a sum below 2, halved: at most 2^-54 each)
MEDIAN_ATOL = ROUTE_ATOL + 2.0 ** -53


@pytest.fixture(scope="module")
def ops():
    from fmri_hip import ops as o
    return o


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------------------------------- kernels
PAD_CASES = [((1, 1, 1), (1, 0, 2), (3, 2, 4)),               # one voxel in a box of fill
             ((5, 7, 3), (2, 0, 1), (9, 7, 6)),               # the tiler's asymmetric padding
             ((5, 7, 3), (-1, -2, 0), (3, 4, 3)),             # a crop
             ((4, 5, 1), (1, 2, 0), (7, 8, 1)),               # Z = 1
             ((33, 17, 9), (4, 1, 2), (40, 20, 12))]          # more than one workgroup, odd pitches
CONVERSIONS = [(np.float64, np.float32), (np.float32, np.float32), (np.float64, np.float64)]


@pytest.mark.parametrize("shape,lo,out_shape", PAD_CASES)
def test_volume_pad_flip_bit_for_bit(ops, shape, lo, out_shape):
    import torch
    rs = np.random.RandomState(sum(shape))
    for src_t, dst_t in CONVERSIONS:
        src = (rs.randn(*shape) * 100).astype(src_t)          # float64 values that round in float32
        d_src = _dev(src)
        for fill in (-3.0, 0.1):
            for mask in range(8):
                dst = torch.full(out_shape, 7.0, dtype=torch.float32 if dst_t == np.float32 else torch.float64, device="cuda")
                ops.volume_pad_flip(d_src, dst, lo, mask, fill)
                want = R.volume_pad_flip(src, out_shape, lo, mask, fill, dst_t)
                assert dst.cpu().numpy().tobytes() == want.tobytes(), (src_t, dst_t, fill, mask)


@pytest.mark.parametrize("dst_t,offsets", [(np.float32, (1, 2, 3)), (np.float64, (1,))])
def test_volume_pad_flip_at_every_store_width(ops, dst_t, offsets):
    """a destination that starts 4 / 8 / 12 bytes into a 16-byte line takes the narrower stores; the elements around it stay"""
    import torch
    shape, lo, out_shape = (33, 17, 9), (4, 1, 2), (40, 20, 11)
    src = np.random.RandomState(5).randn(*shape) * 100
    n = int(np.prod(out_shape))
    want = R.volume_pad_flip(src, out_shape, lo, 5, 0.1, dst_t)
    for off in offsets:
        buf = torch.full((n + 8,), 7.0, dtype=torch.float32 if dst_t == np.float32 else torch.float64, device="cuda")
        ops.volume_pad_flip(_dev(src), buf[off:off + n].view(out_shape), lo, 5, 0.1)
        got = buf.cpu().numpy()
        assert got[off:off + n].tobytes() == want.tobytes(), off
        assert np.all(got[:off] == 7.0) and np.all(got[off + n:] == 7.0), off


@pytest.mark.parametrize("C", [1, 3])
def test_tile_finalize_flip_into_a_slot_bit_for_bit(ops, C):
    import torch
    rs = np.random.RandomState(C)
    ashape, shape, lo = (9, 7, 6), (5, 7, 3), (2, 0, 1)
    acc = rs.randn(*ashape, C)
    cnt = rs.randint(1, 9, ashape).astype(np.int32)
    cnt[2, 0, 1] = 0                                          # two zero counts inside the window [2, 7) x [0, 7) x [1, 4) ...
    cnt[6, 6, 3] = 0
    cnt[0, 0, 0] = 0                                          # ... and one outside
    d_acc, d_cnt = _dev(acc), _dev(cnt)
    for mask in range(8):
        stack = torch.full((3,) + shape + (C,), -9.0, dtype=torch.float64, device="cuda")
        bad = torch.zeros(1, dtype=torch.int32, device="cuda")
        ops.tile_finalize_flip(d_acc, d_cnt, stack[1], bad, lo, mask)
        want, n_bad = R.tile_finalize_flip(acc, cnt, shape, lo, mask)
        got = stack.cpu().numpy()
        assert n_bad == 2 and int(bad.item()) == 2, mask
        assert got[1].tobytes() == want.tobytes(), mask
        assert np.all(got[0] == -9.0) and np.all(got[2] == -9.0), mask


@pytest.mark.parametrize("C", [1, 3])
def test_tile_finalize_flip_plain_is_tile_finalize(ops, C):
    import torch
    rs = np.random.RandomState(7 + C)
    ashape = (33, 17, 9)
    acc = _dev(rs.randn(*ashape, C))
    cnt = rs.randint(0, 9, ashape).astype(np.int32)
    want, got = torch.empty_like(acc), torch.empty_like(acc)
    bad_w, bad_g = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    ops.tile_finalize(acc, _dev(cnt), want, bad_w)
    ops.tile_finalize_flip(acc, _dev(cnt), got, bad_g, (0, 0, 0), 0)
    assert got.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()
    assert int(bad_g.item()) == int(bad_w.item()) == int((cnt == 0).sum()) > 0


def test_refusals_leave_the_output_untouched(ops):
    import torch
    from fmri_hip._lib import F32, F64, lib
    L = lib()
    E_SHAPE, E_ALIGN, E_DTYPE = -1, -2, -5
    s = torch.cuda.current_stream().cuda_stream
    src = torch.zeros((4, 4, 4), dtype=torch.float64, device="cuda")
    dst = torch.full((4, 4, 4), 7.0, dtype=torch.float32, device="cuda")
    lo = (ctypes.c_int32 * 3)(0, 0, 0)
    a, d = src.data_ptr(), dst.data_ptr()
    pad = L.fmri_volume_pad_flip
    assert pad(0, F64, 4, 4, 4, d, F32, 4, 4, 4, lo, 0, 0.0, s) == E_SHAPE
    assert pad(a, F64, 4, 4, 4, 0, F32, 4, 4, 4, lo, 0, 0.0, s) == E_SHAPE
    assert pad(a, F64, 4, 4, 4, d, F32, 4, 4, 4, None, 0, 0.0, s) == E_SHAPE
    assert pad(a, F64, 4, 4, 0, d, F32, 4, 4, 4, lo, 0, 0.0, s) == E_SHAPE
    assert pad(a, F64, 4, 4, 4, d, F32, -4, 4, 4, lo, 0, 0.0, s) == E_SHAPE
    assert pad(a, F64, 4, 4, 4, d, F32, 4, 4, 4, lo, 8, 0.0, s) == E_SHAPE
    assert pad(a, 1, 4, 4, 4, d, F32, 4, 4, 4, lo, 0, 0.0, s) == E_DTYPE
    assert pad(a, F64, 4, 4, 4, d, 2, 4, 4, 4, lo, 0, 0.0, s) == E_DTYPE
    assert pad(a, F64, 4, 4, 4, d + 2, F32, 4, 4, 3, lo, 0, 0.0, s) == E_ALIGN
    with pytest.raises(TypeError):
        ops.volume_pad_flip(src, dst.to(torch.bfloat16), (0, 0, 0), 0, 0.0)
    acc = torch.ones((4, 4, 4, 1), dtype=torch.float64, device="cuda")
    cnt = torch.ones((4, 4, 4), dtype=torch.int32, device="cuda")
    out = torch.full((2, 2, 2, 1), 7.0, dtype=torch.float64, device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    fin = L.fmri_tile_finalize_flip
    A, c, o, b = acc.data_ptr(), cnt.data_ptr(), out.data_ptr(), bad.data_ptr()
    assert fin(0, c, 4, 4, 4, 1, o, 2, 2, 2, lo, 0, b, s) == E_SHAPE
    assert fin(A, 0, 4, 4, 4, 1, o, 2, 2, 2, lo, 0, b, s) == E_SHAPE
    assert fin(A, c, 4, 4, 4, 1, 0, 2, 2, 2, lo, 0, b, s) == E_SHAPE
    assert fin(A, c, 4, 4, 4, 1, o, 2, 2, 2, lo, 0, 0, s) == E_SHAPE
    assert fin(A, c, 4, 4, 4, 1, o, 2, 2, 2, None, 0, b, s) == E_SHAPE
    assert fin(A, c, 4, 4, 4, 0, o, 2, 2, 2, lo, 0, b, s) == E_SHAPE
    assert fin(A, c, 4, 0, 4, 1, o, 2, 2, 2, lo, 0, b, s) == E_SHAPE
    assert fin(A, c, 4, 4, 4, 1, o, 2, 2, 0, lo, 0, b, s) == E_SHAPE
    assert fin(A, c, 4, 4, 4, 1, o, 2, 2, 2, (ctypes.c_int32 * 3)(0, 3, 0), 0, b, s) == E_SHAPE     # reads past acc
    assert fin(A, c, 4, 4, 4, 1, o, 2, 2, 2, (ctypes.c_int32 * 3)(0, 0, -1), 0, b, s) == E_SHAPE    # reads in front of acc
    assert fin(A, c, 4, 4, 4, 1, o, 2, 2, 2, lo, 8, b, s) == E_SHAPE
    assert fin(A, c, 4, 4, 4, 1, o + 4, 2, 2, 1, lo, 0, b, s) == E_ALIGN
    torch.cuda.synchronize()
    assert bool((dst == 7.0).all()) and bool((out == 7.0).all()) and int(bad.item()) == 0


def test_both_kernels_past_two_to_the_31_elements(ops):
    """the 64-bit index forms: a destination / an accumulator of more than 2^31 elements, the data at its far end"""
    import torch
    g = torch.Generator(device="cuda").manual_seed(3)
    src = torch.randn((64, 1024, 1024), generator=g, device="cuda")
    dst = torch.empty((2049, 1024, 1024), dtype=torch.float32, device="cuda")
    assert dst.numel() > 2 ** 31
    ops.volume_pad_flip(src, dst, (1984, 0, 0), 7, -3.0)
    assert torch.equal(dst[1984:2048], src.flip(0, 1, 2))
    assert bool((dst[:1984] == -3.0).all()) and bool((dst[2048:] == -3.0).all())
    del dst
    acc = torch.empty((2049, 1024, 1024, 1), dtype=torch.float64, device="cuda")
    cnt = torch.empty((2049, 1024, 1024), dtype=torch.int32, device="cuda")
    acc[1985:2049, :, :, 0] = src.double()
    cnt[1985:2049] = 4
    out = torch.empty((64, 1024, 1024, 1), dtype=torch.float64, device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    ops.tile_finalize_flip(acc, cnt, out, bad, (1985, 0, 0), 7)
    assert torch.equal(out[..., 0], src.double().flip(0, 1, 2) / 4.0) and int(bad.item()) == 0


# --------------------------------------------------------------------------------------------------------------------------- flows
def _cfg(patch):
    return {"patch_shape": list(patch[:2]), "patch_depth": patch[2]}


def _max_diff(name, got, want):
    d = float(np.abs(np.asarray(got) - np.asarray(want)).max())
    print("route difference %-44s max %.3e" % (name, d))
    return d


@pytest.fixture(scope="module")
def net3d():
    import os
    os.environ["FMRI_DTYPE"] = "bf16"
    import fetal_net.model as fmodel
    patch = (16, 32, 32)
    return fmodel.unet_model_3d(input_shape=(1,) + patch, depth=3, n_base_filters=32), patch


@pytest.fixture(scope="module")
def host_flips(net3d):
    """the kept host route's eight variants of the two 3-D volumes, computed once"""
    from fetal_net import prediction as P
    model, patch = net3d
    out = {}
    for shape in ((24, 48, 40), (24, 27, 40)):                # (24, 27, 40): an odd deficit in y, pad_for_fit (3, 2)
        vol = np.random.RandomState(21).randn(1, *shape)
        out[shape] = (vol, P._predict_flips_host(vol, model, 0.5, _cfg(patch)))
    return out


@pytest.mark.parametrize("shape", [(24, 48, 40), (24, 27, 40)])
def test_predict_flips_3d_resident_equals_host_route(net3d, host_flips, shape):
    import torch
    from fetal_net import prediction as P
    model, patch = net3d
    vol, want = host_flips[shape]
    if shape == (24, 27, 40):
        assert P._geometry_of_shape(model, shape, patch, 0.5)[2][1] == (3, 2)
    got = P.predict_flips(vol, model, 0.5, _cfg(patch))
    assert len(got) == len(want) == 8 and all(isinstance(g, np.ndarray) for g in got)
    worst = 0.0
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape == shape and a.dtype == np.float64
        worst = max(worst, _max_diff("predict_flips 3-D %s variant %d" % (shape, k), a, b))
        np.testing.assert_allclose(a, b, rtol=0, atol=ROUTE_ATOL)
    assert float(np.abs(got[0] - got[7]).max()) > 1e-4        # the flips are real variants, not eight copies
    # tensor in: tensors on the same device, views of one stack
    t = torch.from_numpy(vol).cuda()
    dev = P.predict_flips(t, model, 0.5, _cfg(patch))
    assert len(dev) == 8 and all(torch.is_tensor(d) and d.device == t.device and d.dtype == torch.float64 for d in dev)
    assert len({d.untyped_storage().data_ptr() for d in dev}) == 1 and dev[1].data_ptr() == dev[0].data_ptr() + 8 * int(np.prod(shape))
    for d, b in zip(dev, want):
        np.testing.assert_allclose(d.cpu().numpy(), b, rtol=0, atol=ROUTE_ATOL)


def test_patch_wise_prediction_tensor_in_tensor_out(net3d, host_flips):
    import torch
    from fetal_net import prediction as P
    model, patch = net3d
    vol, want = host_flips[(24, 27, 40)]
    got = P.patch_wise_prediction(model, torch.from_numpy(vol).cuda(), patch, overlap_factor=0.5)
    assert torch.is_tensor(got) and got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (24, 27, 40, 1)
    _max_diff("patch_wise_prediction tensor", got.cpu().numpy()[..., 0], want[0])
    np.testing.assert_allclose(got.cpu().numpy()[..., 0], want[0], rtol=0, atol=ROUTE_ATOL)


def test_predict_flips_2d_asymmetric_slice_padding():
    """an even slice count: pad0 is the asymmetric (2, 1) in z"""
    import fetal_net.model as fmodel
    from fetal_net import prediction as P
    patch = (32, 32, 4)
    model = fmodel.unet_model_2d(input_shape=patch, depth=3, n_base_filters=8, compute_dtype="fp32")
    assert P._geometry_of_shape(model, (40, 48, 12), patch, 0.5)[1][2] == (2, 1)
    vol = np.random.RandomState(2).randn(40, 48, 12) * 50 + 100
    want = P._predict_flips_host(vol, model, 0.5, _cfg(patch))
    got = P.predict_flips(vol, model, 0.5, _cfg(patch))
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape == vol.shape
        _max_diff("predict_flips 2-D variant %d" % k, a, b)
        np.testing.assert_allclose(a, b, rtol=0, atol=ROUTE_ATOL)
    assert float(np.abs(got[0] - got[7]).max()) > 1e-4


def test_three_labels_2d_stack_and_median_per_channel():
    import torch
    import fetal_net.model as fmodel
    from fetal_net import prediction as P
    from fetal_net.pipeline import Stage
    patch = (32, 32, 5)
    model = fmodel.unet_model_2d(input_shape=patch, depth=2, n_base_filters=8, n_labels=3)
    vol = np.random.RandomState(6).randn(40, 27, 9) * 50 + 100       # both paddings: pad0 (2, 2) in z, pad_for_fit (3, 2) in y
    want = np.stack(P._predict_flips_host(vol, model, 0.5, _cfg(patch)))
    assert want.shape == (8, 40, 27, 9, 3)
    dev = P.predict_flips(torch.from_numpy(vol).cuda(), model, 0.5, _cfg(patch))
    assert all(tuple(d.shape) == (40, 27, 9, 3) for d in dev) and len({d.untyped_storage().data_ptr() for d in dev}) == 1
    got = np.stack([d.cpu().numpy() for d in dev])
    _max_diff("predict_flips 2-D three labels", got, want)
    np.testing.assert_allclose(got, want, rtol=0, atol=ROUTE_ATOL)
    med = Stage(model, _cfg(patch), augment="flip", overlap=0.5).infer(vol)
    _max_diff("Stage.infer median, three labels", med, np.median(want, axis=0))
    np.testing.assert_allclose(med, np.median(want, axis=0), rtol=0, atol=MEDIAN_ATOL)


def test_stage_infer_flip_resident(net3d, host_flips):
    import torch
    from fetal_net.pipeline import Stage
    model, patch = net3d
    from fetal_net import prediction as P
    vol = host_flips[(24, 27, 40)][0][0]                      # (X, Y, Z): the flips then mirror the spatial axes both ways
    want = np.stack(P._predict_flips_host(vol, model, 0.5, _cfg(patch)))
    stage = Stage(model, _cfg(patch), augment="flip", overlap=0.5)
    assert stage._resident_refusal(vol) is None
    got = stage.infer(vol)
    assert isinstance(got, np.ndarray) and got.shape == vol.shape
    _max_diff("Stage.infer median", got, np.median(want, axis=0))
    np.testing.assert_allclose(got, np.median(want, axis=0), rtol=0, atol=MEDIAN_ATOL)
    np.testing.assert_allclose(stage._infer_host(vol), np.median(want, axis=0), rtol=0, atol=MEDIAN_ATOL)
    kept = stage.infer(vol, keep_variants=True)
    assert kept.shape == want.shape
    _max_diff("Stage.infer keep_variants", kept, want)
    np.testing.assert_allclose(kept, want, rtol=0, atol=ROUTE_ATOL)
    t = torch.from_numpy(vol).cuda()
    dev = stage.infer(t)
    assert torch.is_tensor(dev) and dev.device == t.device and dev.dtype == torch.float64
    np.testing.assert_allclose(dev.cpu().numpy(), np.median(want, axis=0), rtol=0, atol=MEDIAN_ATOL)
    plain = Stage(model, _cfg(patch), overlap=0.5).infer(vol)
    _max_diff("Stage.infer without augmentation", plain, want[0])
    np.testing.assert_allclose(plain, want[0], rtol=0, atol=ROUTE_ATOL)


def test_predict_volume_device_chain_equals_host_chain(net3d):
    """resolution zoom, border, flips, median, crop and zoom back on one tensor against device=False.  The two arms also differ in their
    zooms (kernel against scipy, 1e-12 * max(1, |want|) by tests/test_gpu_resample.py), so the prediction keeps the tile-loop bar of
    tests/test_gpu_tta.py, 1e-6, which the zoom's own bar is far below.  Measured on the MI355X: prediction 2.2e-16, data 6.3e-13."""
    from scipy import ndimage
    from fetal_net import pipeline
    model, patch = net3d
    vol = ndimage.gaussian_filter(np.random.RandomState(9).randn(40, 64, 48), 2.0) * 400 + 300
    dev = pipeline.predict_volume(vol, model, _cfg(patch), overlap_factor=0.5, xy_scale=0.5, augment="flip")
    host = pipeline.predict_volume(vol, model, _cfg(patch), overlap_factor=0.5, xy_scale=0.5, augment="flip", device=False)
    assert set(dev) == set(host) == {"data", "prediction"}
    for key in ("data", "prediction"):
        assert isinstance(dev[key], np.ndarray) and dev[key].shape == host[key].shape and dev[key].dtype == host[key].dtype
    assert dev["prediction"].shape == vol.shape
    _max_diff("predict_volume data", dev["data"], host["data"])
    _max_diff("predict_volume prediction", dev["prediction"], host["prediction"])
    assert np.all(np.abs(dev["data"] - host["data"]) <= 1e-12 * np.maximum(1.0, np.abs(host["data"])))
    np.testing.assert_allclose(dev["prediction"], host["prediction"], rtol=0, atol=1e-6)


def test_cache_and_fallback(net3d, host_flips):
    import torch
    from fetal_net import prediction as P
    model, patch = net3d
    vol, want = host_flips[(24, 48, 40)]
    before = P.patch_wise_prediction(model, vol, patch, overlap_factor=0.5)
    state = model.__dict__["_tile_state"]
    graphs = {B: pb["graph"] for B, pb in state["per_b"].items()}
    P.predict_flips(vol, model, 0.5, _cfg(patch))
    other = np.random.RandomState(22).randn(*vol.shape)       # a second flip call, another volume of the same shape
    got = P.predict_flips(other, model, 0.5, _cfg(patch))
    for a, b in zip(got, P._predict_flips_host(other, model, 0.5, _cfg(patch))):
        _max_diff("predict_flips, second volume", a, b)
        np.testing.assert_allclose(a, b, rtol=0, atol=ROUTE_ATOL)
    after = P.patch_wise_prediction(model, vol, patch, overlap_factor=0.5)
    np.testing.assert_array_equal(before, after)
    assert model.__dict__["_tile_state"] is state and {B: pb["graph"] for B, pb in state["per_b"].items()} == graphs

    class Foreign(object):                                    # the same network behind the reference's duck type
        output_shape = (None, 1) + patch

        def predict(self, x):
            return model.predict(np.asarray(x))

    small = vol[:, :16, :32, :32]
    got = P.predict_flips(small, Foreign(), 0.5, _cfg(patch))
    assert len(got) == 8 and all(isinstance(g, np.ndarray) and g.shape == (16, 32, 32) for g in got)
    with pytest.raises(TypeError, match="engine Model"):
        P.predict_flips(torch.from_numpy(small).cuda(), Foreign(), 0.5, _cfg(patch))
    with pytest.raises(TypeError, match="truth_data"):
        P.patch_wise_prediction(model, torch.from_numpy(vol).cuda(), patch, overlap_factor=0.5, truth_data=vol)
