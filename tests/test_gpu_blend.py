"""Gaussian-importance blending of the sliding-window tiles on the device.

Kernels: fmri_tile_scatter_weighted, fmri_tile_finalize_weighted, fmri_tile_finalize_flip_weighted and fmri_tile_finalize_labels_weighted
against the float64 restatements of tests/blend_restatement.py.  A voxel that one tile covers holds 0 + w * p (or start + w * p): one
rounding whatever the order, compared bit for bit.  Where n tiles meet, the kernel's atomic adds and the restatement's loop add the same n
terms in possibly different orders; the bound n * 2^-53 * sum(|terms|) per voxel is computed from the terms, not measured.  The three
finalize kernels divide once per element (IEEE division is exactly rounded) and compare exactly: bit for bit.

Flows: `blend="gaussian"` through the device tile loop.  With FMRI_HIPGRAPH=0 the test records the network output and the corners of every
fmri_tile_scatter_weighted call and feeds the recordings to the restatement, so that comparison holds no network tolerance.  Bar of every
flow comparison: the means are below 1 and are quotients of two float64 sums of at most n_cover terms, each within (n_cover - 1) * 2^-53
relative of its exact value, the quotient rounding once more: (2 * n_cover - 1) * 2^-53 < n_cover * 2^-52 (the derivation on top of
tests/test_gpu_tta_resident.py, with the largest cover of the geometry computed by `_cover_max`)."""
import ctypes
import os

import numpy as np
import pytest

import blend_restatement as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from fmri_hip import ops as o
    return o


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _tabs(tile, sigma=0.125):
    from fetal_net.prediction import gaussian_tile_tables
    tabs = gaussian_tile_tables(tile, sigma)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(tabs, R.tables(tile, sigma)))
    return tabs


# ------------------------------------------------------------------------------------------------------------------- scatter kernel
#            name                   tile        volume        corners                                                channels
SCATTER = [("a-disjoint", (5, 6, 7), (12, 6, 7), [(0, 0, 0), (7, 0, 0)], (1, 3)),
           ("b-overlapping", (5, 6, 7), (9, 10, 11), [(0, 0, 0), (2, 3, 1), (4, 4, 4)], (1, 3)),
           ("c-hanging-out", (5, 6, 7), (9, 10, 11), [(-2, 0, 0), (6, 7, 8)], (1, 3)),
           ("d-2d-form", (5, 6, 1), (9, 10, 3), [(0, 0, 0), (2, 3, 0), (4, 4, 0), (4, 4, 2)], (3,)),
           ("e-several-workgroups", (9, 7, 5), (14, 11, 9), [(0, 0, 0), (5, 4, 4), (3, 2, 1), (5, 0, 4)], (1, 3))]


def _scatter_case(ops, tile, vol, corners, C, seed, start):
    """-> (got acc, got wsum, restatement's (acc, wsum, mag, wmag, cover))"""
    rs = np.random.RandomState(seed)
    B = len(corners)
    pred = rs.randn(B, *tile, C).astype(np.float32)
    idx = np.asarray(corners, dtype=np.int32)
    tabs = _tabs(tile)
    acc0 = rs.randn(*vol, C) if start else np.zeros(vol + (C,))
    wsum0 = rs.rand(*vol) + 0.5 if start else np.zeros(vol)
    acc, wsum = _dev(acc0), _dev(wsum0)
    ops.tile_scatter_weighted(_dev(pred), _dev(idx), tile, tuple(_dev(t) for t in tabs), acc, wsum)
    return acc.cpu().numpy(), wsum.cpu().numpy(), R.tile_scatter_weighted(pred, idx, tabs, acc0, wsum0)


@pytest.mark.parametrize("name,tile,vol,corners,channels", SCATTER, ids=[c[0] for c in SCATTER])
def test_tile_scatter_weighted_against_the_restatement(ops, name, tile, vol, corners, channels):
    for C in channels:
        acc, wsum, (w_acc, w_wsum, mag, wmag, cover) = _scatter_case(ops, tile, vol, corners, C, 7 * C + len(name), False)
        once = cover <= 1
        assert acc[once].tobytes() == w_acc[once].tobytes() and wsum[once].tobytes() == w_wsum[once].tobytes(), (name, C)
        assert np.all(acc[cover == 0] == 0) and np.all(wsum[cover == 0] == 0)
        d_acc, d_w = np.abs(acc - w_acc), np.abs(wsum - w_wsum)
        print("%s C=%d: cover up to %d, max |acc - want| %.3e, max |wsum - want| %.3e" % (name, C, cover.max(), d_acc.max(), d_w.max()))
        assert np.all(d_acc <= (cover * 2.0 ** -53)[..., None] * mag), (name, C)
        assert np.all(d_w <= cover * 2.0 ** -53 * wmag), (name, C)
        if name.startswith(("a", "c")):
            assert int(cover.max()) == 1
        else:
            assert int(cover.max()) >= 2
        if name.startswith("c"):                              # the tiles hang out: fewer voxels land than the tiles hold
            assert 0 < int(cover.sum()) < len(corners) * int(np.prod(tile))


@pytest.mark.parametrize("C", [1, 3])
def test_tile_scatter_weighted_accumulates(ops, C):
    """acc and wsum start non-zero (case a: every voxel is covered at most once, start + w * p rounds once): accumulation, not assignment"""
    name, tile, vol, corners, _ = SCATTER[0]
    acc, wsum, (w_acc, w_wsum, _, _, cover) = _scatter_case(ops, tile, vol, corners, C, 40 + C, True)
    assert int(cover.max()) == 1 and int((cover == 0).sum()) > 0
    assert acc.tobytes() == w_acc.tobytes() and wsum.tobytes() == w_wsum.tobytes()
    assert np.all(wsum[cover == 1] > 0.5) and float(np.abs(acc).min()) > 0


# ------------------------------------------------------------------------------------------------------------------ finalize kernels
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("nvox", [1, 255, 257, 1031])
def test_tile_finalize_weighted_bit_for_bit(ops, nvox, C):
    import torch
    rs = np.random.RandomState(nvox + C)
    acc, wsum = rs.randn(nvox, C), rs.rand(nvox) * 3 + 1e-3
    wsum[nvox // 2] = 0.0                                     # one uncovered voxel: divides by 1, counted
    out = torch.full((nvox, C), -9.0, dtype=torch.float64, device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    ops.tile_finalize_weighted(_dev(acc), _dev(wsum), out, bad)
    want, n_bad = R.tile_finalize_weighted(acc, wsum)
    got = out.cpu().numpy()
    assert n_bad == 1 and int(bad.item()) == 1
    assert got.tobytes() == want.tobytes()
    assert got[nvox // 2].tobytes() == acc[nvox // 2].tobytes()
    ops.tile_finalize_weighted(_dev(acc), _dev(wsum), out, bad)          # bad accumulates
    assert int(bad.item()) == 2


@pytest.mark.parametrize("C", [1, 3])
def test_tile_finalize_flip_weighted_bit_for_bit(ops, C):
    import torch
    rs = np.random.RandomState(C)
    for ashape, shape, lo in (((9, 7, 6), (5, 7, 3), (2, 0, 1)), ((7, 8, 1), (4, 5, 1), (1, 2, 0))):          # the second: Z = 1
        acc = rs.randn(*ashape, C)
        wsum = rs.rand(*ashape) * 3 + 1e-3
        wsum[lo[0], lo[1], lo[2]] = 0.0                       # inside the window
        wsum[lo[0] + shape[0] - 1, lo[1] + shape[1] - 1, lo[2] + shape[2] - 1] = 0.0
        wsum[0, 0, 0] = 0.0                                   # outside (lo[0] > 0)
        d_acc, d_wsum = _dev(acc), _dev(wsum)
        for mask in range(8):
            stack = torch.full((3,) + shape + (C,), -9.0, dtype=torch.float64, device="cuda")
            bad = torch.zeros(1, dtype=torch.int32, device="cuda")
            ops.tile_finalize_flip_weighted(d_acc, d_wsum, stack[1], bad, lo, mask)
            want, n_bad = R.tile_finalize_flip_weighted(acc, wsum, shape, lo, mask)
            got = stack.cpu().numpy()
            assert n_bad == 2 and int(bad.item()) == 2, (ashape, mask)
            assert got[1].tobytes() == want.tobytes(), (ashape, mask)
            assert np.all(got[0] == -9.0) and np.all(got[2] == -9.0), (ashape, mask)


@pytest.mark.parametrize("C", [1, 3])
def test_tile_finalize_flip_weighted_at_every_store_width(ops, C):
    """an output 16-byte aligned takes the two-element store, one that starts 8 bytes into a line the single one; the elements around it stay"""
    import torch
    rs = np.random.RandomState(11 + C)
    ashape, shape, lo = (40, 20, 11), (33, 17, 9), (4, 1, 2)
    acc, wsum = rs.randn(*ashape, C), rs.rand(*ashape) + 0.25
    n = int(np.prod(shape)) * C
    want, _ = R.tile_finalize_flip_weighted(acc, wsum, shape, lo, 5)
    for off in (0, 1, 2, 3):
        buf = torch.full((n + 8,), 7.0, dtype=torch.float64, device="cuda")
        bad = torch.zeros(1, dtype=torch.int32, device="cuda")
        assert (buf.data_ptr() + 8 * off) % 16 == 8 * (off % 2)
        ops.tile_finalize_flip_weighted(_dev(acc), _dev(wsum), buf[off:off + n].view(shape + (C,)), bad, lo, 5)
        got = buf.cpu().numpy()
        assert got[off:off + n].tobytes() == want.tobytes(), off
        assert np.all(got[:off] == 7.0) and np.all(got[off + n:] == 7.0) and int(bad.item()) == 0, off


@pytest.mark.parametrize("C", [1, 3])
def test_tile_finalize_flip_weighted_plain_is_tile_finalize_weighted(ops, C):
    import torch
    rs = np.random.RandomState(7 + C)
    ashape = (33, 17, 9)
    acc = _dev(rs.randn(*ashape, C))
    wsum = rs.rand(*ashape)
    wsum[rs.rand(*ashape) < 0.1] = 0.0
    want, got = torch.empty_like(acc), torch.empty_like(acc)
    bad_w, bad_g = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    ops.tile_finalize_weighted(acc, _dev(wsum), want, bad_w)
    ops.tile_finalize_flip_weighted(acc, _dev(wsum), got, bad_g, (0, 0, 0), 0)
    assert got.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()
    assert int(bad_g.item()) == int(bad_w.item()) == int((wsum == 0).sum()) > 0


def test_tile_finalize_labels_weighted_rules(ops):
    """a tie between two channels goes to the first; a maximum EQUAL to the threshold is kept for C > 1 (only < threshold is background)
    and not kept for C == 1 (which needs > threshold); uncovered voxels give 0 and are counted"""
    import torch
    wsum = np.asarray([2.0, 2.0, 2.0, 2.0, 0.0, 4.0])
    acc2 = np.asarray([[1.5, 1.5], [1.0, 1.0], [0.5, 1.5], [0.25, 0.5], [9.0, 9.0], [3.0, 1.0]])
    #  q              .75 .75     .5 .5      .25 .75     .125 .25    uncovered   .75 .25          threshold 0.5
    want2 = np.asarray([3, 3, 7, 0, 0, 3], dtype=np.uint8)
    out = torch.full((6,), 99, dtype=torch.uint8, device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    ops.tile_finalize_labels_weighted(_dev(acc2), _dev(wsum), out, bad, 0.5, (3, 7))
    assert out.cpu().numpy().tolist() == want2.tolist() and int(bad.item()) == 1
    assert R.tile_finalize_labels_weighted(acc2, wsum, 0.5, (3, 7))[0].tolist() == want2.tolist()
    acc1 = np.asarray([[1.5], [1.0], [1.0000000000000002], [0.25], [9.0], [3.0]])
    want1 = np.asarray([7, 0, 7, 0, 0, 7], dtype=np.uint8)   # q = .75, .5 (equal: not kept), the next float64 above .5, .125, uncovered, .75
    out.fill_(99)
    ops.tile_finalize_labels_weighted(_dev(acc1), _dev(wsum), out, bad, 0.5, (7,))
    assert out.cpu().numpy().tolist() == want1.tolist() and int(bad.item()) == 2          # accumulated
    assert R.tile_finalize_labels_weighted(acc1, wsum, 0.5, (7,))[0].tolist() == want1.tolist()


@pytest.mark.parametrize("C,values", [(1, (7,)), (2, (3, 7)), (3, (3, 7, 9))])
def test_tile_finalize_labels_weighted_against_the_restatement(ops, C, values):
    import torch
    rs = np.random.RandomState(C)
    nvox = 1031
    wsum = rs.rand(nvox) * 3 + 1e-3
    acc = rs.rand(nvox, C) * wsum[:, None]
    acc[::7, -1] = acc[::7, 0]                                # ties
    wsum[5] = 0.0
    out = torch.full((nvox,), 99, dtype=torch.uint8, device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    ops.tile_finalize_labels_weighted(_dev(acc), _dev(wsum), out, bad, 0.5, values)
    want, n_bad = R.tile_finalize_labels_weighted(acc, wsum, 0.5, values)
    assert n_bad == 1 and int(bad.item()) == 1 and out.cpu().numpy().tobytes() == want.tobytes()
    assert set(np.unique(want).tolist()) == {0} | set(values)


# ------------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_outputs_untouched(ops):
    """only NULL and misaligned pointers are passed: both are rejected on the host before any launch"""
    import torch
    from fmri_hip._lib import lib
    L = lib()
    E_SHAPE, E_ALIGN = -1, -2
    s = torch.cuda.current_stream().cuda_stream
    tile, vol = (3, 3, 3), (4, 4, 4)
    pred = torch.ones((2,) + tile + (1,), dtype=torch.float32, device="cuda")
    idx = torch.zeros((2, 3), dtype=torch.int32, device="cuda")
    g = torch.ones(3, dtype=torch.float32, device="cuda")
    acc = torch.full(vol + (1,), 7.0, dtype=torch.float64, device="cuda")
    wsum = torch.full(vol, 7.0, dtype=torch.float64, device="cuda")
    out = torch.full((2, 2, 2, 1), 7.0, dtype=torch.float64, device="cuda")
    lab = torch.full((64,), 7, dtype=torch.uint8, device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    P_, I_, G_, A_, W_, O_, L_, B_ = (t.data_ptr() for t in (pred, idx, g, acc, wsum, out, lab, bad))
    lo = (ctypes.c_int32 * 3)(0, 0, 0)
    vals = (ctypes.c_uint8 * 1)(1)

    good = [P_, I_, 2, 3, 3, 3, 1, G_, G_, G_, A_, W_, 4, 4, 4, s]
    for k in (0, 1, 7, 8, 9, 10, 11):                         # NULL for each pointer
        args = list(good)
        args[k] = 0
        assert L.fmri_tile_scatter_weighted(*args) == E_SHAPE, k
    for k in (2, 3, 4, 5, 6, 12, 13, 14):                     # zero extents
        args = list(good)
        args[k] = 0
        assert L.fmri_tile_scatter_weighted(*args) == E_SHAPE, k
    args = list(good)
    args[10] += 4                                             # a misaligned acc
    assert L.fmri_tile_scatter_weighted(*args) == E_ALIGN

    fin = L.fmri_tile_finalize_weighted
    assert fin(0, W_, O_, B_, 8, 1, s) == E_SHAPE and fin(A_, 0, O_, B_, 8, 1, s) == E_SHAPE
    assert fin(A_, W_, 0, B_, 8, 1, s) == E_SHAPE and fin(A_, W_, O_, 0, 8, 1, s) == E_SHAPE
    assert fin(A_, W_, O_, B_, 0, 1, s) == E_SHAPE and fin(A_, W_, O_, B_, 8, 0, s) == E_SHAPE
    assert fin(A_ + 4, W_, O_, B_, 8, 1, s) == E_ALIGN

    flip = L.fmri_tile_finalize_flip_weighted
    assert flip(0, W_, 4, 4, 4, 1, O_, 2, 2, 2, lo, 0, B_, s) == E_SHAPE
    assert flip(A_, 0, 4, 4, 4, 1, O_, 2, 2, 2, lo, 0, B_, s) == E_SHAPE
    assert flip(A_, W_, 4, 4, 4, 1, 0, 2, 2, 2, lo, 0, B_, s) == E_SHAPE
    assert flip(A_, W_, 4, 4, 4, 1, O_, 2, 2, 2, None, 0, B_, s) == E_SHAPE
    assert flip(A_, W_, 4, 4, 4, 1, O_, 2, 2, 2, lo, 0, 0, s) == E_SHAPE
    assert flip(A_, W_, 4, 0, 4, 1, O_, 2, 2, 2, lo, 0, B_, s) == E_SHAPE
    assert flip(A_, W_, 4, 4, 4, 0, O_, 2, 2, 2, lo, 0, B_, s) == E_SHAPE
    assert flip(A_, W_, 4, 4, 4, 1, O_, 2, 2, 0, lo, 0, B_, s) == E_SHAPE
    assert flip(A_, W_, 4, 4, 4, 1, O_, 2, 2, 2, (ctypes.c_int32 * 3)(0, 3, 0), 0, B_, s) == E_SHAPE      # reads past acc
    assert flip(A_, W_, 4, 4, 4, 1, O_, 2, 2, 2, (ctypes.c_int32 * 3)(0, 0, -1), 0, B_, s) == E_SHAPE     # reads in front of acc
    assert flip(A_, W_, 4, 4, 4, 1, O_, 2, 2, 2, lo, 8, B_, s) == E_SHAPE
    assert flip(A_ + 4, W_, 4, 4, 4, 1, O_, 2, 2, 2, lo, 0, B_, s) == E_ALIGN

    labels = L.fmri_tile_finalize_labels_weighted
    assert labels(0, W_, L_, B_, 64, 1, 0.5, vals, s) == E_SHAPE and labels(A_, 0, L_, B_, 64, 1, 0.5, vals, s) == E_SHAPE
    assert labels(A_, W_, 0, B_, 64, 1, 0.5, vals, s) == E_SHAPE and labels(A_, W_, L_, 0, 64, 1, 0.5, vals, s) == E_SHAPE
    assert labels(A_, W_, L_, B_, 0, 1, 0.5, vals, s) == E_SHAPE and labels(A_, W_, L_, B_, 64, 0, 0.5, vals, s) == E_SHAPE
    assert labels(A_, W_, L_, B_, 64, 1, 0.5, None, s) == E_SHAPE
    assert labels(A_ + 4, W_, L_, B_, 64, 1, 0.5, vals, s) == E_ALIGN
    with pytest.raises(ValueError):
        ops.tile_scatter_weighted(pred, idx, tile, (g, g, g[:2]), acc, wsum)
    with pytest.raises(TypeError):
        ops.tile_finalize_weighted(acc, wsum.float(), acc.clone(), bad)
    torch.cuda.synchronize()
    assert bool((acc == 7.0).all()) and bool((wsum == 7.0).all()) and bool((out == 7.0).all()) and bool((lab == 7).all())
    assert int(bad.item()) == 0


# ------------------------------------------------------------------------------------------------------------------------ footprint
@pytest.mark.parametrize("case", [2, 4], ids=["c-hanging-out", "e-several-workgroups"])
def test_footprint_of_the_four_entry_points(ops, case):
    """guard bands around acc, wsum, out and bad (tests/footprint.py): the tiles that hang out of the volume write nothing outside it, the
    last workgroup of an odd-sized launch stays inside.  Where tiles overlap, the sums of the two runs may differ in their last bits
    (atomics): they are `loose` and compared with the restatement under the bound of the scatter test."""
    import torch
    from footprint import audit
    name, tile, vol, corners, _ = SCATTER[case]
    C = 3
    rs = np.random.RandomState(case)
    pred0 = rs.randn(len(corners), *tile, C).astype(np.float32)
    idx0 = np.asarray(corners, dtype=np.int32)
    tabs = _tabs(tile)
    acc_in, wsum_in = rs.randn(*vol, C), rs.rand(*vol) + 0.25
    wsum_in[1, 2, 3] = 0.0
    window, lo = tuple(v - 2 for v in vol), (1, 0, 2)

    def run(a):
        pred, idx = a.input(_dev(pred0), name="pred"), a.input(_dev(idx0), name="corners")
        gx, gy, gz = (a.input(_dev(t), name="table_%d" % k) for k, t in enumerate(tabs))
        acc = a.accumulate(torch.zeros(vol + (C,), dtype=torch.float64, device="cuda"), name="acc")
        wsum = a.accumulate(torch.zeros(vol, dtype=torch.float64, device="cuda"), name="wsum")
        ops.tile_scatter_weighted(pred, idx, tile, (gx, gy, gz), acc, wsum)
        acc2, wsum2 = a.input(_dev(acc_in), name="acc_in"), a.input(_dev(wsum_in), name="wsum_in")
        out = a.output(vol + (C,), torch.float64, name="mean")
        bad = a.accumulate(torch.zeros(1, dtype=torch.int32, device="cuda"), name="bad")
        ops.tile_finalize_weighted(acc2, wsum2, out, bad)
        out_w = a.output(window + (C,), torch.float64, name="mean_window")
        bad_w = a.accumulate(torch.zeros(1, dtype=torch.int32, device="cuda"), name="bad_window")
        ops.tile_finalize_flip_weighted(acc2, wsum2, out_w, bad_w, lo, 5)
        labels = a.output(vol, torch.uint8, name="label_map")
        bad_l = a.accumulate(torch.zeros(1, dtype=torch.int32, device="cuda"), name="bad_labels")
        ops.tile_finalize_labels_weighted(acc2, wsum2, labels, bad_l, 0.1, [3, 1, 4])
        return {"acc": acc, "wsum": wsum, "mean": out, "bad": bad, "mean_window": out_w, "bad_window": bad_w, "label_map": labels,
                "bad_labels": bad_l}
    r0, r1 = audit(run, loose=("acc", "wsum") if case == 4 else ())
    w_acc, w_wsum, mag, wmag, cover = R.tile_scatter_weighted(pred0, idx0, tabs, np.zeros(vol + (C,)), np.zeros(vol))
    for r in (r0, r1):
        assert np.all(np.abs(r["acc"].cpu().numpy() - w_acc) <= (cover * 2.0 ** -53)[..., None] * mag)
        assert np.all(np.abs(r["wsum"].cpu().numpy() - w_wsum) <= cover * 2.0 ** -53 * wmag)
        assert int(r["bad"]) == 1 and int(r["bad_labels"]) == 1
    assert r0["mean"].cpu().numpy().tobytes() == R.tile_finalize_weighted(acc_in, wsum_in)[0].tobytes()
    assert r0["mean_window"].cpu().numpy().tobytes() == R.tile_finalize_flip_weighted(acc_in, wsum_in, window, lo, 5)[0].tobytes()
    assert r0["label_map"].cpu().numpy().tobytes() == R.tile_finalize_labels_weighted(acc_in, wsum_in, 0.1, [3, 1, 4])[0].tobytes()


# --------------------------------------------------------------------------------------------------------------------------- flows
def _cfg(patch):
    return {"patch_shape": list(patch[:2]), "patch_depth": patch[2]}


def _cover_max(model, shape, patch, overlap):
    """the largest number of output tiles on one voxel of the tiler's accumulator"""
    from fetal_net import prediction as P
    is3d, _, _, _, indices, data_shape = P._geometry_of_shape(model, shape, patch, overlap)
    tile = tuple(patch) if is3d else (patch[0], patch[1], 1)
    cover = np.zeros(tuple(int(s) for s in data_shape[:3]), dtype=np.int64)
    for x, y, z in indices:
        cover[x:x + tile[0], y:y + tile[1], z:z + tile[2]] += 1
    assert cover.min() >= 1
    return int(cover.max())


def _max_diff(name, got, want, bar):
    d = float(np.abs(np.asarray(got) - np.asarray(want)).max())
    print("blend difference %-52s max %.3e (bar %.3e)" % (name, d, bar))
    return d


@pytest.fixture(scope="module")
def net3d():
    os.environ["FMRI_DTYPE"] = "bf16"
    import fetal_net.model as fmodel
    patch = (16, 32, 32)
    return fmodel.unet_model_3d(input_shape=(1,) + patch, depth=3, n_base_filters=32), patch


SHAPES = [(24, 48, 40), (24, 27, 40)]                        # (24, 27, 40): an odd deficit in y, pad_for_fit (3, 2)


@pytest.fixture(scope="module")
def blended(net3d):
    """the host-fed device loop's blended means of the two volumes, graphs on, computed once: {shape: (volume, means, bar)}"""
    from fetal_net import prediction as P
    model, patch = net3d
    assert os.environ.get("FMRI_HIPGRAPH", "1") == "1"
    out = {}
    for shape in SHAPES:
        vol = np.random.RandomState(21).randn(1, *shape)
        out[shape] = (vol, P.patch_wise_prediction(model, vol, patch, overlap_factor=0.5, blend="gaussian"),
                      _cover_max(model, shape, patch, 0.5) * 2.0 ** -52)
    return out


@pytest.mark.parametrize("shape", SHAPES)
def test_flow_against_the_restatement(net3d, blended, shape, monkeypatch):
    from fetal_net import prediction as P
    from fmri_hip import ops
    model, patch = net3d
    vol, with_graphs, bar = blended[shape]
    is3d, pad0, fit, vshape, indices, data_shape = P._geometry_of_shape(model, shape, patch, 0.5)
    if shape == (24, 27, 40):
        assert fit[1] == (3, 2)
    calls = []
    real = ops.tile_scatter_weighted

    def recording(pred, idx, tile, tables, acc, wsum):
        calls.append((pred.detach().clone(), idx.detach().clone(), tuple(tile), [t.cpu().numpy() for t in tables]))
        return real(pred, idx, tile, tables, acc, wsum)

    monkeypatch.setenv("FMRI_HIPGRAPH", "0")
    monkeypatch.setattr(ops, "tile_scatter_weighted", recording)
    got = P.patch_wise_prediction(model, vol, patch, overlap_factor=0.5, blend="gaussian")
    monkeypatch.undo()
    assert calls and all(c[2] == patch for c in calls)
    for c in calls:
        assert all(a.tobytes() == b.tobytes() for a, b in zip(c[3], R.tables(patch)))          # the tables the kernel was handed
    preds = np.concatenate([c[0].float().cpu().numpy().reshape((-1,) + patch + (1,)) for c in calls])
    corners = np.concatenate([c[1].cpu().numpy() for c in calls])
    np.testing.assert_array_equal(corners, np.asarray(indices))
    assert float(preds.min()) >= 0.0 and float(preds.max()) <= 1.0               # sigmoid outputs: the means are below 1
    want, n_cover = R.blend_tiles(preds, corners, tuple(int(s) for s in data_shape))
    want = P._unpad(want, fit)
    assert n_cover * 2.0 ** -52 == bar and got.shape == shape + (1,)
    assert _max_diff("graphs off, against the restatement %s" % (shape,), got, want, bar) <= bar
    assert _max_diff("graphs on, against graphs off %s" % (shape,), with_graphs, got, bar) <= bar
    uniform = P.patch_wise_prediction(model, vol, patch, overlap_factor=0.5)
    assert float(np.abs(with_graphs - uniform).max()) > 1e-6                     # the feature is not a no-op


@pytest.mark.parametrize("shape", SHAPES)
def test_resident_loop_equals_the_host_fed_loop(net3d, blended, shape):
    import torch
    from fetal_net import prediction as P
    model, patch = net3d
    vol, want, bar = blended[shape]
    got = P.patch_wise_prediction(model, torch.from_numpy(vol).cuda(), patch, overlap_factor=0.5, blend="gaussian")
    assert torch.is_tensor(got) and got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == shape + (1,)
    assert _max_diff("tensor in, tensor out %s" % (shape,), got.cpu().numpy(), want, bar) <= bar


def test_predict_flips_on_both_routes(net3d, blended):
    from fetal_net import prediction as P
    model, patch = net3d
    shape = (24, 27, 40)
    vol, means, bar = blended[shape]
    host = P._predict_flips_host(vol, model, 0.5, _cfg(patch), "gaussian")
    got = P.predict_flips(vol, model, 0.5, _cfg(patch), blend="gaussian")
    assert len(got) == len(host) == 8
    for k, (a, b) in enumerate(zip(got, host)):
        assert a.shape == b.shape == shape
        assert _max_diff("predict_flips variant %d" % k, a, b, bar) <= bar
    assert _max_diff("predict_flips variant 0 against patch_wise_prediction", got[0], means[..., 0], bar) <= bar
    assert float(np.abs(got[0] - got[7]).max()) > 1e-4
    plain = P.predict_flips(vol, model, 0.5, _cfg(patch))
    assert float(np.abs(np.stack(got) - np.stack(plain)).max()) > 1e-6


def test_stage_infer_resident_against_host(net3d, blended):
    """np.median of 8 is the midpoint of the two middle values: it does not amplify a sup-norm difference, but each side rounds its own
    midpoint (a sum below 2, halved): 2^-53 more, as MEDIAN_ATOL of tests/test_gpu_tta_resident.py"""
    from fetal_net.pipeline import Stage
    model, patch = net3d
    shape = (24, 27, 40)
    vol, _, bar = blended[shape]
    stage = Stage(model, _cfg(patch), augment="flip", overlap=0.5, blend="gaussian")
    assert stage._resident_refusal(vol[0]) is None
    got, host = stage.infer(vol[0]), stage._infer_host(vol[0])
    assert got.shape == host.shape == shape
    assert _max_diff("Stage.infer median", got, host, bar + 2.0 ** -53) <= bar + 2.0 ** -53
    plain = Stage(model, _cfg(patch), augment="flip", overlap=0.5).infer(vol[0])
    assert float(np.abs(got - plain).max()) > 1e-6


def test_two_dimensional_model_with_three_labels():
    """the output tile is (px, py, 1) and C = 3: the weights are in-plane only"""
    import torch
    import fetal_net.model as fmodel
    from fetal_net import prediction as P
    patch = (32, 32, 5)
    model = fmodel.unet_model_2d(input_shape=patch, depth=2, n_base_filters=8, n_labels=3)
    shape = (40, 27, 9)                                       # both paddings: pad0 (2, 2) in z, pad_for_fit (3, 2) in y
    vol = np.random.RandomState(6).randn(1, *shape) * 50 + 100
    bar = _cover_max(model, shape, patch, 0.5) * 2.0 ** -52
    host_fed = P.patch_wise_prediction(model, vol, patch, overlap_factor=0.5, blend="gaussian")
    st = model.__dict__["_tile_state"]
    assert [int(t.numel()) for t in st["tables"]] == [32, 32, 1] and float(st["tables"][2][0]) == 1.0 and "cnt" not in st
    resident = P.patch_wise_prediction(model, torch.from_numpy(vol).cuda(), patch, overlap_factor=0.5, blend="gaussian")
    assert host_fed.shape == shape + (3,) and tuple(resident.shape) == shape + (3,)
    assert _max_diff("2-D, three labels: resident against host-fed", resident.cpu().numpy(), host_fed, bar) <= bar
    uniform = P.patch_wise_prediction(model, vol, patch, overlap_factor=0.5)
    assert float(np.abs(host_fed - uniform).max()) > 1e-6
    host = P._predict_flips_host(vol[0], model, 0.5, _cfg(patch), "gaussian")
    got = P.predict_flips(vol[0], model, 0.5, _cfg(patch), blend="gaussian")
    assert _max_diff("2-D, three labels: predict_flips", np.stack(got), np.stack(host), bar) <= bar


@pytest.mark.parametrize("is3d", [True, False], ids=["3d", "2d"])
def test_label_map_is_the_label_rule_of_the_blended_means(is3d, monkeypatch):
    from oracle import unet_oracle as O
    import fetal_net.model as fmodel
    from fetal_net.prediction import get_prediction_labels, patch_wise_label_map, patch_wise_prediction
    monkeypatch.setenv("FMRI_DTYPE", "fp32")
    if is3d:
        kw = dict(input_shape=(1, 16, 16, 8), depth=2, n_base_filters=8, n_labels=3)
        model, spec, patch = fmodel.unet_model_3d(**kw), O.Spec(**kw), (16, 16, 8)
    else:
        kw = dict(input_shape=(16, 16, 5), depth=2, n_base_filters=8, n_labels=3)
        model, spec, patch = fmodel.unet_model_2d(**kw), O.Spec(ndim=2, **kw), (16, 16, 5)
    W = spec.init_weights(13)
    last = spec.final["name"] + "/kernel"                   # wider logits: every label and the background occur in the map
    W[last] = W[last] * 8
    model.set_weights_dict(W)
    data = np.random.RandomState(6).randn(1, 20, 20, 12)
    labels = (4, 1, 9)
    pred = patch_wise_prediction(model=model, data=data, patch_shape=patch, overlap_factor=0.5, blend="gaussian")
    want = get_prediction_labels(np.moveaxis(pred, -1, 0)[np.newaxis], threshold=0.5, labels=labels)[0]
    got = patch_wise_label_map(model=model, data=data, patch_shape=patch, overlap_factor=0.5, threshold=0.5, labels=labels, blend="gaussian")
    assert got.shape == (20, 20, 12) and got.dtype == np.uint8
    assert got.tobytes() == np.ascontiguousarray(want, dtype=np.uint8).tobytes()
    assert set(np.unique(want).tolist()) == {0, 1, 4, 9}


def test_the_tile_state_is_keyed_on_blend(net3d, blended):
    from fetal_net import prediction as P
    model, patch = net3d
    shape = (24, 48, 40)
    vol, want, bar = blended[shape]
    plain_before = P.patch_wise_prediction(model, vol, patch, overlap_factor=0.5)
    st_plain = model.__dict__["_tile_state"]
    assert len(st_plain["key"]) == 7 and st_plain["key"][-2:] == (0, 0)       # the unweighted key is what it was before the keyword existed
    assert "cnt" in st_plain and "wsum" not in st_plain and "tables" not in st_plain
    again = P.patch_wise_prediction(model, vol, patch, overlap_factor=0.5, blend="gaussian")
    st_blend = model.__dict__["_tile_state"]
    assert st_blend is not st_plain and st_blend["key"][-1] == ("gaussian", 0.125) and st_blend["key"][:-1] == st_plain["key"]
    assert "wsum" in st_blend and "cnt" not in st_blend and len(st_blend["tables"]) == 3
    assert _max_diff("blended again after a plain call", again, want, bar) <= bar
    other = P.patch_wise_prediction(model, vol, patch, overlap_factor=0.5, blend="gaussian", blend_sigma_scale=0.25)
    assert model.__dict__["_tile_state"]["key"][-1] == ("gaussian", 0.25) and float(np.abs(other - again).max()) > 1e-6
    plain_after = P.patch_wise_prediction(model, vol, patch, overlap_factor=0.5)
    assert model.__dict__["_tile_state"]["key"] == st_plain["key"]
    assert plain_after.tobytes() == plain_before.tobytes()
    once_more = P.patch_wise_prediction(model, vol, patch, overlap_factor=0.5, blend="gaussian")
    assert _max_diff("blended once more", once_more, want, bar) <= bar
