"""The resident tile loop's host side (no GPU): the numpy restatements of fmri_volume_pad_flip / fmri_tile_finalize_flip are numpy's own
pad / flip / crop, the two entry points are declared, bound and exported, the geometry the resident loop tiles by is the host route's,
and without a device predict_flips and Stage.infer compute what they did before the resident route existed."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

import tta_resident_restatement as R
from conftest import ROOT

NEW = ("fmri_volume_pad_flip", "fmri_tile_finalize_flip")


def _np_pad_flip(src, out_shape, lo, mask, fill, dtype):
    """np.pad(np.flip(src, axes), ..., constant_values=fill), cut to out_shape starting lo voxels in front of the volume, then astype"""
    flipped = np.flip(src, axis=R.masks_axes(mask)) if mask else src
    before = [max(int(v), 0) for v in lo]
    start = [max(-int(v), 0) for v in lo]
    after = [max(0, s + o - b - n) for s, o, b, n in zip(start, out_shape, before, src.shape)]
    padded = np.pad(flipped, list(zip(before, after)), mode="constant", constant_values=fill)
    return padded[tuple(slice(s, s + o) for s, o in zip(start, out_shape))].astype(dtype)


@pytest.mark.parametrize("mask", range(8))
def test_pad_flip_restatement_is_numpys_pad_of_the_flipped_volume(mask):
    rs = np.random.RandomState(mask)
    for src_t, dst_t in ((np.float64, np.float32), (np.float32, np.float32), (np.float64, np.float64)):
        for fill in (-3.0, 0.1):
            for shape, lo, out_shape in (((1, 1, 1), (1, 0, 2), (3, 2, 4)), ((5, 7, 3), (2, 0, 1), (9, 7, 6)), ((5, 7, 3), (-1, -2, 0), (3, 4, 3)),
                                         ((4, 5, 1), (1, 2, 0), (7, 8, 1)), ((6, 4, 5), (3, -1, 2), (8, 2, 9))):
                src = (rs.randn(*shape) * 100).astype(src_t)
                got = R.volume_pad_flip(src, out_shape, lo, mask, fill, dst_t)
                want = _np_pad_flip(src, out_shape, lo, mask, fill, dst_t)
                assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (src_t, dst_t, fill, shape, lo)


@pytest.mark.parametrize("mask", range(8))
@pytest.mark.parametrize("C", [1, 3])
def test_finalize_flip_restatement_is_the_flipped_crop_of_the_means(mask, C):
    from fetal_net.prediction import _unpad, flip_it
    rs = np.random.RandomState(10 * mask + C)
    pads = [(2, 2), (0, 0), (1, 2)]                           # asymmetric in z, none in y
    shape = (5, 7, 3)
    ashape = tuple(n + p[0] + p[1] for n, p in zip(shape, pads))
    acc = rs.randn(*ashape, C)
    cnt = rs.randint(1, 9, ashape).astype(np.int32)
    got, bad = R.tile_finalize_flip(acc, cnt, shape, [p[0] for p in pads], mask)
    want = flip_it(_unpad(acc / cnt[..., None], pads), R.masks_axes(mask))
    assert bad == 0 and got.tobytes() == np.ascontiguousarray(want).tobytes()
    cnt[2, 0, 1] = 0                                          # inside the window
    cnt[6, 6, 2] = 0                                          # inside
    cnt[0, 0, 0] = 0                                          # outside
    got, bad = R.tile_finalize_flip(acc, cnt, shape, [p[0] for p in pads], mask)
    assert bad == 2 and got.tobytes() == np.ascontiguousarray(flip_it(_unpad(acc / np.maximum(cnt, 1)[..., None], pads), R.masks_axes(mask))).tobytes()


def test_header_binding_table_and_library_agree_on_the_new_entry_points():
    from fmri_hip._lib import LIB_PATH, SIGNATURES, F64, lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fmri_hip.h")).read(), flags=re.S)
    assert re.search(r"FMRI_F64\s*=\s*%d\b" % F64, src)
    for name in NEW:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, src)
        assert m, "%s is not declared in include/fmri_hip.h" % name
        params = [p.strip() for p in m.group(1).split(",")]
        assert name in SIGNATURES and len(SIGNATURES[name]) == len(params), name
        for param, ctype in zip(params, SIGNATURES[name]):
            want = ctypes.c_void_p if "*" in param or "fmri_stream_t" in param else ctypes.c_double if param.startswith("double") else ctypes.c_int
            assert ctype is want, (name, param, ctype)
    if not os.path.exists(LIB_PATH):
        import __graft_entry__ as g
        g.build()
    L = lib()
    for name in NEW:
        assert hasattr(L, name), name


def test_refusals_launch_nothing_and_need_no_device():
    """every refusal is decided on the host before anything is enqueued: the codes come back without a GPU"""
    from fmri_hip._lib import LIB_PATH, F32, F64, lib
    if not os.path.exists(LIB_PATH):
        import __graft_entry__ as g
        g.build()
    L = lib()
    E_SHAPE, E_ALIGN, E_DTYPE = -1, -2, -5
    lo = (ctypes.c_int32 * 3)(0, 0, 0)
    p, q = 4096, 8192                                         # never dereferenced
    pad = L.fmri_volume_pad_flip
    assert pad(0, F64, 2, 2, 2, q, F32, 2, 2, 2, lo, 0, 0.0, None) == E_SHAPE
    assert pad(p, F64, 2, 2, 2, 0, F32, 2, 2, 2, lo, 0, 0.0, None) == E_SHAPE
    assert pad(p, F64, 2, 2, 2, q, F32, 2, 2, 2, None, 0, 0.0, None) == E_SHAPE
    assert pad(p, F64, 2, 0, 2, q, F32, 2, 2, 2, lo, 0, 0.0, None) == E_SHAPE
    assert pad(p, F64, 2, 2, 2, q, F32, 2, 2, -1, lo, 0, 0.0, None) == E_SHAPE
    assert pad(p, F64, 2, 2, 2, q, F32, 2, 2, 2, lo, 8, 0.0, None) == E_SHAPE
    assert pad(p, 1, 2, 2, 2, q, F32, 2, 2, 2, lo, 0, 0.0, None) == E_DTYPE          # bf16
    assert pad(p, F64, 2, 2, 2, q, 2, 2, 2, 2, lo, 0, 0.0, None) == E_DTYPE          # u8
    assert pad(p + 4, F64, 2, 2, 2, q, F32, 2, 2, 2, lo, 0, 0.0, None) == E_ALIGN
    fin = L.fmri_tile_finalize_flip
    assert fin(0, p, 4, 4, 4, 1, q, 2, 2, 2, lo, 0, p, None) == E_SHAPE
    assert fin(p, p, 4, 4, 4, 1, q, 2, 2, 2, None, 0, p, None) == E_SHAPE
    assert fin(p, p, 4, 4, 4, 1, q, 2, 2, 2, lo, 0, 0, None) == E_SHAPE
    assert fin(p, p, 4, 4, 4, 0, q, 2, 2, 2, lo, 0, p, None) == E_SHAPE
    assert fin(p, p, 4, 4, 4, 1, q, 2, 0, 2, lo, 0, p, None) == E_SHAPE
    assert fin(p, p, 4, 4, 4, 1, q, 2, 2, 5, lo, 0, p, None) == E_SHAPE              # the window is larger than acc
    assert fin(p, p, 4, 4, 4, 1, q, 2, 2, 2, (ctypes.c_int32 * 3)(0, 3, 0), 0, p, None) == E_SHAPE    # lo + n leaves acc
    assert fin(p, p, 4, 4, 4, 1, q, 2, 2, 2, (ctypes.c_int32 * 3)(-1, 0, 0), 0, p, None) == E_SHAPE
    assert fin(p, p, 4, 4, 4, 1, q, 2, 2, 2, lo, -1, p, None) == E_SHAPE
    assert fin(p + 4, p, 4, 4, 4, 1, q, 2, 2, 2, lo, 0, p, None) == E_ALIGN


class _Foreign(object):
    """a model behind the reference's duck type: position-dependent, so that a wrong flip shows"""

    def __init__(self, patch):
        self.output_shape = (None, 1) + tuple(patch)
        self.ramp = np.linspace(0.5, 1.5, int(np.prod(patch))).reshape(patch)

    def predict(self, x):
        return np.tanh(np.asarray(x, dtype=np.float64) * self.ramp)


def _flips_as_before(data, model, overlap_factor, config):
    """predict_flips as it stood before the resident route (reference prediction.py:65-85)"""
    from fetal_net.prediction import flip_it, patch_wise_prediction
    patch_shape = list(config["patch_shape"]) + [config["patch_depth"]]
    out = []
    for r in range(4):
        for axes in itertools.combinations([0, 1, 2], r):
            pred = patch_wise_prediction(model=model, data=np.expand_dims(flip_it(data, axes).squeeze(), 0), overlap_factor=overlap_factor,
                                         patch_shape=patch_shape).squeeze()
            out.append(flip_it(pred, axes).squeeze())
    return out


@pytest.mark.parametrize("lead", [(), (1,)])
def test_predict_flips_and_stage_infer_without_a_device_are_unchanged(lead):
    from fetal_net import prediction as P
    from fetal_net.pipeline import Stage
    patch = (8, 8, 4)
    model = _Foreign(patch)
    cfg = {"patch_shape": list(patch[:2]), "patch_depth": patch[2]}
    vol = np.random.RandomState(4).randn(*(lead + (12, 10, 6)))
    assert P._device_tile_loop_refusal(model) is not None
    want = _flips_as_before(vol, model, 0.5, cfg)
    got = P.predict_flips(vol, model, 0.5, cfg)
    assert len(got) == 8
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)
    if not lead:
        assert float(np.abs(got[0] - got[7]).max()) > 1e-4
        for keep in (False, True):
            out = Stage(model, cfg, augment="flip", overlap=0.5, device=False).infer(vol, keep_variants=keep)
            np.testing.assert_array_equal(out, np.stack(want) if keep else np.median(np.stack(want), axis=0))
        np.testing.assert_array_equal(Stage(model, cfg, overlap=0.5, device=False).infer(vol), want[0])


def test_flip_variant_masks_say_what_the_host_route_does():
    """data (X, Y, Z): one mask both ways; data (1, X, Y, Z): numpy mirrors the axes as numbered, so the forward flip of axis k acts on
    spatial axis k - 1 (axis 0 is the singleton) while the backward flip of the squeezed prediction acts on spatial axis k"""
    from fetal_net import prediction as P
    from fetal_net.prediction import flip_it
    rs = np.random.RandomState(0)
    for shape in ((4, 5, 3), (1, 4, 5, 3)):
        data = rs.randn(*shape)
        variants = P._flip_variants(shape)
        assert len(variants) == 8 and variants[0] == (0, 0)
        for axes, (fwd, back) in zip(P.FLIP_AXES, variants):
            np.testing.assert_array_equal(flip_it(data, axes).squeeze(), np.flip(data.squeeze(), axis=R.masks_axes(fwd)))
            np.testing.assert_array_equal(flip_it(data.squeeze(), axes), np.flip(data.squeeze(), axis=R.masks_axes(back)))
    assert P._flip_variants((2, 4, 5, 3)) is None and P._flip_variants((4, 1, 3)) is None


def test_shape_only_geometry_is_the_host_geometry():
    """the resident loop tiles by `_geometry_of_shape`; the host route pads by `_geometry`: same paddings, corners and extents, including
    the asymmetric pad_for_fit of an odd deficit and the asymmetric pad0 of an even slice count"""
    from fetal_net import prediction as P

    class M3(object):
        output_shape = (None, 1, 16, 32, 32)

    class M2(object):
        output_shape = (None, 32, 32, 1)
        _input_layout = "channels_last_2d"

    for model, patch, shape in ((M3, (16, 32, 32), (24, 27, 40)), (M2, (32, 32, 4), (40, 48, 12)), (M2, (32, 32, 4), (20, 48, 3))):
        data = np.random.RandomState(1).randn(1, *shape)
        is3d, pad0, fit, data_0, indices, data_shape = P._geometry(model, data, patch, 0.5)
        g = P._geometry_of_shape(model, shape, patch, 0.5)
        assert g[0] == is3d and g[1] == pad0 and g[2] == fit and g[3] == data_0.shape and list(g[5]) == list(data_shape)
        np.testing.assert_array_equal(g[4], indices)
    assert P._geometry_of_shape(M3, (24, 27, 40), (16, 32, 32), 0.5)[2][1] == (3, 2)
    assert P._geometry_of_shape(M2, (40, 48, 12), (32, 32, 4), 0.5)[1][2] == (2, 1)
