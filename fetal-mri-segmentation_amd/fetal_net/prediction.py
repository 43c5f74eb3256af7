"""Sliding-window inference with the reference surface (reference fetal_net/prediction.py:88-210, :277-361).

`patch_wise_prediction` keeps the reference's geometry exactly (overlap interpolation, 1st-percentile padding, tile
index set, mean of overlapping tiles in float64).  With a model built by this package the whole tile loop stays on the
MI355X: the padded volume is uploaded once, tiles are gathered on the device (fmri_tile_gather), pushed through the
engine and overlap-added in float64 on the device (fmri_tile_scatter_accumulate / fmri_tile_finalize); one hipGraph per
tile-batch size replays gather -> network -> scatter.  A 2-D model with previous-slice truth channels (`truth_data` with
`prev_truth_index` / `prev_truth_size`) stays on the device as well: the padded truth volume goes up beside the data and the gather appends
its slices to every tile (fmri_tile_gather_stack).  A volume that is already on the device - a float64 CUDA tensor, or the one upload
of `predict_flips` / `fetal_net.pipeline` - runs the same captured loop without touching the host: fmri_volume_pad_flip writes the
mirrored, padded volume, fmri_tile_finalize_flip the cropped, un-mirrored means (`_resident_overlap_add`).  Any other object with
`.output_shape` / `.predict(ndarray)` (the reference's duck-typing contract) is driven through the same geometry with host-side tiles.
Beyond the reference, `blend="gaussian"` (keyword-only, default None = the reference's uniform mean) weights every tile voxel by a Gaussian
of its distance to the tile centre on all of these routes (`gaussian_tile_tables`; fmri_tile_scatter_weighted / fmri_tile_finalize*_weighted).
"""
import gc
import itertools
import os

import numpy as np

from .augment import contrast_augment, generate_permutation_keys, permute_data, reverse_permute_data
from .engine_model import Model
from .utils.patches import get_patch_from_3d_data
from .utils.threaded_generator import ThreadedGenerator


def get_set_of_patch_indices_full(start, stop, step):
    axes = []
    for a, b, s in zip(start, stop, step):
        idx = list(range(int(a), int(b) + 1, int(s)))
        if int(b) % int(s) > 0:
            idx.append(int(b))
        axes.append(idx)
    return np.array(list(itertools.product(*axes)))


def batch_iterator(indices, batch_size, data_0, patch_shape, truth_0, prev_truth_index, truth_patch_shape):
    i = 0
    while i < len(indices):
        batch, curr = [], []
        while len(batch) < batch_size and i < len(indices):
            ix = indices[i]
            patch = get_patch_from_3d_data(data_0, patch_shape=patch_shape, patch_index=ix)
            if truth_0 is not None:
                t_ix = list(ix[:2]) + [ix[2] + prev_truth_index]
                patch = np.concatenate([patch, get_patch_from_3d_data(truth_0, patch_shape=truth_patch_shape, patch_index=t_ix)],
                                       axis=-1)
            batch.append(patch)
            curr.append(ix)
            i += 1
        yield [batch, curr]


def _half_pads(delta):
    return [(int(np.ceil(d / 2)), int(np.floor(d / 2))) for d in delta]


def _is3d(model):
    """the reference counts the output axes longer than 1 (prediction.py:120-121), which takes a 2-D model with several labels - output
    (N, X, Y, L) - for a 3-D one: a model that names its layout (this package's, or a foreign object with `_input_layout`) is asked"""
    layout = getattr(model, "_input_layout", None)
    if layout in ("channels_first_3d", "channels_last_2d"):
        return layout == "channels_first_3d"
    return int(np.sum(np.array(model.output_shape[1:]) > 1)) > 2


def _geometry_of_shape(model, shape, patch_shape, overlap_factor):
    """the tiling of a volume of `shape` (X, Y, Z), values aside: is3d, the two paddings, the padded extent, the tile corners, the
    accumulator's extent"""
    out_shape = model.output_shape
    is3d = _is3d(model)
    prediction_shape = tuple(out_shape[-3:]) if is3d else tuple(out_shape[-3:-1]) + (1,)
    min_overlap = np.subtract(patch_shape, prediction_shape)
    max_overlap = np.subtract(patch_shape, (1, 1, 1))
    overlap = min_overlap + (overlap_factor * (max_overlap - min_overlap)).astype(int)
    pad0 = _half_pads(np.subtract(patch_shape, prediction_shape))
    shape_0 = tuple(int(n) + p[0] + p[1] for n, p in zip(shape, pad0))
    pad_for_fit = _half_pads(np.maximum(np.subtract(patch_shape, shape_0), 0))
    vshape = tuple(n + p[0] + p[1] for n, p in zip(shape_0, pad_for_fit))
    indices = get_set_of_patch_indices_full((0, 0, 0), np.subtract(vshape, patch_shape), np.subtract(patch_shape, overlap))
    data_shape = list(np.asarray(shape) + np.sum(pad_for_fit, -1))
    data_shape += [out_shape[1]] if is3d else [out_shape[-1]]
    return is3d, pad0, pad_for_fit, vshape, indices, data_shape


def _geometry(model, data, patch_shape, overlap_factor):
    is3d, pad0, pad_for_fit, vshape, indices, data_shape = _geometry_of_shape(model, data.shape[-3:], patch_shape, overlap_factor)
    # the reference pads with the 1st percentile unconditionally (prediction.py:138-146); with zero pad widths np.pad returns the data
    # unchanged, so the percentile (a sort-sized pass over the whole volume, twice) is only computed when something is padded
    data_0 = data[0]
    if np.sum(pad0) > 0:
        data_0 = np.pad(data_0, pad0, mode='constant', constant_values=np.percentile(data_0, q=1))
    if np.sum(pad_for_fit) > 0:
        data_0 = np.pad(data_0, pad_for_fit, 'constant', constant_values=np.percentile(data_0, q=1))
    assert tuple(data_0.shape) == vshape
    return is3d, pad0, pad_for_fit, data_0, indices, data_shape


def _unpad(arr, pad_for_fit):
    if np.sum(pad_for_fit) > 0:
        sl = tuple(slice(p[0] if p[0] else None, -p[1] if p[1] else None) for p in pad_for_fit)
        arr = arr[sl]
    return arr


BLEND_MODES = (None, "gaussian")
DEFAULT_SIGMA_SCALE = 0.125                  # nnU-Net's and MONAI's value


def gaussian_tile_tables(tile, sigma_scale=DEFAULT_SIGMA_SCALE):
    """The importance weights of a Gaussian-blended output tile (px, py, pz), one float32 table per axis:
        g_a[i] = float32(exp(-0.5 * ((i - (p_a - 1) / 2) / (sigma_scale * p_a))**2)),  i = 0 .. p_a - 1,
    computed in float64 and rounded once; an axis of extent 1 gives [1.0].  This is the only place that computes them: the host loop,
    the kernels (fmri_tile_scatter_weighted reads these tables) and the tests all take the weight of a tile voxel as
    w = (float64(gx[x]) * float64(gy[y])) * float64(gz[z]).  At the default sigma_scale the smallest entry lies above exp(-8), so w
    cannot underflow."""
    s = _sigma_scale(sigma_scale)
    tables = []
    for p in tile:
        p = int(p)
        if p <= 0:
            raise ValueError("gaussian_tile_tables: tile extents must be positive (got %r)" % (tuple(tile),))
        i = np.arange(p, dtype=np.float64)
        tables.append(np.exp(-0.5 * ((i - (p - 1) / 2.0) / (s * p)) ** 2).astype(np.float32))
    return tables


def _sigma_scale(sigma_scale):
    s = float(sigma_scale)
    if not (np.isfinite(s) and s > 0):
        raise ValueError("blend_sigma_scale must be a positive finite number (got %r)" % (sigma_scale,))
    return s


def _blend_key(blend, sigma_scale):
    """the checked (blend, sigma_scale) pair the tile loops are keyed by: (None, None) for the unweighted mean"""
    if blend not in BLEND_MODES:
        raise ValueError("blend must be None or 'gaussian' (got %r)" % (blend,))
    s = _sigma_scale(sigma_scale)
    return (blend, s) if blend is not None else (None, None)


def _tile_weights(tile, sigma_scale):
    """float64 (px, py, pz): w = (gx[x] * gy[y]) * gz[z] of `gaussian_tile_tables`, in the order every route multiplies in"""
    gx, gy, gz = (g.astype(np.float64) for g in gaussian_tile_tables(tile, sigma_scale))
    return (gx[:, None, None] * gy[None, :, None]) * gz[None, None, :]


def patch_wise_prediction(model, data, patch_shape, overlap_factor=0, batch_size=5, permute=False, truth_data=None,
                          prev_truth_index=None, prev_truth_size=None, *, blend=None, blend_sigma_scale=DEFAULT_SIGMA_SCALE):
    """data (1,X,Y,Z) -> (X,Y,Z,C) float64 mean of all tiles covering each voxel.  A float64 CUDA tensor stays one: the tile loop then
    runs on the resident volume (`_resident_overlap_add`) and the means come back as a CUDA tensor; that form needs the device tile loop
    (an engine model, no permute, no truth_data) and raises TypeError where it does not apply.
    blend: None - the reference's rule, every tile counts the same - or 'gaussian': every tile voxel counts with the Gaussian importance
    weight of `gaussian_tile_tables` (sigma = blend_sigma_scale * tile extent per axis), sum(w * p) / sum(w), on every route."""
    return _patch_wise(model, data, patch_shape, overlap_factor, batch_size, permute, truth_data, prev_truth_index, prev_truth_size, None,
                       _blend_key(blend, blend_sigma_scale))


def patch_wise_label_map(model, data, patch_shape, overlap_factor=0, batch_size=5, threshold=0.5, labels=None, permute=False,
                         truth_data=None, prev_truth_index=None, prev_truth_size=None, *, blend=None,
                         blend_sigma_scale=DEFAULT_SIGMA_SCALE):
    """data (1,X,Y,Z) -> (X,Y,Z) uint8 label map: get_prediction_labels of patch_wise_prediction's mean, taken on the device.  The tile
    loop is patch_wise_prediction's - same captured graphs, same slab pipeline - with fmri_tile_finalize_labels in place of
    fmri_tile_finalize, so one byte per voxel comes down instead of 8 * C.  Wherever patch_wise_prediction leaves the device path
    (permute, a foreign model object) the label map is get_prediction_labels of its result.  blend / blend_sigma_scale: as for
    patch_wise_prediction (the label rule is then applied to the blended means, fmri_tile_finalize_labels_weighted)."""
    n_labels = int(model.output_shape[1] if _is3d(model) else model.output_shape[-1])
    values = _label_values(n_labels, labels)
    out = _patch_wise(model, data, patch_shape, overlap_factor, batch_size, permute, truth_data, prev_truth_index, prev_truth_size,
                      (float(threshold), values), _blend_key(blend, blend_sigma_scale))
    if out.dtype != np.uint8:                                # the host path's float64 means (X, Y, Z, C)
        out = np.asarray(prediction_to_image(np.moveaxis(out, -1, 0)[np.newaxis], label_map=True, threshold=threshold,
                                             labels=values)).astype(np.uint8)
    return out


def _label_values(n_labels, labels):
    values = list(range(1, n_labels + 1)) if labels is None else [int(v) for v in labels]
    if len(values) != n_labels:
        raise ValueError("labels %r: %d values for %d output channels" % (labels, len(values), n_labels))
    return values


def _patch_wise(model, data, patch_shape, overlap_factor, batch_size, permute, truth_data, prev_truth_index, prev_truth_size, label_map,
                blend=(None, None)):
    """patch_wise_prediction (label_map None) / patch_wise_label_map ((threshold, values): the device path then returns the uint8 map);
    blend: the pair of `_blend_key`"""
    if _is_device_tensor(data):                              # a float64 CUDA tensor stays one (the convention of fetal_net.preprocess)
        if label_map is not None:
            raise TypeError("patch_wise_label_map takes host volumes (got a device tensor)")
        return _patch_wise_resident(model, data, patch_shape, overlap_factor, batch_size, permute, truth_data, blend)
    is3d, pad0, pad_for_fit, data_0, indices, data_shape = _geometry(model, data, patch_shape, overlap_factor)
    layout2d = getattr(model, "_input_layout", "") == "channels_last_2d"
    # previous-slice truth on the device: 2-D models only (a 3-D model's truth channels are concatenated along z, reference prediction.py:100-110)
    truth_ok = truth_data is None or (not is3d and layout2d and prev_truth_index is not None and bool(prev_truth_size))
    on_device = isinstance(model, Model) and truth_ok and not permute and model._unsupported is None and (is3d or layout2d)
    if on_device:
        truth_0 = None
        if truth_data is not None:
            truth_0 = np.pad(truth_data[0], pad0, mode='constant', constant_values=0)
            truth_0 = np.pad(truth_0, pad_for_fit, 'constant', constant_values=0)
        out, count_ok = _device_overlap_add(model, data_0, indices, patch_shape, batch_size, data_shape, is3d, truth_0=truth_0,
                                            aux_dz=int(prev_truth_index) if truth_0 is not None else 0,
                                            aux_nz=int(prev_truth_size) if truth_0 is not None else 0, label_map=label_map, blend=blend)
        assert count_ok, 'Found zeros in count'
        out = _unpad(out, pad_for_fit)
        assert np.array_equal(out.shape[:3], data[0].shape), 'prediction shape wrong'
        return out

    if truth_data is not None:
        truth_0 = np.pad(truth_data[0], pad0, mode='constant', constant_values=0)
        truth_0 = np.pad(truth_0, pad_for_fit, 'constant', constant_values=0)
        truth_patch_shape = list(patch_shape[:2]) + [prev_truth_size]
    else:
        truth_0, truth_patch_shape = None, None
    tb_iter = iter(ThreadedGenerator(batch_iterator(indices, batch_size, data_0, patch_shape, truth_0, prev_truth_index,
                                                    truth_patch_shape), queue_maxsize=50))
    predicted_output = np.zeros(data_shape)
    blended = blend[0] is not None
    # blended: the float64 weight sums (X, Y, Z) take the place of the counts (the device rule, fmri_tile_scatter_weighted)
    predicted_count = np.zeros(data_shape[:3]) if blended else np.zeros(data_shape, dtype=np.int16)
    weights = {}                                             # output-tile extent -> float64 weights
    for curr_batch, batch_indices in tb_iter:
        curr_batch = np.asarray(curr_batch)
        if is3d:
            curr_batch = np.expand_dims(curr_batch, 1)
        prediction = predict(model, curr_batch, permute=permute)
        prediction = prediction.transpose([0, 2, 3, 4, 1]) if is3d else np.expand_dims(prediction, -2)
        for patch, (x, y, z) in zip(prediction, batch_indices):
            xl, yl, zl = patch.shape[:-1]
            if blended:
                w = weights.get((xl, yl, zl))
                if w is None:
                    w = weights[(xl, yl, zl)] = _tile_weights((xl, yl, zl), blend[1])
                predicted_output[x:x + xl, y:y + yl, z:z + zl, :] += w[..., None] * patch
                predicted_count[x:x + xl, y:y + yl, z:z + zl] += w
                continue
            predicted_output[x:x + xl, y:y + yl, z:z + zl, :] += patch
            predicted_count[x:x + xl, y:y + yl, z:z + zl] += 1
    assert np.all(predicted_count > 0), 'Found zeros in count'
    if blended:
        predicted_count = predicted_count[..., None]
    predicted_output, predicted_count = _unpad(predicted_output, pad_for_fit), _unpad(predicted_count, pad_for_fit)
    assert np.array_equal(predicted_count.shape[:-1], data[0].shape), 'prediction shape wrong'
    return predicted_output / predicted_count


def _tile_loop_state(model, vshape, n, patch_shape, batch_size, data_shape, is3d=True, aux_dz=0, aux_nz=0, blend=(None, None)):
    """-> (state, tile-group size).  The static buffers of the device tile loop (volume, accumulators, tile batch, index list) and one
    captured hipGraph per distinct batch size - gather -> network -> float64 overlap-add - cached on the model and re-used for every
    following volume of the same padded shape `vshape` tiled into `n` tiles, whichever loop drives them (`_device_overlap_add` from host
    memory, `_resident_overlap_add` from a device tensor).  2-D models: a tile (px, py, slices) IS the channels-last input of the
    network (the slice stack is the channel axis) and its output is one slice (px, py, 1); with aux_nz every tile carries aux_nz more
    channels, its truth slices from aux_dz slices past the tile's corner (reference batch_iterator, prediction.py:98-114).
    blend (the pair of `_blend_key`): 'gaussian' appends the pair to the key; the state then holds the three device tables of the output
    tile and the float64 weight sums `wsum` instead of the counts `cnt`, and the captured body ends in fmri_tile_scatter_weighted."""
    import torch
    from fmri_hip import ops
    patch = tuple(int(p) for p in patch_shape)
    vshape = tuple(int(s) for s in vshape)
    ashape = tuple(int(s) for s in data_shape)
    use_graph = os.environ.get("FMRI_HIPGRAPH", "1") == "1"
    if not is3d:
        # 2-D: a tile is a 5-slice stack and the caller's batch (reference default 5) is far too small to fill the device - the MFMA
        # kernels also want the slice count in multiples of 4.  The overlap-add does not depend on how tiles are grouped (float64 sums)
        batch_size = max(batch_size, 64)
    else:
        # 3-D: the caller's batch (reference default 5) leaves a 1-tile remainder on the usual 36-tile volume and every forward pass pays its
        # kernel tails; tiles are grouped by at least 12 and the groups are evened out (36 -> 3 x 12: device loop 52.4 -> 50.4 ms).  As above
        # the result does not depend on the grouping.
        groups = -(-n // max(batch_size, 12))
        batch_size = -(-n // groups)
    sizes = sorted({min(batch_size, n - i) for i in range(0, n, batch_size)}, reverse=True)
    aux_nz = int(aux_nz)
    aux_dz = int(aux_dz) if aux_nz else 0
    assert aux_nz == 0 or not is3d
    blended = blend[0] is not None
    key = (vshape, ashape, patch, tuple(sizes), use_graph, aux_dz, aux_nz)
    if blended:
        key += (tuple(blend),)                               # (the unweighted key ends in aux_dz, aux_nz)
    st = model.__dict__.get("_tile_state")
    if st is None or st["key"] != key:
        st = dict(key=key, vol=torch.empty(vshape, dtype=torch.float32, device="cuda"),
                  aux=torch.empty(vshape, dtype=torch.float32, device="cuda") if aux_nz else None,
                  acc=torch.zeros(ashape, dtype=torch.float64, device="cuda"), per_b={})
        if blended:
            st["wsum"] = torch.zeros(ashape[:3], dtype=torch.float64, device="cuda")
            st["tables"] = tuple(torch.from_numpy(g).cuda() for g in gaussian_tile_tables(patch if is3d else (patch[0], patch[1], 1), blend[1]))
        else:
            st["cnt"] = torch.zeros(ashape[:3], dtype=torch.int32, device="cuda")
        for B in sizes:
            eng = model.engine(B)
            # 3-D: (B, px, py, pz, 1) = NDHWC with one channel; 2-D: (1, B, px, py, slices [+ truth slices]) = the planar layout, slices as channels
            tshape = (B,) + patch + (1,) if is3d else (1, B, patch[0], patch[1], patch[2] + aux_nz)
            opatch = patch if is3d else (patch[0], patch[1], 1)
            pb = dict(idx=torch.zeros((B, 3), dtype=torch.int32, device="cuda"),
                      tiles=torch.empty(tshape, dtype=eng.dtype, device="cuda"), graph=None)

            def body(pb=pb, B=B, opatch=opatch):
                e = model.engine(B)
                if aux_nz:
                    ops.tile_gather_stack(st["vol"], st["aux"], pb["idx"], patch, aux_dz, aux_nz, pb["tiles"])
                else:
                    ops.tile_gather(st["vol"], pb["idx"], patch, pb["tiles"])
                e.predict(pb["tiles"])
                if blended:
                    ops.tile_scatter_weighted(e.probs, pb["idx"], opatch, st["tables"], st["acc"], st["wsum"])
                else:
                    ops.tile_scatter_accumulate(e.probs, pb["idx"], opatch, st["acc"], st["cnt"])

            pb["body"] = body
            if use_graph:
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    body()                                   # warm-up outside capture (lazy allocations, module loads)
                torch.cuda.current_stream().wait_stream(side)
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                # No cyclic garbage collection while the stream is capturing: a collector run that happens to free an old CUDAGraph /
                # stream / event (the per-batch closures above sit in reference cycles, so earlier tile states die by the cycle
                # collector, at an arbitrary allocation) destroys HIP objects mid-capture, which HIP refuses - and a failing destructor
                # aborts the process.  Collect now, outside the capture, and keep the collector off until the capture has ended.
                gc_was_on = gc.isenabled()
                gc.collect()
                gc.disable()
                try:
                    with torch.cuda.graph(g):
                        body()
                finally:
                    if gc_was_on:
                        gc.enable()
                pb["graph"] = g
            st["per_b"][B] = pb
        model.__dict__["_tile_state"] = st
    return st, batch_size


def _device_overlap_add(model, data_0, indices, patch_shape, batch_size, data_shape, is3d=True, truth_0=None, aux_dz=0, aux_nz=0,
                        label_map=None, blend=(None, None)):
    """Upload once, then per tile batch the captured gather -> network -> float64 overlap-add of `_tile_loop_state`, all on the device.
    truth_0 (2-D models): the padded truth volume (data_0's extent), see `_tile_loop_state`.
    label_map (threshold, values): finished slabs become label bytes on the device (fmri_tile_finalize_labels) and the uint8 map
    (X, Y, Z) is what comes down and is returned; None: the float64 means (X, Y, Z, C).
    blend (the pair of `_blend_key`): with 'gaussian' the slabs are divided by their weight sums (fmri_tile_finalize_weighted /
    fmri_tile_finalize_labels_weighted)."""
    import torch
    from fmri_hip import ops
    patch = tuple(int(p) for p in patch_shape)
    vshape = tuple(int(s) for s in data_0.shape)
    ashape = tuple(int(s) for s in data_shape)
    n = len(indices)
    aux_nz = int(aux_nz) if truth_0 is not None else 0
    aux_dz = int(aux_dz) if aux_nz else 0
    assert aux_nz == 0 or tuple(truth_0.shape) == vshape
    st, batch_size = _tile_loop_state(model, vshape, n, patch, batch_size, ashape, is3d, aux_dz, aux_nz, blend)
    blended = blend[0] is not None
    div = st["wsum"] if blended else st["cnt"]
    # ---- the volume goes up and the result comes down in x-slabs, pipelined with the tile groups (23 % of a volume's
    # time was host work - a pageable 42 MB upload in front of the first tile and a pageable 84 MB float64 download behind the last).
    # Tiles are ordered x-major (itertools.product), so tile group g only needs the x-range up to its last tile's end, and every voxel
    # in front of the NEXT group's first tile is final once group g has run: slab k of the volume is copied into a pinned buffer
    # (converting copy for non-fp32 callers) and uploaded on a copy stream while group k - 1 computes; finished slabs are divided by
    # their counts and downloaded into a pinned result while the later groups compute.  The result array is backed by pinned memory
    # that is this call's own (torch's caching host allocator recycles it when the caller drops the array).
    if st.get("up_stream") is None:
        st["up_stream"], st["down_stream"] = torch.cuda.Stream(), torch.cuda.Stream()
        st["pin_in"] = torch.empty(vshape, dtype=torch.float32, pin_memory=True)
    if aux_nz and st.get("pin_aux") is None:
        st["pin_aux"] = torch.empty(vshape, dtype=torch.float32, pin_memory=True)
    up, down = st["up_stream"], st["down_stream"]
    main = torch.cuda.current_stream()
    st["acc"].zero_()
    div.zero_()
    idx_all = torch.from_numpy(np.ascontiguousarray(indices, dtype=np.int32)).cuda()
    if label_map is None:
        out_dev = torch.empty_like(st["acc"])
        out_host = torch.empty(ashape, dtype=torch.float64, pin_memory=True)
    else:
        out_dev = torch.empty(ashape[:3], dtype=torch.uint8, device="cuda")
        out_host = torch.empty(ashape[:3], dtype=torch.uint8, pin_memory=True)
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    pin_np, src = st["pin_in"].numpy(), np.asarray(data_0)
    pin_aux, src_aux = (st["pin_aux"].numpy(), np.asarray(truth_0)) if aux_nz else (None, None)
    starts_x = [int(ix[0]) for ix in indices]
    up_to = 0                                   # x-planes uploaded so far
    done_to = 0                                 # x-planes finalised and on their way down
    up.wait_stream(main)                        # (the previous volume's gathers have read st["vol"]; uploads never wait for this volume's tiles)
    for i in range(0, n, batch_size):
        hi = min(n, i + batch_size)
        need = min(vshape[0], max(starts_x[i:hi]) + patch[0])
        if need > up_to:
            np.copyto(pin_np[up_to:need], src[up_to:need], casting="unsafe")
            if aux_nz:
                np.copyto(pin_aux[up_to:need], src_aux[up_to:need], casting="unsafe")
            with torch.cuda.stream(up):
                st["vol"][up_to:need].copy_(st["pin_in"][up_to:need], non_blocking=True)
                if aux_nz:
                    st["aux"][up_to:need].copy_(st["pin_aux"][up_to:need], non_blocking=True)
            up_to = need
            main.wait_stream(up)
        bidx = idx_all[i:hi]
        pb = st["per_b"][int(bidx.shape[0])]
        pb["idx"].copy_(bidx)
        if pb["graph"] is not None:
            pb["graph"].replay()
        else:
            pb["body"]()
        final = ashape[0] if hi >= n else min(ashape[0], min(starts_x[hi:]))
        if final > done_to:
            if label_map is None:
                (ops.tile_finalize_weighted if blended else ops.tile_finalize)(st["acc"][done_to:final], div[done_to:final],
                                                                               out_dev[done_to:final], bad)
            else:
                (ops.tile_finalize_labels_weighted if blended else ops.tile_finalize_labels)(
                    st["acc"][done_to:final], div[done_to:final], out_dev[done_to:final], bad, *label_map)
            down.wait_stream(main)
            with torch.cuda.stream(down):
                out_host[done_to:final].copy_(out_dev[done_to:final], non_blocking=True)
            done_to = final
    down.synchronize()
    main.synchronize()
    return out_host.numpy(), int(bad.item()) == 0


def _is_device_tensor(data):
    return type(data).__module__.startswith("torch") and hasattr(data, "is_cuda") and bool(data.is_cuda)


def _device_tile_loop_refusal(model, permute=False, truth_data=None):
    """None when the device tile loop applies to `model` without previous-slice truth, else the reason it does not"""
    if not isinstance(model, Model):
        return "the model is no engine Model of this package (%s)" % type(model).__name__
    if model._unsupported is not None:
        return "the engine does not run this model (%s)" % (model._unsupported,)
    if getattr(model, "_input_layout", "") not in ("channels_first_3d", "channels_last_2d"):
        return "the model's input layout %r has no device tile loop" % (getattr(model, "_input_layout", None),)
    if permute:
        return "permute=True runs on host tiles"
    if truth_data is not None:
        return "truth_data comes with host volumes only"
    return None


def _resident_overlap_add(model, vol, patch_shape, overlap_factor, batch_size, variants, stack, blend=(None, None)):
    """The device tile loop on a volume that is already there.  vol: float64 CUDA tensor (X, Y, Z), unpadded; variants: one
    (forward flip mask, backward flip mask) pair per slot of stack, a float64 CUDA tensor (K, X, Y, Z, C).  Per variant: the mirrored,
    padded fp32 volume of the tiler is written by fmri_volume_pad_flip (the 1st-percentile pad constants come from ops.percentile_f64,
    once per call - mirroring does not change them - and only when something is padded), the captured graphs of `_tile_loop_state`
    replay over the same index list as the host-fed loop, and fmri_tile_finalize_flip writes the means, cropped and mirrored back, into
    the variant's slot (blend 'gaussian', the pair of `_blend_key`: fmri_tile_finalize_flip_weighted divides by the weight sums).  Nothing
    is copied to the host but the count of uncovered voxels, once, at the end."""
    import torch
    from fmri_hip import ops
    shape = tuple(int(s) for s in vol.shape)
    is3d, pad0, pad_for_fit, vshape, indices, data_shape = _geometry_of_shape(model, shape, patch_shape, overlap_factor)
    patch = tuple(int(p) for p in patch_shape)
    n = len(indices)
    with torch.cuda.device(vol.device):
        st, batch_size = _tile_loop_state(model, vshape, n, patch, batch_size, data_shape, is3d, blend=blend)
        blended = blend[0] is not None
        div = st["wsum"] if blended else st["cnt"]
        assert tuple(stack.shape) == (len(variants),) + shape + (int(data_shape[3]),) and stack.dtype == torch.float64
        lo0, lo1 = [p[0] for p in pad0], [p[0] for p in pad_for_fit]
        padded0, padded1 = np.sum(pad0) > 0, np.sum(pad_for_fit) > 0
        fill0 = fill1 = 0.0
        mid = None                                   # the float64 volume between the two paddings, when both are there
        if padded0 or padded1:
            fill0 = fill1 = float(ops.percentile_f64(vol, 1))
        if padded0 and padded1:
            mid = torch.empty(tuple(s + p[0] + p[1] for s, p in zip(shape, pad0)), dtype=torch.float64, device=vol.device)
            fill1 = float(ops.percentile_f64(ops.volume_pad_flip(vol, mid, lo0, 0, fill0), 1))
        idx_all = torch.from_numpy(np.ascontiguousarray(indices, dtype=np.int32)).to(vol.device)
        bad = torch.zeros(1, dtype=torch.int32, device=vol.device)
        if st.get("up_stream") is not None:
            torch.cuda.current_stream().wait_stream(st["up_stream"])
        for k, (fwd, back) in enumerate(variants):
            if mid is not None:
                ops.volume_pad_flip(ops.volume_pad_flip(vol, mid, lo0, fwd, fill0), st["vol"], lo1, 0, fill1)
            else:
                ops.volume_pad_flip(vol, st["vol"], lo0 if padded0 else lo1, fwd, fill0)
            st["acc"].zero_()
            div.zero_()
            for i in range(0, n, batch_size):
                bidx = idx_all[i:min(n, i + batch_size)]
                pb = st["per_b"][int(bidx.shape[0])]
                pb["idx"].copy_(bidx)
                if pb["graph"] is not None:
                    pb["graph"].replay()
                else:
                    pb["body"]()
            (ops.tile_finalize_flip_weighted if blended else ops.tile_finalize_flip)(st["acc"], div, stack[k], bad, lo1, back)
        assert int(bad.item()) == 0, 'Found zeros in count'
    return stack


def _resident_stack(model, vol, n_variants):
    import torch
    n_out = int(model.output_shape[1] if _is3d(model) else model.output_shape[-1])
    return torch.empty((n_variants,) + tuple(int(s) for s in vol.shape) + (n_out,), dtype=torch.float64, device=vol.device)


def _patch_wise_resident(model, data, patch_shape, overlap_factor, batch_size, permute, truth_data, blend=(None, None)):
    """patch_wise_prediction of a float64 CUDA tensor (1, X, Y, Z) -> float64 CUDA tensor (X, Y, Z, C)"""
    import torch
    why = _device_tile_loop_refusal(model, permute, truth_data)
    if why is None and not (data.dtype == torch.float64 and data.dim() == 4 and data.shape[0] == 1 and data.numel() > 0):
        why = "a float64 tensor (1, X, Y, Z) is needed (got %s %s)" % (data.dtype, tuple(data.shape))
    if why is not None:
        raise TypeError("patch_wise_prediction of a device tensor needs the device tile loop: " + why)
    vol = data[0].contiguous()
    return _resident_overlap_add(model, vol, patch_shape, overlap_factor, batch_size, [(0, 0)], _resident_stack(model, vol, 1), blend)[0]


def get_prediction_labels(prediction, threshold=0.5, labels=None):
    """prediction (n_samples, L, X, Y, Z) -> a list of uint8 label maps (X, Y, Z), one per sample: argmax over the label axis plus 1 (ties go
    to the lowest index), 0 where the maximum lies below `threshold`, then mapped through `labels` (value k becomes labels[k - 1]).
    Reference prediction.py:214-227.  Departure: the reference's line 218 takes argmax(..., axis=1) of a sample that has already lost its
    batch axis and never adds 1, so its `labels[value - 1]` mapping and its docstring describe what is implemented here, not what it runs."""
    prediction = np.asarray(prediction)
    n_labels = prediction.shape[1]
    values = np.asarray([0] + _label_values(n_labels, labels), dtype=np.uint8)
    out = []
    for sample in prediction:
        label_data = np.argmax(sample, axis=0) + 1
        label_data[np.max(sample, axis=0) < threshold] = 0
        out.append(values[label_data])
    return out


def multi_class_prediction(prediction):
    """one array per label channel of a prediction (1, L, X, Y, Z) (reference prediction.py:268-274, which wraps them in Nifti1Image; this
    package writes NIfTI through utils.nifti)"""
    prediction = np.asarray(prediction)
    return [prediction[0, i] for i in range(prediction.shape[1])]


def prediction_to_image(prediction, label_map=False, threshold=0.5, labels=None):
    """reference prediction.py:243-265, returning arrays: one channel -> its volume, as a label map labels[0] (default 1) where it is
    > threshold; several channels -> the label map of get_prediction_labels, or the list of multi_class_prediction.  Note the two rules
    differ at equality: one channel needs > threshold, several keep a maximum equal to the threshold (only < threshold is background)."""
    prediction = np.asarray(prediction)
    if prediction.shape[1] == 1:
        data = prediction[0, 0]
        if label_map:
            label_map_data = np.zeros(prediction[0, 0].shape, np.int8)
            label_map_data[data > threshold] = labels[0] if labels else 1
            data = label_map_data
        return data
    if label_map:
        return get_prediction_labels(prediction, threshold=threshold, labels=labels)[0]
    return multi_class_prediction(prediction)


def predict(model, data, permute=False):
    """reference prediction.py:354-361"""
    if permute:
        return np.asarray([predict_with_permutations(model, data[b]) for b in range(data.shape[0])])
    return model.predict(data)


def predict_with_permutations(model, data):
    """mean over the 48 permutation keys of un-permuted predictions (reference prediction.py:362-367); data (C, X, Y, Z).
    Keys that act identically (only rotate_y and the three flips act) are predicted once and weighted by their multiplicity."""
    groups = {}
    for key in generate_permutation_keys():
        groups.setdefault((key[0][0], key[1], key[2], key[3]), []).append(key)
    total, n = None, 0
    for keys in groups.values():
        pred = reverse_permute_data(model.predict(permute_data(data, keys[0])[np.newaxis])[0], keys[0])
        total = pred * len(keys) if total is None else total + pred * len(keys)
        n += len(keys)
    return total / n


def flip_it(data_, axes):
    """mirror along every axis in `axes` (an involution: applying it twice restores the input)"""
    axes = tuple(int(a) for a in axes)
    return np.flip(data_, axis=axes) if axes else data_


FLIP_AXES = [axes for r in range(4) for axes in itertools.combinations([0, 1, 2], r)]      # the reference's variant order


def _predict_flips_host(data, model, overlap_factor, config, blend=None, blend_sigma_scale=DEFAULT_SIGMA_SCALE):
    """the 8 axis-flip variants, each mirrored with numpy, predicted patch-wise from host memory and flipped back (reference
    prediction.py:65-85): the route of models without the device tile loop, and the other arm of tools/bench_tta.py"""
    patch_shape = list(config["patch_shape"]) + [config["patch_depth"]]
    predictions = []
    for axes in FLIP_AXES:
        flipped = flip_it(data, axes)
        pred = patch_wise_prediction(model=model, data=np.expand_dims(flipped.squeeze(), 0), overlap_factor=overlap_factor,
                                     patch_shape=patch_shape, blend=blend, blend_sigma_scale=blend_sigma_scale).squeeze()
        predictions.append(flip_it(pred, axes).squeeze())
    return predictions


def _flip_variants(shape):
    """(forward mask, backward mask) of every variant for `data` of `shape`, or None where the masks cannot say what the host route
    does.  The host route mirrors the axes of `data` as given and mirrors the squeezed prediction (X, Y, Z[, C]) back along the same axis
    NUMBERS: for data (X, Y, Z) the two are one mask; for data (1, X, Y, Z) - the reference's call - axis 0 is the singleton, so the
    forward flip of axis k mirrors spatial axis k - 1 and the backward flip mirrors spatial axis k."""
    from fmri_hip.ops import flip_mask_of
    if len(shape) == 4 and shape[0] == 1:
        lead = 1
    elif len(shape) == 3:
        lead = 0
    else:
        return None
    if min(shape[lead:]) < 2:                                 # squeeze() would drop a spatial axis
        return None
    return [(flip_mask_of(a - lead for a in axes if a >= lead), flip_mask_of(axes)) for axes in FLIP_AXES]


def resident_tta_default():
    """whether host volumes take the resident route by default (FMRI_TTA_RESIDENT=0 keeps them on the host-fed route: A/B runs)"""
    return os.environ.get("FMRI_TTA_RESIDENT", "1") != "0"


def _resident_flip_stack(vol, model, overlap_factor, patch_shape, variants, blend=None, blend_sigma_scale=DEFAULT_SIGMA_SCALE):
    """the variants' predictions of a float64 CUDA volume (X, Y, Z) as one resident stack (K, X, Y, Z, C)"""
    return _resident_overlap_add(model, vol, patch_shape, overlap_factor, 5, variants, _resident_stack(model, vol, len(variants)),
                                 _blend_key(blend, blend_sigma_scale))


def _upload_f64(arr):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float64)).cuda()


def _download(t):
    """device tensor -> numpy array backed by pinned memory of its own (one asynchronous copy, then a wait)"""
    import torch
    host = torch.empty(tuple(t.shape), dtype=t.dtype, pin_memory=True)
    host.copy_(t, non_blocking=True)
    torch.cuda.current_stream().synchronize()
    return host.numpy()


def predict_flips(data, model, overlap_factor, config, *, blend=None, blend_sigma_scale=DEFAULT_SIGMA_SCALE):
    """the 8 axis-flip variants, each predicted patch-wise and flipped back; returns the list (reference prediction.py:65-85).  With a
    model that has the device tile loop the volume goes up once, every variant is mirrored, tiled and mirrored back on the device
    (`_resident_overlap_add`) and the stack of 8 comes down once; a float64 CUDA tensor stays one: the list then holds 8 views of one
    resident stack (8, X, Y, Z[, C]).  Any other model takes `_predict_flips_host`.  blend / blend_sigma_scale: as for
    patch_wise_prediction, for every variant."""
    _blend_key(blend, blend_sigma_scale)
    patch_shape = list(config["patch_shape"]) + [config["patch_depth"]]
    tensor = _is_device_tensor(data)
    why = _device_tile_loop_refusal(model)
    variants = _flip_variants(tuple(data.shape)) if why is None else None
    if tensor:
        import torch
        if why is None and (variants is None or data.dtype != torch.float64):
            why = "a float64 tensor (X, Y, Z) or (1, X, Y, Z) is needed (got %s %s)" % (data.dtype, tuple(data.shape))
        if why is not None:
            raise TypeError("predict_flips of a device tensor needs the device tile loop: " + why)
    elif variants is None or not (isinstance(data, np.ndarray) and data.dtype == np.float64 and resident_tta_default()
                                  and _hip_rotate_ok()):
        return _predict_flips_host(data, model, overlap_factor, config, blend, blend_sigma_scale)
    vol = data if tensor else _upload_f64(data)
    stack = _resident_flip_stack(vol.reshape(vol.shape[-3:]).contiguous(), model, overlap_factor, patch_shape, variants, blend,
                                 blend_sigma_scale)
    if stack.shape[-1] == 1:
        stack = stack[..., 0]
    if not tensor:
        stack = _download(stack)
    return [stack[k] for k in range(len(variants))]


# --------------------------------------------------------------------------------------------------- agreement of the TTA variants
TTA_MAPS = ("mean", "variance", "entropy", "disagreement")
TTA_MAX_VARIANTS, TTA_MAX_CHANNELS = 64, 16


def agreement_scores(counts):
    """(variant_dice (K, C), estimated_dice (C,), volume_cv (C,)) from the set sizes counts (C, 2K + 1) = [|M|, |V_0| .. |V_K-1|,
    |V_0 & M| .. |V_K-1 & M|] per channel: the Dice of every variant's mask with the consensus mask, 2 i / (a + b), 1.0 where both are
    empty; its mean over the variants (the "estimated Dice" of TTA self-training); and the population standard deviation of the variants'
    volumes |V_k| over their mean, 0.0 where the mean is 0."""
    counts = np.asarray(counts, dtype=np.int64)
    if counts.ndim != 2 or counts.shape[1] < 3 or counts.shape[1] % 2 == 0:
        raise ValueError("counts (C, 2K + 1) are needed (got %s)" % (counts.shape,))
    K = (counts.shape[1] - 1) // 2
    a, b, i = counts[:, :1], counts[:, 1:1 + K], counts[:, 1 + K:]
    both = (a + b).astype(np.float64)
    dice = np.where(both == 0, 1.0, 2.0 * i / np.where(both == 0, 1.0, both))
    vol = b.astype(np.float64)
    mean = vol.mean(axis=1)
    cv = np.where(mean == 0, 0.0, vol.std(axis=1) / np.where(mean == 0, 1.0, mean))
    return np.ascontiguousarray(dice.T), dice.mean(axis=1), cv


class TTAAgreement(object):
    """What K test-time variants of one prediction agree on (`tta_agreement`).  `median` and the requested maps of TTA_MAPS (`mean`,
    `variance`: the population variance, `entropy`: the binary entropy of the mean in bits, `disagreement`: the share of variants on the
    other side of the threshold than the median) are shaped like one variant, arrays or device tensors as the input was; a map that was
    not asked for is None.  `counts` (C, 2K + 1) int64, `variant_dice` (K, C), `estimated_dice` (C,), `volume_cv` (C,): numpy, see
    `agreement_scores`.  They describe the grid the variants are on."""

    def __init__(self, median, maps, counts, threshold):
        self.median = median
        for name in TTA_MAPS:
            setattr(self, name, maps.get(name))
        self.threshold = float(threshold)
        self.counts = np.asarray(counts, dtype=np.int64)
        self.variant_dice, self.estimated_dice, self.volume_cv = agreement_scores(self.counts)

    def map_names(self):
        return ("median",) + tuple(name for name in TTA_MAPS if getattr(self, name) is not None)

    def with_maps(self, fn):
        """the same counts and scores with every map replaced by fn(map): how the pipeline takes the maps back to the input grid"""
        maps = {name: fn(getattr(self, name)) for name in self.map_names()}
        return TTAAgreement(maps.pop("median"), maps, self.counts, self.threshold)

    def as_dict(self):
        out = {name: getattr(self, name) for name in self.map_names()}
        out.update(threshold=self.threshold, counts=self.counts, variant_dice=self.variant_dice, estimated_dice=self.estimated_dice,
                   volume_cv=self.volume_cv)
        return out


def _checked_maps(maps):
    maps = tuple(maps)
    if any(m not in TTA_MAPS for m in maps) or len(set(maps)) != len(maps):
        raise ValueError("maps must be distinct names of %s (got %r)" % (TTA_MAPS, maps))
    return maps


def _variants_stack(variants):
    """a list of K variants or a stack of them -> (one float64 stack (K, X, Y, Z[, C]), whether it is a device tensor).  A list of views
    that lie one behind the other in one device buffer - what `predict_flips` returns for a tensor - is taken as that buffer, not copied."""
    if isinstance(variants, (list, tuple)):
        if len(variants) == 0:
            raise ValueError("1 to %d variants are needed (got 0)" % TTA_MAX_VARIANTS)
        if all(_is_device_tensor(v) for v in variants):
            import torch
            first = variants[0]
            step = first.numel() * first.element_size()
            if first.is_contiguous() and all(v.is_contiguous() and v.shape == first.shape and v.dtype == first.dtype
                                             and v.untyped_storage().data_ptr() == first.untyped_storage().data_ptr()
                                             and v.data_ptr() == first.data_ptr() + k * step for k, v in enumerate(variants)):
                variants = torch.as_strided(first, (len(variants),) + tuple(first.shape), (first.numel(),) + tuple(first.stride()))
            else:
                variants = torch.stack(list(variants))
        else:
            variants = np.stack([np.asarray(v) for v in variants])
    tensor = _is_device_tensor(variants)
    if not tensor:
        variants = np.asarray(variants)
    import torch
    if variants.dtype != (torch.float64 if tensor else np.float64):
        raise ValueError("float64 variants are needed (got %s)" % (variants.dtype,))
    shape = tuple(variants.shape)
    if len(shape) not in (4, 5) or min(shape[1:], default=0) < 1:
        raise ValueError("variants (K, X, Y, Z) or (K, X, Y, Z, C) are needed (got %s)" % (shape,))
    if not 1 <= shape[0] <= TTA_MAX_VARIANTS:
        raise ValueError("1 to %d variants are needed (got %d)" % (TTA_MAX_VARIANTS, shape[0]))
    if len(shape) == 5 and shape[4] > TTA_MAX_CHANNELS:
        raise ValueError("at most %d channels are supported (got %d)" % (TTA_MAX_CHANNELS, shape[4]))
    return variants, tensor


def _tta_agreement_host(stack, threshold, maps):
    """numpy in the operation order of fmri_tta_agreement_f64 (include/fmri_hip.h): the same bits, the entropy up to the two log2"""
    K = stack.shape[0]
    C = stack.shape[4] if stack.ndim == 5 else 1
    srt = np.sort(stack, axis=0)
    out = {"median": (srt[(K - 1) // 2] + srt[K // 2]) / 2.0}
    del srt
    if set(maps) & {"mean", "variance", "entropy"}:
        total = stack[0].copy()
        for k in range(1, K):
            total = total + stack[k]
        mu = total / float(K)
        if "mean" in maps:
            out["mean"] = mu
        if "variance" in maps:
            q = np.zeros_like(mu)
            for k in range(K):
                d = stack[k] - mu
                q = q + d * d
            out["variance"] = q / float(K)
        if "entropy" in maps:
            p = np.minimum(np.maximum(mu, 0.0), 1.0)
            inside = (p > 0.0) & (p < 1.0)
            pi = p[inside]
            qi = 1.0 - pi
            ent = np.zeros_like(mu)
            ent[inside] = -(pi * np.log2(pi) + qi * np.log2(qi))
            out["entropy"] = ent
    V = stack > threshold
    M = out["median"] > threshold
    if "disagreement" in maps:
        out["disagreement"] = (V != M[np.newaxis]).sum(axis=0).astype(np.float64) / float(K)
    Vc, Mc = V.reshape(K, -1, C), M.reshape(-1, C)
    counts = np.empty((C, 2 * K + 1), dtype=np.int64)
    counts[:, 0] = Mc.sum(axis=0)
    counts[:, 1:1 + K] = Vc.sum(axis=1).T
    counts[:, 1 + K:] = (Vc & Mc[np.newaxis]).sum(axis=1).T
    return out, counts


def _tta_agreement_device(stack, threshold, maps):
    """the device form on a float64 CUDA stack (K, X, Y, Z[, C]); one read-back: the counts"""
    from fmri_hip import ops
    C = int(stack.shape[4]) if stack.dim() == 5 else 1
    out = ops.tta_agreement_f64(stack.contiguous(), threshold, channels=C, maps=maps, counts=True)
    return out, out.pop("counts").cpu().numpy()


def tta_agreement(variants, threshold=0.5, *, maps=TTA_MAPS, device=None):
    """How far K test-time variants of one prediction agree, without a truth -> TTAAgreement.  `variants`: a list of K predictions or
    their stack, (K, X, Y, Z) or (K, X, Y, Z, C) with C independent sigmoid channels, float64: what `predict_flips` returns and what
    `predict_augment` stacks, numpy or CUDA tensors (tensors in, tensor maps out).  Voxel-wise: the median, and of `maps` the mean, the
    population variance, the binary entropy of the mean (bits) and the share of variants that disagree with the median's label
    (`> threshold`, the rule of `prediction_to_image`).  Per case and channel: the sizes of the consensus mask, of every variant's mask and
    of their intersections, and from them every variant's Dice with the consensus, their mean (the estimated Dice) and the coefficient
    of variation of the variants' volumes.  device: None / True / False as for `pipeline.Zoom`; on the device one kernel reads the stack
    once (`fmri_hip.ops.tta_agreement_f64`), on the host numpy does the same operations in the same order: the same bits, but for the
    entropy's log2."""
    maps = _checked_maps(maps)
    stack, tensor = _variants_stack(variants)
    if tensor:
        if device is not None and not device:
            raise ValueError("a device tensor cannot take the host form")
        out, counts = _tta_agreement_device(stack, threshold, maps)
        return TTAAgreement(out.pop("median"), out, counts, threshold)
    from .pipeline import _use_device
    if _use_device(stack[..., 0] if stack.ndim == 5 else stack, device):
        out, counts = _tta_agreement_device(_upload_f64(stack), threshold, maps)
        out = {name: _download(t) for name, t in out.items()}
    else:
        out, counts = _tta_agreement_host(stack, threshold, maps)
    return TTAAgreement(out.pop("median"), out, counts, threshold)


def _hip_rotate_ok():
    try:
        import torch
        from fmri_hip._lib import lib
        if not torch.cuda.is_available():
            return False
        lib()
        return True
    except Exception:
        return False


class _TTAVariant:
    """One random test-time variant of a volume: intensity window, mirror axes, optional x/y swap, in-plane rotation angle.
    `draw` consumes numpy's global RNG in the order the reference's loop does (two window draws, the angle, three mirror coins, the
    swap coin: reference prediction.py:34-42) - a seeded run therefore produces the reference's variants (tests/golden/augment_golden.*)."""
    __slots__ = ("lo", "hi", "angle", "mirror", "swap")

    @classmethod
    def draw(cls, vmin, vmax, jitter=0.10, max_angle=30):
        v = cls()
        span = vmax - vmin
        v.lo = vmin + jitter * np.random.uniform(-1, 1) * span
        v.hi = vmax + jitter * np.random.uniform(-1, 1) * span
        v.angle = np.random.uniform(-max_angle, max_angle)
        v.mirror = tuple(np.flatnonzero(np.random.choice([True, False], size=3)))
        v.swap = bool(np.random.choice([True, False]))
        return v

    @staticmethod
    def _rotate(vol, angle, order, reshape):
        """scipy.ndimage.rotate(vol, angle, order=order, reshape=reshape) - scipy's own arithmetic in float64, equal to 1e-12; a
        160x256x256 volume takes scipy 1-2 s per rotation, 64 rotations per predict_augment call.  FMRI_TTA_TORCH_ROTATE unset or
        'auto': the HIP kernels (fmri_hip.ops.rotate_f64) when a GPU and the library are there, else scipy; =1 forces the torch form
        (fetal_net.spline_rotate, on the GPU when there is one, else on the host), =0 scipy"""
        mode = os.environ.get("FMRI_TTA_TORCH_ROTATE", "auto")
        import torch
        if mode == "auto" and vol.ndim == 3 and vol.size > 0 and _hip_rotate_ok():
            from fmri_hip import ops
            dvol = torch.from_numpy(np.ascontiguousarray(vol, dtype=np.float64)).cuda()
            return ops.rotate_f64(dvol, angle, order=order, reshape=reshape).cpu().numpy()
        if mode == "0" or (mode == "auto" and not torch.cuda.is_available()) or vol.ndim != 3:
            from scipy import ndimage
            return ndimage.rotate(vol, angle, order=order, reshape=reshape)
        from .spline_rotate import rotate
        dev = "cuda" if torch.cuda.is_available() else "cpu"
        return rotate(torch.from_numpy(np.ascontiguousarray(vol, dtype=np.float64)).to(dev), angle, order=order, reshape=reshape).cpu().numpy()

    def forward(self, vol):
        """volume -> variant: window, mirror, swap, rotate (quadratic spline, shape kept)"""
        out = flip_it(contrast_augment(vol, self.lo, self.hi), self.mirror)
        if self.swap:
            out = np.swapaxes(out, 0, 1)
        return self._rotate(out, self.angle, 2, False)

    def inverse(self, pred):
        """prediction of the variant -> frame of the original volume.  The back-rotation keeps scipy's defaults (cubic spline,
        reshape=True), as the reference's does - the result can be larger than the input when angle != 0."""
        out = self._rotate(pred, -self.angle, 3, True)
        if self.swap:
            out = np.swapaxes(out, 0, 1)
        return flip_it(out, self.mirror)


def predict_augment(data, model, overlap_factor, patch_shape, num_augments=32, *, blend=None, blend_sigma_scale=DEFAULT_SIGMA_SCALE):
    """Random intensity / mirror / swap / rotation variants of the volume (reference prediction.py:25-62), each predicted patch-wise on
    the device tile loop and mapped back; the volume-sized spline rotations run on the device too (fetal_net.spline_rotate).  Like the
    reference, stacking succeeds only when all back-rotated predictions end up with one shape (num_augments = 1, or equal angles).
    blend / blend_sigma_scale: as for patch_wise_prediction, for every variant."""
    _blend_key(blend, blend_sigma_scale)
    vmin, vmax = data.min(), data.max()
    vol = data.squeeze()
    out = []
    for _ in range(num_augments):
        variant = _TTAVariant.draw(vmin, vmax)
        pred = patch_wise_prediction(model=model, data=variant.forward(vol)[np.newaxis], overlap_factor=overlap_factor,
                                     patch_shape=patch_shape, blend=blend, blend_sigma_scale=blend_sigma_scale).squeeze()
        out.append(variant.inverse(pred).squeeze())
    return np.stack(out, axis=0)


def run_validation_case(data_index, output_dir, model, data_file, training_modalities, patch_shape, overlap_factor=0,
                        permute=False, prev_truth_index=None, prev_truth_size=None, use_augmentations=False, *, output_label_map=False,
                        threshold=0.5, labels=None, postprocess_labels=None, blend=None, blend_sigma_scale=DEFAULT_SIGMA_SCALE):
    """Predict one case of an opened data file (any object with `.root.data[i]` / `.root.truth[i]`) and write
    data_<modality>.nii.gz, truth.nii.gz, prediction.nii.gz under output_dir (reference prediction.py:277-330).
    output_label_map (reference docstring :284-288): also write prediction_labels.nii.gz, the uint8 label map of the prediction
    (prediction_to_image's rules with `threshold` and `labels`).
    postprocess_labels: None, or a dict of `fetal_net.postprocess.postprocess_label_map` options (may be empty; `threshold` and `labels`
    above are its defaults): together with output_label_map, prediction_labels.nii.gz is then the cleaned label map of the prediction.
    blend / blend_sigma_scale: how overlapping tiles are combined, as for patch_wise_prediction (a case predicted whole has no tiles)."""
    from .utils.nifti import save_nifti
    _blend_key(blend, blend_sigma_scale)
    if not os.path.exists(output_dir):
        os.makedirs(output_dir)
    test_data = np.asarray([data_file.root.data[data_index]])
    test_truth_data = np.asarray([data_file.root.truth[data_index]]) if prev_truth_index is not None else None
    for i, modality in enumerate(training_modalities):
        save_nifti(test_data[i], os.path.join(output_dir, "data_{0}.nii.gz".format(modality)))
    save_nifti(np.asarray(data_file.root.truth[data_index]), os.path.join(output_dir, "truth.nii.gz"))
    if tuple(patch_shape) == tuple(test_data.shape[-3:]):
        prediction = predict(model, test_data[:, np.newaxis] if test_data.ndim == 4 else test_data, permute=permute)
        mode = "whole"
    elif use_augmentations:
        mode = "augment"
        prediction = predict_augment(data=test_data, model=model, overlap_factor=overlap_factor, patch_shape=patch_shape, blend=blend,
                                     blend_sigma_scale=blend_sigma_scale)
    else:
        prediction = patch_wise_prediction(model=model, data=test_data, overlap_factor=overlap_factor, patch_shape=patch_shape,
                                           truth_data=test_truth_data, prev_truth_index=prev_truth_index,
                                           prev_truth_size=prev_truth_size, blend=blend, blend_sigma_scale=blend_sigma_scale)[np.newaxis]
        mode = "patches"
    if output_label_map:
        if mode == "whole":                                   # (1, L, X, Y, Z) as the model gives it
            channels_first = prediction
        elif mode == "augment":                               # the stack of single-channel variants: their mean
            channels_first = np.mean(prediction, axis=0)[np.newaxis, np.newaxis]
        else:                                                 # (1, X, Y, Z, C)
            channels_first = np.moveaxis(prediction, -1, 1)
        if postprocess_labels is not None:
            from .postprocess import postprocess_label_map
            options = dict(dict(threshold=threshold, labels=labels), **postprocess_labels)
            label_data = postprocess_label_map(np.ascontiguousarray(np.moveaxis(np.asarray(channels_first, dtype=np.float64)[0], 0, -1)),
                                               **options)
        else:
            label_data = np.asarray(prediction_to_image(channels_first, label_map=True, threshold=threshold,
                                                        labels=labels)).astype(np.uint8)
        save_nifti(label_data, os.path.join(output_dir, "prediction_labels.nii.gz"))
    prediction = prediction.squeeze()
    filename = os.path.join(output_dir, "prediction.nii.gz")
    save_nifti(prediction, filename)
    return filename


def run_validation_cases(validation_keys_file, model_file, training_modalities, hdf5_file, patch_shape, output_dir=".",
                         overlap_factor=0, permute=False, prev_truth_index=None, prev_truth_size=None, use_augmentations=False,
                         data_file=None, model=None, *, output_label_map=False, threshold=0.5, labels=None, postprocess_labels=None,
                         blend=None, blend_sigma_scale=DEFAULT_SIGMA_SCALE):
    """reference prediction.py:333-351.  `hdf5_file` is opened with `fetal_net.data.open_data_file` (plain-layout files through libhdf5,
    PyTables files through PyTables when installed); callers may instead pass an already opened duck-typed `data_file` (and a `model`).
    The keyword-only arguments are run_validation_case's and go to every case."""
    import glob
    import pickle
    from .training import load_old_model
    with open(validation_keys_file, "rb") as f:
        validation_indices = pickle.load(f)
    if model is None:
        candidates = glob.glob(model_file + '*.h5')
        model = load_old_model(max(candidates, key=os.path.getmtime))      # newest checkpoint (reference fetal/utils.py:42-43)
    own = data_file is None
    if own:
        from .data import open_data_file
        data_file = open_data_file(hdf5_file, "r")
    has_ids = 'subject_ids' in data_file.root

    def case_dir(index):
        label = data_file.root.subject_ids[index].decode('utf-8') if has_ids else "validation_case_{}".format(index)
        return os.path.join(output_dir, label)

    try:
        return [run_validation_case(data_index=i, output_dir=case_dir(i), model=model, data_file=data_file,
                                    training_modalities=training_modalities, overlap_factor=overlap_factor, permute=permute,
                                    patch_shape=patch_shape, prev_truth_index=prev_truth_index, prev_truth_size=prev_truth_size,
                                    use_augmentations=use_augmentations, output_label_map=output_label_map, threshold=threshold,
                                    labels=labels, postprocess_labels=postprocess_labels, blend=blend,
                                    blend_sigma_scale=blend_sigma_scale) for i in validation_indices]
    finally:
        if own:
            data_file.close()
