"""Binary clean-up of a probability volume (same entry points and defaults as reference fetal_net/postprocess.py:7-19): gaussian
smoothing, threshold, hole filling, largest connected component.

`postprocess_prediction` cleans one volume into a boolean mask.  `postprocess_label_map` cleans every channel of a channels-last
prediction (X, Y, Z, L) by the same four steps and merges the cleaned masks into one uint8 label map.

The host form of both is the definition: scipy.ndimage per channel (what the reference runs), numpy for the merge.  When a GPU and the
HIP library are there and the input is float64, i.e. the output of `patch_wise_prediction`, both run the one device implementation of
csrc/postprocess.hip instead: the L masks of a voxel are the low bits of one uint32 word, and hole filling and the component search
work on all channels at once (`fmri_correlate1d_cl_f64`, `fmri_threshold_bits_f64`, `fmri_fill_holes_bits_step`,
`fmri_largest_components_bits_step`, `fmri_label_map_bits`); a single volume is that chain at L = 1.  The gaussian sums in scipy's own
order in fp64, the rest is integer work, so host and device produce the same mask voxel for voxel and the same label bytes
(tests/test_gpu_postprocess.py, tests/test_gpu_postprocess_labels.py).  `device=` forces one or the other."""
import numpy as np
from scipy import ndimage


def get_main_connected_component(data):
    """boolean mask of the largest 6-connected component of `data` (all False when there is none)"""
    components, count = ndimage.label(data)
    if count == 0:
        return np.zeros(components.shape, dtype=bool)          # the reference raises on the argmax of an empty list here
    voxels_per_component = np.bincount(components.ravel(), minlength=count + 1)[1:]
    return components == 1 + int(np.argmax(voxels_per_component))


def _device_ok(pred, ndims=(3,)):
    if not (isinstance(pred, np.ndarray) and pred.ndim in ndims and pred.dtype == np.float64):
        return False
    try:
        import torch
        from fmri_hip._lib import lib
        if not torch.cuda.is_available():
            return False
        lib()
        return True
    except Exception:
        return False


def postprocess_prediction(pred, gaussian_std=1, threshold=0.5, fill_holes=True, connected_component=True, device=None):
    """device=None: the device path when it applies (see the module header), else scipy; True / False force one"""
    if device is None:
        device = _device_ok(pred)
    if device:
        return _label_map_on_device(pred, 1, gaussian_std, threshold, fill_holes, connected_component, [1], False) != 0
    mask = ndimage.gaussian_filter(pred, gaussian_std) > threshold
    steps = []
    if fill_holes:
        steps.append(ndimage.binary_fill_holes)
    if connected_component:
        steps.append(get_main_connected_component)
    for step in steps:
        mask = step(mask)
    return mask


MAX_LABELS = 32          # fmri_hip.ops.MAX_LABELS: the channels of a voxel are the bits of one word


def _label_bytes(n_labels, labels):
    """fmri_hip.ops.label_values' rule without the device package: n_labels distinct integers in 1..255, default 1..n_labels"""
    given = list(range(1, n_labels + 1)) if labels is None else list(labels)
    try:
        values = [int(v) for v in given]
    except (TypeError, ValueError):
        values = None
    if values is None or len(values) != n_labels or any(v != g or not 1 <= v <= 255 for v, g in zip(values, given)) \
            or len(set(values)) != len(values):
        raise ValueError("labels %r: %d distinct integers in 1..255, one per label channel" % (labels, n_labels))
    return values


def postprocess_label_map(prediction, gaussian_std=1, threshold=0.5, fill_holes=True, connected_component=True, labels=None, device=None):
    """uint8 label map (X, Y, Z) of a float64 prediction (X, Y, Z, L), channels last as `patch_wise_prediction` returns it ((X, Y, Z)
    means L = 1), 1 <= L <= 32.  With S_l = gaussian_filter(prediction[..., l], gaussian_std) and M_l = postprocess_prediction(
    prediction[..., l], gaussian_std, threshold, fill_holes, connected_component): a voxel in no M_l gets 0, any other voxel gets
    labels[l*], l* = the argmax of S_l over the channels whose M_l holds the voxel, ties to the lowest channel.  `labels`: L distinct
    values in 1..255 (default 1..L), anything else is a ValueError.

    - A voxel that only hole filling put into M_l has S_l <= threshold and still competes with its S_l.
    - The test is "> threshold" per channel, as in postprocess_prediction; get_prediction_labels keeps a maximum EQUAL to the threshold,
      so the two differ at equality.
    - For L = 1 the result is labels[0] * postprocess_prediction(...).
    NaN input is not specified.

    device=None: the device path when a GPU and the library are there and the input is a float64 array of 3 or 4 dimensions, else the
    host path; True / False force one.  A float64 CUDA tensor in gives a uint8 CUDA tensor out, with no round trip."""
    is_tensor = not isinstance(prediction, np.ndarray) and hasattr(prediction, "is_cuda")
    if not is_tensor:
        prediction = np.asarray(prediction)
    if prediction.ndim not in (3, 4):
        raise ValueError("prediction: (X, Y, Z, L) or (X, Y, Z), got shape %r" % (tuple(prediction.shape),))
    n_labels = 1 if prediction.ndim == 3 else int(prediction.shape[3])
    if not 1 <= n_labels <= MAX_LABELS:
        raise ValueError("prediction: 1 to %d label channels, got %d" % (MAX_LABELS, n_labels))
    values = _label_bytes(n_labels, labels)
    if device is None:
        device = bool(prediction.is_cuda) if is_tensor else _device_ok(prediction, (3, 4))
    if device:
        return _label_map_on_device(prediction, n_labels, gaussian_std, threshold, fill_holes, connected_component, values, is_tensor)
    if is_tensor:
        prediction = prediction.cpu().numpy()
    pred4 = prediction.reshape(prediction.shape[:3] + (n_labels,))
    smoothed = np.stack([ndimage.gaussian_filter(pred4[..., l], gaussian_std) for l in range(n_labels)])
    masks = np.stack([postprocess_prediction(pred4[..., l], gaussian_std, threshold, fill_holes, connected_component, device=False)
                      for l in range(n_labels)])
    index = np.argmax(np.where(masks, smoothed, -np.inf), axis=0) + 1          # np.argmax: the first of equal maxima
    index[~masks.any(axis=0)] = 0
    return np.asarray([0] + values, dtype=np.uint8)[index]


def _label_map_on_device(pred, n_labels, gaussian_std, threshold, fill_holes, connected_component, values, keep_on_device):
    import torch
    from fmri_hip import ops
    vol = pred if isinstance(pred, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(pred, dtype=np.float64)).cuda()
    vol = vol.contiguous().reshape(tuple(vol.shape[:3]) + (n_labels,))
    smoothed = ops.gaussian_filter_channels_f64(vol, gaussian_std)
    words = ops.threshold_bits_f64(smoothed, threshold)
    if fill_holes:
        words = ops.binary_fill_holes_bits(words, n_labels)
    if connected_component:
        words = ops.largest_components_bits(words, n_labels)
    out = ops.label_map_from_bits(words, smoothed, values)
    return out if keep_on_device else out.cpu().numpy()
