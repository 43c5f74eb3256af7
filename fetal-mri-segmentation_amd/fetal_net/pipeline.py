"""Whole-volume, optionally two-stage prediction - the behaviour of the reference's production entry point
(reference prod/predict_nifti2.py:25-160) - organised as data instead of as a script:

    Stage          what one model needs: the model, its patch geometry, intensity preparation, test-time augmentation, tile overlap
    Resampling     a geometric change of the volume together with its inverse for the prediction (zoom back, crop back)
    VolumePipeline a first Stage over the whole volume and, optionally, a second Stage over the padded bounding box of the first mask

Each resampling applied on the way in is pushed on a stack and undone in reverse on the way out, so the prediction always comes back on
the voxel grid of the input.  On the device run the model work (the tile loop behind `patch_wise_prediction`, the TTA variants, the
mask clean-up when `postprocess_prediction` takes its device path) and, when a GPU and the HIP library are there, the volume-sized
arithmetic around it: the spline zoom of `Zoom` in both directions, the median over the TTA variants (`fmri_hip.ops.zoom_f64`,
`median_stack_f64`, tests/test_gpu_resample.py) and the intensity preparation in front of the model - the percentile window, the named
`preproc` filter of `fetal_net.preprocess` and the z-scoring (`fmri_hip.ops.window_intensities_f64`, `laplace_f64`,
`gaussian_gradient_magnitude_f64`, `norm_minmax_f64`, `normalize_f64`, tests/test_gpu_intensity.py): scipy's and numpy's own arithmetic
in float64, so host and device give the same values.  `Stage.intensities` uploads the volume once, runs window -> scaling zoom ->
filter -> z-score on the device tensor and downloads once.  With a model that has the device tile loop the first stage is ONE chain on
one tensor - resolution zoom, intensities, border, the tile loop of every flip variant, their median, crop, zoom back
(`VolumePipeline._run_first_resident`, `Stage._infer_resident`): one upload, one download each for what the model saw and for its
prediction, and a float64 CUDA tensor stays one.  Elsewhere (a foreign model, a caller's own `preproc`, `augment='all'`, `device=False`)
the calls upload their input and download their result, and border and crop are host passes; the second stage's crop and paste always
are.  File I/O is the caller's (`fetal_net.utils.nifti`).  `predict_volume(...)` keeps the keyword
surface of the reference's `main()` for callers that want the one-call form.
"""
import numpy as np
from scipy import ndimage

from . import preprocess
from .postprocess import _device_ok, postprocess_prediction
from . import prediction
from .prediction import patch_wise_prediction, predict_augment, predict_flips
from .utils.cut_relevant_areas import check_bounding_box, find_bounding_box

ROI_PADDING = (16, 16, 8)          # margin around the first-stage mask (reference predict_nifti2.py:31)
CONTEXT_MARGIN = 3                 # voxels of minimum-valued border the first model sees around the volume (reference :131)


# ------------------------------------------------------------------------------------------------------------ intensity preparation
def _wants_device(data, device):
    """the `device=` rule of fetal_net.preprocess: a CUDA tensor stays on the device; None = a float64 3-D ndarray with a GPU and the
    library there"""
    if preprocess._is_device_tensor(data):
        if device is not None and not device:
            raise ValueError("a device tensor cannot take the host form")
        return True
    return _device_ok(data) if device is None else bool(device)


def window_intensities_data(data, min_percent=1, max_percent=99, out_min=0.0, out_max=255.0, device=None):
    """SimpleITK IntensityWindowing(image, p_lo, p_hi) restated (reference fetal/preprocess.py:50-55): the [p_lo, p_hi] percentile window
    is mapped linearly onto [0, 255], values outside it are clamped.  device: as in `fetal_net.preprocess` (None / True / False; a
    float64 CUDA tensor stays one) - the device form selects the percentiles' order statistics and maps on the GPU, same values."""
    if _wants_device(data, device):
        from fmri_hip import ops
        return preprocess._dispatch(data, True, lambda t: ops.window_intensities_f64(t, min_percent, max_percent, out_min, out_max), None)
    data = np.asarray(data, dtype=np.float64)
    lo, hi = np.percentile(data, min_percent), np.percentile(data, max_percent)
    if hi == lo:
        return np.full(data.shape, out_min)
    return (np.clip(data, lo, hi) - lo) * ((out_max - out_min) / (hi - lo)) + out_min


def normalize_data(data, mean, std, device=None):
    """reference fetal_net/normalize.py:66-69.  device: a float64 CUDA tensor stays one; True = the device form for an array.  None keeps
    an array on the host: one subtraction and one division per voxel take less time there (13 ms at 160x256x256) than the transfer of
    the volume to the device and back (16-24 ms end to end, profiles/r06_intensity_timing.log) - the device form pays inside a chain
    that is already on the device (`Stage.intensities`)."""
    if preprocess._is_device_tensor(data) or device:
        from fmri_hip import ops
        return preprocess._dispatch(data, True, lambda t: ops.normalize_f64(t, mean, std), None)
    return (np.asarray(data, dtype=np.float64) - mean) / std


INTENSITY_METHODS = {"window_1_99": window_intensities_data}


# ------------------------------------------------------------------------------------------------------------------ building blocks
class Resampling(object):
    """a change of the sampling grid and how a prediction made on the new grid returns to the old one"""

    def forward(self, vol):
        raise NotImplementedError

    def backward(self, pred):
        raise NotImplementedError


def _use_device(arr, device):
    """the `device=` convention of postprocess_prediction for arrays with three trailing spatial axes: None = the device path when a
    GPU and the library are there and the array is float64; True / False force one"""
    if device is None:
        return isinstance(arr, np.ndarray) and arr.ndim >= 3 and arr.size > 0 and _device_ok(arr[(0,) * (arr.ndim - 3)])
    return bool(device)


def _on_device(fn, arr):
    import torch
    return fn(torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float64)).cuda()).cpu().numpy()


def median_of_variants(variants, device=None):
    """np.median(variants, axis=0) of a stack [K, X, Y, Z]; on the device (same values) for K <= 64 under the `device=` rule of Zoom"""
    variants = np.asarray(variants)
    if variants.ndim == 4 and 1 <= variants.shape[0] <= 64 and _use_device(variants, device):
        from fmri_hip import ops
        return _on_device(ops.median_stack_f64, variants)
    return np.median(variants, axis=0)


class Zoom(Resampling):
    """scipy zoom by per-axis factors; predictions return with `order_back` (0 for the model-specific scaling, 1 for the resolution change,
    as the reference does at predict_nifti2.py:139-143).  device=None: `fmri_hip.ops.zoom_f64` (scipy's arithmetic on the device) when a
    GPU and the library are there and the array is float64 with three trailing spatial axes, else scipy; True / False force one."""

    def __init__(self, factors, order_back, device=None):
        self.factors = [float(f) for f in np.broadcast_to(factors, (3,))]
        self.order_back = order_back
        self.device = device

    def forward(self, vol):
        if preprocess._is_device_tensor(vol):
            from fmri_hip import ops
            return ops.zoom_f64(vol, self.factors, order=3)
        if np.ndim(vol) == 3 and _use_device(vol, self.device):
            from fmri_hip import ops
            return _on_device(lambda v: ops.zoom_f64(v, self.factors, order=3), vol)
        return ndimage.zoom(vol, self.factors)

    def backward(self, pred):
        # leading axes (a stack of TTA variants) are left alone
        back = [1.0 / f for f in self.factors]
        if preprocess._is_device_tensor(pred):
            import torch
            from fmri_hip import ops
            out = [ops.zoom_f64(one, back, order=self.order_back) for one in pred.reshape((-1,) + tuple(pred.shape[-3:]))]
            return out[0] if pred.dim() == 3 else torch.stack(out).reshape(tuple(pred.shape[:-3]) + tuple(out[0].shape))
        if _use_device(pred, self.device):
            from fmri_hip import ops
            flat = pred.reshape((-1,) + pred.shape[-3:])
            out = [_on_device(lambda v: ops.zoom_f64(v, back, order=self.order_back), one) for one in flat]
            return np.stack(out).reshape(pred.shape[:-3] + out[0].shape)
        lead = [1.0] * (pred.ndim - 3)
        return ndimage.zoom(pred, lead + back, order=self.order_back)


class Border(Resampling):
    """a constant border of the volume's minimum on the way in, cropped off the prediction on the way out"""

    def __init__(self, width):
        self.width = int(width)

    def forward(self, vol):
        if preprocess._is_device_tensor(vol):                 # a float64 CUDA volume stays one: fmri_minmax_f64, fmri_volume_pad_flip
            return self._resized(vol, self.width, minimum_fill=True)
        return np.pad(vol, self.width, mode="constant", constant_values=vol.min())

    def backward(self, pred):
        w = self.width
        if preprocess._is_device_tensor(pred):
            return self._resized(pred, -w) if w else pred
        return pred[(Ellipsis,) + (slice(w, -w),) * 3] if w else pred

    @staticmethod
    def _resized(t, w, minimum_fill=False):
        """the three trailing axes of a float64 CUDA tensor grown by w voxels of the volume's minimum on every side (w < 0: cropped)"""
        import torch
        from fmri_hip import ops
        t = t.contiguous()
        fill = ops.minmax_f64(t)[0] if minimum_fill else 0.0
        out = torch.empty(tuple(t.shape[:-3]) + tuple(int(n) + 2 * w for n in t.shape[-3:]), dtype=t.dtype, device=t.device)
        for src, dst in zip(t.reshape((-1,) + tuple(t.shape[-3:])), out.reshape((-1,) + tuple(out.shape[-3:]))):
            ops.volume_pad_flip(src, dst, (w, w, w), 0, fill)
        return out


class Box(Resampling):
    """crop to [start, end) of a volume of `shape`; predictions are pasted back into zeros"""

    def __init__(self, start, end, shape):
        self.start, self.end, self.shape = np.asarray(start), np.asarray(end), tuple(shape)

    def forward(self, vol):
        return vol[tuple(slice(a, b) for a, b in zip(self.start, self.end))]

    def backward(self, pred):
        room = [(int(a), int(s - b)) for a, b, s in zip(self.start, self.end, self.shape)]
        return np.pad(pred, [(0, 0)] * (pred.ndim - 3) + room, mode="constant", constant_values=0)


class Stage(object):
    """One model of the pipeline and everything that belongs to it.  `config`: the model's experiment config (`patch_shape`,
    `patch_depth`, optional `scale_data`, optional `preproc`: a callable, or the name of a filter in `fetal_net.preprocess` as in the
    reference's configs); `intensity`: None or a key of INTENSITY_METHODS; `norm`: None or {'mean', 'std'}; `augment`: None | 'flip' (the
    8 flips) | 'all' (`n_augment` random variants); `device`: where the stage's intensity preparation, its zoom and the median over its
    variants run (None / True / False as for `Zoom`); `blend` / `blend_sigma_scale` (keyword-only): how overlapping tiles are combined, None
    (every tile counts the same) or 'gaussian', as for `prediction.patch_wise_prediction`; `threshold` (keyword-only): the label rule
    `> threshold` that `infer(..., agreement=True)` counts the variants' masks by."""

    def __init__(self, model, config, intensity=None, norm=None, augment=None, n_augment=0, overlap=0.9, device=None, *, blend=None,
                 blend_sigma_scale=prediction.DEFAULT_SIGMA_SCALE, threshold=0.5):
        if intensity is not None and intensity not in INTENSITY_METHODS:
            raise Exception("Unknown preprocess: {}".format(intensity))
        if augment not in (None, "flip", "all"):
            raise ValueError("Unknown augmentation {}".format(augment))
        pre = config.get("preproc")
        self.preproc, self.preproc_named = pre, False
        if isinstance(pre, str) and pre in preprocess.__all__:
            self.preproc, self.preproc_named = getattr(preprocess, pre), True       # reference predict_nifti2.py:67-69
        elif pre is not None and not callable(pre):
            raise TypeError("config['preproc'] must be a callable or one of %s of fetal_net.preprocess (got %r)" % (preprocess.__all__, pre))
        self.model, self.config, self.intensity, self.norm = model, config, intensity, norm
        self.augment, self.n_augment, self.overlap, self.device = augment, n_augment, overlap, device
        prediction._blend_key(blend, blend_sigma_scale)
        self.blend = dict(blend=blend, blend_sigma_scale=blend_sigma_scale)
        self.threshold = float(threshold)

    @property
    def patch(self):
        return list(self.config["patch_shape"]) + [self.config["patch_depth"]]

    def intensities(self, vol, resamplings=None):
        """windowing -> the model-specific scaling (recorded in `resamplings`) -> the config's own hook -> z-scoring, in the reference's
        order.  Under the device rule (a float64 volume [X,Y,Z]) the steps run on ONE device tensor: one upload, one download; a caller's
        own callable is handed a numpy array in between, as on the host.  A float64 CUDA tensor [X,Y,Z] stays one."""
        if preprocess._is_device_tensor(vol):
            scale = self.config.get("scale_data") if resamplings is not None else None
            pre = self.preproc if resamplings is not None else None
            if pre is not None and not self.preproc_named:
                raise TypeError("a caller's own preproc callable takes host volumes (got a device tensor)")
            norm = self.norm if self.norm is not None and any(self.norm.values()) else None
            return self._intensities_on_device(vol, resamplings, scale, pre, norm)
        scale = self.config.get("scale_data") if resamplings is not None else None
        pre = self.preproc if resamplings is not None else None
        norm = self.norm if self.norm is not None and any(self.norm.values()) else None
        # the z-score alone is quicker on the host than the volume's round trip to the device (normalize_data): under the default rule
        # the chain goes to the device for the steps that pay there
        work = self.intensity is not None or scale is not None or (pre is not None and self.preproc_named) or (
            self.device and (pre is not None or norm is not None))
        if work and isinstance(vol, np.ndarray) and vol.ndim == 3 and vol.dtype == np.float64 and vol.size and _use_device(vol, self.device):
            return self._intensities_on_device(vol, resamplings, scale, pre, norm)
        if self.intensity is not None:
            vol = INTENSITY_METHODS[self.intensity](vol, device=False)
        if scale is not None:
            step = Zoom(scale, order_back=0, device=self.device)
            resamplings.append(step)
            vol = step.forward(vol)
        if pre is not None:
            vol = pre(vol, device=False) if self.preproc_named else pre(vol)
        if norm is not None:
            vol = normalize_data(vol, mean=norm["mean"], std=norm["std"], device=False)
        return vol

    def _intensities_on_device(self, vol, resamplings, scale, pre, norm):
        import torch
        from fmri_hip import ops
        keep = preprocess._is_device_tensor(vol)               # the caller's tensor in, the tensor this chain ends with out
        t = vol if keep else torch.from_numpy(np.ascontiguousarray(vol)).cuda()
        if self.intensity is not None:
            t = INTENSITY_METHODS[self.intensity](t)
        if scale is not None:
            step = Zoom(scale, order_back=0, device=self.device)
            resamplings.append(step)
            t = ops.zoom_f64(t, step.factors, order=3)
        if pre is not None and self.preproc_named:
            t = pre(t)
        elif pre is not None:
            back = np.asarray(pre(t.cpu().numpy()))
            if norm is None or not (back.ndim == 3 and back.dtype == np.float64 and back.size):
                return back if norm is None else normalize_data(back, mean=norm["mean"], std=norm["std"], device=False)
            t = torch.from_numpy(np.ascontiguousarray(back)).cuda()
        if norm is not None:
            t = ops.normalize_f64(t, norm["mean"], norm["std"])
        return t if keep else t.cpu().numpy()

    def infer(self, vol, keep_variants=False, agreement=False):
        """probabilities of `vol` [X,Y,Z]: tiled prediction, or the median over the stage's test-time augmentation variants.  With a
        model that has the device tile loop and `augment` None or 'flip' the volume goes up once, the variants are mirrored, tiled and
        mirrored back on the device, their median is taken on the resident stack and the result comes down once (`_infer_resident`); a
        float64 CUDA tensor stays one.  'all' and foreign models take `_infer_host`.
        agreement=True -> (that result, the `prediction.TTAAgreement` of the variants: uncertainty maps, set sizes, estimated Dice).  On
        the resident route ONE kernel (`ops.tta_agreement_f64`) then reads the stack in place of the median kernel and writes the median
        with the maps; with keep_variants=True it is taken from the very stack that is returned.  One variant has nothing to agree
        with: augment=None raises ValueError."""
        if agreement and self.augment is None:
            raise ValueError("agreement=True needs test-time variants: augment='flip' or 'all' (got None)")
        why = self._resident_refusal(vol)
        if why is None:
            return self._infer_resident(vol, keep_variants, agreement)
        if preprocess._is_device_tensor(vol):
            raise TypeError("Stage.infer of a device tensor needs the resident tile loop: " + why)
        return self._infer_host(vol, keep_variants, agreement)

    def _resident_refusal(self, vol):
        """None when `vol` takes the resident route, else the reason it does not"""
        if self.augment == "all":
            return "augment='all' rotates its variants on the host route"
        why = prediction._device_tile_loop_refusal(self.model)
        if why is not None:
            return why
        if preprocess._is_device_tensor(vol):
            import torch
            ok = vol.dtype == torch.float64 and vol.dim() == 3 and min(vol.shape) > 1
        else:
            ok = isinstance(vol, np.ndarray) and vol.dtype == np.float64 and vol.ndim == 3 and min(vol.shape) > 1
            if ok and not (prediction.resident_tta_default() and _use_device(vol, self.device)):
                return "the host route is asked for (device=False, FMRI_TTA_RESIDENT=0) or no GPU is there"
        return None if ok else "a float64 volume [X,Y,Z] with every extent above 1 is needed"

    def _infer_resident(self, vol, keep_variants, agreement=False):
        from fmri_hip import ops
        tensor = preprocess._is_device_tensor(vol)
        t = vol.contiguous() if tensor else prediction._upload_f64(vol)
        variants = prediction._flip_variants(tuple(t.shape)) if self.augment == "flip" else [(0, 0)]
        stack = prediction._resident_flip_stack(t, self.model, self.overlap, self.patch, variants, **self.blend)
        if stack.shape[-1] == 1:
            stack = stack[..., 0]
        if self.augment != "flip":
            out = stack[0]
        elif agreement:
            maps, counts = prediction._tta_agreement_device(stack, self.threshold, prediction.TTA_MAPS)
            if not tensor:
                maps = {name: prediction._download(m) for name, m in maps.items()}
            agreed = prediction.TTAAgreement(maps.pop("median"), maps, counts, self.threshold)
            if not keep_variants:
                return agreed.median, agreed
            return (stack if tensor else prediction._download(stack)), agreed
        else:
            out = stack if keep_variants else ops.median_stack_f64(stack)
        return out if tensor else prediction._download(out)

    def _infer_host(self, vol, keep_variants=False, agreement=False):
        """the route of foreign models and of augment='all': every variant a patch_wise_prediction of a host volume, the stack of their
        results reduced by `median_of_variants` (also the other arm of tools/bench_tta.py); agreement=True: `prediction.tta_agreement`
        of that stack under the stage's `device=` rule, its median the result"""
        if self.augment == "all":
            variants = predict_augment(vol, model=self.model, overlap_factor=self.overlap, num_augments=self.n_augment, patch_shape=self.patch,
                                       **self.blend)
        elif self.augment == "flip":
            variants = np.stack(prediction._predict_flips_host(vol, model=self.model, overlap_factor=self.overlap, config=self.config,
                                                               **self.blend))
        else:
            return np.asarray(patch_wise_prediction(model=self.model, data=vol[np.newaxis], overlap_factor=self.overlap,
                                                    patch_shape=self.patch, **self.blend)).squeeze()
        if agreement:
            variants = np.asarray(variants)
            agreed = prediction.tta_agreement(variants, self.threshold, device=self.device)
            return np.asarray(variants if keep_variants else agreed.median).squeeze(), agreed
        return np.asarray(variants if keep_variants else median_of_variants(variants, self.device)).squeeze()


def _undo(pred, resamplings):
    for step in reversed(resamplings):
        pred = step.backward(pred)
    return pred


class VolumePipeline(object):
    """first Stage on the whole volume; optional second Stage on the region of interest the first one finds.  `resolution`: (xy, z) zoom
    applied before the first model and undone (order 1) on its prediction; `mask_options`: arguments of the clean-up that turns the first
    prediction into the region-of-interest mask; `device`: where the resolution zoom runs (None / True / False as for `Zoom`)."""

    def __init__(self, first, second=None, resolution=(1.0, 1.0), roi_padding=ROI_PADDING, mask_options=None, device=None):
        self.first, self.second, self.device = first, second, device
        self.resolution = tuple(1.0 if r is None else float(r) for r in resolution)
        self.roi_padding = roi_padding
        self.mask_options = dict(gaussian_std=0.5, threshold=0.5) if mask_options is None else dict(mask_options)

    def run_first(self, volume, keep_variants=False, agreement=False):
        """-> (what the first model saw before its border, its prediction on the input grid); agreement=True adds a third element, the
        `prediction.TTAAgreement` of the first stage's variants: its maps brought back to the input grid by the steps that bring the
        prediction back (crop, zoom back), its counts and scores as taken on the grid the model saw"""
        if self._chain_on_device(volume):
            return self._run_first_resident(volume, keep_variants, agreement)
        steps = []
        vol = volume
        xy, z = self.resolution
        if (xy, z) != (1.0, 1.0):
            steps.append(Zoom([xy, xy, z], order_back=1, device=self.device))
            vol = steps[-1].forward(vol)
        vol = self.first.intensities(vol, steps)
        seen = vol
        steps.append(Border(CONTEXT_MARGIN))
        if agreement:
            pred, agreed = self.first.infer(steps[-1].forward(vol), keep_variants, True)
            return seen, _undo(pred, steps), agreed.with_maps(lambda m: _undo(m, steps))
        pred = self.first.infer(steps[-1].forward(vol), keep_variants)
        return seen, _undo(pred, steps)

    def _chain_on_device(self, volume):
        """whether run_first's steps all have a device form for `volume`: then they run on ONE tensor"""
        first = self.first
        if preprocess._is_device_tensor(volume):
            return True
        if not (isinstance(volume, np.ndarray) and volume.ndim == 3 and volume.dtype == np.float64 and volume.size):
            return False
        if first.preproc is not None and not first.preproc_named:
            return False                                      # a caller's own callable works on host arrays
        if not (_use_device(volume, self.device) and _use_device(volume, first.device) and prediction.resident_tta_default()):
            return False
        if first.augment == "all" or prediction._device_tile_loop_refusal(first.model) is not None:
            return False
        out_shape = first.model.output_shape                  # (Border.backward crops the three LAST axes: one label, squeezed away)
        return int(out_shape[1] if prediction._is3d(first.model) else out_shape[-1]) == 1

    def _run_first_resident(self, volume, keep_variants, agreement=False):
        """run_first on one device tensor: resolution zoom, intensities, border, tile loop and variants, crop, zoom back - one upload,
        and one download each for what the model saw and for its prediction (a CUDA tensor in gives CUDA tensors out)"""
        tensor = preprocess._is_device_tensor(volume)
        t = volume if tensor else prediction._upload_f64(volume)
        steps = []
        xy, z = self.resolution
        if (xy, z) != (1.0, 1.0):
            steps.append(Zoom([xy, xy, z], order_back=1, device=self.device))
            t = steps[-1].forward(t)
        seen = self.first.intensities(t, steps)
        steps.append(Border(CONTEXT_MARGIN))
        down = (lambda m: m) if tensor else prediction._download
        if agreement:
            pred, agreed = self.first.infer(steps[-1].forward(seen), keep_variants, True)
            return down(seen), down(_undo(pred, steps)), agreed.with_maps(lambda m: down(_undo(m, steps)))
        pred = _undo(self.first.infer(steps[-1].forward(seen), keep_variants), steps)
        return (seen, pred) if tensor else (prediction._download(seen), prediction._download(pred))

    def region_of_interest(self, mask):
        lo, hi = find_bounding_box(mask)
        check_bounding_box(mask, lo, hi)
        if self.roi_padding is not None:
            lo = np.maximum(lo - np.asarray(self.roi_padding), 0)
            hi = np.minimum(hi + np.asarray(self.roi_padding), np.asarray(mask).shape)
        return Box(lo, hi, np.asarray(mask).shape)

    def run_second(self, volume, mask, keep_variants=False, agreement=False):
        """the second model on the box around `mask`, cut from the ORIGINAL volume and prepared with the second stage's own parameters
        (no scaling hook at this stage, as in the reference); zero outside the box.  agreement=True -> (that, the second stage's
        `prediction.TTAAgreement`): its maps pasted into zeros like the prediction, its counts and scores those of the box"""
        box = self.region_of_interest(mask)
        roi = self.second.intensities(box.forward(np.asarray(volume, dtype=np.float64)))
        if agreement:
            pred, agreed = self.second.infer(roi, keep_variants, True)
            return box.backward(pred), agreed.with_maps(box.backward)
        return box.backward(self.second.infer(roi, keep_variants))

    def __call__(self, volume, keep_variants=False, agreement=False):
        """-> {'data', 'prediction'[, 'mask', 'prediction_roi']}; agreement=True adds 'agreement' (and 'agreement_roi' with a second
        stage): the `prediction.TTAAgreement` of each stage's variants, see `run_first` / `run_second`.  A float64 CUDA volume takes the
        one-stage pipeline (tensors in, tensors out); the second stage's crop and paste are host passes"""
        if preprocess._is_device_tensor(volume):
            if self.second is not None:
                raise TypeError("a device tensor takes a one-stage pipeline: the second stage crops and pastes on the host")
            volume = volume.squeeze()
        else:
            volume = np.asarray(volume, dtype=np.float64).squeeze()
        if agreement:
            seen, pred, agreed = self.run_first(volume, keep_variants, True)
            out = {"data": seen, "prediction": pred, "agreement": agreed}
        else:
            seen, pred = self.run_first(volume, keep_variants)
            out = {"data": seen, "prediction": pred}
        if self.second is not None:
            out["mask"] = postprocess_prediction(pred.squeeze(), **self.mask_options)
            if agreement:
                out["prediction_roi"], out["agreement_roi"] = self.run_second(volume, out["mask"], keep_variants, True)
            else:
                out["prediction_roi"] = self.run_second(volume, out["mask"], keep_variants)
        return out


def predict_volume(data, model, config, overlap_factor=0.9, preprocess_method=None, norm_params=None, augment=None, num_augment=0,
                   model2=None, config2=None, preprocess_method2=None, norm_params2=None, augment2=None, num_augment2=0,
                   z_scale=None, xy_scale=None, return_all_preds=False, device=None, *, blend=None,
                   blend_sigma_scale=prediction.DEFAULT_SIGMA_SCALE, return_agreement=False):
    """One-call form with the argument names of the reference's `main()` (predict_nifti2.py:98-160), on arrays: `data` = the volume as read
    from the NIfTI file.  Returns a dict: 'data' (the prepared volume the first model saw, before its border), 'prediction' (first stage, on
    the input grid) and, with model2 / config2, 'mask' and 'prediction_roi' (second stage on the padded bounding box, volume-sized).
    `device` (not in the reference): where the intensity preparation, the zooms and the variant medians run - None / True / False as for
    `Zoom`.  config['preproc'] may name a filter of `fetal_net.preprocess`, as the reference's configs do.
    `blend` / `blend_sigma_scale` (not in the reference): how both stages combine overlapping tiles, as for `Stage`.
    `return_agreement` (not in the reference): adds 'agreement' and, with a second stage, 'agreement_roi': the `prediction.TTAAgreement`
    of each stage's test-time variants (every stage then needs an `augment`).  Their maps (median, mean, variance, entropy,
    disagreement) come back on the input grid through the steps the prediction takes back (crop, zoom back, box); their counts,
    variant Dice, estimated Dice and volume spread are passed through as taken on the grid the model saw.  Without the flag the
    returned dict is what it was.  `data` may be a float64 CUDA tensor where the first stage takes the resident route and there is no
    second stage: tensors in, tensors out (the agreement's counts and scores stay numpy)."""
    if config2 is not None and model2 is None:
        raise ValueError("config2 given without model2")
    blending = dict(blend=blend, blend_sigma_scale=blend_sigma_scale)
    first = Stage(model, config, preprocess_method, norm_params, augment, num_augment, overlap_factor, device, **blending)
    second = None if config2 is None else Stage(model2, config2, preprocess_method2, norm_params2, augment2, num_augment2, overlap_factor,
                                                device, **blending)
    return VolumePipeline(first, second, resolution=(xy_scale, z_scale), device=device)(data, keep_variants=return_all_preds,
                                                                                        agreement=return_agreement)


def secondary_prediction(mask, vol, config2, model2, preprocess_method2=None, norm_params2=None, overlap_factor=0.9, augment2=None,
                         num_augment=32, return_all_preds=False, padding=ROI_PADDING, *, blend=None,
                         blend_sigma_scale=prediction.DEFAULT_SIGMA_SCALE, return_agreement=False):
    """the second stage alone (reference predict_nifti2.py:25-53), for callers that already hold a first-stage mask; `blend` /
    `blend_sigma_scale` as for `Stage`.  return_agreement=True -> (the prediction, the stage's `prediction.TTAAgreement`): maps pasted
    back like the prediction, counts and scores as taken on the box the model saw"""
    stage = Stage(model2, config2, preprocess_method2, norm_params2, augment2, num_augment, overlap_factor, blend=blend,
                  blend_sigma_scale=blend_sigma_scale)
    return VolumePipeline(None, stage, roi_padding=padding).run_second(np.asarray(vol), mask, keep_variants=return_all_preds,
                                                                       agreement=return_agreement)
