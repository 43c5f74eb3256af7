"""Training-patch generator that never leaves the MI355X.

The reference builds each patch on one host thread (fetal_net/generator.py:222-328: random corner -> augment_data or
extract_patch -> convert_data) and Keras copies the batch to the device; with the convolutions at MFMA speed that thread is the
bottleneck.  Here every (padded) volume of the split is uploaded once - 288 GB of HBM holds any dataset of this kind - and a patch
is: the reference's random draws on the host (same order, same generators => same transformation for the same seed), then one
fmri_affine_sample_batch launch for the image (trilinear, cval = volume minimum) and one for the labels (nearest, cval = 0) straight
into the batch tensors, then the elementwise intensity passes.  The generator yields torch CUDA tensors in the reference's logical
layouts ((N,1,X,Y,Z) / (N,X,Y,C) float32 images, uint8 labels); Model.train_on_batch / fit_generator take them as they are.
A data file with a non-empty `mask` array (the distance masks of the mask-weighted loss, reference generator.py:18-21) makes the generator
yield ([x, masks], y) like the reference's convert_data (generator.py:397-401): the mask patch is sampled like the labels (nearest, outside
= 0, same transformation) at the label slices.  As in the reference the masks of a FILE are not padded with the volumes.
`distance_masks=sampling` makes the masks at load time instead, for a file that has none: the exact Euclidean distance of every voxel
to the nearest voxel of the other class (fetal_net/utils/create_distance_masks.py, csrc/postprocess.hip), computed on the device from the
PADDED label volume - the grid the sampler draws its corners on, so mask and labels line up voxel for voxel and no crop leaves the mask.
The padding is background.  It changes no background voxel's distance (it adds no foreground), and no foreground voxel's as long as
the labels do not touch the volume's border: a padded voxel clamped to the original extent is a border voxel, background as well, and
no farther along any axis.  Labels that do touch the border see the padding as background there - as the sampled label patches do.

`device_data_generator` keeps the keyword arguments of the reference's `data_generator` (generator.py:222-225).
Applied augmenters: flip, scale, iso_scale, rotate, translate, piecewise_affine, elastic_transform (imgaug), contrast,
intensity_multiplication, gaussian_filter (skimage.filters.gaussian), poisson_noise (the reference's shot_noise), speckle_noise,
gaussian_noise, coarse_dropout (imgaug CoarseDropout) - in the reference's order (augment.py:344-375), i.e. everything the reference's
default config switches on (fetal/config_utils.py:81-123).  The three imgaug augmenters follow imgaug 0.4.0 as published (the reference
does not pin a version and the package is not installed here: their oracle says "parity unpinned", oracle/augment_oracle.py); the elastic
warp restates `_map_coordinates`' scipy branch, not the cv2.remap branch imgaug prefers for float images when cv2 is importable.
imgaug's piecewise_affine (commented out in the reference's default config, config_utils.py:101-103) is applied as well when configured,
between the affine sampling and the elastic transform (augment.py:344-347), on the reference's 2 x 2 grid.
The noise fields (normal, uniform and Poisson draws) are made inside the kernels by a counter-based generator (Philox4x32-10 keyed by
`noise_seed`; csrc/augment.hip), not by numpy: same distributions, other streams.  The patches of a batch are PLANNED one after the other
on the host (every draw of the reference, in its order) and then LAUNCHED together, one launch per step of ONE chain (`_Sampler.plan` /
`_chain`, previous-slice truth channels included).  The steps without a batch kernel (piecewise affine, the Gaussian filter, elastic fields
wider than the in-kernel generator covers) run inside that chain for the patches that drew them; drop_easy_patches' interleaved draws and
`batched=False` run the same chain on batches of one - same draws, same batches (tests/golden/generator_chain_digests.json).

Departures from the reference: four optional `augment` keys it does not have, the acquisition effects of a fetal stack of 2-D slices -
slice_motion, gamma, bias_field, slice_intensity (fetal_net/augment.py: draw_mri_parameters and the float64 host forms).  There is no
reference ordering to keep for them: their draws come from a generator of their own (seeded from `noise_seed`; numpy's global state, python's
`random` and the imgaug state above are not advanced, so every other draw of a configuration stays what it was), slice motion rides inside
the affine gather (one in-plane rigid map per slice, labels / mask / previous-slice truth under the image slice they belong to: no second
resampling), and gamma, bias field and slice gain are ONE launch behind contrast / intensity_multiplication and before the filter and the
noises - acquisition before noise.  A configuration without these keys draws nothing and launches nothing new.
"""
import random
import warnings

import numpy as np

from .augment import MRI_KEYS, distort_image, draw_augment_parameters, draw_mri_parameters

_UNSUPPORTED = ()                          # every augmenter of reference augment.py:222-377 is applied


class DeviceDataFile(object):
    """The volumes of a data file, padded as the reference pads them for training (generator.py:13-57: DataFileDummy with
    `samples_pad`, then pad_samples), resident in HBM: .data[i] float32 (X,Y,Z), .truth[i] uint8 (X,Y,Z), .stats min / max.
    .mask[i] float32: the file's masks (unpadded), or with `distance_masks` (a voxel spacing per axis, or True for the reference's
    (0.4, 0.4, 3.0)) the distance mask of the padded labels, made on the device; None when there are neither."""

    def __init__(self, data_file, patch_shape, samples_pad=3, truth_downsample=None, indices=None, device="cuda", distance_masks=None):
        import torch
        ds = truth_downsample or 1
        root = data_file.root
        n = len(root.data)
        self.indices = list(range(n)) if indices is None else list(indices)
        self.data, self.truth, self.min, self.max, self.mask = {}, {}, {}, {}, None
        if hasattr(root, "mask") and root.mask is not None and len(root.mask):
            if distance_masks is not None:
                raise ValueError("the data file already has masks: distance_masks would replace them")
            self.mask = {}
        elif distance_masks is not None:
            from .utils.create_distance_masks import sampling as default_sampling
            from fmri_hip import ops
            spacing = default_sampling if distance_masks is True else distance_masks
        self.subject_ids = [s for s in root.subject_ids] if hasattr(root, "subject_ids") else None
        out_shape = [patch_shape[0] // ds, patch_shape[1] // ds, 1]
        padding = np.ceil(np.subtract(patch_shape, out_shape) / 2).astype(int)
        made = {}
        for i in self.indices:
            d = np.asarray(root.data[i])
            t = np.asarray(root.truth[i])
            d = np.pad(d, samples_pad, "constant", constant_values=d.min())
            t = np.pad(t, samples_pad, "constant", constant_values=0)
            dmin, dmax = float(np.min(d)), float(np.max(d))
            d = np.pad(d, [(p, p) for p in padding], "constant", constant_values=dmin)
            t = np.pad(t, [(p, p) for p in padding], "constant", constant_values=0)
            fit = np.ceil(np.maximum(np.subtract(patch_shape, d.shape) + 1, 0) / 2).astype(int)
            d = np.pad(d, [(p, p) for p in fit], "constant", constant_values=dmin)
            fit = np.ceil(np.maximum(np.subtract(patch_shape, t.shape) + 1, 0) / 2).astype(int)
            t = np.pad(t, [(p, p) for p in fit], "constant", constant_values=0)
            self.data[i] = torch.from_numpy(np.ascontiguousarray(d, dtype=np.float32)).to(device)
            self.truth[i] = torch.from_numpy(np.ascontiguousarray(t).astype(np.uint8)).to(device)
            self.min[i], self.max[i] = dmin, dmax
            if self.mask is not None:
                self.mask[i] = torch.from_numpy(np.ascontiguousarray(np.asarray(root.mask[i]), dtype=np.float32)).to(device)
            elif distance_masks is not None:
                made[i] = ops.distance_mask_u8((self.truth[i] != 0).to(torch.uint8), spacing).float()
        if distance_masks is not None:
            self.mask = made
        self.device = device
        self._mask_edge = {}

    def mask_for_crops(self, i):
        """the mask as the reference's un-augmented path sees it: a crop that runs past the (unpadded) mask is completed with edge values
        (reference utils/patches.py:66-90), so the volume is grown with replicated borders up to the padded label volume's extent"""
        if i not in self._mask_edge:
            import torch
            m = self.mask[i]
            grow = [max(int(t) - int(s), 0) for t, s in zip(self.truth[i].shape, m.shape)]
            if any(grow):
                m = torch.nn.functional.pad(m[None, None], (0, grow[2], 0, grow[1], 0, grow[0]), mode="replicate")[0, 0].contiguous()
            self._mask_edge[i] = m
        return self._mask_edge[i]

    def nbytes(self):
        return sum(v.numel() * 4 for v in self.data.values()) + sum(v.numel() for v in self.truth.values()) + \
            sum(v.numel() * 4 for v in (self.mask or {}).values())


def random_list_generator(index_list):
    while True:
        np.random.seed()                                   # the reference re-seeds from the OS on every pass (generator.py:194-197)
        yield from random.sample(index_list, len(index_list))


def list_generator(index_list):
    while True:
        yield from index_list


COARSE_MIN_SIZE = 3


def _coarse_grid(shape2d, size_percent, rng):
    """imgaug parameters.FromLowerResolution: one size_percent per axis - a list is a choice among its values (the reference's default
    [0.10, 0.30]), a tuple a uniform range, a number itself; grid = int(extent * percent), at least MIN_SIZE = 3 per side (the `min_size`
    imgaug 0.4.0's CoarseDropout passes to FromLowerResolution: a patch under 30 voxels at 10 % still drops cells, not whole slices)"""
    out = []
    for extent in shape2d:
        if isinstance(size_percent, list):
            sp = size_percent[int(rng.randint(len(size_percent)))]
        elif isinstance(size_percent, tuple):
            sp = rng.uniform(size_percent[0], size_percent[1])
        else:
            sp = size_percent
        out.append(max(int(extent * sp), COARSE_MIN_SIZE))
    return tuple(out)


class _Sampler(object):
    def __init__(self, ddf, patch_shape, augment, truth_index, truth_size, prev_truth_index, prev_truth_size, strict, noise_seed):
        import torch
        from fmri_hip import ops
        self.torch, self.ops = torch, ops
        self.ddf = ddf
        self.patch_shape = tuple(int(v) for v in patch_shape)
        self.augment = augment
        self.truth_index, self.truth_size = truth_index, truth_size
        self.prev_truth_index, self.prev_truth_size = prev_truth_index, prev_truth_size
        self.n_chan = self.patch_shape[2] + (prev_truth_size if prev_truth_index is not None else 0)
        self.stats_b = self.ws_b = None                  # the chain's [B] workspaces, made on first use
        self.seed, self.seq = int(noise_seed), 0
        self.batched = True
        self.gen = torch.Generator(device=ddf.device)
        self.gen.manual_seed(noise_seed)
        # imgaug keeps its own random state (the reference's numpy / python streams are not advanced by its draws): the grid sizes of the coarse
        # dropout come from a private host generator, everything per voxel from the device generator
        self.host_rng = np.random.RandomState(noise_seed)
        # the fetal keys (slice_motion, gamma, bias_field, slice_intensity) draw from a third state: adding them moves no other draw
        self.mri_rng = np.random.RandomState((int(noise_seed) ^ 0x4D5249) & 0xFFFFFFFF)
        self.mri = augment is not None and any(augment.get(k) is not None for k in MRI_KEYS)
        if augment is not None:
            bad = [k for k in _UNSUPPORTED if augment.get(k) is not None]
            if bad:
                msg = "augmenters not applied on the device path: %s" % ", ".join(bad)
                if strict:
                    raise NotImplementedError(msg)
                warnings.warn(msg)

    def _next_seq(self):
        # the kernels take the call number as uint32 and 0 means "this patch skips the step": wrap inside 1 .. 2^32 - 1
        self.seq = self.seq % 0xFFFFFFFF + 1
        return self.seq

    def plan(self, index):
        """every HOST draw of one patch, in the reference's order (numpy's global state, python's `random`, this sampler's private imgaug
        state and the call numbers of its in-kernel draws), and the matrices they give - nothing is enqueued.  -> dict for launch / _chain."""
        ddf, ps = self.ddf, self.patch_shape
        data, truth = ddf.data[index], ddf.truth[index]
        corner = [np.random.randint(low=0, high=h) for h in np.array(truth.shape) - np.array(ps)]
        q = {"index": index, "corner": corner, "corners": None, "elastic_seq": 0, "elastic_rng": True, "shot_seq": 0, "speckle_seq": 0,
             "gaussian_seq": 0, "dropout_seq": 0, "grid": (1, 1), "mri": None}
        if self.augment is not None:
            p = draw_augment_parameters(self.augment, 3, ddf.min[index], ddf.max[index])
            geo = dict(flip_axis=p["flip_axis"], scale_factor=p["scale_factor"], rotate_factor=p["rotate_factor"], translate_factor=p["translate_factor"])
            _, A = distort_image(data, np.eye(4), **geo)
            _, At = distort_image(truth, np.eye(4), **geo)
            Am = distort_image(ddf.mask[index], np.eye(4), **geo)[1] if ddf.mask is not None else None
        else:
            p, A, At, Am = None, np.eye(4), np.eye(4), np.eye(4)
        q.update(p=p, A=A, At=At, Am=Am)
        if p is None:
            return q
        # imgaug's two geometric augmenters, each a resampling of its own as in the reference: piecewise affine (augment.py:344-347; a 2 x 2 grid:
        # the four corners move by Normal(0, scale) of the extent, clipped to the image; two triangles), then the elastic transform (:349-353).
        # ONE set of moved corners / ONE in-plane displacement field for every slice and for image (bilinear), truth, previous-slice truth and mask
        if p["piecewise_affine_scale"] > 0:
            h, w = float(ps[0]), float(ps[1])
            grid = np.array([[0, 0], [0, w], [h, 0], [h, w]], dtype=np.float64)
            corners = grid + self.host_rng.normal(0.0, p["piecewise_affine_scale"], size=(4, 2)) * np.array([h, w])
            corners[:, 0] = np.clip(corners[:, 0], 0, h - 1)
            corners[:, 1] = np.clip(corners[:, 1], 0, w - 1)
            q["corners"] = corners
        if p["elastic_transform_scale"] > 0:
            q["elastic_rng"] = self.ops.elastic_ksize(float(self.augment["elastic_transform"]["sigma"])) <= self.ops.ELASTIC_RNG_KMAX
            q["elastic_seq"] = self._next_seq() if q["elastic_rng"] else -1
        q["need_intensity"] = bool(p["contrast"] is not None or p["intensity_multiplication"] != 1 or p["apply_speckle_noise"] or p["apply_gaussian_noise"]
                                   or p["apply_gaussian_filter"] or p["apply_poisson_noise"] or p["coarse_dropout"])
        if self.mri:
            q["mri"] = draw_mri_parameters(self.augment, ps, self.mri_rng)
            q["need_intensity"] = q["need_intensity"] or self._mri_intensity(q)
        if p["apply_poisson_noise"]:
            q["shot_seq"] = self._next_seq()
        if p["apply_speckle_noise"]:
            q["speckle_seq"] = self._next_seq()
        if p["apply_gaussian_noise"]:
            q["gaussian_seq"] = self._next_seq()
        if p["coarse_dropout"]:
            # reference augment.py:373-375 (last step): imgaug CoarseDropout(p=rate, size_percent, per_channel) in a [0, 255] scaling
            q["grid"] = _coarse_grid((ps[0], ps[1]), self.augment["coarse_dropout"]["size_percent"], self.host_rng)
            q["dropout_seq"] = self._next_seq()
        return q

    @staticmethod
    def _mri_intensity(q):
        r = q["mri"]
        return r is not None and (r["gamma"] != 0 or r["bias_coef"] is not None or r["slice_gain"] is not None)

    def _upload(self, a):
        """a small host array -> device on the current stream, through pinned memory: enqueue-only like the launches (a copy from pageable
        memory would make the host wait for the stream)"""
        return self.torch.from_numpy(a).pin_memory().to(self.ddf.device, non_blocking=True)

    def _slice_tables(self, plans):
        """the slice-motion tables of `plans` as ONE device tensor (B, slices, 6) float64 (identity rows for a patch that drew none), uploaded
        on the current stream; None when no patch drew slice motion - the plain gathers are called then"""
        if not any(q["mri"] is not None and q["mri"]["slice_table"] is not None for q in plans):
            return None
        tab = np.tile(np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0]), (len(plans), self.patch_shape[2], 1))
        for b, q in enumerate(plans):
            if q["mri"] is not None and q["mri"]["slice_table"] is not None:
                tab[b] = q["mri"]["slice_table"]
        return self._upload(tab)

    def _mri_intensity_launch(self, plans, x, stats, ws):
        """gamma, bias field and slice gain of `plans` on the dense image slices x (B, X, Y, slices): one launch, one upload for the gains"""
        mri = [q["mri"] if self._mri_intensity(q) else None for q in plans]
        if not any(r is not None for r in mri):
            return
        gains = None
        if any(r is not None and r["slice_gain"] is not None for r in mri):
            g = np.ones((len(plans), self.patch_shape[2]), dtype=np.float32)
            for b, r in enumerate(mri):
                if r is not None and r["slice_gain"] is not None:
                    g[b] = r["slice_gain"]
            gains = self._upload(g)
        self.ops.mri_intensity_ws_batch(x, stats, ws, [0.0 if r is None else r["gamma"] for r in mri], [None if r is None else r["bias_coef"] for r in mri],
                                        [gains[b] if r is not None and r["slice_gain"] is not None else None for b, r in enumerate(mri)],
                                        [self.ddf.min[q["index"]] for q in plans])

    def sample_into(self, index, x_slot, y_slot, m_slot=None):
        """one patch: x_slot: float32 view (X, Y, n_chan) of the batch tensor; y_slot: uint8 view (X, Y, truth_size); m_slot: float32 view
        (X, Y, truth_size) for the distance mask, when the data file has masks"""
        self._chain([self.plan(index)], x_slot.unsqueeze(0), y_slot.unsqueeze(0), None if m_slot is None else m_slot.unsqueeze(0))

    def launch(self, plans, x, y, m=None):
        """x (B, X, Y, n_chan) float32, y (B, X, Y, truth_size) uint8, m like y in float32 or None: the patches of `plans`, in order - launched
        together, or (batched=False) each as a batch of one"""
        if self.batched:
            self._chain(plans, x, y, m)
        else:
            for b, q in enumerate(plans):
                self._chain([q], x[b:b + 1], y[b:b + 1], None if m is None else m[b:b + 1])

    def _chain(self, plans, x, y, m):
        """THE chain, in the reference's order, ONE launch per step for all of `plans` (fmri_*_batch): 2-4 gathers, the elastic fields and 2-4
        warps, the min / max, then only the intensity steps some patch drew.  The steps without a batch kernel - piecewise affine, the Gaussian
        filter, elastic fields wider than the one-launch field kernel - run inside it for the patches that drew them, in batch order.  A patch
        without a warp in a warped batch goes through the batch warp with zero fields: the identity, bit for bit.  With previous-slice truth
        channels the image slices are sampled, warped and augmented in a dense (B, X, Y, slices) staging tensor and copied in front of the
        truth channels, which are sampled (nearest, outside = 0) and warped with the same fields."""
        ops, ddf, torch, ps = self.ops, self.ddf, self.torch, self.patch_shape
        B = len(plans)
        prev = self.prev_truth_index is not None
        xd = torch.empty((B,) + tuple(ps), device=x.device, dtype=torch.float32) if prev else x        # the image slices, dense
        idx = [q["index"] for q in plans]
        tshape = (ps[0], ps[1], self.truth_size)
        warped = any(q["elastic_seq"] for q in plans)
        d = None
        if warped:
            alphas = [q["p"]["elastic_transform_scale"] if q["elastic_seq"] else 0.0 for q in plans]
            sigma = self.augment["elastic_transform"]["sigma"]
            if all(q["elastic_rng"] for q in plans):
                d = ops.elastic_fields_rng_batch((ps[0], ps[1]), alphas, sigma, self.seed, [q["elastic_seq"] for q in plans], device=x.device)
            else:                                            # a kernel wider than ELASTIC_RNG_KMAX: host fields from self.gen, patch after patch
                d = torch.zeros((B, 2, ps[0], ps[1]), device=x.device, dtype=torch.float32)
                for b, q in enumerate(plans):
                    if q["elastic_seq"]:
                        d[b, 0], d[b, 1] = ops.elastic_fields((ps[0], ps[1]), alphas[b], sigma, generator=self.gen)
        corners_t = [(q["corner"][0], q["corner"][1], q["corner"][2] + self.truth_index) for q in plans]
        table = self._slice_tables(plans)                    # None unless some patch drew slice motion: the plain gather then

        def sample(vols, affines, corners, size, dst, order, cvals, z_off, dst_ld=None):
            """gather (output slice k moved by table row k + z_off), then imgaug's two resamplings: piecewise affine on the patches that drew
            one (reference augment.py:344-347), the elastic warp on all (:349-353) -> dst"""
            t = torch.empty((B,) + tuple(size), device=dst.device, dtype=dst.dtype) if warped else dst
            ops.affine_sample_batch(vols, affines, corners, size, t, order, cvals, table=table, z_off=z_off, out_ld=None if warped else dst_ld)
            for b, q in enumerate(plans):
                if q["corners"] is not None:
                    ops.piecewise_affine(t[b].clone(), q["corners"], order, t[b])
            if warped:
                ops.elastic_warp_batch(t, d, order, dst)

        # image: trilinear, outside = the volume's minimum; labels: nearest, outside = 0 (identity affine = the plain crop)
        sample([ddf.data[i] for i in idx], [q["A"] for q in plans], [q["corner"] for q in plans], ps, xd, 1, [ddf.min[i] for i in idx], 0)
        sample([ddf.truth[i] for i in idx], [q["At"] for q in plans], corners_t, tshape, y, 0, [0.0] * B, self.truth_index)
        if m is not None:
            # augmented: outside the mask = 0 (interpolate_affine_range, cval 0); plain crop: edge values
            src = [ddf.mask[q["index"]] if q["p"] is not None else ddf.mask_for_crops(q["index"]) for q in plans]
            sample(src, [q["Am"] for q in plans], corners_t, tshape, m, 0, [0.0] * B, self.truth_index)
        if prev:
            corners_p = [(q["corner"][0], q["corner"][1], q["corner"][2] + self.prev_truth_index) for q in plans]
            sample([ddf.truth[i] for i in idx], [q["At"] for q in plans], corners_p, (ps[0], ps[1], self.prev_truth_size), x[..., ps[2]:], 0,
                   [0.0] * B, self.prev_truth_index, dst_ld=self.n_chan)
        if any(q["p"] is not None and q["need_intensity"] for q in plans):
            self._intensity(plans, xd)
        if prev:
            x[..., :ps[2]] = xd

    def _intensity(self, plans, x):
        """the intensity steps of the chain on the dense image slices x (B, X, Y, slices).  Every step wants the image's range
        (rescale_intensity's out_range, MinMaxScaler): taken ONCE, then each kernel that rewrites a patch leaves its new range in stats[b] for
        the next one; the noise draws are made in the kernels (Philox keyed by noise_seed, one counter value per call) - fmri_hip.h"""
        ops = self.ops
        B = len(plans)
        stats, ws = self._workspace(B)
        ops.minmax_ws_batch(x, stats, ws)
        params = []
        for q in plans:
            p = q["p"]
            if p is None or (p["contrast"] is None and p["intensity_multiplication"] == 1):
                params.append((0, 0.0, 0.0, 1.0))
            else:
                lo, hi = p["contrast"] if p["contrast"] is not None else (0.0, 0.0)
                params.append((2 if p["contrast"] is not None else 1, lo, hi, p["intensity_multiplication"]))
        if any(r[0] for r in params):
            ops.rescale_intensity_ws_batch(x, stats, ws, params)
        self._mri_intensity_launch(plans, x, stats, ws)                  # acquisition effects: behind the reference's contrast, before its noises
        # order of reference augment.py:354-367: gaussian filter, shot (poisson) noise, speckle, gaussian noise; coarse dropout last
        for b, q in enumerate(plans):
            if q["p"] is not None and q["p"]["apply_gaussian_filter"]:
                img = x[b]
                smooth = ops.gaussian_filter_f32(img, q["p"]["gaussian_sigma"])
                if smooth is not img:
                    img.copy_(smooth)
                ops.minmax_ws(img, stats[b], ws[b])
        if any(q["shot_seq"] for q in plans):
            ops.shot_noise_rng_batch(x, stats, ws, self.seed, [q["shot_seq"] for q in plans])
        for key, aug_key, kind in (("speckle_seq", "speckle_noise", 1), ("gaussian_seq", "gaussian_noise", 0)):
            if any(q[key] for q in plans):
                ops.noise_rng_batch(x, stats, ws, kind, self.augment[aug_key]["sigma"], self.seed, [q[key] for q in plans])
        if any(q["dropout_seq"] for q in plans):
            cd = self.augment["coarse_dropout"]
            ops.coarse_dropout_rng_batch(x, [q["grid"] for q in plans], cd["rate"], stats, bool(cd.get("per_channel", True)), self.seed,
                                         [q["dropout_seq"] for q in plans])

    def _workspace(self, B):
        if self.stats_b is None or self.stats_b.shape[0] < B:
            self.stats_b, self.ws_b = self.ops.aug_workspace(self.ddf.device, max(B, 2))
        return self.stats_b[:B], self.ws_b[:B]


def device_data_generator(data_file, index_list, batch_size=1, n_labels=1, labels=None, augment=None, patch_shape=None,
                          shuffle_index_list=True, skip_blank=True, truth_index=-1, truth_size=1, truth_downsample=None, truth_crop=True,
                          categorical=True, prev_truth_index=None, prev_truth_size=None, drop_easy_patches=False, is3d=False,
                          samples_pad=3, strict=False, noise_seed=0, device="cuda", prefetch=0, batched=True, distance_masks=None):
    """Endless generator of (x, y) CUDA tensors.  `data_file`: a DeviceDataFile, or anything with .root.data / .root.truth
    (uploaded here).  3-D: x (N,1,X,Y,Z), y (N,1,X,Y,truth_size); 2-D: x (N,X,Y,C), y (N,X,Y,truth_size).  skip_blank and
    drop_easy_patches read one scalar back per patch (they decide on the host whether the patch is kept), everything else is
    enqueue-only.

    n_labels > 1 (categorical=False, no masks): y holds n_labels binary channels, channel l = (label map == labels[l]), labels = 1 .. n_labels
    by default (reference generator.py:404-419) - 3-D (N, n_labels, X, Y, truth_size), 2-D (N, X, Y, n_labels) with truth_size == 1.  skip_blank
    and drop_easy_patches still decide on the raw label map: a patch that only holds values outside `labels` is kept and expands to zeros.
    n_labels == 1 yields the raw label map and never reads `labels`.

    distance_masks (None | True | spacing per axis): for a data file without masks, make the distance masks of the mask-weighted loss on
    the device when the volumes are uploaded (DeviceDataFile) and yield ([x, masks], y); a DeviceDataFile handed in was built with its own.

    batched: launch the patches of a batch together, one launch per step of the sampling / augmentation chain (the default; a step without a
    batch kernel runs for the patches that drew it); False: the same chain patch by patch, each a batch of one - same draws, same batches.

    prefetch (0 | n): n > 0 starts a producer thread with a HIP stream of its own that keeps up to n batches ready (the role of Keras'
    GeneratorEnqueuer behind the reference's fit_generator, training.py:110-124).  A batch is 11-13 short gather / element-wise launches
    (~0.34 ms of device time with the reference's default augmentation) which then run BESIDE the consumer's training step; a consumer
    that reads a scalar back every step (`train_on_batch`) leaves no other way to overlap them.  The consumer's current stream waits for the batch's
    event before the yield; the tensors are registered with that stream (record_stream) so the allocator does not recycle them under a
    step still in flight.  Draw order, and therefore every batch, is the same as with prefetch=0 (tests/test_gpu_augment.py); the draws
    of batch k+1 ... k+n come from numpy's global state BEFORE batch k is handed out, so a caller that re-seeds between batches wants
    prefetch=0 (the default).  With prefetch > 0 those draws happen on the producer THREAD against the process-global numpy / `random` states:
    anything else in the process that draws from them (a validation generator on the main thread, for one) interleaves with the
    producer by timing, and the batches of both stop being reproducible - seeded reproducibility holds for prefetch=0 only.
    `Model.fit_generator` has its own producer thread and copy stream: leave prefetch at 0 there."""
    n_labels = int(n_labels)
    if n_labels > 1:
        # several labels: the label patch is expanded into n_labels binary channels (get_multi_class_labels) by one launch per batch, behind
        # everything that samples, warps and keeps / drops patches on the raw label map
        if categorical:
            raise ValueError("n_labels > 1 with categorical=True: to_categorical(y, 2) is binary (pass categorical=False)")
        if distance_masks is not None or getattr(data_file, "mask", None) is not None or \
                (not isinstance(data_file, DeviceDataFile) and hasattr(data_file.root, "mask") and data_file.root.mask is not None
                 and len(data_file.root.mask)):
            raise ValueError("n_labels > 1 with distance masks: the cross-entropy weight is per voxel, multi-label masks are not supported")
        labels = tuple(range(1, n_labels + 1)) if labels is None else tuple(labels)
        if len(labels) != n_labels:
            raise ValueError("labels %r: %d values for n_labels = %d" % (labels, len(labels), n_labels))
        if not is3d and truth_size != 1:
            raise ValueError("n_labels > 1 on a 2-D model needs truth_size == 1 (got %r)" % (truth_size,))
        from fmri_hip.ops import label_values
        label_values(labels)
    return _generate(data_file, index_list, batch_size, n_labels, labels, augment, patch_shape, shuffle_index_list, skip_blank, truth_index,
                     truth_size, truth_downsample, categorical, prev_truth_index, prev_truth_size, drop_easy_patches, is3d, samples_pad, strict,
                     noise_seed, device, prefetch, batched, distance_masks)


def _generate(data_file, index_list, batch_size, n_labels, labels, augment, patch_shape, shuffle_index_list, skip_blank, truth_index,
              truth_size, truth_downsample, categorical, prev_truth_index, prev_truth_size, drop_easy_patches, is3d, samples_pad, strict,
              noise_seed, device, prefetch, batched, distance_masks):
    """the generator behind device_data_generator, which has checked the label arguments (a generator function's body only runs at the
    first next(): the checks belong to the call)"""
    import torch
    if truth_downsample is not None and truth_downsample > 1:
        raise NotImplementedError("truth_downsample is not part of the device generator")
    if patch_shape is None:
        raise ValueError("the device generator samples patches; patch_shape is required")
    ddf = data_file if isinstance(data_file, DeviceDataFile) else DeviceDataFile(data_file, patch_shape, samples_pad, truth_downsample,
                                                                                 indices=sorted(set(index_list)), device=device,
                                                                                 distance_masks=distance_masks)
    sampler = _Sampler(ddf, patch_shape, augment, truth_index, truth_size, prev_truth_index, prev_truth_size, strict, noise_seed)
    sampler.batched = bool(batched)
    index_generator = random_list_generator(index_list) if shuffle_index_list else list_generator(index_list)
    ps = sampler.patch_shape

    last_done = [None]

    def produce():
        # the sampler's range / workspace buffers are reused batch after batch: a caller that pulls batches under changing streams must not
        # start batch k + 1's chain while batch k's still runs on another stream (same stream: ordered anyway, the wait is free)
        cur = torch.cuda.current_stream()
        if last_done[0] is not None:
            cur.wait_event(last_done[0])
        out = produce_batch()
        last_done[0] = torch.cuda.Event()
        last_done[0].record(cur)
        return out

    def produce_batch():
        x = torch.empty((batch_size, ps[0], ps[1], sampler.n_chan), device=ddf.device, dtype=torch.float32)
        y = torch.empty((batch_size, ps[0], ps[1], truth_size), device=ddf.device, dtype=torch.uint8)
        m = torch.empty((batch_size, ps[0], ps[1], truth_size), device=ddf.device, dtype=torch.float32) if ddf.mask is not None else None
        filled = 0
        while filled < batch_size and drop_easy_patches:
            # the keep / drop draw of a patch comes from numpy's stream BETWEEN its draws and the next patch's: patch by patch, as the reference
            index = next(index_generator)
            sampler.sample_into(index, x[filled], y[filled], None if m is None else m[filled])
            truth_mean = float(y[filled][16:-16, 16:-16, :].float().mean().item())
            if 1 - np.abs(truth_mean - 0.5) < np.random.random():
                continue
            if skip_blank and not bool(y[filled].any().item()):
                continue
            filled += 1
        while filled < batch_size:
            # the patches still missing, planned in the reference's draw order and launched together; blank ones (skip_blank) are dropped behind
            # ONE read-back, the kept ones move up in order and the next round plans the rest: the same patches in the same slots as one by one
            need = batch_size - filled
            plans = [sampler.plan(next(index_generator)) for _ in range(need)]
            sampler.launch(plans, x[filled:], y[filled:], None if m is None else m[filled:])
            keep = list(range(need))
            if skip_blank:
                keep = [i for i, f in enumerate(y[filled:].reshape(need, -1).any(dim=1).tolist()) if f]
            for dst, src in enumerate(keep):
                if dst != src:
                    for t in (x, y, m):
                        if t is not None:
                            t[filled + dst].copy_(t[filled + src])
            filled += len(keep)
        yy = y
        if n_labels > 1:
            # (N, X, Y, T) label bytes -> (N, X, Y, T, L) binary channels, channels last: 2-D (T = 1) yields (N, X, Y, L); 3-D yields the
            # permuted VIEW (N, L, X, Y, T) of that buffer, which Model._to_device_y's permute(0, 2, 3, 4, 1).contiguous() takes back for free
            ye = sampler.ops.labels_expand_u8(y, labels)
            return (x.unsqueeze(1), ye.permute(0, 4, 1, 2, 3), None) if is3d else (x, ye.squeeze(3), None)
        if categorical:
            # keras.utils.to_categorical(y, 2) (reference generator.py:390-391): a trailing axis of size 1 is dropped before the one-hot
            # axis is appended - (N,X,Y,1) -> (N,X,Y,2), (N,X,Y,T>1) -> (N,X,Y,T,2) - float32
            yc = y.squeeze(-1) if y.shape[-1] == 1 else y
            yy = torch.stack([1 - yc, yc], dim=-1).float()
        if is3d:
            xo, yo, mo = x.unsqueeze(1), yy.unsqueeze(1), (None if m is None else m.unsqueeze(1))
        else:
            xo, yo, mo = x, yy, m
        return xo, yo, mo

    if not prefetch:
        while True:
            xo, yo, mo = produce()
            yield (xo if mo is None else [xo, mo]), yo

    import queue
    import threading
    dev_index = torch.device(ddf.device).index if torch.device(ddf.device).index is not None else torch.cuda.current_device()
    side = torch.cuda.Stream(device=dev_index)
    side.wait_stream(torch.cuda.current_stream())      # the volumes were uploaded on the caller's stream: order the side stream behind it once
    ready_q = queue.Queue(maxsize=int(prefetch))
    stop = threading.Event()

    def put(item):
        while not stop.is_set():
            try:
                ready_q.put(item, timeout=0.05)
                return
            except queue.Full:
                pass

    def producer():
        try:
            torch.cuda.set_device(dev_index)
            with torch.cuda.stream(side):
                while not stop.is_set():
                    batch = produce()
                    ready = torch.cuda.Event()
                    ready.record(side)
                    put((batch, ready, None))
        except BaseException as e:                     # handed to the consumer: a generator that dies silently would hang the training loop
            put((None, None, e))

    worker = threading.Thread(target=producer, name="device_data_generator", daemon=True)
    worker.start()
    try:
        while True:
            batch, ready, err = ready_q.get()
            if err is not None:
                raise err
            xo, yo, mo = batch
            consumer = torch.cuda.current_stream()
            consumer.wait_event(ready)
            for t in (xo, yo, mo):
                if t is not None:
                    t.record_stream(consumer)
            yield (xo if mo is None else [xo, mo]), yo
    finally:                                           # generator closed or collected: stop the producer, let it leave its put()
        stop.set()
        worker.join(timeout=10.0)


def get_multi_class_labels(data, n_labels, labels=None):
    """reference fetal_net/generator.py:404-419: data (n, 1, ...) label map -> (n, n_labels, ...) int8, channel l = (data == labels[l]), labels =
    1 .. n_labels by default.  A numpy array gives a numpy array; a CUDA uint8 tensor goes through fmri_labels_expand_u8 and gives a CUDA int8
    tensor (a permuted view of the channels-last buffer the kernel writes)."""
    if data.shape[1] != 1:
        raise ValueError("get_multi_class_labels: a label map (n, 1, ...) is needed (got %s)" % (tuple(data.shape),))
    values = list(range(1, n_labels + 1)) if labels is None else list(labels)
    if len(values) != n_labels:
        raise ValueError("labels %r: %d values for n_labels = %d" % (labels, len(values), n_labels))
    if isinstance(data, np.ndarray):
        y = np.zeros((data.shape[0], n_labels) + tuple(data.shape[2:]), np.int8)
        for l, v in enumerate(values):
            y[:, l][data[:, 0] == v] = 1
        return y
    import torch
    from fmri_hip import ops
    if not (isinstance(data, torch.Tensor) and data.is_cuda and data.dtype == torch.uint8):
        raise TypeError("get_multi_class_labels: a numpy array or a CUDA uint8 tensor")
    out = ops.labels_expand_u8(data[:, 0].contiguous(), values)               # (n, ..., L)
    nd = out.dim()
    return out.view(torch.int8).permute(0, nd - 1, *range(1, nd - 1))
