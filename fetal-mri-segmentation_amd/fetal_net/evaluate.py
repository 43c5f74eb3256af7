"""Scoring predicted masks against the truth (reference fetal/evaluate.py: `get_fetal_envelope_mask`, `dice_coefficient` and the loop over
the case folders `run_validation_cases` writes), extended by the scores segmentation papers report per case: volume overlap and
difference, sensitivity, precision and the surface distances - Hausdorff distance, its 95th percentile, average symmetric surface
distance, by the definitions of medpy.metric.binary's hd / hd95 / assd.  No pandas, matplotlib or nibabel: the reference's boxplot and
loss graph are not restated.

Definitions, with T and P the truth and prediction masks and a = |T|, b = |P|, ab = |T n P| (voxel counts):
  dice = 2 ab / (a + b)      vod = ab / (a + b - ab)      volume_difference = (b - a) / a      sensitivity = ab / a      precision = ab / b
  volume_truth, volume_prediction = a, b times the voxel volume (the product of the spacing)
  surface of a mask = mask ^ binary_erosion(mask, generate_binary_structure(3, connectivity)): its voxels with a neighbour outside it,
    the outside of the volume counting as background
  d(T -> P) = the Euclidean distances, in units of the spacing, from the surface voxels of T to the nearest surface voxel of P
  hd = max(max d(T -> P), max d(P -> T))    hd95 = 95th percentile of both sets taken together    assd = mean(mean d(T -> P), mean d(P -> T))
Every ratio is one float64 division of integers: 0 / 0 is NaN, x / 0 is inf, nothing raises.  When either mask is empty there is no
surface to measure to and the three surface scores are NaN.

Two implementations: scipy.ndimage and numpy on the host, and the kernels at the end of csrc/postprocess.hip behind
fmri_hip.ops.segmentation_scores_u8 (tests/test_gpu_evaluate.py compares them).  `device=` follows fetal_net.pipeline: None = the
device form when a GPU and the HIP library are there, else the host form; True / False force one."""
import collections
import csv
import glob
import os

import numpy as np
from scipy import ndimage

from .utils.create_distance_masks import _device_ok

__all__ = ["get_fetal_envelope_mask", "dice_coefficient", "evaluate_case", "evaluate_case_labels", "evaluate_cases"]

KEYS = ("dice", "vod", "volume_truth", "volume_prediction", "volume_difference", "sensitivity", "precision", "hd", "hd95", "assd")


def get_fetal_envelope_mask(data):
    return data > 0


def _ratio(num, den):
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.float64(num) / np.float64(den))


def dice_coefficient(truth, prediction):
    """2 * sum(truth * prediction) / (sum(truth) + sum(prediction)) of two masks (nonzero = in the mask), as one float64 division of
    the integer counts: the float the reference's expression gives for boolean arrays.  NaN when both are empty."""
    t, p = np.asarray(truth) != 0, np.asarray(prediction) != 0
    return _ratio(2 * int(np.count_nonzero(t & p)), int(np.count_nonzero(t)) + int(np.count_nonzero(p)))


def _spacing(spacing):
    if spacing is None:
        return None
    sp = [float(spacing)] * 3 if np.isscalar(spacing) else [float(v) for v in spacing]
    if len(sp) != 3 or not all(v > 0 and np.isfinite(v) for v in sp):
        raise ValueError("spacing: one positive number, or one per axis of the 3-D volume (got %r)" % (spacing,))
    return tuple(sp)


def _border(mask, structure):
    return mask ^ ndimage.binary_erosion(mask, structure=structure, iterations=1)


def _surface_scores_host(t, p, spacing, connectivity, percentile=95):
    if not t.any() or not p.any():
        return float("nan"), float("nan"), float("nan")
    structure = ndimage.generate_binary_structure(3, connectivity)
    bt, bp = _border(t, structure), _border(p, structure)
    d_tp = ndimage.distance_transform_edt(~bp, sampling=spacing)[bt]
    d_pt = ndimage.distance_transform_edt(~bt, sampling=spacing)[bp]
    return (float(max(d_tp.max(), d_pt.max())), float(np.percentile(np.hstack((d_tp, d_pt)), percentile)),
            float(np.mean((d_tp.mean(), d_pt.mean()))))


def evaluate_case(truth, prediction, spacing=None, connectivity=1, device=None):
    """The scores of one case -> an ordered dict with the keys of `KEYS` (module docstring), Python floats.  truth, prediction: 3-D
    arrays of one shape, nonzero = in the mask (callers binarise: `get_fetal_envelope_mask`, a threshold, one label of several);
    spacing: the voxel size per axis (None = 1); connectivity: 1, 2 or 3, the neighbourhood that decides what a surface voxel is.
    The device form uploads the two masks as uint8 once and reads back a handful of scalars."""
    t, p = np.asarray(truth) != 0, np.asarray(prediction) != 0
    if t.ndim != 3 or t.shape != p.shape or t.size == 0:
        raise ValueError("two non-empty 3-D volumes of one shape are needed (got %s, %s)" % (t.shape, p.shape))
    if connectivity not in (1, 2, 3):
        raise ValueError("connectivity: 1, 2 or 3 (got %r)" % (connectivity,))
    spacing = _spacing(spacing)
    if device is None:
        device = _device_ok(t)
    if device:
        import torch
        from fmri_hip import ops
        both = np.empty((2,) + t.shape, dtype=np.uint8)                    # C order whatever the inputs' layout (NIfTI data is Fortran order)
        both[0], both[1] = t, p
        both = torch.from_numpy(both).cuda()
        res = ops.segmentation_scores_u8(both[0], both[1], spacing, connectivity)
        (a, b, ab), hd, hd95, assd = res["counts"], res["hd"], res["hd95"], res["assd"]
    else:
        a, b, ab = int(np.count_nonzero(t)), int(np.count_nonzero(p)), int(np.count_nonzero(t & p))
        hd, hd95, assd = _surface_scores_host(t, p, spacing, connectivity)
    return _row(a, b, ab, hd, hd95, assd, spacing)


def _row(a, b, ab, hd, hd95, assd, spacing):
    voxel = float(np.prod(spacing)) if spacing is not None else 1.0
    return collections.OrderedDict((
        ("dice", _ratio(2 * ab, a + b)), ("vod", _ratio(ab, a + b - ab)), ("volume_truth", a * voxel), ("volume_prediction", b * voxel),
        ("volume_difference", _ratio(b - a, a)), ("sensitivity", _ratio(ab, a)), ("precision", _ratio(ab, b)),
        ("hd", float(hd)), ("hd95", float(hd95)), ("assd", float(assd))))


def evaluate_case_labels(truth, prediction, labels, spacing=None, connectivity=1, device=None):
    """The scores of one case per label -> {label: row}, every row as evaluate_case gives it for the masks truth == label and
    prediction == label.  truth, prediction: integer label maps (3-D, one shape); labels: the values to score, 1 to 32 distinct integers in
    1..255.  The device form uploads the two maps once, counts all labels in one pass (fmri_label_counts_u8) and runs the surface
    kernels on each label's masks; the host form loops evaluate_case."""
    t, p = np.asarray(truth), np.asarray(prediction)
    if t.ndim != 3 or t.shape != p.shape or t.size == 0:
        raise ValueError("two non-empty 3-D volumes of one shape are needed (got %s, %s)" % (t.shape, p.shape))
    if connectivity not in (1, 2, 3):
        raise ValueError("connectivity: 1, 2 or 3 (got %r)" % (connectivity,))
    from fmri_hip.ops import label_values
    label_values(labels)                                                   # 1 to 32 distinct integers in 1..255, else ValueError
    labels = [int(v) for v in labels]
    spacing = _spacing(spacing)
    if device is None:
        device = _device_ok(t)
    rows = collections.OrderedDict()
    if not device:
        for v in labels:
            rows[v] = evaluate_case(t == v, p == v, spacing=spacing, connectivity=connectivity, device=False)
        return rows
    import torch
    from fmri_hip import ops
    both = np.zeros((2,) + t.shape, dtype=np.uint8)                        # C order; a value outside 0..255 is no label: it becomes 0
    for k, m in enumerate((t, p)):
        np.copyto(both[k], m, casting="unsafe", where=(m >= 0) & (m <= 255))
    both = torch.from_numpy(both).cuda()
    counts = ops.label_counts_u8(both[0], both[1], labels)
    for v, (a, b, ab) in zip(labels, counts):
        if a and b:
            res = ops.surface_metrics_u8((both[0] == v).to(torch.uint8), (both[1] == v).to(torch.uint8), spacing, connectivity)
            hd, hd95, assd = res["hd"], res["hd95"], res["assd"]
        else:                                                              # an empty mask: no surface to measure to
            hd = hd95 = assd = float("nan")
        rows[v] = _row(a, b, ab, hd, hd95, assd, spacing)
    return rows


def evaluate_cases(prediction_dir, out_csv=None, spacing=None, connectivity=1, device=None, threshold=0.5, labels=None):
    """The reference script's loop over the case folders `fetal_net.prediction.run_validation_cases` writes: every directory under
    `prediction_dir` that holds truth.nii.gz and prediction.nii.gz is scored with `evaluate_case`; anything else - a plain file, as in
    the reference, and also a folder that lacks one of the two images - is skipped.  The truth is binarised with
    `get_fetal_envelope_mask`; a prediction that is not integer typed (probabilities) is thresholded at `threshold`, an integer one is
    taken as labels (> 0).  spacing=None: the lengths of the columns of the truth image's affine.
    -> {subject_id: row}, in sorted order; with `out_csv` also one line per case (header: subject_id, then the row's keys).
    labels (a list of label values): score per label instead - the truth is taken as a label map, and so is the integer-typed
    prediction_labels.nii.gz of the case folder or, without one, an integer-typed prediction.nii.gz (a folder with neither is skipped)
    -> {subject_id: {label: row}}, and the CSV gets one line per (case, label) with a `label` column behind subject_id."""
    from .utils.nifti import load_nifti
    rows = collections.OrderedDict()
    for case_folder in sorted(glob.glob(os.path.join(prediction_dir, "*"))):
        truth_file = os.path.join(case_folder, "truth.nii.gz")
        prediction_file = os.path.join(case_folder, "prediction.nii.gz")
        if not (os.path.isdir(case_folder) and os.path.exists(truth_file) and os.path.exists(prediction_file)):
            continue
        if labels is not None:
            label_file = os.path.join(case_folder, "prediction_labels.nii.gz")
            label_data = np.squeeze(load_nifti(label_file if os.path.exists(label_file) else prediction_file))
            if not np.issubdtype(label_data.dtype, np.integer):
                continue
            truth, affine = load_nifti(truth_file, return_affine=True)
            case_spacing = spacing if spacing is not None else tuple(float(v) for v in np.linalg.norm(affine[:3, :3], axis=0))
            rows[os.path.basename(case_folder)] = evaluate_case_labels(np.squeeze(truth), label_data, labels, spacing=case_spacing,
                                                                       connectivity=connectivity, device=device)
            continue
        truth, affine = load_nifti(truth_file, return_affine=True)
        prediction = np.squeeze(load_nifti(prediction_file))
        truth = np.squeeze(truth)
        prediction = prediction > 0 if np.issubdtype(prediction.dtype, np.integer) else prediction > threshold
        case_spacing = spacing if spacing is not None else tuple(float(v) for v in np.linalg.norm(affine[:3, :3], axis=0))
        rows[os.path.basename(case_folder)] = evaluate_case(get_fetal_envelope_mask(truth), prediction, spacing=case_spacing,
                                                            connectivity=connectivity, device=device)
    if out_csv is not None:
        with open(out_csv, "w", newline="") as f:
            w = csv.writer(f)
            if labels is not None:
                w.writerow(("subject_id", "label") + KEYS)
                for subject_id, per_label in rows.items():
                    for label, row in per_label.items():
                        w.writerow([subject_id, label] + [repr(row[k]) for k in KEYS])
                return rows
            w.writerow(("subject_id",) + KEYS)
            for subject_id, row in rows.items():
                w.writerow([subject_id] + [repr(row[k]) for k in KEYS])
    return rows
