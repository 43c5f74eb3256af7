"""Distance masks of the mask-weighted loss (reference fetal_net/utils/create_distance_masks.py, a bare script there): for every subject
`dists = distance_transform_edt(truth, sampling) + distance_transform_edt(1 - truth, sampling)` - one summand is 0 at every voxel, so
the mask is the distance of a voxel to the nearest voxel of the other class, in millimetres of the given voxel spacing.

Two implementations of the same definition, switched like `postprocess_prediction`: scipy.ndimage on the host (what the reference
runs) and the device kernels of csrc/postprocess.hip (`fmri_edt_two_class_u8`: both fields through one set of three passes), identical
with unit spacing and equal to a few ulp otherwise (tests/test_gpu_distance.py).  Nonzero means foreground, as scipy reads it.  A volume
that holds a single class has no nearest voxel of the other one: the device path gives +inf there, scipy numbers that are not distances.

The module constants are the reference script's; `create_distance_masks()` is its loop, `add_distance_masks()` the same for a data
file, and `DeviceDataFile(..., distance_masks=sampling)` makes the masks at load time without touching any file."""
import glob
import os

import numpy as np
from scipy import ndimage

dataset_folder = ''
ext = '.gz'
sampling = (0.4, 0.4, 3.0)


def _device_ok(truth):
    if np.ndim(truth) != 3:
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


def create_distance_mask(truth, sampling=sampling, device=None):
    """numpy label volume -> float64 distance mask.  device=None: the device path when a GPU and the library are there (3-D volumes),
    else scipy; True / False force one"""
    fg = np.asarray(truth) != 0
    if device is None:
        device = _device_ok(fg)
    if device:
        import torch
        from fmri_hip import ops
        vol = torch.from_numpy(np.ascontiguousarray(fg).view(np.uint8)).cuda()
        return ops.distance_mask_u8(vol, sampling).cpu().numpy()
    return ndimage.distance_transform_edt(fg, sampling=sampling) + ndimage.distance_transform_edt(~fg, sampling=sampling)


def create_distance_masks(dataset_folder=dataset_folder, ext=ext, sampling=sampling, device=None):
    """the reference script's loop: for every <dataset_folder>/*/truth.nii<ext> write dists.nii.gz (float64, identity affine) beside it.
    -> the files written"""
    from .nifti import load_nifti, save_nifti
    written = []
    for mask_path in sorted(glob.glob(os.path.join(dataset_folder, '*', 'truth.nii' + ext))):
        subject_dir = os.path.dirname(mask_path)
        print(os.path.basename(subject_dir))
        dists = create_distance_mask(load_nifti(mask_path), sampling=sampling, device=device)
        written.append(save_nifti(dists, os.path.join(subject_dir, 'dists.nii.gz'), np.eye(4)))
    return written


def add_distance_masks(in_file, out_file, sampling=sampling, device=None):
    """data file -> plain data file with the same `data`, `truth` and `subject_ids` and one distance mask per subject"""
    from ..data import open_data_file, write_plain_data_file
    f = open_data_file(in_file)
    try:
        root = f.root
        if 'mask' in root and len(root.mask):
            raise ValueError("%s already has masks" % in_file)
        n = len(root.data)
        data = [np.asarray(root.data[i]) for i in range(n)]
        truth = [np.asarray(root.truth[i]) for i in range(n)]
        ids = [s for s in root.subject_ids] if 'subject_ids' in root else None
    finally:
        f.close()
    masks = [create_distance_mask(t, sampling=sampling, device=device) for t in truth]
    return write_plain_data_file(out_file, data, truth, mask=masks, subject_ids=ids)
