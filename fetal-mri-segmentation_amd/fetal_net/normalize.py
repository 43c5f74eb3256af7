"""Normalisation of a data file's volumes (reference fetal_net/normalize.py:66-92): `normalize_data`, `normalize_data_storage` ('all':
every volume with the mean of the per-volume means and the mean of the per-volume standard deviations) and
`normalize_data_storage_each` ('each': every volume with its own statistics).  The reference's foreground / crop helpers (nilearn) are
not part of this package.

`storage` is any mutable sequence of float64 volumes: a list, or the VLArray of an open PyTables file.  `device` follows the package
convention (`fetal_net.preprocess`): None = the device form when a GPU and the HIP library are there, True / False force one.  The
device form takes every volume's mean and standard deviation from `fmri_hip.ops.moments_f64` (compensated sums in an order fixed by the
size: within a few ulp of the exact values, where numpy's pairwise sums are within a few tens) and maps with `ops.normalize_f64`, which
is numpy's subtract and divide bit for bit; the host form is the reference's numpy arithmetic.  The two forms therefore agree to the
rounding of the statistics, not bit for bit - `fetal_net.data.write_data_to_file` documents what that means for a data file."""
import numpy as np

from .pipeline import normalize_data  # noqa: F401  (reference normalize.py:66-69, with the package's device= rule)
from .postprocess import _device_ok

_AXES = (-1, -2, -3)


def _use_device(storage, device):
    if device is None:
        return len(storage) > 0 and all(_device_ok(np.asarray(storage[i])) for i in range(len(storage)))
    return bool(device)


def _upload(vol):
    import torch
    vol = np.asarray(vol)
    if vol.ndim != 3 or vol.size == 0:
        raise ValueError("the device form normalises non-empty volumes [X,Y,Z] (got shape %r)" % (vol.shape,))
    return torch.from_numpy(np.ascontiguousarray(vol, dtype=np.float64)).cuda()


def combine_statistics(means, stds):
    """the 'all' rule (reference normalize.py:79-80): the mean of the per-volume means, the mean of the per-volume stds"""
    return np.asarray(means).mean(axis=0), np.asarray(stds).mean(axis=0)


def normalize_data_storage(storage, device=None):
    """reference normalize.py:72-83 -> (storage, mean, std); the volumes of `storage` are replaced by (volume - mean) / std"""
    n = len(storage)
    if _use_device(storage, device):
        from fmri_hip import ops
        moments = [ops.moments_f64(_upload(storage[i]))[:2] for i in range(n)]
        mean, std = combine_statistics([m[0] for m in moments], [m[1] for m in moments])
        for i in range(n):
            storage[i] = ops.normalize_f64(_upload(storage[i]), float(mean), float(std)).cpu().numpy()
        return storage, mean, std
    means, stds = [], []
    for i in range(n):
        data = storage[i]
        means.append(data.mean(axis=_AXES))
        stds.append(data.std(axis=_AXES))
    mean, std = combine_statistics(means, stds)
    for i in range(n):
        storage[i] = (storage[i] - mean) / std
    return storage, mean, std


def normalize_data_storage_each(storage, device=None):
    """reference normalize.py:86-92 -> (storage, None, None); every volume with its own mean and standard deviation"""
    on_device = _use_device(storage, device)
    for i in range(len(storage)):
        data = storage[i]
        if on_device:
            from fmri_hip import ops
            t = _upload(data)
            mean, std = ops.moments_f64(t)[:2]
            storage[i] = ops.normalize_f64(t, mean, std).cpu().numpy()
        else:
            storage[i] = (data - data.mean(axis=_AXES)) / data.std(axis=_AXES)
    return storage, None, None
