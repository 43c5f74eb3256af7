"""The named intensity filters a config selects with `"preproc": "<name>"` (same names and definitions as reference
fetal_net/preprocess.py:5-27; the reference resolves the name with getattr on that module, fetal/utils.py:13-14,
prod/predict_nifti2.py:67-69): norm_minmax, laplace, laplace_norm, grad, grad_norm.

Two implementations of each definition: scipy / numpy on the host (what the reference runs), and the kernels at the end of
csrc/postprocess.hip behind fmri_hip.ops (`laplace_f64`, `gaussian_gradient_magnitude_f64`, `norm_minmax_f64`), which restate scipy's
and numpy's arithmetic in float64 operation by operation, so the two give the same values (tests/test_gpu_intensity.py).

`device=` follows `fetal_net.postprocess.postprocess_prediction`: None = the device form for a float64 3-D ndarray when a GPU and the
HIP library are there, else the host form; True / False force one (True takes the array as float64).  A float64 CUDA tensor [X,Y,Z]
goes in and comes out as a tensor, so a chain of steps stays on the device (`fetal_net.pipeline.Stage.intensities`)."""
import sys

import numpy as np
from scipy import ndimage

from .postprocess import _device_ok

__all__ = ["norm_minmax", "laplace", "laplace_norm", "grad", "grad_norm"]

GRAD_SIGMA = (1, 1, 1)


def _is_device_tensor(d):
    torch = sys.modules.get("torch")
    return torch is not None and isinstance(d, torch.Tensor) and d.is_cuda


def _dispatch(d, device, on_device, on_host):
    """`on_device` (tensor -> tensor) or `on_host` (ndarray -> ndarray) of `d` under the `device=` rule of this module"""
    if _is_device_tensor(d):
        if device is not None and not device:
            raise ValueError("a device tensor cannot take the host form")
        return on_device(d)
    if device is None:
        device = _device_ok(d)
    if device:
        import torch
        return on_device(torch.from_numpy(np.ascontiguousarray(d, dtype=np.float64)).cuda()).cpu().numpy()
    return on_host(d)


def _ops():
    from fmri_hip import ops
    return ops


def _norm_minmax_host(d):
    return -1 + 2 * (d - d.min()) / (d.max() - d.min())


def _grad_host(d):
    return ndimage.gaussian_gradient_magnitude(d, sigma=GRAD_SIGMA)


def norm_minmax(d, device=None):
    return _dispatch(d, device, lambda t: _ops().norm_minmax_f64(t), _norm_minmax_host)


def laplace(d, device=None):
    return _dispatch(d, device, lambda t: _ops().laplace_f64(t), ndimage.laplace)


def laplace_norm(d, device=None):
    return _dispatch(d, device, lambda t: _ops().norm_minmax_f64(_ops().laplace_f64(t)), lambda a: _norm_minmax_host(ndimage.laplace(a)))


def grad(d, device=None):
    return _dispatch(d, device, lambda t: _ops().gaussian_gradient_magnitude_f64(t, GRAD_SIGMA), _grad_host)


def grad_norm(d, device=None):
    return _dispatch(d, device, lambda t: _ops().norm_minmax_f64(_ops().gaussian_gradient_magnitude_f64(t, GRAD_SIGMA)),
                     lambda a: _norm_minmax_host(_grad_host(a)))
