"""Loss / metric tokens with the reference names (reference fetal_net/metrics.py:7-100).

The builders look losses up by name (`getattr(fetal_net.metrics, config['loss'])`, reference fetal/train_fetal.py:31)
and compare them by identity (`loss_function != dice_coefficient_loss`, reference unet3d/unet.py:82), so each is a
module-level callable.  Inside a training step the Dice loss and the compiled metrics are computed on the device by
fmri_sigmoid_dice_fwd/bwd; called directly with arrays these functions evaluate the same formulas on the host (numpy,
float64) for evaluation scripts.
"""
from functools import partial

import numpy as np


def _f(a):
    return np.asarray(a, dtype=np.float64)


def dice_coefficient(y_true, y_pred, smooth=1.):
    yt, yp = _f(y_true).ravel(), _f(y_pred).ravel()
    return (2. * np.sum(yt * yp) + smooth) / (np.sum(yt) + np.sum(yp) + smooth)


def vod_coefficient(y_true, y_pred, binarize=True, smooth=1.):
    yt, yp = _f(y_true).ravel(), _f(y_pred).ravel()
    if binarize:
        yt, yp = (yt > 0.5).astype(np.float64), (yp > 0.5).astype(np.float64)
    inter = np.sum(yt * yp)
    return (inter + smooth) / (np.sum(yt) + np.sum(yp) - inter + smooth)


def dice_coefficient_loss(y_true, y_pred):
    return -dice_coefficient(y_true, y_pred)


def vod_coefficient_loss(y_true, y_pred):
    return -vod_coefficient(y_true, y_pred, binarize=False)


def double_dice_loss(y_true, y_pred, ratio=10.0):
    return -dice_coefficient(y_true, y_pred) + ratio * dice_coefficient(1 - _f(y_true), y_pred)


def weighted_dice_coefficient(y_true, y_pred, axis=(-3, -2, -1), smooth=0.00001):
    yt, yp = _f(y_true), _f(y_pred)
    return np.mean(2. * (np.sum(yt * yp, axis=axis) + smooth / 2) / (np.sum(yt, axis=axis) + np.sum(yp, axis=axis) + smooth))


def weighted_dice_coefficient_loss(y_true, y_pred):
    return -weighted_dice_coefficient(y_true, y_pred)


def label_wise_dice_coefficient(y_true, y_pred, label_index):
    return dice_coefficient(_f(y_true)[..., label_index], _f(y_pred)[..., label_index])


def get_label_dice_coefficient_function(label_index):
    f = partial(label_wise_dice_coefficient, label_index=label_index)
    f.__setattr__('__name__', 'label_{0}_dice_coef'.format(label_index))
    return f


def label_wise_metrics(n_labels, include_label_wise_dice_coefficients):
    """the metrics reference unet3d/unet.py:75-80 (commented out there) adds: one label-wise Dice per label when the flag is set and the
    model has several labels, else none"""
    if include_label_wise_dice_coefficients and n_labels > 1:
        return [get_label_dice_coefficient_function(i) for i in range(n_labels)]
    return []


def weighted_cross_entropy_loss(y_true, y_pred, weight_mask=None):
    yt = _f(y_true)
    yp = np.clip(_f(y_pred), 1e-7, 1 - 1e-7)
    xent = -(yt * np.log(yp) + (1 - yt) * np.log(1 - yp))
    if weight_mask is not None:
        xent = weight_mask * xent
    return np.mean(xent)


def binary_crossentropy(y_true, y_pred):
    yt = _f(y_true)
    yp = np.clip(_f(y_pred), 1e-7, 1 - 1e-7)
    return np.mean(-(yt * np.log(yp) + (1 - yt) * np.log(1 - yp)), axis=-1)


def dice_and_xent(y_true, y_pred, xent_weight=1.0, weight_mask=None):
    return dice_coef_loss(y_true, y_pred) + xent_weight * weighted_cross_entropy_loss(y_true, y_pred, weight_mask)


def _focal_loss(gamma=2., alpha=.5):
    def focal_loss_fixed(y_true, y_pred):
        yt, yp = _f(y_true), _f(y_pred)
        pt_1 = np.where(yt == 1, yp, np.ones_like(yp))
        pt_0 = np.where(yt == 0, yp, np.zeros_like(yp))
        return -np.sum(alpha * (1. - pt_1) ** gamma * np.log(pt_1)) - np.sum((1 - alpha) * pt_0 ** gamma * np.log(1. - pt_0))

    return focal_loss_fixed


class MaskInput(object):
    """placeholder for the model's second input (the distance mask) that `dice_and_xent_mask` closes over in the reference
    (isensee2017.py:85-88: loss_function = loss_function(mask_input))"""


def dice_and_xent_mask(weight_mask, xent_weight=1.0, dist_sigma=3):
    def _loss(y_true, y_pred):
        return dice_and_xent(y_true, y_pred, xent_weight=xent_weight, weight_mask=np.exp(-_f(weight_mask) / dist_sigma))

    # what the device path needs to know: Dice + xent_weight * mean(exp(-mask / dist_sigma) * cross-entropy), mask = 2nd model input
    _loss.mask_weighted = isinstance(weight_mask, MaskInput)
    _loss.xent_weight, _loss.dist_sigma = float(xent_weight), float(dist_sigma)
    _loss.__name__ = "dice_and_xent_mask"
    return _loss


# ---- overlap losses beyond the reference's table (DESIGN.md "Overlap losses"): functions of the per-label sums I = sum y p, Sy = sum y,
# Sp = sum p, labels on the LAST axis as in label_wise_dice_coefficient.  On the device: fmri_overlap_coeffs / fmri_overlap_loss_bwd.
def _label_sums(y_true, y_pred, per_label=True):
    """I, Sy, Sp: one float64 array entry per label, or (per_label=False) of everything together - each summed as dice_coefficient sums"""
    yt, yp = _f(y_true), _f(y_pred)
    cols = [(yt[..., l].ravel(), yp[..., l].ravel()) for l in range(yt.shape[-1])] if per_label else [(yt.ravel(), yp.ravel())]
    return (np.array([np.sum(t * p) for t, p in cols]), np.array([np.sum(t) for t, _ in cols]), np.array([np.sum(p) for _, p in cols]))


def _tversky(i, sy, sp, alpha, beta, smooth):
    # I + alpha (Sp - I) + beta (Sy - I) + s, written so that alpha = beta = s = 1/2 is dice_coefficient(smooth=1) to the last bit
    return (i + smooth) / ((1. - alpha - beta) * i + (beta * sy + alpha * sp) + smooth)


def tversky_coefficient(y_true, y_pred, alpha=0.3, beta=0.7, smooth=1.0, per_label=False):
    """(I + s) / (I + alpha FP + beta FN + s) with the soft counts FP = Sp - I, FN = Sy - I: over all labels together, or
    (per_label=True) the mean of the labels' own coefficients.  alpha = beta = s = 1/2 is dice_coefficient(smooth=1)."""
    i, sy, sp = _label_sums(y_true, y_pred, per_label)
    return float(np.mean(_tversky(i, sy, sp, alpha, beta, smooth)))


def _overlap_token(fn, name, kind, **params):
    fn.__name__ = name
    fn.overlap_kind = kind                     # fmri_overlap_coeffs' kind
    fn.loss_params = dict(params)              # what a checkpoint records next to the name (keras_h5 / training.load_old_model)
    for k, v in params.items():
        setattr(fn, k, v)
    return fn


def tversky_loss(alpha=0.3, beta=0.7, smooth=1.0, per_label=False):
    """-tversky_coefficient: beta > alpha punishes false negatives harder than false positives (Salehi et al. 2017)"""
    alpha, beta, smooth, per_label = float(alpha), float(beta), float(smooth), bool(per_label)

    def _loss(y_true, y_pred):
        return -tversky_coefficient(y_true, y_pred, alpha, beta, smooth, per_label)

    return _overlap_token(_loss, "tversky_loss", 2 if per_label else 0, alpha=alpha, beta=beta, smooth=smooth, per_label=per_label)


def focal_tversky_loss(alpha=0.3, beta=0.7, gamma=4. / 3, smooth=1.0, per_label=False):
    """(1 - T)^(1/gamma) (Abraham & Khan 2019); per_label: the mean over the labels.  (The device gradient takes the derivative at
    max(1 - T, 1e-7): it has a pole at T = 1 for gamma > 1.)"""
    alpha, beta, gamma, smooth, per_label = float(alpha), float(beta), float(gamma), float(smooth), bool(per_label)

    def _loss(y_true, y_pred):
        i, sy, sp = _label_sums(y_true, y_pred, per_label)
        return float(np.mean(np.maximum(1. - _tversky(i, sy, sp, alpha, beta, smooth), 0.) ** (1. / gamma)))

    return _overlap_token(_loss, "focal_tversky_loss", 3 if per_label else 1, alpha=alpha, beta=beta, gamma=gamma, smooth=smooth,
                          per_label=per_label)


def generalised_dice_loss(y_true, y_pred, smooth=1e-5):
    """1 - (2 sum_l w_l I_l + s) / (sum_l w_l (Sy_l + Sp_l) + s), w_l = 1 / Sy_l^2 (Sudre et al. 2017).  A label absent from the batch takes
    the largest weight among the labels present; with no label present all weights are 1."""
    i, sy, sp = _label_sums(y_true, y_pred)
    present = sy > 0
    w = np.ones_like(sy)
    if present.any():
        w = np.where(present, 1. / np.where(present, sy, 1.) ** 2, 0.)
        w = np.where(present, w, w.max())
    return float(1. - (2. * np.sum(w * i) + smooth) / (np.sum(w * (sy + sp)) + smooth))


generalised_dice_loss.overlap_kind = 4
generalised_dice_loss.smooth = 1e-5
generalized_dice_loss = generalised_dice_loss


def dice_and_boundary(mask_input, boundary_weight=0.01):
    """dice_coefficient_loss + boundary_weight * mean(phi * p), phi = (1 - 2 y) * mask the signed distance to the boundary (negative inside;
    Kervadec et al. 2019).  mask_input: the model's second input, RAW - each voxel's distance to the nearest voxel of the other class, as the
    generators yield it ([x, masks]); single label."""
    boundary_weight = float(boundary_weight)

    def _loss(y_true, y_pred):
        yt, yp = _f(y_true), _f(y_pred)
        return dice_coefficient_loss(yt, yp) + boundary_weight * np.mean((1. - 2. * yt) * _f(mask_input) * yp)

    _loss.mask_input = isinstance(mask_input, MaskInput)          # the device path feeds the model's second input to the loss kernels
    _overlap_token(_loss, "dice_and_boundary", 0, boundary_weight=boundary_weight)
    _loss.alpha = _loss.beta = _loss.smooth = 0.5                 # Tversky(1/2, 1/2, s = 1/2) = dice_coefficient(smooth = 1)
    return _loss


dice_coef = dice_coefficient
dice_coef_loss = dice_coefficient_loss
binary_crossentropy_loss = binary_crossentropy
focal_loss = _focal_loss()

# losses differentiated on the device (fmri_sigmoid_loss_bwd); the rest build but raise at the first training step
DEVICE_LOSSES = (dice_coefficient_loss, binary_crossentropy_loss, dice_and_xent, focal_loss, vod_coefficient_loss, double_dice_loss,
                 weighted_dice_coefficient_loss)
# ... and from per-label sums (fmri_overlap_loss_bwd): a token, or what one of these factories returns
OVERLAP_LOSSES = (tversky_loss, focal_tversky_loss, generalised_dice_loss, dice_and_boundary)
