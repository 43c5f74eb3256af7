"""Float64 numpy restatement of the optimizer updates of include/fmri_hip.h (fmri_sgd_step, fmri_rmsprop_step, fmri_adam_step_ex) and of
the gradient they see.  Source: Keras 2.2.4 keras/optimizers.py as published (Optimizer.get_gradients, clip_norm, SGD / RMSprop / Adam
.get_updates).  PARITY-UNPINNED: no Keras could be run next to it, so this file pins the kernels to the published formulas as restated
here, not to a Keras run.

Inputs are the float32 arrays the kernels read; hyper-parameters are rounded to float32 first (the kernels receive floats); everything
after that is float64.  `bounds` holds the rounding counts the tests assert (derivation in tests/test_gpu_optimizers.py).
"""
import math

import numpy as np

U = 2.0 ** -24          # unit roundoff of float32


def f32(v):
    return float(np.float32(v))


def gradient(G, grad_scale=1.0, norm=None, clipnorm=0.0, clipvalue=0.0):
    """g = grad_scale * G; norm >= clipnorm > 0: g * clipnorm / norm; clipvalue > 0: clamp.  norm: the float32 value the kernel reads."""
    g = f32(grad_scale) * np.asarray(G, np.float64)
    clipnorm, clipvalue = f32(clipnorm or 0.0), f32(clipvalue or 0.0)
    if norm is not None and clipnorm > 0.0 and f32(norm) >= clipnorm:
        g = g * clipnorm / f32(norm)
    if clipvalue > 0.0:
        g = np.clip(g, -clipvalue, clipvalue)
    return g


def lr_at(lr, decay, k):
    """the learning rate of step k (1-based): Keras multiplies by 1 / (1 + decay * iterations) with the count BEFORE the step"""
    return lr / (1.0 + decay * (k - 1))


def adam_lr_t(lr, beta_1, beta_2, k):
    return lr * math.sqrt(1.0 - beta_2 ** k) / (1.0 - beta_1 ** k)


def sgd_slot(g, m, lr, momentum):
    """-> (v, a*s, b*h): the new moment and the two terms it is blended from"""
    lr, momentum = f32(lr), f32(momentum)
    m = np.asarray(m, np.float64)
    return momentum * m - lr * g, momentum * m, lr * g


def sgd_increment(g, v, lr, momentum, nesterov):
    """the parameter increment from the NEW moment v"""
    lr, momentum = f32(lr), f32(momentum)
    v = np.asarray(v, np.float64)
    return momentum * v - lr * g if nesterov else v


def rmsprop_slot(g, a, rho):
    rho = f32(rho)
    a = np.asarray(a, np.float64)
    return rho * a + (1.0 - rho) * g * g, rho * a, (1.0 - rho) * g * g


def rmsprop_increment(g, a_new, lr, eps):
    return -f32(lr) * g / (np.sqrt(np.asarray(a_new, np.float64)) + f32(eps))


def adam_slots(g, m, v, beta_1, beta_2):
    b1, b2 = f32(beta_1), f32(beta_2)
    m, v = np.asarray(m, np.float64), np.asarray(v, np.float64)
    return (b1 * m + (1.0 - b1) * g, b1 * m, (1.0 - b1) * g), (b2 * v + (1.0 - b2) * g * g, b2 * v, (1.0 - b2) * g * g)


def adam_increment(m_new, denom_new, lr_t, eps):
    """denom_new: the new v, or the new vhat = max(vhat, v) with AMSGrad"""
    return -f32(lr_t) * np.asarray(m_new, np.float64) / (np.sqrt(np.asarray(denom_new, np.float64)) + f32(eps))


def slot_bound(a_s, b_h):
    return 16.0 * U * (np.abs(a_s) + np.abs(b_h))


def param_bound(p_new, delta):
    return U * np.abs(p_new) + 8.0 * U * np.abs(delta)
