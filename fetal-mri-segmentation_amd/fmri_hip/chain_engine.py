"""A trainable network in front of a FROZEN segmenter, as one engine (reference fetal_net/model/norm/NormNet.py:10-30: `norm_net_model`).

    x -> norm net (LayerGraphEngine with a linear output) -> logits, fp32 -> cast to the segmenter's dtype -> segmenter -> loss

One training step: norm forward; cast; segmenter forward + loss; segmenter backward(params=False), which ends in dL/d(its input);
that gradient is the `dprobs` of the norm net's backward(seg_loss=False); the optimizer steps the norm net only.  Nothing of the segmenter moves: its
P, M, V, t and BatchNormalization moving statistics are bit-identical after any number of steps.

Frozen-segmenter semantics (the precedent of fetal_net.adversarial.CombinedModel, and Keras 2.2 under learning phase 1 with
`trainable = False`): in a training step the frozen network RUNS IN TRAINING MODE - its SpatialDropout is active and BatchNormalization
normalises with the batch statistics - but the moving averages are not updated.  predict() and evaluation run both networks in inference
mode.

The two networks may compute in different dtypes.  The object has the duck type `fetal_net.engine_model.Model` and the device tile loop of
`patch_wise_prediction` use; every buffer is allocated in set_batch, so predict() can be captured in a hipGraph.
"""
import torch

from . import ops


class ChainEngine(object):
    def __init__(self, norm, seg):
        if not getattr(norm, "linear", False):
            raise ValueError("the network in front must have a linear output (isensee2017_model_3d(activation_name=None))")
        if not getattr(seg, "input_grad", False) or not seg.training:
            raise ValueError("the frozen segmenter's engine must be built with input_grad=True")
        if getattr(norm, "deterministic", False) != getattr(seg, "deterministic", False) or (
                getattr(seg, "deterministic", False) and not getattr(seg, "frozen", False)):
            raise ValueError("FMRI_DETERMINISTIC=1: the network in front holds the deterministic-gradient registration, the segmenter's engine "
                             "must be built frozen=True under the same switch")
        self.norm, self.seg = norm, seg
        self.deterministic = bool(getattr(norm, "deterministic", False))       # both engines on ordered routes, the registration is norm's
        self.dtype, self.dev, self.training, self.dist = norm.dtype, norm.dev, norm.training, norm.dist
        self.plan = seg.plan                     # output geometry: labels and spatial dims of the segmenter
        self.sums = seg.sums                     # the metric sums are the segmenter's (one tensor for the engine's lifetime)
        self._xseg = {}
        # the segmenter's input: UNetEngine takes its logical channels, a channel-padded LayerGraphEngine its physical ones (zeros behind)
        self._cin = norm.plan.n_labels
        self._cseg = seg.shape[seg.input_name][0] if hasattr(seg, "input_name") else seg.plan.in_channels
        self._moving = dict(update_moving=False) if hasattr(seg, "moving") else {}
        self.set_batch(norm.N)

    # ---- what Model reads and sets on its engine: the loss is the segmenter's, parameters and optimizer state are the norm net's
    loss_kind = property(lambda self: self.seg.loss_kind, lambda self, v: setattr(self.seg, "loss_kind", v))
    loss_param = property(lambda self: self.seg.loss_param, lambda self, v: setattr(self.seg, "loss_param", v))
    loss_overlap = property(lambda self: self.seg.loss_overlap, lambda self, v: setattr(self.seg, "loss_overlap", v))
    beta1 = property(lambda self: self.norm.beta1, lambda self, v: setattr(self.norm, "beta1", v))
    t = property(lambda self: self.norm.t, lambda self, v: setattr(self.norm, "t", v))
    P = property(lambda self: self.norm.P)
    G = property(lambda self: self.norm.G)
    M = property(lambda self: self.norm.M)
    V = property(lambda self: self.norm.V)
    Vhat = property(lambda self: self.norm.Vhat)
    opt = property(lambda self: self.norm.opt)
    n_flat = property(lambda self: self.norm.n_flat)
    N = property(lambda self: self.norm.N)
    logits = property(lambda self: self.seg.logits)
    probs = property(lambda self: self.seg.probs)
    _dummy_y = property(lambda self: self.seg._dummy_y)
    label_metrics = property(lambda self: self.seg.label_metrics)

    def set_label_metrics(self, n):
        self.seg.set_label_metrics(n)

    def log_sums(self):
        return self.seg.log_sums()

    def keras_to_flat(self, W):
        return self.norm.keras_to_flat(W)

    def flat_to_keras(self, host, moving=True):
        return self.norm.flat_to_keras(host, moving=moving)

    def load_keras_weights(self, W):
        self.norm.load_keras_weights(W)

    def export_keras_weights(self):
        return self.norm.export_keras_weights()

    def close(self):
        self.norm.close()

    def adam_step(self, lr, **kw):
        self.norm.adam_step(lr, **kw)

    def set_optimizer(self, spec=None):
        self.norm.set_optimizer(spec)

    def optimizer_step(self, lr, **kw):
        self.norm.optimizer_step(lr, **kw)

    @staticmethod
    def metrics_from_sums(s, smooth=1.0, loss_kind=0, loss_param=1.0):
        from .engine_base import EngineBase
        return EngineBase.metrics_from_sums(s, smooth, loss_kind, loss_param)

    # ---- buffers
    def set_batch(self, N):
        self.norm.set_batch(N)
        self.seg.set_batch(N)
        if N not in self._xseg:
            self._xseg[N] = torch.zeros((N,) + tuple(self.plan.spatial) + (self._cseg,), dtype=self.seg.dtype, device=self.dev)
        self.x_seg = self._xseg[N]

    # ---- steps
    def forward(self, x, bn_training=None):
        self.norm.forward(x, bn_training=bn_training)
        lg = self.norm.logits                     # fp32 [nvox][labels]: the normalised volume
        if self._cseg == self._cin:
            ops.cast(lg.reshape(-1), self.x_seg.reshape(-1))
        else:
            self.x_seg.view(-1, self._cseg)[:, :self._cin].copy_(lg)
        kw = self._moving if (self.training if bn_training is None else bn_training) else {}
        return self.seg.forward(self.x_seg, bn_training=bn_training, **kw)

    def loss_forward(self, y_true, weight=None):
        return self.seg.loss_forward(y_true, weight)

    def predict(self, x):
        self.forward(x, bn_training=False)
        self.seg.sums.zero_()
        ops.sigmoid_dice_fwd(self.seg.logits, self.seg._dummy_y, self.seg.probs, self.seg.sums)
        return self.seg.probs

    def backward(self, y_true, grad_scale=1.0, weight=None):
        """after forward + loss_forward: the segmenter's frozen pass down to dL/d(its input), then the norm net's backward on that gradient"""
        self.seg.backward(y_true, grad_scale=grad_scale, weight=weight, params=False)
        self.norm.backward(self.norm._dummy_y, dprobs=self.seg.input_gradient(), dprobs_scale=1.0, seg_loss=False)

    def train_step(self, x, y_true, lr, weight=None):
        self.forward(x)
        self.seg.loss_forward(y_true, weight)
        self.backward(y_true, grad_scale=(self.dist.grad_scale if self.dist is not None else 1.0), weight=weight)
        self.norm.optimizer_step(lr)
        return self.seg.sums
