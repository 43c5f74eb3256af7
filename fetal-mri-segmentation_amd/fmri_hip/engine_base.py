"""What the two engines share: `UNetEngine` (engine.py, the hand-scheduled U-Net) and `LayerGraphEngine` (graph_engine.py, the layer-graph
interpreter) differ in how they schedule a step, not in what surrounds the schedule.

`EngineBase` holds that part: the flat fp32 parameter store (P, its gradient G and the optimizer slots M / V, all in the engine's `layout`),
the loss head (sigmoid + metric sums, the seg-loss gradient), the Keras optimizers (Adam by default; SGD, RMSprop, AMSGrad and gradient
clipping through set_optimizer: one launch per step for each), Keras weight export / import and the weight-gradient side stream.  An
engine sets `layout` / `n_flat` and calls `_alloc_params`, keeps `logits` / `probs` / `dlogits` / `_dummy_y` of the current batch, and
provides `forward`, `backward`, `refresh_weight_copies`, `keras_to_flat` and `flat_to_keras`.

`read_switches` is the one place where the engines look at their FMRI_* environment switches: once, in `__init__`, into `self.sw`.  Buffers
are sized and kernel routes planned from those values, so a switch that changes afterwards changes nothing (nor under a captured hipGraph).

The module-level helpers convert Keras kernels: a Glorot-uniform draw, and a conv kernel (k,)*nd + (Cin, Cout) <-> the flat
[k^3][Cout][Cin] image the engines keep in P (a 2-D kernel is the centre kd plane of that image).
"""
import math
import os
import weakref

import numpy as np
import torch

from . import ops
from ._lib import lib


def read_switches(**defaults):
    """FMRI_<NAME> for every NAME=default given.  A True default is on unless the variable is "0", a False one is off unless it is "1",
    an int default is replaced by int(value)."""
    out = {}
    for name, d in defaults.items():
        v = os.environ.get("FMRI_" + name)
        out[name] = d if v is None else (v != "0") if d is True else (v == "1") if d is False else int(v)
    return out


_DET_OWNER = []          # [weakref to the engine that holds the process-wide fmri_set_deterministic registration]
_DET_SCRATCH = []        # [the slab of the ordered normalisation statistics, as registered with fmri_set_deterministic_scratch]


def _release_deterministic(token):
    if _DET_OWNER and _DET_OWNER[0] is token:
        _DET_OWNER.clear()
        _DET_SCRATCH.clear()
        try:
            ops.set_deterministic(None, None)                # (takes the scratch registration back as well)
        except Exception:                                    # interpreter shutdown: the library may be gone already
            pass


def register_deterministic(eng, grad, shadow):
    """fmri_set_deterministic keeps raw device pointers process-wide: ONE engine may hold the registration, and it is given back when
    that engine dies or is closed (a stale registration redirected a later engine's gradients into freed memory).
    grad: the buffer the engine's gradient kernels write (dw / db pointers), shadow: its zeroed int64 twin."""
    if _DET_OWNER and _DET_OWNER[0]() is not None:
        raise RuntimeError("FMRI_DETERMINISTIC=1: another engine of this process holds the deterministic-gradient registration "
                           "(one deterministic engine per process at a time; call its close() first)")
    _DET_OWNER.clear()
    ref = weakref.ref(eng)
    _DET_OWNER.append(ref)
    ops.set_deterministic(grad, shadow, _DET_SCRATCH[0] if _DET_SCRATCH else None)
    eng._det_finalizer = weakref.finalize(eng, _release_deterministic, ref)


def reserve_deterministic_scratch(nbytes, dev):
    """the process-wide slab of the ordered normalisation statistics holds at least nbytes from here on.  It only grows; every engine
    of the process - the registered one and a frozen one next to it - shares it, their normalisation calls being ordered on one stream."""
    if nbytes <= 0 or (_DET_SCRATCH and _DET_SCRATCH[0].numel() * 8 >= nbytes):
        return
    _DET_SCRATCH[:] = [torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)]
    ops.set_deterministic_scratch(_DET_SCRATCH[0])


def refuse_overlap_data_parallel(loss_kind, dist_ctx):
    """the overlap losses are differentiated from per-label sums, which no data-parallel context all-reduces: refused by name there"""
    if ops.is_overlap_loss(loss_kind) and dist_ctx is not None and dist_ctx.world > 1:
        name = [k for k, v in ops.LOSS_KINDS.items() if v == loss_kind][0]
        raise NotImplementedError("%s (with dice_and_boundary, one of the overlap losses: %s) is differentiated from per-label sums, which "
                                  "are not all-reduced: data-parallel training takes one of the other losses"
                                  % (name, ", ".join(sorted(k for k, v in ops.LOSS_KINDS.items() if ops.is_overlap_loss(v)))))


# The optimizer of EngineBase.optimizer_step: Keras 2.2.4's Adam / SGD / RMSprop with their argument names (keras/optimizers.py as
# published; parity-unpinned, see include/fmri_hip.h).  The default is the plain Adam every builder compiles with.
DEFAULT_OPTIMIZER = dict(kind="adam", beta_1=0.9, beta_2=0.999, epsilon=1e-7, decay=0.0, amsgrad=False,      # adam
                         momentum=0.0, nesterov=False,                                                       # sgd
                         rho=0.9,                                                                            # rmsprop (epsilon, decay: above)
                         clipnorm=0.0, clipvalue=0.0)


class EngineBase(object):
    def __init__(self, dtype, device, training, dist_ctx, frozen=False, **switches):
        """switches: the engine's own FMRI_* switches and their defaults (read_switches), next to FMRI_WGRAD_STREAM and FMRI_DETERMINISTIC
        which both engines have"""
        lib()  # fail loudly if the HIP library is missing
        self.dtype, self.dev, self.training, self.dist = dtype, torch.device(device), training, dist_ctx
        self.sw = read_switches(WGRAD_STREAM=True, DETERMINISTIC=False, **switches)
        # FMRI_DETERMINISTIC=1: bit-reproducible training steps (same weights + same batch -> the same bits in every gradient and metric).
        # Gradient partial sums meet as fixed-point integers in a shadow of the buffer the gradient kernels write (_det_register), the
        # normalisation reductions add their workgroups' partials in block order (_det_reserve_norm), and the engines keep to kernel
        # routes whose sums are ordered.  One registered engine per process at a time.
        # frozen: an engine that is only ever run with backward(params=False) next to the registered one (the segmenter of
        # norm_net_model): it writes no parameter gradient anybody reads, so it takes no registration, but it runs the ordered routes.
        self.deterministic = bool(training and self.dev.type == "cuda" and self.sw["DETERMINISTIC"])
        self.frozen = bool(frozen)
        self.t = 0                       # optimizer step counter (Keras' `iterations`)
        self.beta1 = 0.9                 # Adam's beta_1 when adam_step is given none (fetal_net.adversarial sets the optimizer's)
        self.opt = dict(DEFAULT_OPTIMIZER)            # what optimizer_step runs (set_optimizer)
        self.Vhat = None                              # AMSGrad's running maximum of V: allocated by set_optimizer when asked for
        self._gnorm_work = self._gnorm = None         # clipnorm: workspace and {sum of squares, norm} of ops.grad_sumsq
        self.loss_kind, self.loss_param = 0, 1.0      # ops.LOSS_KINDS: 0 = dice_coefficient_loss
        self.loss_overlap = (0.5, 0.5, 1.0, 0.0)      # (alpha, beta, gamma, boundary_weight) of an overlap loss; loss_param is its smooth
        # the weight gradients run on their own stream (FMRI_WGRAD_STREAM=0: on the main stream)
        self._wg_stream = torch.cuda.Stream(device=self.dev) if (training and self.dev.type == "cuda" and self.sw["WGRAD_STREAM"]) else None
        # ONE tensor for the engine's lifetime: captured hipGraphs of other batch sizes keep its address (re-creating it per buffer
        # set left them writing into freed memory, which the allocator then handed to the tile index list of the next volume)
        # Behind the 16 metric sums, in the same tensor: the 3 * L label-wise sums (ops.label_sums) of a model that carries label-wise Dice
        # metrics (label_metrics = L, set by the model; 0: no launch, nothing read back) - one pinned read-back takes both (log_sums).
        # Behind those, for the overlap losses only (ops.SUMS_BD ...): the boundary sum, the coefficient pairs and the loss value
        self._sums_all = torch.zeros(ops.SUMS_TOTAL, dtype=torch.float64, device=self.dev)
        self.sums = self._sums_all[:16]
        self.label_metrics = 0

    def _alloc_params(self):
        """P in the engine's layout (n_flat fp32 values) and, when training, G, M and V of the same size"""
        self.P = torch.zeros(self.n_flat, dtype=torch.float32, device=self.dev)
        if self.training:
            self.G, self.M, self.V = torch.zeros_like(self.P), torch.zeros_like(self.P), torch.zeros_like(self.P)

    # ------------------------------------------------------------------------------------------------ deterministic mode
    def _det_register(self, grad):
        """deterministic mode: the int64 shadow G64 of `grad` - the buffer the weight-gradient kernels of this engine write - and the
        process-wide registration (a frozen engine takes none)"""
        if not self.deterministic or self.frozen:
            return
        self._det_grad = grad
        self.G64 = torch.zeros(grad.numel(), dtype=torch.int64, device=self.dev)
        register_deterministic(self, grad, self.G64)

    def _det_reserve_norm(self, calls):
        """deterministic mode: room in the ordered-statistics slab for every normalisation call (N, V, C, per_instance) of a buffer set"""
        if self.deterministic:
            reserve_deterministic_scratch(max([ops.norm_det_workspace_bytes(*c) for c in calls] + [0]), self.dev)

    def _det_finish(self):
        """end of backward: the registered buffer += the fixed-point sums of every gradient kernel of this pass"""
        if self.deterministic and not self.frozen:
            ops.deterministic_finish(self._det_grad, self.G64)

    def _det_check_backward(self, params):
        if self.deterministic and self.frozen and params:
            raise NotImplementedError("FMRI_DETERMINISTIC=1: this engine was built frozen (it holds no deterministic-gradient registration): "
                                      "backward(params=False) only")

    def close(self):
        """give up the process-wide deterministic registration (FMRI_DETERMINISTIC=1; also done when the engine is garbage-collected)"""
        fin = self.__dict__.pop("_det_finalizer", None)
        if fin is not None:
            fin()

    # ------------------------------------------------------------------------------------------------ Keras weights
    def load_keras_weights(self, W):
        self.P.copy_(torch.from_numpy(self.keras_to_flat(W)))
        self.refresh_weight_copies()

    def export_keras_weights(self):
        return self.flat_to_keras(self.P.detach().cpu().numpy())

    # ------------------------------------------------------------------------------------------------ loss
    def loss_forward(self, y_true, weight=None):
        """y_true uint8 [nvox*L] device.  probs + the 8 metric sums (accumulated into zeroed self.sums)."""
        self.sums.zero_()
        overlap = ops.is_overlap_loss(self.loss_kind)
        if overlap:
            weight, dist = None, weight              # the model's second input is the distance mask itself (dice_and_boundary)
            refuse_overlap_data_parallel(self.loss_kind, self.dist)
        ops.sigmoid_dice_fwd(self.logits, y_true, self.probs, self.sums, weight=weight)
        if self.label_metrics or overlap:
            # (one launch for both: the label-wise metrics read the sums the loss is differentiated from)
            ops.label_sums(self.probs.reshape(-1), y_true, self.plan.n_labels, self._sums_all[16:])
        if overlap:
            L = self.plan.n_labels
            alpha, beta, gamma, bweight = self.loss_overlap
            bd = None
            if dist is not None:
                bd = self._sums_all[ops.SUMS_BD:ops.SUMS_BD + 1]
                ops.boundary_sum(self.probs.reshape(-1), y_true, dist, bd)
            ops.overlap_coeffs(self._sums_all[16:], self.sums, self._overlap_coef(), L, self.loss_kind - ops.LOSS_OVERLAP, alpha, beta, gamma,
                               self.loss_param, bd=bd, boundary_weight=bweight)
        if self.loss_kind == ops.LOSS_WEIGHTED_DICE:
            ns, nl = self._wdice_groups()
            if getattr(self, "_gsums", None) is None or self._gsums.numel() < 3 * ns * nl:
                self._gsums = torch.zeros(3 * ns * nl, dtype=torch.float64, device=self.dev)
            ops.weighted_dice_fwd(self.probs, y_true, self._gsums, self.sums, ns, nl)
        if self.dist is not None and self.dist.world > 1 and self.dist.global_dice:
            self.dist.all_reduce_sums(self.sums)
        return self.sums

    def _overlap_coef(self):
        """the [L][2] coefficient pairs + two value slots of the overlap losses, ending at the fixed value slots of _sums_all"""
        return self._sums_all[ops.SUMS_OVERLAP_VALUE - 2 * self.plan.n_labels:]

    def log_sums(self):
        """what a step's read-back copies: the 16 metric sums, with the [L][3] label-wise sums behind them when label_metrics is set; an
        overlap loss: the whole tensor, the loss value of fmri_overlap_coeffs included"""
        if ops.is_overlap_loss(self.loss_kind):
            return self._sums_all
        return self._sums_all[:16 + 3 * self.label_metrics] if self.label_metrics else self.sums

    def set_label_metrics(self, n):
        """n = the model's label count when it carries label_<i>_dice_coef metrics, else 0"""
        n = int(n)
        if n and n != self.plan.n_labels:
            raise ValueError("label-wise metrics for %d labels on an engine with %d" % (n, self.plan.n_labels))
        if n and self.dist is not None and self.dist.world > 1:
            raise NotImplementedError("label-wise Dice metrics (include_label_wise_dice_coefficients) are not all-reduced: build the model "
                                      "without them for data-parallel training")
        self.label_metrics = n

    def _wdice_groups(self):
        """(groups along the batch axis, labels per group) of weighted_dice_coefficient's axis=(-3,-2,-1) (reference metrics.py:39): the 3-D
        models' (N, labels, X, Y, Z) tensors give one Dice per (sample, label), the 2-D models' (N, X, Y, labels) one per slice"""
        if self.plan.ndim == 2:
            return self.N, 1
        return self.N, self.plan.n_labels

    def predict(self, x):
        self.forward(x, bn_training=False)
        self.sums.zero_()
        # sigmoid only (y_true is irrelevant for probs): reuse the fused kernel with an all-zero label buffer
        ops.sigmoid_dice_fwd(self.logits, self._dummy_y, self.probs, self.sums)
        return self.probs

    def _seg_loss_bwd(self, y_true, grad_scale, weight, dprobs, dprobs_scale, seg_loss):
        """dlogits of the segmentation loss (after loss_forward), plus the chain of an outside gradient `dprobs` on the probabilities"""
        if seg_loss and self.loss_kind == ops.LOSS_WEIGHTED_DICE:
            ns, nl = self._wdice_groups()
            ops.weighted_dice_bwd(self.probs, y_true, self._gsums, self.sums, self.dlogits, ns, nl, grad_scale=grad_scale)
        elif seg_loss and ops.is_overlap_loss(self.loss_kind):
            L = self.plan.n_labels
            bscale = self.loss_overlap[3] / float(self.probs.numel() // L) if weight is not None else 0.0
            ops.overlap_loss_bwd(self.probs.reshape(-1), y_true, self._overlap_coef(), self.dlogits.reshape(-1), L, dist=weight,
                                 boundary_scale=bscale, grad_scale=grad_scale)
        elif seg_loss:
            ops.sigmoid_loss_bwd(self.probs, y_true, self.sums, self.dlogits, self.loss_kind, self.loss_param, smooth=1.0, grad_scale=grad_scale,
                                 weight=weight)
        if dprobs is not None:
            ops.sigmoid_chain(self.probs, dprobs, self.dlogits, scale=dprobs_scale, accumulate=seg_loss)

    # ------------------------------------------------------------------------------------------------ weight-gradient stream
    def _wgrad(self, fn):
        """run fn, which enqueues weight-gradient kernels, on the side stream behind everything the main stream has enqueued so far
        (inline without a side stream).  The weight gradients are off the critical path of the backward pass (nothing reads them before
        the optimizer step): they run next to the input-gradient chain of the main stream.  (A third stream for the U-Net's first conv's
        weight gradient - HBM-bound, ready last - measured nothing: 13.09-13.13 ms either way.)"""
        if self._wg_stream is None:
            fn()
            return
        self._wg_stream.wait_stream(torch.cuda.current_stream(self.dev))
        with torch.cuda.stream(self._wg_stream):
            fn()

    def _join_wgrad(self):
        """end of backward: the main stream waits for the side stream's weight gradients"""
        if self._wg_stream is not None:
            torch.cuda.current_stream(self.dev).wait_stream(self._wg_stream)

    def grad_streams(self):
        """streams that enqueue parameter-gradient kernels during backward (a gradient bucket is complete when all of them got there)"""
        return [st for st in (getattr(self, "_main_stream", None), self._wg_stream) if st is not None]

    # ------------------------------------------------------------------------------------------------ optimizer
    def adam_step(self, lr, beta1=None, beta2=0.999, eps=1e-7, grad_scale=1.0):
        beta1 = self.beta1 if beta1 is None else beta1
        self.t += 1
        lr_t = lr * math.sqrt(1.0 - beta2 ** self.t) / (1.0 - beta1 ** self.t)
        ops.adam_step(self.P, self.G, self.M, self.V, lr_t, beta1, beta2, eps, grad_scale)
        self.refresh_weight_copies()

    def set_optimizer(self, spec=None):
        """spec: the keys of DEFAULT_OPTIMIZER that differ from it (fetal_net.optimizers' objects give theirs; None = the default, plain
        Adam).  SGD keeps its moments in M, RMSprop its accumulators in V, AMSGrad gets a third buffer Vhat; the sum-of-squares workspace
        and its two float64 results exist only with clipnorm > 0.  A change of the optimizer kind starts the slots and the step count
        afresh."""
        spec = dict(spec or {})
        unknown = sorted(set(spec) - set(DEFAULT_OPTIMIZER))
        if unknown:
            raise ValueError("optimizer spec: unknown key(s) %s" % ", ".join(unknown))
        opt = dict(DEFAULT_OPTIMIZER, **spec)
        if opt["kind"] not in ("adam", "sgd", "rmsprop"):
            raise ValueError("optimizer kind %r (this engine steps adam, sgd and rmsprop)" % (opt["kind"],))
        for k in ("clipnorm", "clipvalue"):                   # Keras: a clip argument that is not > 0 is off
            opt[k] = float(opt[k]) if opt[k] is not None and float(opt[k]) > 0.0 else 0.0
        if self.training and opt["kind"] != self.opt["kind"]:
            self.M.zero_()
            self.V.zero_()
            self.t = 0
        if opt["kind"] == "adam":
            self.beta1 = float(opt["beta_1"])
        if self.training and opt["kind"] == "adam" and opt["amsgrad"] and self.Vhat is None:
            self.Vhat = torch.zeros_like(self.P)
        if self.training and opt["clipnorm"] > 0.0 and self._gnorm is None:
            self._gnorm_work, self._gnorm = ops.grad_sumsq_workspace(self.dev)
        self.opt = opt

    def optimizer_step(self, lr, grad_scale=1.0):
        """one optimizer launch over the flat buffers, after backward() - which ends with the deterministic finish and the data-parallel
        all-reduce, so the norm below is that of the reduced gradient on every rank.  Plain Adam (the default) is adam_step: the one
        fmri_adam_step launch.  `decay` is Keras': step k (1-based) runs at lr / (1 + decay * (k - 1))."""
        o = self.opt
        if o["decay"] > 0.0:
            lr = lr / (1.0 + o["decay"] * self.t)
        clips = o["clipnorm"] > 0.0 or o["clipvalue"] > 0.0
        if o["kind"] == "adam" and not o["amsgrad"] and not clips:
            return self.adam_step(lr, beta2=o["beta_2"], eps=o["epsilon"], grad_scale=grad_scale)
        gnorm = None
        if o["clipnorm"] > 0.0:
            gnorm = ops.grad_sumsq(self.G, grad_scale, self._gnorm_work, self._gnorm)
        clip = dict(grad_scale=grad_scale, gnorm=gnorm, clipnorm=o["clipnorm"], clipvalue=o["clipvalue"])
        self.t += 1
        if o["kind"] == "sgd":
            ops.sgd_step(self.P, self.G, self.M, lr, o["momentum"], o["nesterov"], **clip)
        elif o["kind"] == "rmsprop":
            ops.rmsprop_step(self.P, self.G, self.V, lr, o["rho"], o["epsilon"], **clip)
        else:
            lr_t = lr * math.sqrt(1.0 - o["beta_2"] ** self.t) / (1.0 - self.beta1 ** self.t)
            ops.adam_step_ex(self.P, self.G, self.M, self.V, self.Vhat if o["amsgrad"] else None, lr_t, self.beta1, o["beta_2"], o["epsilon"],
                             **clip)
        self.refresh_weight_copies()

    def train_step(self, x, y_true, lr, weight=None):
        """one full step: forward, Dice, backward, (all-reduce), optimizer.  Returns the device tensor of metric sums."""
        self.forward(x)
        self.loss_forward(y_true, weight)
        # data parallel: with the global-batch Dice sums the ranks' gradients are summed (scale 1); with per-rank losses
        # (global_dice=False) the all-reduce sum is turned into the mean by scaling each rank's loss gradient by 1/world
        self.backward(y_true, grad_scale=(self.dist.grad_scale if self.dist is not None else 1.0), weight=weight)
        self.optimizer_step(lr)
        return self.sums

    @staticmethod
    def metrics_from_sums(s, smooth=1.0, loss_kind=0, loss_param=1.0):
        s = [float(v) for v in s]
        dice = (2.0 * s[0] + smooth) / (s[1] + s[2] + smooth)
        vod = (s[3] + smooth) / (s[4] + s[5] - s[3] + smooth)
        return dict(loss=ops.loss_value_from_sums(s, loss_kind, loss_param, smooth), dice_coefficient=dice, vod_coefficient=vod,
                    binary_accuracy=s[6] / max(s[7], 1.0))


def glorot_uniform(rs, shape):
    """Keras glorot_uniform kernel of `shape` = receptive field + (fan-in channels, fan-out channels), drawn from RandomState rs"""
    rf = int(np.prod(shape[:-2]))
    lim = math.sqrt(6.0 / (rf * shape[-2] + rf * shape[-1]))
    return rs.uniform(-lim, lim, size=shape).astype(np.float32)


def kernel_to_flat(k, size):
    """Keras conv kernel (size,)*3 + (Cin, Cout) -> the flat [size^3][Cout][Cin] image; a 2-D kernel (size, size, Cin, Cout) becomes the
    centre kd plane of the size^3 image (the caller checks the shape)"""
    k = np.asarray(k, np.float32)
    cin, cout = k.shape[-2:]
    if k.ndim == 4:
        k3 = np.zeros((size,) * 3 + (cin, cout), np.float32)
        k3[size // 2] = k
        k = k3
    return k.reshape((size,) * 3 + (cin, cout)).transpose(0, 1, 2, 4, 3).reshape(-1)


def flat_to_kernel(flat, size, cin, cout, nd):
    """inverse of kernel_to_flat: the Keras kernel (size,)*nd + (Cin, Cout) of a flat [size^3][Cout][Cin] image (2-D: its centre kd plane)"""
    k = flat.reshape((size,) * 3 + (cout, cin)).transpose(0, 1, 2, 4, 3)
    return (k[size // 2] if nd == 2 else k).copy()
