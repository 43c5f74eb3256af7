"""`norm_net_model` with the reference signature (reference fetal_net/model/norm/NormNet.py:10-30): an Isensee network with a linear output
in front of a previously trained, FROZEN segmenter.  Only the network in front is trained, on the segmenter's loss: it learns to map
volumes of a new scanner or protocol into the intensity domain the segmenter was trained on.

Both networks are engines on the device, chained by fmri_hip.chain_engine.ChainEngine: the segmenter's backward pass runs without
parameter work and ends in dL/d(its input), which is the gradient on the norm net's output.  The frozen segmenter runs in training mode
during a training step (SpatialDropout active, BatchNormalization on batch statistics, moving averages NOT updated) - Keras 2.2 under
learning phase 1 with `trainable = False`, and what fetal_net.adversarial.CombinedModel does with its discriminator.

`old_model_path` is a checkpoint path (opened with `load_old_model`) or - this package's one extension - an already built `Model`.
Checkpoints hold the norm net's layers and the builder call; the segmenter is re-opened from `old_model_path` (a nested-model HDF5 that
Keras itself could re-open is not written).
"""
from collections import OrderedDict

import numpy as np

from ...engine_model import Adam, Model
from ...metrics import dice_coefficient, dice_coefficient_loss, vod_coefficient
from ..unet3d.isensee2017 import isensee2017_model_3d


class NormNetModel(Model):
    """Keras-Model duck type of the chain.  `layers` are the norm net's (what a checkpoint stores and `load_weights` maps onto);
    `norm_net` and `seg_net` are the two models."""

    def __init__(self, norm_net, seg_net, builder_kwargs, old_model):
        Model.__init__(self, norm_net.layers, None, "norm_net_model", builder_kwargs, "channels_first_3d", name="NormNetModel")
        self.norm_net, self.seg_net, self._old_model = norm_net, seg_net, old_model
        self.outputs = list(seg_net.outputs)
        self.output_shape = seg_net.output_shape

    def engine(self, batch, training=True):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("no GPU visible: the fetal_net hot path has no CPU implementation")
        if self._engine is None:
            from fmri_hip.chain_engine import ChainEngine
            self._engine = ChainEngine(self.norm_net.engine(batch), self.seg_net.engine(batch))
            if self._pending_weights is not None:
                self._engine.load_keras_weights(self._pending_weights)
                self._pending_weights = None
            self._sync_optimizer(self._engine)
            if getattr(self, "_pending_opt", None) is not None:
                self._apply_optimizer_state(self._pending_opt)
        self._sync_optimizer(self._engine)
        self._engine.set_batch(batch)
        self._set_label_metrics(self._engine)
        if self.loss is not None:
            try:
                self._engine.loss_kind, self._engine.loss_param = self._loss_kind()
            except NotImplementedError:
                pass
        return self._engine

    def _compute_dtype(self):
        return self.norm_net._compute_dtype()

    def save(self, path, include_optimizer=True, weights_only=False):
        if not weights_only and not isinstance(self._old_model, str):
            raise ValueError("this NormNetModel was built from a Model instance: a checkpoint records the segmenter by its path - save the "
                             "segmenter and build norm_net_model(old_model_path=<that file>), or use save_weights")
        return Model.save(self, path, include_optimizer=include_optimizer, weights_only=weights_only)


def _check_segmenter(seg, n_labels, input_shape):
    want = (int(n_labels),) + tuple(int(v) for v in input_shape[1:])
    if getattr(seg, "_input_layout", None) != "channels_first_3d" or len(seg.input_shape) != 5:
        raise ValueError("norm_net_model: the segmenter must be a 3-D channels-first model, old_model_path holds a 2-D one (input %s)"
                         % (seg.input_shape,))
    last = seg.layers[-1]
    if not (last.class_name == "Activation" and last.config.get("activation") == "sigmoid"):
        raise ValueError("norm_net_model: the segmenter must end in a sigmoid, old_model_path ends in %s %r"
                         % (last.class_name, last.config.get("activation")))
    if seg._unsupported is not None:
        raise ValueError("norm_net_model: the segmenter does not run on the engine: " + seg._unsupported)
    have = tuple(int(v) for v in seg.input_shape[1:])
    if have[0] != want[0]:
        raise ValueError("norm_net_model: channel mismatch - the segmenter reads %d channels, the norm net writes n_labels = %d" % (have[0], want[0]))
    if have[1:] != want[1:]:
        raise ValueError("norm_net_model: spatial mismatch - the segmenter reads %s, input_shape is %s" % (have[1:], want[1:]))


def norm_net_model(input_shape=(1, 128, 128, 128), n_base_filters=16, depth=5, dropout_rate=0.3, n_segmentation_levels=3, n_labels=1,
                   optimizer=Adam, initial_learning_rate=5e-4, loss_function=dice_coefficient_loss, old_model_path=None, **kargs):
    if old_model_path is None:
        raise ValueError("norm_net_model needs old_model_path: the checkpoint (or Model) of the trained segmenter it is put in front of")
    if kargs.get("mask_shape") is not None:
        raise NotImplementedError("norm_net_model has no mask_shape (the reference builder takes none)")
    input_shape = tuple(int(v) for v in input_shape)
    extra = dict(compute_dtype=kargs["compute_dtype"]) if "compute_dtype" in kargs else {}
    norm_net = isensee2017_model_3d(input_shape, n_base_filters, depth, dropout_rate, n_segmentation_levels, n_labels, optimizer,
                                    initial_learning_rate, loss_function, activation_name=None, **extra)
    if isinstance(old_model_path, Model):
        seg_net = old_model_path
    else:
        from ...training import load_old_model
        seg_net = load_old_model(str(old_model_path))
    _check_segmenter(seg_net, n_labels, input_shape)
    seg_net.trainable = False
    if seg_net._engine is not None and not (getattr(seg_net._engine, "input_grad", False) and getattr(seg_net._engine, "frozen", False)):
        # an engine built for plain use: rebuild it (same weights) so that its backward pass ends in dL/d(input) - and, under
        # FMRI_DETERMINISTIC=1, so that it gives the deterministic-gradient registration back: the norm net takes it
        seg_net._pending_weights = OrderedDict((k, np.asarray(v)) for k, v in seg_net._engine.export_keras_weights().items())
        seg_net._engine.close()
        seg_net._engine = None
    # (trainable = False above makes Model.engine build it frozen: the segmenter writes no parameter gradient anybody reads, so under
    # FMRI_DETERMINISTIC=1 it takes no registration - one per process, the trainable norm net's - while its normalisation layers still
    # sum in block order)
    seg_net._engine_kwargs = dict(seg_net._engine_kwargs, input_grad=True)
    builder_kwargs = dict(input_shape=input_shape, n_base_filters=n_base_filters, depth=depth, dropout_rate=dropout_rate,
                          n_segmentation_levels=n_segmentation_levels, n_labels=n_labels, initial_learning_rate=initial_learning_rate,
                          loss_function=loss_function, old_model_path=old_model_path if isinstance(old_model_path, Model) else str(old_model_path),
                          **extra)
    model = NormNetModel(norm_net, seg_net, builder_kwargs, builder_kwargs["old_model_path"])
    metrics = ['binary_accuracy', vod_coefficient]
    if loss_function != dice_coefficient_loss:
        metrics += [dice_coefficient]
    model.compile(optimizer=optimizer(lr=initial_learning_rate), loss=loss_function, metrics=metrics)
    return model
