"""The optimizers a model of this package compiles with: Keras 2.2.4's `Adam`, `SGD` and `RMSprop` with their constructor arguments and
defaults, `clipnorm` / `clipvalue` included, plus `get` and `deserialize` (keras/optimizers.py as published - no Keras was at hand to run
against, so what is restated here and in the kernels is parity-unpinned).

The objects are tokens: hyper-parameters and the `lr` attribute the callbacks read and write.  The update itself is one HIP launch over the
engine's flat buffers (fmri_hip.engine_base.EngineBase.optimizer_step), which `engine_spec()` configures.  The reference's builders take
the class and call it as `optimizer(lr=initial_learning_rate)`; models without that keyword take an instance through `model.compile`.
"""
import numpy as np


def _f32(v):
    """a hyper-parameter Keras keeps in a float32 variable, as its get_config reports it"""
    return float(np.float32(v))


class Optimizer(object):
    """`clipnorm`: the gradients are scaled by clipnorm / norm when their global L2 norm is at least clipnorm; `clipvalue`: every gradient
    element is clamped to [-clipvalue, clipvalue] (after the norm clip, Keras' order).  A value that is not > 0 means off."""

    kind = None

    def __init__(self, clipnorm=None, clipvalue=None, **kwargs):
        if kwargs:
            raise TypeError("Unexpected keyword argument passed to optimizer: " + sorted(kwargs)[0])
        self.clipnorm = float(clipnorm) if clipnorm is not None and float(clipnorm) > 0.0 else None
        self.clipvalue = float(clipvalue) if clipvalue is not None and float(clipvalue) > 0.0 else None

    def _clip_config(self):
        out = {}
        if self.clipnorm is not None:
            out["clipnorm"] = self.clipnorm
        if self.clipvalue is not None:
            out["clipvalue"] = self.clipvalue
        return out

    @classmethod
    def from_config(cls, config):
        return cls(**config)

    def _clip_spec(self):
        return dict(clipnorm=self.clipnorm or 0.0, clipvalue=self.clipvalue or 0.0)


class SGD(Optimizer):
    """v = momentum * m - lr * g; m <- v; p <- p + momentum * v - lr * g with Nesterov, else p <- p + v"""

    kind = "sgd"

    def __init__(self, lr=0.01, momentum=0., decay=0., nesterov=False, **kwargs):
        Optimizer.__init__(self, **kwargs)
        self.lr, self.momentum, self.decay, self.nesterov = float(lr), float(momentum), float(decay), bool(nesterov)

    def keras_config(self):
        """the `config` of Keras' optimizer_config (variables as their float32 values), clip arguments only when set"""
        return dict(lr=_f32(self.lr), momentum=_f32(self.momentum), decay=_f32(self.decay), nesterov=self.nesterov, **self._clip_config())

    def get_config(self):
        return dict(lr=self.lr, momentum=self.momentum, decay=self.decay, nesterov=self.nesterov, **self._clip_config())

    def engine_spec(self):
        return dict(kind="sgd", momentum=self.momentum, nesterov=self.nesterov, decay=self.decay, **self._clip_spec())


class RMSprop(Optimizer):
    """a <- rho * a + (1 - rho) * g^2; p <- p - lr * g / (sqrt(a) + epsilon)"""

    kind = "rmsprop"

    def __init__(self, lr=0.001, rho=0.9, epsilon=None, decay=0., **kwargs):
        Optimizer.__init__(self, **kwargs)
        self.lr, self.rho, self.decay = float(lr), float(rho), float(decay)
        self.epsilon = 1e-7 if epsilon is None else float(epsilon)          # None: K.epsilon()

    def keras_config(self):
        return dict(lr=_f32(self.lr), rho=_f32(self.rho), decay=_f32(self.decay), epsilon=self.epsilon, **self._clip_config())

    def get_config(self):
        return dict(lr=self.lr, rho=self.rho, decay=self.decay, epsilon=self.epsilon, **self._clip_config())

    def engine_spec(self):
        return dict(kind="rmsprop", rho=self.rho, epsilon=self.epsilon, decay=self.decay, **self._clip_spec())


class Adam(Optimizer):
    """Keras Adam (epsilon outside the square root); amsgrad: vhat <- max(vhat, v) stands in the denominator"""

    kind = "adam"

    def __init__(self, lr=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-7, decay=0., amsgrad=False, **kwargs):
        Optimizer.__init__(self, **kwargs)
        self.lr, self.beta_1, self.beta_2 = float(lr), beta_1, beta_2
        self.epsilon = 1e-7 if epsilon is None else epsilon
        self.decay, self.amsgrad = float(decay), bool(amsgrad)

    def keras_config(self):
        return dict(lr=_f32(self.lr), beta_1=_f32(self.beta_1), beta_2=_f32(self.beta_2), decay=_f32(self.decay),
                    epsilon=float(self.epsilon), amsgrad=self.amsgrad, **self._clip_config())

    def get_config(self):
        """lr, beta_1, beta_2, epsilon - and the later arguments only where they were given something"""
        out = dict(lr=self.lr, beta_1=self.beta_1, beta_2=self.beta_2, epsilon=self.epsilon)
        if self.decay:
            out["decay"] = self.decay
        if self.amsgrad:
            out["amsgrad"] = True
        out.update(self._clip_config())
        return out

    def engine_spec(self):
        return dict(kind="adam", beta_1=float(self.beta_1), beta_2=float(self.beta_2), epsilon=float(self.epsilon), decay=self.decay,
                    amsgrad=self.amsgrad, **self._clip_spec())


_CLASSES = {"adam": Adam, "sgd": SGD, "rmsprop": RMSprop}


def deserialize(config):
    """{"class_name": ..., "config": {...}} (a checkpoint's optimizer_config) -> optimizer; ValueError for a class this package has not"""
    name = config["class_name"]
    cls = _CLASSES.get(str(name).lower())
    if cls is None:
        raise ValueError("Unknown optimizer: %s (available: Adam, SGD, RMSprop)" % name)
    return cls.from_config(dict(config.get("config") or {}))


def serialize(optimizer):
    return {"class_name": type(optimizer).__name__, "config": optimizer.keras_config()}


def get(identifier):
    """an optimizer from an instance (returned as it is), a class name ('sgd', 'RMSprop', ...: default arguments) or a config dictionary"""
    if isinstance(identifier, Optimizer):
        return identifier
    if isinstance(identifier, dict):
        return deserialize(identifier)
    if isinstance(identifier, str):
        return deserialize({"class_name": identifier, "config": {}})
    raise ValueError("Could not interpret optimizer identifier: %r" % (identifier,))
