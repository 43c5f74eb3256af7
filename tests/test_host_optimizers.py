"""fetal_net.optimizers on the host: Keras 2.2.4's constructor defaults and configs (literal dictionaries from the published
keras/optimizers.py; parity-unpinned - no Keras could be run), the checkpoint layouts per class, and what load_old_model rebuilds."""
import json
import os
import warnings

import numpy as np
import pytest

from fetal_net.utils import hdf5

needs_h5 = pytest.mark.skipif(not hdf5.available(), reason="no libhdf5 on this machine")


def _f32(v):
    return float(np.float32(v))


def _model(**kw):
    import fetal_net.model as models
    return models.unet_model_3d(input_shape=(1, 8, 16, 16), depth=2, n_base_filters=4, **kw)


def _random_weights(model, seed=0):
    from fetal_net import keras_h5
    rng = np.random.RandomState(seed)
    return dict((k, rng.standard_normal(s).astype(np.float32)) for k, s in keras_h5.weight_shapes(model).items())


# ------------------------------------------------------------------------------------------------------------------ classes
def test_defaults_and_configs_are_keras_224s():
    from fetal_net.optimizers import SGD, Adam, RMSprop
    assert SGD().get_config() == {"lr": 0.01, "momentum": 0.0, "decay": 0.0, "nesterov": False}
    assert RMSprop().get_config() == {"lr": 0.001, "rho": 0.9, "decay": 0.0, "epsilon": 1e-7}          # epsilon=None: K.epsilon()
    assert RMSprop(epsilon=None).epsilon == 1e-7
    assert Adam().keras_config() == {"lr": _f32(0.001), "beta_1": _f32(0.9), "beta_2": _f32(0.999), "decay": 0.0, "epsilon": 1e-7,
                                     "amsgrad": False}
    # what Keras writes: the float32 values of its variables, python floats for epsilon, clip arguments only when set
    assert SGD().keras_config() == {"lr": _f32(0.01), "momentum": 0.0, "decay": 0.0, "nesterov": False}
    assert RMSprop().keras_config() == {"lr": _f32(0.001), "rho": _f32(0.9), "decay": 0.0, "epsilon": 1e-7}
    assert SGD(clipnorm=1.0).keras_config()["clipnorm"] == 1.0 and "clipvalue" not in SGD(clipnorm=1.0).keras_config()
    assert RMSprop(clipvalue=0.5).get_config()["clipvalue"] == 0.5
    got = Adam(lr=0.1, amsgrad=True, decay=0.5, clipnorm=2.0, clipvalue=3.0).get_config()
    assert got == {"lr": 0.1, "beta_1": 0.9, "beta_2": 0.999, "epsilon": 1e-7, "decay": 0.5, "amsgrad": True, "clipnorm": 2.0, "clipvalue": 3.0}
    with pytest.raises(TypeError):
        SGD(beta_1=0.5)


def test_adam_is_engine_models_adam_and_keeps_its_four_key_config():
    import fetal_net.engine_model as EM
    import fetal_net.model as models
    from fetal_net import optimizers
    assert optimizers.Adam is EM.Adam is models.Adam and models.SGD is optimizers.SGD and models.RMSprop is optimizers.RMSprop
    assert EM.Adam(0.002, 0.5, 0.99, 1e-6).get_config() == dict(lr=0.002, beta_1=0.5, beta_2=0.99, epsilon=1e-6)
    assert list(EM.Adam().get_config()) == ["lr", "beta_1", "beta_2", "epsilon"]


def test_clip_arguments_not_above_zero_mean_off():
    from fetal_net.optimizers import SGD, Adam, RMSprop
    for cls in (SGD, RMSprop, Adam):
        for off in (0, 0.0, -1.0, None):
            o = cls(clipnorm=off, clipvalue=off)
            assert o.clipnorm is None and o.clipvalue is None
            assert "clipnorm" not in o.keras_config() and "clipvalue" not in o.get_config()
            assert o.engine_spec()["clipnorm"] == 0.0 and o.engine_spec()["clipvalue"] == 0.0
        assert cls(clipnorm=1.5).engine_spec()["clipnorm"] == 1.5


def test_get_and_deserialize_round_trip():
    from fetal_net import optimizers as O
    for o in (O.SGD(lr=0.02, momentum=0.5, decay=1e-4, nesterov=True, clipvalue=0.5), O.RMSprop(lr=0.003, rho=0.8, epsilon=1e-5),
              O.Adam(lr=0.004, beta_1=0.5, amsgrad=True, clipnorm=1.0), O.Adam()):
        doc = O.serialize(o)
        assert doc["class_name"] == type(o).__name__
        back = O.deserialize(json.loads(json.dumps(doc)))
        assert type(back) is type(o) and back.keras_config() == o.keras_config() and back.engine_spec()["kind"] == o.kind
        assert O.get(doc).keras_config() == o.keras_config()
        assert O.get(o) is o
    assert type(O.get("sgd")) is O.SGD and type(O.get("RMSprop")) is O.RMSprop and type(O.get("adam")) is O.Adam
    with pytest.raises(ValueError, match="Nadam"):
        O.deserialize({"class_name": "Nadam", "config": {"lr": 0.002}})
    with pytest.raises(ValueError):
        O.get(3)


def test_builders_take_the_class_and_compile_takes_the_object():
    import fetal_net.model as models
    from fetal_net.optimizers import SGD, RMSprop
    m = models.isensee2017_model_3d(input_shape=(1, 16, 16, 16), depth=3, n_base_filters=4, optimizer=SGD, initial_learning_rate=0.05)
    assert type(m.optimizer) is SGD and m.optimizer.lr == 0.05 and m.optimizer.momentum == 0.0
    m2 = models.isensee2017_model(input_shape=(32, 32, 1), depth=3, n_base_filters=4, optimizer=RMSprop, initial_learning_rate=0.003)
    assert type(m2.optimizer) is RMSprop and m2.optimizer.lr == 0.003
    u = _model()
    u.compile(optimizer=SGD(lr=0.1, momentum=0.9), loss=u.loss, metrics=u.metrics)
    assert u.optimizer.engine_spec() == dict(kind="sgd", momentum=0.9, nesterov=False, decay=0.0, clipnorm=0.0, clipvalue=0.0)


def test_callbacks_work_through_lr():
    from fetal_net.engine_model import LearningRateScheduler, ReduceLROnPlateau
    from fetal_net.optimizers import RMSprop
    u = _model()
    u.compile(optimizer=RMSprop(lr=0.01), loss=u.loss, metrics=u.metrics)
    cb = LearningRateScheduler(lambda epoch, lr: lr * 0.5)
    cb.set_model(u)
    cb.on_epoch_begin(0)
    assert u.optimizer.lr == 0.005
    rp = ReduceLROnPlateau(factor=0.1, patience=1)
    rp.set_model(u)
    rp.on_train_begin()
    logs = {"val_loss": 1.0}
    rp.on_epoch_end(0, logs)
    rp.on_epoch_end(1, {"val_loss": 1.0})
    assert logs["lr"] == 0.005 and u.optimizer.lr == pytest.approx(0.0005)


# ------------------------------------------------------------------------------------------------------------------ training_config
def test_training_config_per_class_and_unchanged_for_the_default_model():
    from fetal_net import keras_h5
    from fetal_net.optimizers import SGD, Adam, RMSprop
    u = _model(initial_learning_rate=3e-4)
    # the exact document this package wrote before it had any optimizer but Adam
    assert json.dumps(keras_h5.training_config(u)["optimizer_config"]) == json.dumps(
        {"class_name": "Adam", "config": {"lr": _f32(3e-4), "beta_1": _f32(0.9), "beta_2": _f32(0.999), "decay": 0.0, "epsilon": 1e-7,
                                          "amsgrad": False}})
    for o in (SGD(lr=0.1, nesterov=True, clipnorm=1.0), RMSprop(rho=0.8), Adam(amsgrad=True, clipvalue=0.5)):
        u.compile(optimizer=o, loss=u.loss, metrics=u.metrics)
        assert keras_h5.training_config(u)["optimizer_config"] == {"class_name": type(o).__name__, "config": o.keras_config()}

    class Foreign(object):                      # an object of any other type: its lr, with Adam's defaults
        lr = 0.25

        def get_config(self):
            return {"lr": self.lr}
    u.compile(optimizer=Foreign(), loss=u.loss, metrics=u.metrics)
    assert keras_h5.training_config(u)["optimizer_config"]["class_name"] == "Adam"
    assert keras_h5.training_config(u)["optimizer_config"]["config"]["lr"] == 0.25


# ------------------------------------------------------------------------------------------------------------------ Keras-layout files
def _write_keras_style_file(path, model, W, optimizer_config, names, arrays):
    """a file laid out the way Keras 2.2.4 `model.save()` lays it out, written with the raw binding (not with keras_h5.save_model):
    `names` / `arrays` are optimizer.weights by position"""
    from fetal_net import keras_h5
    tc = keras_h5.training_config(model)
    tc["optimizer_config"] = optimizer_config
    with hdf5.File(path, "w") as f:
        f.attrs["keras_version"] = b"2.2.4"
        f.attrs["backend"] = b"tensorflow"
        f.attrs["model_config"] = json.dumps(keras_h5.model_config(model)).encode()
        f.attrs["training_config"] = json.dumps(tc).encode()
        g = f.create_group("model_weights")
        keras_h5.write_weights_group(g, model, W)
        g.close()
        og = f.create_group("optimizer_weights")
        og.attrs["weight_names"] = np.asarray([nm.encode() for nm in names], dtype="S")
        for nm, a in zip(names, arrays):
            og.create_dataset(nm, data=a).close()
        og.close()


def _slots(model, seed, count):
    from fetal_net import keras_h5
    keys, shapes = keras_h5.trainable_keys(model), keras_h5.weight_shapes(model)
    rng = np.random.RandomState(seed)
    return keys, [dict((k, rng.random_sample(shapes[k]).astype(np.float32)) for k in keys) for _ in range(count)]


def _var(cls, i):
    return "training/%s/Variable%s:0" % (cls, "" if i == 0 else "_%d" % i)


@needs_h5
def test_keras_layout_files_open_with_the_right_slots(tmp_path):
    from fetal_net import keras_h5
    from fetal_net.optimizers import SGD, Adam, RMSprop, serialize
    model = _model()
    W = _random_weights(model)
    model.set_weights_dict(W)
    keys, (a, b, c) = _slots(model, 4, 3)
    n = len(keys)
    # SGD: [iterations] + moments
    path = str(tmp_path / "sgd.h5")
    _write_keras_style_file(path, model, W, serialize(SGD(momentum=0.9)), ["SGD/iterations:0"] + [_var("SGD", i) for i in range(n)],
                            [np.int64(31)] + [a[k] for k in keys])
    st = keras_h5.read_optimizer(path, model)
    assert st["class_name"] == "SGD" and st["iterations"] == 31 and list(st["slots"]) == ["moments"]
    assert all(np.array_equal(st["slots"]["moments"][k], a[k]) for k in keys)
    # RMSprop: the accumulators alone - Keras 2.2.4 leaves iterations out of RMSprop.weights
    path = str(tmp_path / "rms.h5")
    _write_keras_style_file(path, model, W, serialize(RMSprop()), [_var("RMSprop", i) for i in range(n)], [a[k] for k in keys])
    st = keras_h5.read_optimizer(path, model)
    assert st["class_name"] == "RMSprop" and st["iterations"] == 0 and list(st["slots"]) == ["accumulators"]
    assert all(np.array_equal(st["slots"]["accumulators"][k], a[k]) for k in keys)
    # Adam with amsgrad: parameter-shaped vhats
    path = str(tmp_path / "ams.h5")
    _write_keras_style_file(path, model, W, serialize(Adam(amsgrad=True)), ["Adam/iterations:0"] + [_var("Adam", i) for i in range(3 * n)],
                            [np.int64(9)] + [s[k] for s in (a, b, c) for k in keys])
    st = keras_h5.read_optimizer(path, model)
    assert st["class_name"] == "Adam" and st["iterations"] == 9 and list(st["slots"]) == ["m", "v", "vhat"]
    assert all(np.array_equal(st["slots"]["vhat"][k], c[k]) and np.array_equal(st["slots"]["m"][k], a[k]) for k in keys)
    # a wrong slot count: ValueError, which load_weights turns into the warning it always gave
    path = str(tmp_path / "bad.h5")
    _write_keras_style_file(path, model, W, serialize(SGD()), ["SGD/iterations:0"] + [_var("SGD", i) for i in range(n - 1)],
                            [np.int64(1)] + [a[k] for k in keys[:-1]])
    with pytest.raises(ValueError, match="optimizer_weights holds"):
        keras_h5.read_optimizer(path, model)
    model.compile(optimizer=SGD(), loss=model.loss, metrics=model.metrics)
    with pytest.warns(UserWarning, match="optimizer state"):
        model.load_weights(path)


@needs_h5
def test_package_written_files_use_keras_positions(tmp_path):
    from fetal_net import keras_h5
    from fetal_net.optimizers import SGD, Adam, RMSprop
    for opt, slot_names, lead in ((SGD(momentum=0.9), ["moments"], 1), (RMSprop(), ["accumulators"], 0), (Adam(amsgrad=True), ["m", "v", "vhat"], 1)):
        model = _model()
        model.set_weights_dict(_random_weights(model))
        model.compile(optimizer=opt, loss=model.loss, metrics=model.metrics)
        keys, arrs = _slots(model, 8, len(slot_names))
        model._pending_opt = dict(class_name=type(opt).__name__, iterations=12, slots=dict(zip(slot_names, arrs)))
        path = str(tmp_path / (type(opt).__name__ + ".h5"))
        model.save(path)
        cls, n = type(opt).__name__, len(keys)
        with hdf5.File(path) as f:
            names = [bytes(x).decode() for x in f["optimizer_weights"].attrs["weight_names"]]
            assert names == (["%s/iterations:0" % cls] if lead else []) + [_var(cls, i) for i in range(len(slot_names) * n)]
            for si, arr in enumerate(arrs):
                for i, k in enumerate(keys):
                    assert np.array_equal(f["optimizer_weights"][names[lead + si * n + i]][()], arr[k])
        st = keras_h5.read_optimizer(path, model)
        assert st["iterations"] == (12 if lead else 0) and list(st["slots"]) == slot_names


@pytest.mark.parametrize("container", ["h5", "npz"] if hdf5.available() else ["npz"])
def test_load_old_model_rebuilds_rmsprop_with_its_state_pending(container, tmp_path, monkeypatch):
    from fetal_net.optimizers import RMSprop
    from fetal_net.training import load_old_model
    monkeypatch.setenv("FMRI_CHECKPOINT_FORMAT", container)
    model = _model()
    W = _random_weights(model)
    model.set_weights_dict(W)
    model.compile(optimizer=RMSprop(lr=0.0025, rho=0.85, epsilon=1e-5, decay=1e-3), loss=model.loss, metrics=model.metrics)
    keys, (acc,) = _slots(model, 2, 1)
    model._pending_opt = dict(class_name="RMSprop", iterations=40, slots=dict(accumulators=acc))
    path = str(tmp_path / "rms.h5")
    model.save(path)
    assert hdf5.is_hdf5(path) == (container == "h5")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = load_old_model(path, verbose=False)
    o = got.optimizer
    assert type(o) is RMSprop and (o.lr, o.rho, o.epsilon, o.decay) == (0.0025, 0.85, 1e-5, 1e-3)
    st = got.get_optimizer_slots()
    assert st["class_name"] == "RMSprop" and st["iterations"] == 0 and list(st["slots"]) == ["accumulators"]
    assert all(np.array_equal(st["slots"]["accumulators"][k], acc[k]) for k in keys)
    with pytest.raises(TypeError, match="get_optimizer_slots"):
        got.get_optimizer_state()
    assert all(np.array_equal(got.get_weights_dict()[k], W[k]) for k in W)


@needs_h5
def test_a_keras_optimizer_this_package_has_not_warns_and_gives_adam(tmp_path):
    from fetal_net.optimizers import Adam
    from fetal_net.training import load_old_model
    model = _model()
    W = _random_weights(model)
    model.set_weights_dict(W)
    keys, (a, b) = _slots(model, 6, 2)
    n = len(keys)
    path = str(tmp_path / "nadam.h5")
    cfg = {"class_name": "Nadam", "config": {"lr": _f32(0.002), "beta_1": _f32(0.9), "beta_2": _f32(0.999), "epsilon": 1e-7,
                                             "schedule_decay": 0.004}}
    _write_keras_style_file(path, model, W, cfg, ["Nadam/iterations:0"] + [_var("Nadam", i) for i in range(2 * n)],
                            [np.int64(3)] + [s[k] for s in (a, b) for k in keys])
    with pytest.warns(UserWarning) as rec:
        got = load_old_model(path, verbose=False)
    assert any("Nadam" in str(w.message) and "fresh Adam" in str(w.message) for w in rec)
    assert type(got.optimizer) is Adam and got.optimizer.lr == _f32(0.002) and got.get_optimizer_slots() is None
    assert all(np.array_equal(got.get_weights_dict()[k], W[k]) for k in W)


# ------------------------------------------------------------------------------------------------------------------ adversarial
def test_adversarial_models_refuse_anything_but_plain_adam():
    import fetal_net.model as models
    from fetal_net.adversarial import CombinedModel
    from fetal_net.optimizers import SGD, Adam, RMSprop
    dis = models.discriminator_image_3d(input_shape=(2, 16, 16, 16), n_base_filters=4, depth=2)
    with pytest.raises(NotImplementedError, match="SGD"):
        dis.compile(optimizer=SGD(), loss=dis.loss, metrics=dis.metrics)
    with pytest.raises(NotImplementedError, match="amsgrad"):
        dis.compile(optimizer=Adam(amsgrad=True), loss=dis.loss, metrics=dis.metrics)
    gen = models.unet_model_3d(input_shape=(1, 16, 16, 16), depth=2, n_base_filters=4)
    CombinedModel(gen, dis)                                   # Adam on both sides: as ever
    gen.compile(optimizer=RMSprop(), loss=gen.loss, metrics=gen.metrics)
    with pytest.raises(NotImplementedError, match="RMSprop"):
        CombinedModel(gen, dis)
