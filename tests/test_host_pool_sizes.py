"""Host side of the pool-size / SpatialDropout2D options of unet_model_3d and unet_model_2d: which engine a builder call is routed to, what
is still refused and why, the build-time divisibility check, and the checkpoint round trip.  No GPU: no engine is built."""
import json

import numpy as np
import pytest

import fetal_net.model as fmodel


def _random_weights(model, seed=0):
    from fetal_net import keras_h5
    rng = np.random.RandomState(seed)
    return dict((k, rng.standard_normal(shape).astype(np.float32)) for k, shape in keras_h5.weight_shapes(model).items())


@pytest.mark.parametrize("build", [
    lambda: fmodel.unet_model_3d(input_shape=(1, 16, 16, 4), pool_size=(2, 2, 1), depth=3, n_base_filters=4),
    lambda: fmodel.unet_model_3d(input_shape=(1, 16, 16, 4), pool_size=(2, 2, 1), depth=3, n_base_filters=4, batch_normalization=True),
    lambda: fmodel.unet_model_3d(input_shape=(1, 27, 16, 16), pool_size=(3, 4, 1), depth=3, n_base_filters=4),
    lambda: fmodel.unet_model_2d(input_shape=(16, 16, 5), depth=3, n_base_filters=4, dropout_rate=0.2),
    lambda: fmodel.unet_model_2d(input_shape=(16, 16, 5), depth=3, n_base_filters=4, dropout_rate=0.2, pool_size=(2, 1)),
    lambda: fmodel.unet_model_2d(input_shape=(16, 16, 5), depth=3, n_base_filters=4, pool_size=(1, 2)),
])
def test_new_options_are_routed_to_the_layer_graph_engine(build):
    m = build()
    assert m._unsupported is None
    assert getattr(m, "_graph_engine", False) is True


def test_all_twos_without_dropout_keep_the_hand_scheduled_engine():
    for m in (fmodel.unet_model_3d(input_shape=(1, 16, 16, 16), depth=3, n_base_filters=4),
              fmodel.unet_model_3d(input_shape=(1, 16, 16, 16), depth=3, n_base_filters=4, deconvolution=True),
              fmodel.unet_model_2d(input_shape=(16, 16, 5), depth=3, n_base_filters=4),
              fmodel.unet_model_2d(input_shape=(16, 16, 5), depth=3, n_base_filters=4, deconvolution=True)):
        assert m._unsupported is None and not getattr(m, "_graph_engine", False)


def test_the_layers_carry_the_pool_size():
    m = fmodel.unet_model_3d(input_shape=(1, 16, 16, 4), pool_size=(2, 2, 1), depth=3, n_base_filters=4)
    pools = [l for l in m.layers if l.class_name == "MaxPooling3D"]
    ups = [l for l in m.layers if l.class_name == "UpSampling3D"]
    assert [l.config["pool_size"] for l in pools] == [(2, 2, 1)] * 2 and [l.config["size"] for l in ups] == [(2, 2, 1)] * 2
    assert [l.output_shape for l in pools] == [(None, 8, 8, 8, 4), (None, 16, 4, 4, 4)]
    assert m.output_shape == (None, 1, 16, 16, 4)


@pytest.mark.parametrize("build", [
    lambda: fmodel.unet_model_3d(input_shape=(1, 16, 16, 4), pool_size=(2, 2, 1), depth=3, n_base_filters=4, deconvolution=True),
    lambda: fmodel.unet_model_2d(input_shape=(16, 16, 5), depth=3, n_base_filters=4, pool_size=(2, 1), deconvolution=True),
    lambda: fmodel.unet_model_2d(input_shape=(16, 16, 5), depth=3, n_base_filters=4, dropout_rate=0.2, deconvolution=True),
])
def test_deconvolution_with_a_new_option_is_refused_with_its_reason(build):
    m = build()
    assert not getattr(m, "_graph_engine", False)
    assert "deconvolution=True" in m._unsupported and "transposed" in m._unsupported
    with pytest.raises(NotImplementedError, match="transposed"):
        m.predict(np.zeros((1,) + tuple(m.input_shape[1:])))


@pytest.mark.parametrize("build", [
    lambda: fmodel.unet_model_3d(input_shape=(1, 16, 16, 16), pool_size=(1, 1, 1), depth=3, n_base_filters=4),
    lambda: fmodel.unet_model_2d(input_shape=(16, 16, 5), pool_size=(1, 1), depth=3, n_base_filters=4),
    lambda: fmodel.unet_model_3d(input_shape=(1, 25, 16, 16), pool_size=(5, 2, 2), depth=3, n_base_filters=4),
])
def test_pool_sizes_the_kernels_do_not_take_are_refused(build):
    m = build()
    assert m._unsupported and "pool_size" in m._unsupported and not getattr(m, "_graph_engine", False)
    with pytest.raises(NotImplementedError):
        m.predict(np.zeros((1,) + tuple(m.input_shape[1:])))


def test_a_dimension_the_poolings_do_not_divide_is_a_build_time_error_that_names_the_axis():
    with pytest.raises(ValueError, match=r"axis 2 has 6 voxels.*2 \*\* \(depth - 1\) = 4"):
        fmodel.unet_model_3d(input_shape=(1, 16, 16, 6), pool_size=(2, 2, 2), depth=3, n_base_filters=4)
    with pytest.raises(ValueError, match=r"axis 0 has 12 voxels.*3 \*\* \(depth - 1\) = 9"):
        fmodel.unet_model_3d(input_shape=(1, 12, 16, 6), pool_size=(3, 2, 1), depth=3, n_base_filters=4)
    with pytest.raises(ValueError, match=r"axis 1 has 10 voxels"):
        fmodel.unet_model_2d(input_shape=(16, 10, 5), pool_size=(1, 2), depth=3, n_base_filters=4)
    fmodel.unet_model_3d(input_shape=(1, 16, 16, 6), pool_size=(2, 2, 1), depth=3, n_base_filters=4)       # an unpooled axis may be anything


@pytest.mark.parametrize("which", ["unet3d_pool221", "unet2d_dropout"])
def test_checkpoint_round_trip(tmp_path, which):
    """save -> load_old_model from the file alone: the same pool_size and dropout_rate, the same layer list, equal weights - and, where
    the file is Keras HDF5, the builder call inferred from the layer configs alone says the same"""
    from fetal_net.training import load_old_model
    from fetal_net.utils import hdf5
    if which == "unet3d_pool221":
        model = fmodel.unet_model_3d(input_shape=(1, 16, 16, 4), pool_size=(2, 2, 1), depth=3, n_base_filters=4)
    else:
        model = fmodel.unet_model_2d(input_shape=(16, 16, 5), depth=3, n_base_filters=4, dropout_rate=0.2, pool_size=(2, 1))
    W = _random_weights(model)
    model.set_weights_dict(W)
    path = str(tmp_path / "model.h5")
    model.save(path)
    again = load_old_model(path, verbose=False)
    assert again._builder == model._builder and again._unsupported is None and again._graph_engine
    assert tuple(again._builder_kwargs["pool_size"]) == tuple(model._builder_kwargs["pool_size"])
    if which == "unet2d_dropout":
        assert abs(again._builder_kwargs["dropout_rate"] - 0.2) < 1e-12
    assert [(l.name, l.class_name, l.output_shape) for l in again.layers] == [(l.name, l.class_name, l.output_shape) for l in model.layers]
    for a, b in zip(again.layers, model.layers):
        for key in ("pool_size", "size", "rate"):
            assert a.config.get(key) == b.config.get(key), (a.name, key)
    W2 = again.get_weights_dict()
    assert set(W2) == set(W) and all(np.array_equal(W2[k], W[k]) for k in W)
    if hdf5.is_hdf5(path):
        from fetal_net import keras_h5
        with hdf5.File(path) as f:
            mc = json.loads(bytes(f.attrs["model_config"]).decode())
            tc = json.loads(bytes(f.attrs["training_config"]).decode())
        name, kw = keras_h5.infer_builder(mc, tc)
        assert name == model._builder and tuple(kw["pool_size"]) == tuple(model._builder_kwargs["pool_size"])
        if which == "unet2d_dropout":
            assert abs(kw["dropout_rate"] - 0.2) < 1e-12
        rebuilt = getattr(fmodel, name)(**{k: v for k, v in kw.items() if k != "loss_function"})
        assert rebuilt._graph_engine and [l.name for l in rebuilt.layers] == [l.name for l in model.layers]
