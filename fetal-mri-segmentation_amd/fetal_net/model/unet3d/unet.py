"""`unet_model_3d` with the reference signature and topology (reference fetal_net/model/unet3d/unet.py:17-138), returning
a Keras-Model duck type whose compute runs on the MI355X engine.

Topology: `depth` encoder levels of two [Conv3D 3x3x3 'same' -> (BatchNorm | InstanceNorm)? -> ReLU] blocks with
n_base_filters*2^level and twice that many filters, MaxPooling3D between levels; decoder levels of
(UpSampling3D | Conv3DTranspose k2 s2) -> concatenate([up, skip], axis=1) -> two conv blocks with the skip's filter count;
Conv3D(n_labels, 1x1x1) -> Activation(activation_name).  pool_size (2, 2, 2) runs on the hand-scheduled engine; any other pool size with
per-axis factors 1..4 - (2, 2, 1) for anisotropic volumes - on the layer-graph engine (UpSampling3D only).  Compiled with Adam(lr) and metrics
['binary_accuracy', vod_coefficient] (+ dice_coefficient when the loss is not the Dice loss).
"""
from ...engine_model import Adam, Model
from ...metrics import dice_coefficient, dice_coefficient_loss, label_wise_metrics, vod_coefficient
from ..graph import Graph


def conv_block(g, x, n_filters, batch_normalization=False, kernel=(3, 3, 3), activation=None, padding='same', strides=(1, 1, 1),
               instance_normalization=False):
    """one [conv -> norm? -> activation] block (reference create_convolution_block, unet.py:89-115)"""
    h = g.conv(x, n_filters, kernel, strides=strides, padding=padding)
    if batch_normalization:
        h = g.batch_norm(h, axis=1)
    elif instance_normalization:
        h = g.instance_norm(h, axis=1)
    if activation is None:
        return g.activation(h, 'relu')
    if activation == 'leaky_relu':
        return g.leaky_relu(h)
    return g.activation(h, activation)


def up_block(g, x, pool_size, deconvolution, kernel_size=(2, 2, 2), strides=(2, 2, 2)):
    """reference get_up_convolution (unet.py:132-138): transposed conv keeps the channel count, else nearest x2"""
    if deconvolution:
        return g.deconv(x, x.shape[1], kernel_size, strides)
    return g.up_sample(x, pool_size)


def pool_route(pool_size, nd, deconvolution, dropout=False):
    """How a U-Net with these options runs.  -> (graph_engine, refused): graph_engine = True sends the model to the layer-graph engine -
    a pool size other than all 2s (per-axis factors 1..4, its pooling / up-sampling kernels take the factors at run time) or, 2-D,
    SpatialDropout2D (`dropout`); refused = why the model cannot run at all, or None.  All 2s without dropout keeps the hand-scheduled
    engine."""
    twos = tuple(pool_size) == (2,) * nd
    if twos and not dropout:
        return False, None
    if len(pool_size) != nd or not all(float(p).is_integer() and 1 <= p <= 4 for p in pool_size):
        return False, "pool_size %s: the pooling kernels take per-axis factors 1..4" % (pool_size,)
    if all(p == 1 for p in pool_size):
        return False, "pool_size %s pools nothing" % (pool_size,)
    if deconvolution:
        what = ([] if twos else ["pool_size %s" % (pool_size,)]) + (["dropout_rate > 0 (SpatialDropout2D)"] if dropout else [])
        return False, ("%s with deconvolution=True: the reference's transposed convolution up-samples by 2 whatever the pool size, and the "
                       "layer-graph engine that runs these options has no transposed-convolution op" % " and ".join(what))
    return True, None


def check_pool_divides(input_spatial, pool_size, depth):
    """ValueError at build time when `depth - 1` poolings do not divide a spatial axis: Keras fails at the concatenate whose up-sampled
    half has lost voxels; the message names the axis"""
    for axis, (s, p) in enumerate(zip(input_spatial, pool_size)):
        if s % (p ** (depth - 1)):
            raise ValueError("input_shape: spatial axis %d has %d voxels, not divisible by pool_size %d ** (depth - 1) = %d: the "
                             "concatenate of the shallowest decoder level would not match" % (axis, s, p, p ** (depth - 1)))


def unet_model_3d(input_shape, pool_size=(2, 2, 2), n_labels=1, initial_learning_rate=0.00001, deconvolution=False, depth=4,
                  n_base_filters=32, include_label_wise_dice_coefficients=False, batch_normalization=False,
                  activation_name="sigmoid", loss_function=dice_coefficient_loss, **kargs):
    input_shape = tuple(int(v) for v in input_shape)
    pool_size = tuple(pool_size)
    graph_engine, refused = pool_route(pool_size, 3, deconvolution)
    if not deconvolution and refused is None:
        check_pool_divides(input_shape[1:], pool_size, depth)
    g = Graph()
    x = g.input(input_shape)
    skips = []
    h = x
    for level in range(depth):
        h = conv_block(g, h, n_base_filters * (2 ** level), batch_normalization=batch_normalization)
        h = conv_block(g, h, n_base_filters * (2 ** level) * 2, batch_normalization=batch_normalization)
        skips.append(h)
        if level < depth - 1:
            h = g.max_pool(h, pool_size)
    for level in range(depth - 2, -1, -1):
        up = up_block(g, h, pool_size, deconvolution)
        cat = g.concat([up, skips[level]], axis=1)
        h = conv_block(g, cat, skips[level].shape[1], batch_normalization=batch_normalization)
        h = conv_block(g, h, skips[level].shape[1], batch_normalization=batch_normalization)
    h = g.conv(h, n_labels, (1, 1, 1))
    g.activation(h, activation_name)

    unsupported = []
    if refused:
        unsupported.append(refused)
    if activation_name != "sigmoid":
        unsupported.append("activation_name %r (only 'sigmoid', or None on isensee2017_model_3d)" % (activation_name,))
    builder_kwargs = dict(input_shape=input_shape, pool_size=pool_size, n_labels=n_labels, initial_learning_rate=initial_learning_rate,
                          deconvolution=deconvolution, depth=depth, n_base_filters=n_base_filters,
                          batch_normalization=batch_normalization, activation_name=activation_name, loss_function=loss_function)
    if "compute_dtype" in kargs:
        builder_kwargs["compute_dtype"] = kargs["compute_dtype"]
    label_metrics = label_wise_metrics(n_labels, include_label_wise_dice_coefficients)
    if label_metrics:
        builder_kwargs["include_label_wise_dice_coefficients"] = True
    plan_args = dict(in_channels=input_shape[0], spatial=input_shape[1:], depth=depth, n_base_filters=n_base_filters,
                     n_labels=n_labels, ndim=3, norm="batch" if batch_normalization else None, deconvolution=bool(deconvolution))
    model = Model(g.layers, plan_args, "unet_model_3d", builder_kwargs, "channels_first_3d")
    if graph_engine:
        model._graph_engine = True
    if unsupported:
        model._unsupported = ", ".join(unsupported)
    metrics = ['binary_accuracy', vod_coefficient]
    if loss_function != dice_coefficient_loss:
        metrics += [dice_coefficient]
    metrics += label_metrics
    model.compile(optimizer=Adam(lr=initial_learning_rate), loss=loss_function, metrics=metrics)
    return model


# reference-named helpers (other builders import them from here: reference isensee2017.py:7)
def create_convolution_block(input_layer, n_filters, batch_normalization=False, kernel=(3, 3, 3), activation=None, padding='same',
                             strides=(1, 1, 1), instance_normalization=False, graph=None):
    if graph is None:
        raise TypeError("create_convolution_block needs the recording graph (graph=...) in this implementation")
    return conv_block(graph, input_layer, n_filters, batch_normalization, kernel, activation, padding, strides, instance_normalization)


def compute_level_output_shape(n_filters, depth, pool_size, image_shape):
    return tuple([None, n_filters] + [int(s // (p ** depth)) for s, p in zip(image_shape, pool_size)])
