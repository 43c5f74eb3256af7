"""norm_net_model without a GPU: the recorded graph of the linear Isensee network, what the builders refuse, the segmenter checks of
`norm_net_model`, and the two C entry points of the first-layer input gradient in the header, the binding table and the library."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

import fetal_net.model as fmodel

SP = (16, 16, 16)
KW = dict(n_base_filters=4, depth=3, dropout_rate=0, n_segmentation_levels=2)


def test_linear_isensee_graph_is_supported_and_ends_in_linear():
    for name in (None, "linear"):
        m = fmodel.isensee2017_model_3d((1,) + SP, activation_name=name, **KW)
        last = m.layers[-1]
        assert last.class_name == "Activation" and last.config["activation"] == "linear"
        assert m._unsupported is None
    assert fmodel.isensee2017_model_3d((1,) + SP, **KW).layers[-1].config["activation"] == "sigmoid"


def test_softmax_stays_refused_everywhere_and_linear_on_the_other_three():
    builders = [lambda a: fmodel.unet_model_3d((1,) + SP, depth=2, n_base_filters=8, activation_name=a),
                lambda a: fmodel.unet_model_2d((32, 32, 5), depth=2, n_base_filters=8, activation_name=a),
                lambda a: fmodel.isensee2017_model((32, 32, 5), activation_name=a),
                lambda a: fmodel.isensee2017_model_3d((1,) + SP, activation_name=a, **KW)]
    for b in builders:
        assert "softmax" in b("softmax")._unsupported
    for b in builders[:3]:
        for a in (None, "linear"):
            assert "only 'sigmoid', or None on isensee2017_model_3d" in b(a)._unsupported
        assert b("sigmoid")._unsupported is None


def test_norm_net_model_needs_a_matching_3d_sigmoid_segmenter():
    with pytest.raises(ValueError, match="old_model_path"):
        fmodel.norm_net_model((1,) + SP, **KW)
    cases = [(fmodel.unet_model_2d((16, 16, 5), depth=2, n_base_filters=8), "2-D"),
             (fmodel.unet_model_3d((2,) + SP, depth=2, n_base_filters=8), "channel mismatch"),
             (fmodel.unet_model_3d((1, 16, 16, 32), depth=2, n_base_filters=8), "spatial mismatch"),
             (fmodel.unet_model_3d((1,) + SP, depth=2, n_base_filters=8, activation_name="softmax"), "sigmoid"),
             (fmodel.unet_model_3d((1,) + SP, depth=2, n_base_filters=8, pool_size=(5, 5, 5)), "does not run on the engine")]
    for seg, what in cases:
        with pytest.raises(ValueError, match=what):
            fmodel.norm_net_model((1,) + SP, old_model_path=seg, **KW)


def test_norm_net_model_surface():
    seg = fmodel.unet_model_3d((1,) + SP, depth=2, n_base_filters=8)
    m = fmodel.norm_net_model((1,) + SP, old_model_path=seg, **KW)
    assert type(m).__name__ == "NormNetModel" and m.name == "NormNetModel"
    assert m.seg_net is seg and m.norm_net.layers[-1].config["activation"] == "linear"
    assert m.input_shape == (None, 1) + SP and m.output_shape == (None, 1) + SP
    assert m.metrics_names == ["loss", "binary_accuracy", "vod_coefficient"]
    assert seg._engine_kwargs == {"input_grad": True} and seg.trainable is False
    import fetal_net.metrics as FM
    m2 = fmodel.norm_net_model((1,) + SP, old_model_path=seg, loss_function=FM.dice_and_xent, **KW)
    assert m2.metrics_names == ["loss", "binary_accuracy", "vod_coefficient", "dice_coefficient"]


def test_first_dgrad_entry_points_are_declared_bound_and_exported():
    from fmri_hip._lib import BF16, F32, LIB_PATH, SIGNATURES, lib
    names = ("fmri_conv3d_first_dgrad_ok", "fmri_conv3d_first_dgrad")
    header = open(os.path.join(ROOT, "include", "fmri_hip.h")).read()
    for n in names:
        assert re.search(r"\bint %s\s*\(" % n, header), n
        assert n in SIGNATURES
    assert len(SIGNATURES["fmri_conv3d_first_dgrad_ok"]) == 6 and len(SIGNATURES["fmri_conv3d_first_dgrad"]) == 11
    if not os.path.exists(LIB_PATH):
        import __graft_entry__ as g
        g.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB_PATH]).decode()
    for n in names:
        assert re.search(r"\bT %s\b" % n, out), n
    L = lib()
    # the 3-D range of the first-layer kernels (a host-side query: no GPU needed)
    assert L.fmri_conv3d_first_dgrad_ok(1, 32, 64, 128, 128, BF16) == 1
    assert L.fmri_conv3d_first_dgrad_ok(4, 64, 4, 16, 32, BF16) == 1
    for bad in ((1, 32, 64, 128, 128, F32), (1, 48, 4, 16, 32, BF16), (1, 32, 4, 16, 48, BF16), (1, 32, 4, 8, 32, BF16),
                (1, 32, 6, 16, 32, BF16), (5, 32, 4, 16, 32, BF16), (0, 32, 4, 16, 32, BF16)):
        assert L.fmri_conv3d_first_dgrad_ok(*bad) == 0, bad
    assert L.fmri_conv3d_first_dgrad(None, 32, None, None, 1, 4, 16, 32, 1, BF16, None) == -1          # NULL pointers: FMRI_E_SHAPE, nothing launched
