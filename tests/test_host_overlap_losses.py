"""Host side of the overlap losses (Tversky, focal Tversky, Generalised Dice, Dice + boundary): the float64 numpy forms of
fetal_net.metrics against fp64 torch autograd of the written formulas, the factories' attributes, what compile() makes of the tokens, the
data-parallel refusal and the checkpoint record.  No GPU."""
import json

import numpy as np
import pytest
import torch

import fetal_net.metrics as M


def _batch(seed, L=3, shape=(2, 5, 6, 7)):
    rs = np.random.RandomState(seed)
    return (rs.rand(*shape, L) > 0.7).astype(np.uint8), rs.rand(*shape, L)


def _sums(y, p):
    """per-label I, Sy, Sp as float64 torch tensors of the last axis' labels"""
    yt, pt = torch.from_numpy(y.astype(np.float64)).reshape(-1, y.shape[-1]), torch.from_numpy(p).reshape(-1, p.shape[-1])
    return (yt * pt).sum(0), yt.sum(0), pt.sum(0)


def _tversky(i, sy, sp, a, b, s):
    return (i + s) / (i + a * (sp - i) + b * (sy - i) + s)


@pytest.mark.parametrize("a,b", [(0.5, 0.5), (0.3, 0.7), (0.0, 1.0)])
@pytest.mark.parametrize("per_label", [False, True])
def test_tversky_forms_against_the_written_formula(a, b, per_label):
    y, p = _batch(1)
    i, sy, sp = _sums(y, p)
    if not per_label:
        i, sy, sp = i.sum(), sy.sum(), sp.sum()
    T = _tversky(i, sy, sp, a, b, 1.0)
    assert M.tversky_coefficient(y, p, a, b, 1.0, per_label) == pytest.approx(float(T.mean()), rel=1e-13)
    assert M.tversky_loss(a, b, 1.0, per_label)(y, p) == pytest.approx(-float(T.mean()), rel=1e-13)
    for g in (1.0, 4.0 / 3, 2.0):
        assert M.focal_tversky_loss(a, b, g, 1.0, per_label)(y, p) == pytest.approx(float(((1 - T) ** (1 / g)).mean()), rel=1e-13)


def test_tversky_half_half_half_is_the_dice_coefficient_to_the_last_bit():
    for seed in range(20):
        y, p = _batch(seed)
        assert M.tversky_coefficient(y, p, 0.5, 0.5, smooth=0.5) == M.dice_coefficient(y, p, smooth=1.0)
        assert M.tversky_loss(0.5, 0.5, 0.5)(y, p) == M.dice_coefficient_loss(y, p)


def test_label_mean_tversky_half_half_half_is_the_mean_label_wise_dice():
    for seed in range(20):
        y, p = _batch(seed)
        want = np.mean([M.label_wise_dice_coefficient(y, p, l) for l in range(3)])
        assert M.tversky_coefficient(y, p, 0.5, 0.5, 0.5, per_label=True) == pytest.approx(want, rel=1e-15)


def _gdl_ref(y, p, s=1e-5):
    i, sy, sp = _sums(y, p)
    present = sy > 0
    if bool(present.any()):
        w = torch.where(present, 1.0 / torch.where(present, sy, torch.ones_like(sy)) ** 2, torch.zeros_like(sy))
        w = torch.where(present, w, w.max())
    else:
        w = torch.ones_like(sy)
    return float(1 - (2 * (w * i).sum() + s) / ((w * (sy + sp)).sum() + s)), w


def test_generalised_dice_loss_and_its_absent_label_rule():
    y, p = _batch(3)
    ref, w = _gdl_ref(y, p)
    assert M.generalised_dice_loss(y, p) == pytest.approx(ref, rel=1e-13)
    assert M.generalized_dice_loss is M.generalised_dice_loss
    # one label absent: it takes the largest weight among the labels present
    y1 = y.copy()
    y1[..., 1] = 0
    ref1, w1 = _gdl_ref(y1, p)
    assert float(w1[1]) == float(max(w1[0], w1[2])) and M.generalised_dice_loss(y1, p) == pytest.approx(ref1, rel=1e-13)
    # written out: the absent label's probability mass counts with that weight
    i, sy, sp = (t.numpy() for t in _sums(y1, p))
    wl = np.array([1 / sy[0] ** 2, max(1 / sy[0] ** 2, 1 / sy[2] ** 2), 1 / sy[2] ** 2])
    assert M.generalised_dice_loss(y1, p) == pytest.approx(1 - (2 * (wl * i).sum() + 1e-5) / ((wl * (sy + sp)).sum() + 1e-5), rel=1e-13)
    # no label present at all: all weights 1
    y0 = np.zeros_like(y)
    assert M.generalised_dice_loss(y0, p) == pytest.approx(1 - 1e-5 / (p.sum() + 1e-5), rel=1e-13)


def test_dice_and_boundary_host_form():
    rs = np.random.RandomState(4)
    y = (rs.rand(2, 1, 6, 5, 4) > 0.6).astype(np.uint8)
    p, mask = rs.rand(*y.shape), rs.rand(*y.shape) * 5
    f = M.dice_and_boundary(mask, boundary_weight=0.05)
    want = M.dice_coefficient_loss(y, p) + 0.05 * np.mean((1.0 - 2.0 * y) * mask * p)
    assert f(y, p) == pytest.approx(want, rel=1e-14)
    assert f.mask_input is False and M.dice_and_boundary(M.MaskInput()).mask_input is True


def test_factories_carry_their_parameters():
    f = M.tversky_loss()
    assert (f.alpha, f.beta, f.smooth, f.per_label, f.overlap_kind, f.__name__) == (0.3, 0.7, 1.0, False, 0, "tversky_loss")
    f = M.tversky_loss(0.4, 0.6, smooth=0.5, per_label=True)
    assert (f.alpha, f.beta, f.smooth, f.per_label, f.overlap_kind) == (0.4, 0.6, 0.5, True, 2)
    assert f.loss_params == dict(alpha=0.4, beta=0.6, smooth=0.5, per_label=True)
    f = M.focal_tversky_loss()
    assert (f.alpha, f.beta, f.gamma, f.smooth, f.per_label, f.overlap_kind, f.__name__) == (0.3, 0.7, 4.0 / 3, 1.0, False, 1, "focal_tversky_loss")
    assert M.focal_tversky_loss(per_label=True).overlap_kind == 3
    assert M.generalised_dice_loss.overlap_kind == 4 and M.generalised_dice_loss.smooth == 1e-5
    f = M.dice_and_boundary(M.MaskInput(), boundary_weight=0.02)
    assert (f.boundary_weight, f.mask_input, f.overlap_kind, f.alpha, f.beta, f.smooth, f.__name__) == (0.02, True, 0, 0.5, 0.5, 0.5, "dice_and_boundary")
    assert not getattr(f, "mask_weighted", False)                # its mask is not turned into exp(-mask / sigma)
    assert M.dice_and_boundary(M.MaskInput()).boundary_weight == 0.01


def _unet(**kw):
    from fetal_net.model import unet_model_3d
    return unet_model_3d((1, 16, 16, 16), depth=2, n_base_filters=8, n_labels=3, **kw)


def test_compile_accepts_the_tokens():
    from fmri_hip import ops
    m = _unet()
    for loss, kind, param, ov in [
            (M.tversky_loss(), 7, 1.0, (0.3, 0.7, 1.0, 0.0)),
            (M.tversky_loss, 7, 1.0, (0.3, 0.7, 1.0, 0.0)),                                  # the bare factory, as getattr(metrics, name) gives it
            (M.focal_tversky_loss(0.3, 0.7, 1.5), 8, 1.0, (0.3, 0.7, 1.5, 0.0)),
            (M.tversky_loss(0.5, 0.5, 0.5, per_label=True), 9, 0.5, (0.5, 0.5, 1.0, 0.0)),
            (M.focal_tversky_loss(per_label=True), 10, 1.0, (0.3, 0.7, 4.0 / 3, 0.0)),
            (M.generalised_dice_loss, 11, 1e-5, (0.5, 0.5, 1.0, 0.0)),
            (M.generalized_dice_loss, 11, 1e-5, (0.5, 0.5, 1.0, 0.0))]:
        m.compile(loss=loss)
        assert m._loss_kind() == (kind, param) and m._loss_overlap() == ov
        assert ops.is_overlap_loss(kind) and kind - ops.LOSS_OVERLAP == m.loss.overlap_kind
    assert sorted(v for v in ops.LOSS_KINDS.values()) == list(range(12)) and ops.LOSS_WEIGHTED_DICE == 6 < ops.LOSS_OVERLAP
    m.compile(loss=M.weighted_cross_entropy_loss)
    with pytest.raises(NotImplementedError, match="focal_tversky_loss.*generalised_dice_loss.*tversky_loss"):
        m._loss_kind()


def test_mask_shape_builder_takes_dice_and_boundary_and_still_refuses_the_rest():
    from fetal_net.model import isensee2017_model_3d
    kw = dict(input_shape=(1, 16, 16, 16), n_base_filters=8, depth=3, mask_shape=(1, 16, 16, 16))
    m = isensee2017_model_3d(loss_function=M.dice_and_boundary, **kw)
    assert m._unsupported is None and m._loss_kind() == (7, 0.5) and m._loss_overlap() == (0.5, 0.5, 1.0, 0.01)
    assert "dice_coefficient" in [getattr(f, "__name__", f) for f in m.metrics]
    m = isensee2017_model_3d(loss_function=M.dice_and_xent_mask, **kw)
    assert m._unsupported is None and m._loss_kind() == (2, 1.0)
    m = isensee2017_model_3d(loss_function=lambda mask: M.tversky_loss(), **kw)
    assert m._unsupported == "mask_shape with a loss factory other than dice_and_xent_mask"


def test_loss_value_of_an_overlap_kind_is_the_slot_the_coefficient_kernel_writes():
    from fmri_hip import ops
    from fmri_hip.engine_base import EngineBase
    s = np.zeros(ops.SUMS_TOTAL)
    s[7], s[ops.SUMS_OVERLAP_VALUE] = 10.0, -0.625
    assert ops.SUMS_BD == 16 + 3 * ops.MAX_LABELS and ops.SUMS_OVERLAP_VALUE - 2 * ops.MAX_LABELS > ops.SUMS_BD
    for kind in range(7, 12):
        assert ops.loss_value_from_sums(s, kind) == -0.625
        assert EngineBase.metrics_from_sums(s, 1.0, kind, 1.0)["loss"] == -0.625
    with pytest.raises(ValueError):
        ops.loss_value_from_sums(s[:16], 7)


class _TwoRanks(object):
    world, global_dice, grad_scale = 2, True, 1.0


def test_a_two_rank_context_refuses_the_overlap_losses_by_name():
    from fmri_hip import ops
    from fmri_hip.engine_base import refuse_overlap_data_parallel
    for name in ("tversky_loss", "focal_tversky_loss", "label_tversky_loss", "label_focal_tversky_loss", "generalised_dice_loss"):
        with pytest.raises(NotImplementedError, match="^" + name + " .*all-reduced"):
            refuse_overlap_data_parallel(ops.LOSS_KINDS[name], _TwoRanks())
        refuse_overlap_data_parallel(ops.LOSS_KINDS[name], None)
    for kind in range(7):                                       # the existing losses train data-parallel as before
        refuse_overlap_data_parallel(kind, _TwoRanks())


def test_checkpoint_record_round_trip():
    from fetal_net import training
    m = _unet()
    m.compile(loss=M.focal_tversky_loss(0.3, 0.7, 1.5))
    meta = json.loads(json.dumps(m._checkpoint_meta()))
    assert meta["loss"] == "focal_tversky_loss"
    assert meta["builder_kwargs"]["loss_function"] == {"__callable__": "focal_tversky_loss",
                                                       "params": dict(alpha=0.3, beta=0.7, gamma=1.5, smooth=1.0, per_label=False)}
    again = training._builder_call(meta["builder"], meta["builder_kwargs"])
    assert again.loss is not m.loss and again.loss.__name__ == "focal_tversky_loss"
    assert again._loss_kind() == m._loss_kind() == (8, 1.0) and again._loss_overlap() == m._loss_overlap() == (0.3, 0.7, 1.5, 0.0)
    y, p = _batch(9)
    assert again.loss(y, p) == m.loss(y, p)
    # built with the loss, rather than compiled afterwards
    meta = json.loads(json.dumps(_unet(loss_function=M.tversky_loss(0.2, 0.8, per_label=True))._checkpoint_meta()))
    again = training._builder_call(meta["builder"], meta["builder_kwargs"])
    assert again._loss_kind() == (9, 1.0) and again._loss_overlap() == (0.2, 0.8, 1.0, 0.0)
    # parameterless tokens and records written before this change: a name alone, resolved as before
    meta = json.loads(json.dumps(_unet(loss_function=M.generalised_dice_loss)._checkpoint_meta()))
    assert meta["builder_kwargs"]["loss_function"] == {"__callable__": "generalised_dice_loss"}
    assert training._builder_call(meta["builder"], meta["builder_kwargs"]).loss is M.generalised_dice_loss
    old = dict(meta["builder_kwargs"], loss_function={"__callable__": "dice_coefficient_loss"})
    assert training._builder_call(meta["builder"], old).loss is M.dice_coefficient_loss
