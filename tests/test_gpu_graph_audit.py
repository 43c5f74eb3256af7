"""The layer-graph engine audited op by op against float64 (tests/graph_audit.py), on every route of fmri_hip/graph_engine.py.

The whole-network bf16 comparisons (test_isensee_bf16_padded_engine: 0.35 / 0.27, the discriminator's 0.6 / 0.38) carry the bf16 noise that
instance normalisation amplifies through the network; a dropped tap of a 27-tap image sits inside them.  Here every op is recomputed from
the engine's OWN stored inputs, so a record holds one rounding of the storage type plus fp32 accumulation, and each case asserts the routes
it is there for (a case cannot pass by falling back): the channel-padded 27-tap images behind map_p / map_g and cin_map, 1x1x1 kernels at
tap 13, the stride-2 parity route Ws2 with and without its 64-slot weight gradient, the up-sampling parity route Wup with and without its
parity-form weight gradient, the sampled (`_sub`) strides with the `gfull` scatter, `_accum` / `_slice_into`, the concat split, the dense
head on a padded source.

Not reached: the `_c32` route (the kd-sharing weight-gradient kernel fed a 32-channel dy) asks for >= 0.1 TFLOP per launch, far above these
sizes (every case asserts it is off); test_kd_sharing_weight_gradient_kernels_are_exact covers that kernel.

Bars: gpu_util's rule - every limit <= 2x the error measured on MI355X against the float64 reference (FMRI_MEASURE=1; raw output:
profiles/r06_graph_audit_measure.log, the largest of 8 runs per class: profiles/r06_graph_audit_bars_measured.json).  rtol is derived, not measured (graph_audit.audit): k * 2^-8 for a bf16 tensor that k kernels wrote or
accumulated into, 0 for fp32 tensors and parameter gradients; `atol` below is what is left for the fp32 accumulation order, relative to
max |ref|, `l2` the l2-relative error.
"""
import gc

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import graph_audit as GA          # noqa: E402
from gpu_util import bar          # noqa: E402

# caps: conditions, not measurements.  One bf16 rounding is ~1e-3 l2; the smallest structural error the audit is for (one tap of 27 ~ 0.19,
# one channel of 128 ~ 0.09) stays >= 9x above them.
CAP_STORED_L2 = 1e-2
CAP_PARAM = 1e-4

# class of record -> (atol, l2) limits, each <= 2x the largest value measured over the cases (the comment: measured atol, l2).
# Classes: `fwd.<kind>` (conv_up / conv_s2: the Wup / Ws2 parity routes; conv_direct: the direct 1x1x1 / stride-2 kernels of the exact-size
# engines), `tgrad.k<consumers>` (`_up`: one of them a Wup conv; `_up0`: one of them a conv with the fused nearest x2 outside the parity
# route), `<dW|db|dgamma|dbeta>.<kind>`, `db.conv_cancel` (bias of a conv that feeds a normalisation: a sum that cancels, judged on
# sum |dz|), `stats` (mean and 1 / s of a normalisation), `dlogits` (Gt of the logits' source = the rounded dlogits: exact).
#
# What the figures say.  A bf16 tensor written by ONE kernel in one rounding (fwd.conv / conv_s2 / norm / add / dropout / avgpool, tgrad.k1)
# sits inside rtol = 2^-8 up to an atol of 1e-9 .. 4e-7 - the fp32 accumulation error of a value next to a rounding boundary - and shows the
# l2 of one bf16 rounding, 1.7e-3.  Four classes carry a second rounding that rtol |ref| cannot cover where the terms cancel, and their
# atol is 1.5e-3 .. 2.9e-3 of max |ref| (l2 2.4e-3 .. 2.9e-3):
#   * fwd.conv_up, tgrad.*_up: the Wup route adds up to 8 fp32 taps into one parity filter and rounds the SUM to bf16; the reference rounds
#     every tap on its own.  The difference is a weight perturbation of 2^-9 relative size, i.e. an output error of the size of the bf16
#     rounding itself but not proportional to the output element;
#   * tgrad.*_up0: the full-resolution input gradient is stored in bf16, then its 2 x 2 (x 2) voxels are added and rounded again;
#   * tgrad.k2*: every contribution is rounded on its own, then the accumulated sum (`_accum`, `_slice_into`) once more.
# Against the op-level tests of the same kernels: bf16 tensors - test_gpu_ops.TOL / NORM_TOL / DIRECT_TOL are (5e-3, 1e-4), PARITY_TOL
# (6e-3, 6e-3): every bar here is inside them (rtol 3.9e-3).  fp32 tensors - TOL (2e-6, 2e-6) allows 4e-6 at the largest elements, fwd.conv
# here 4.6e-6: measured 2.3e-6 at the two-source 48-channel convolution, 27 x 48 products per sum against the op test's 27 x 16.
# Weight gradients - WG_TOL bf16 (2e-6, 2e-6), fp32 (1e-5, 2e-6): dW.conv 2.2e-6 / 2.1e-6 with rtol 0 is inside both at the large elements
# and 10 % above at the small ones (sums over 65536 voxels x 2 samples, measured 1.1e-6); DIRECT_TOL dw (2.7e-7 bf16, 2.6e-6 fp32) against
# dW.conv_direct: the direct kernels' sums here run over up to 32768 voxels x 2 samples, the op test's over 4096.
BARS = {
    "bf16": {
        "dW.conv":               (2.2e-06, 1.0e-06),      # measured 1.12e-06, 5.21e-07
        "dW.conv_direct":        (1.4e-06, 1.0e-06),      # measured 7.07e-07, 5.37e-07
        "dW.dense":              (8.1e-07, 6.4e-07),      # measured 4.07e-07, 3.23e-07
        "db.conv":               (1.2e-06, 1.2e-06),      # measured 6.15e-07, 6.15e-07
        "db.conv_cancel":        (4.9e-08, 3.4e-08),      # measured 2.46e-08, 1.71e-08
        "db.conv_direct":        (2.3e-07, 2.3e-07),      # measured 1.20e-07, 1.20e-07
        "db.conv_direct_cancel": (2.6e-08, 1.0e-08),      # measured 1.32e-08, 5.13e-09
        "db.dense":              (3.7e-07, 4.8e-07),      # measured 1.87e-07, 2.42e-07
        "dbeta.norm":            (7.1e-07, 6.7e-07),      # measured 3.57e-07, 3.38e-07
        "dgamma.norm":           (7.0e-07, 5.7e-07),      # measured 3.53e-07, 2.88e-07
        "dlogits":               (0.0e+00, 0.0e+00),      # measured 0.00e+00, 0.00e+00
        "fwd.add":               (0.0e+00, 3.5e-03),      # measured 0.00e+00, 1.80e-03
        "fwd.avgpool":           (0.0e+00, 3.4e-03),      # measured 0.00e+00, 1.71e-03
        "fwd.conv":              (2.7e-07, 3.3e-03),      # measured 1.35e-07, 1.70e-03
        "fwd.conv_direct":       (6.0e-08, 3.3e-03),      # measured 3.01e-08, 1.66e-03
        "fwd.conv_s2":           (9.3e-08, 3.3e-03),      # measured 4.69e-08, 1.66e-03
        "fwd.conv_up":           (4.6e-03, 5.7e-03),      # measured 2.31e-03, 2.88e-03
        "fwd.dense":             (3.0e-06, 2.1e-06),      # measured 1.54e-06, 1.07e-06
        "fwd.dropout":           (0.0e+00, 3.3e-03),      # measured 0.00e+00, 1.67e-03
        "fwd.gap":               (0.0e+00, 0.0e+00),      # measured 0.00e+00, 0.00e+00
        "fwd.maxpool":           (0.0e+00, 0.0e+00),      # measured 0.00e+00, 0.00e+00
        "fwd.norm":              (2.0e-08, 3.3e-03),      # measured 1.03e-08, 1.69e-03
        "fwd.upsample":          (0.0e+00, 0.0e+00),      # measured 0.00e+00, 0.00e+00
        "stats":                 (1.4e-07, 8.3e-08),      # measured 7.36e-08, 4.18e-08
        "tgrad.k1":              (7.9e-07, 3.4e-03),      # measured 3.96e-07, 1.71e-03
        "tgrad.k1_up":           (3.2e-03, 5.1e-03),      # measured 1.64e-03, 2.58e-03
        "tgrad.k1_up0":          (3.0e-03, 4.9e-03),      # measured 1.51e-03, 2.45e-03
        "tgrad.k2":              (4.1e-03, 4.8e-03),      # measured 2.08e-03, 2.44e-03
        "tgrad.k2_up":           (5.1e-03, 5.1e-03),      # measured 2.57e-03, 2.60e-03
        "tgrad.k2_up0":          (5.7e-03, 5.0e-03),      # measured 2.88e-03, 2.53e-03
    },
    "fp32": {
        "dW.conv":               (1.3e-06, 8.9e-07),      # measured 6.91e-07, 4.47e-07
        "dW.conv_direct":        (2.1e-06, 1.3e-06),      # measured 1.09e-06, 6.84e-07
        "db.conv_cancel":        (9.1e-08, 4.7e-08),      # measured 4.57e-08, 2.37e-08
        "db.conv_direct":        (5.1e-07, 5.1e-07),      # measured 2.55e-07, 2.55e-07
        "db.conv_direct_cancel": (1.1e-07, 7.1e-08),      # measured 5.73e-08, 3.59e-08
        "dbeta.norm":            (8.6e-07, 7.6e-07),      # measured 4.33e-07, 3.82e-07
        "dgamma.norm":           (4.0e-07, 3.6e-07),      # measured 2.03e-07, 1.85e-07
        "dlogits":               (0.0e+00, 0.0e+00),      # measured 0.00e+00, 0.00e+00
        "fwd.add":               (1.1e-07, 5.4e-08),      # measured 5.55e-08, 2.74e-08
        "fwd.conv":              (4.6e-06, 1.8e-06),      # measured 2.31e-06, 9.50e-07
        "fwd.conv_direct":       (2.3e-06, 1.2e-06),      # measured 1.16e-06, 6.27e-07
        "fwd.dropout":           (6.6e-08, 5.1e-08),      # measured 3.33e-08, 2.56e-08
        "fwd.norm":              (2.3e-07, 1.0e-07),      # measured 1.17e-07, 5.30e-08
        "fwd.upsample":          (0.0e+00, 0.0e+00),      # measured 0.00e+00, 0.00e+00
        "stats":                 (1.3e-07, 6.2e-08),      # measured 6.89e-08, 3.11e-08
        "tgrad.k1":              (3.7e-06, 1.6e-06),      # measured 1.87e-06, 8.21e-07
        "tgrad.k1_up0":          (9.2e-07, 6.8e-07),      # measured 4.63e-07, 3.41e-07
        "tgrad.k2":              (2.1e-06, 1.0e-06),      # measured 1.09e-06, 5.27e-07
        "tgrad.k2_up0":          (5.7e-07, 2.4e-07),      # measured 2.86e-07, 1.20e-07
    },
}
# the largest atol of a bf16 tensor written by one kernel in one rounding; graph_audit.LARGEST_SINGLE_KERNEL_BAR is what the fault detection,
# here and in tests/test_host_graph_audit.py, is held against
SINGLE_KERNEL = ("fwd.conv", "fwd.conv_s2", "fwd.conv_direct", "fwd.norm", "fwd.add", "fwd.dropout", "fwd.avgpool", "fwd.maxpool", "fwd.upsample",
                 "tgrad.k1")


def _perturb(W, seed=5):
    r2 = np.random.RandomState(seed)
    for k in W:
        if k.endswith(("/bias", "/beta")):
            W[k] = (r2.randn(*W[k].shape) * 0.05).astype(np.float32)
        if k.endswith("/gamma"):
            W[k] = (1.0 + r2.randn(*W[k].shape) * 0.1).astype(np.float32)
    return W


def _classes(eng, snap, recs):
    consumers = {}
    for o in snap["ops"]:
        for i in o["ins"]:
            consumers.setdefault(i, []).append(o)
    by_out = {o["out"]: o for o in snap["ops"]}
    # the exact-size engines run 1x1x1 and isotropic stride-2 convolutions on the direct kernels
    direct = lambda r: r["kind"] == "conv" and not eng.pad and (by_out[r["op"]]["k"] != 3 or (by_out[r["op"]]["sub"] is None and by_out[r["op"]]["strides"][0] != 1))
    out = []
    for r in recs:
        if r["what"] == "fwd":
            kind = r["kind"]
            if kind == "conv":
                kind = "conv_up" if r["name"] in eng.Wup else ("conv_s2" if r["name"] in eng.Ws2 else ("conv_direct" if direct(r) else "conv"))
            out.append("fwd." + kind)
        elif r["what"] == "tgrad":
            cs = consumers[r["tensor"]]
            tag = "_up" if any(c["name"] in eng.Wup for c in cs) else ("_up0" if any(c["up0"] for c in cs) else "")
            out.append("tgrad.k%d%s" % (r["k"], tag))
        elif r["what"] in ("stats", "dlogits"):
            out.append(r["what"])
        else:
            out.append("%s.%s%s%s" % (r["what"], r["kind"], "_direct" if direct(r) else "", "_cancel" if r["cancel"] else ""))
    return out


def _judge(case, eng, snap, recs):
    """print the case's summary, hold every record to its class's bar and to the caps, the padding to exactly zero"""
    mode = "bf16" if eng.dtype == torch.bfloat16 else "fp32"
    assert not (eng.pad and any(eng._c32.values()))          # (the `_c32` route is out of reach at these sizes: module docstring)
    cls = _classes(eng, snap, recs)
    worst = {}
    for c, r in zip(cls, recs):
        w = worst.setdefault(c, dict(atol=0.0, l2=0.0, n=0, at=None))
        if max(r["err"], r["l2"]) >= max(w["atol"], w["l2"]):
            w["at"] = r["op"]
        w["atol"], w["l2"], w["n"] = max(w["atol"], r["err"]), max(w["l2"], r["l2"]), w["n"] + 1
    print("\naudit %s (%s): %d ops, %d records" % (case, mode, len(snap["ops"]), len(recs)))
    for c in sorted(worst):
        w = worst[c]
        print("  %-22s n %3d  atol %.3e  l2 %.3e  (worst at %s)" % (c, w["n"], w["atol"], w["l2"], w["at"]))
    for c, r in zip(cls, recs):
        what = (case, r["op"], r["what"], r["err"], r["l2"])
        assert np.isfinite(r["err"]) and np.isfinite(r["l2"]), what
        if r["what"] in ("fwd", "tgrad", "dlogits"):
            assert r["l2"] <= CAP_STORED_L2, what
        elif r["what"] != "stats":
            assert r["err"] <= CAP_PARAM and r["l2"] <= CAP_PARAM, what
    for c in sorted(worst):
        limit = BARS[mode].get(c, (0.0, 0.0))
        bar("graph_audit.%s.%s.atol" % (mode, c), worst[c]["atol"], limit[0])
        bar("graph_audit.%s.%s.l2" % (mode, c), worst[c]["l2"], limit[1])
    # the padding channels of every activation are exactly zero, the logits' gradient is zero beyond the labels, and no gradient entry
    # outside the logical parameters is set (map_g must not gather from non-zero padding)
    for name, v in snap["pad_max"].items():
        assert v == 0.0, (case, "padding of T", name, v)
    assert snap["gpad_max"][snap["logits_src"]] == 0.0
    for name, v in snap["grad_pad"].items():
        assert v == 0.0, (case, "gradient outside the logical parameters", name, v)
    return cls


def _step(eng, xd, yd):
    eng.forward(xd)
    if eng.head == "dense":
        eng.bce_forward(yd)
    else:
        eng.loss_forward(yd)
    eng.backward(yd)
    torch.cuda.synchronize()
    return GA.snapshot(eng, xd)


def _detect(snap, clean, classes, at, fault, key):
    """the reference of op `at` restated with a known mistake.  The record `key` must stand > 100x above the largest bar of a bf16 tensor
    written by one kernel, >= 9x above the cap on any stored tensor in l2, and >= 25x above both bars of its own class (the classes with a
    second rounding have bars of 3e-3 .. 5.7e-3: one tap of 27, ~0.19, cannot stand 100x above those)"""
    ops = {o["out"]: o for o in snap["ops"]}
    only = {at} if fault != "missing_consumer" else {o["out"] for o in snap["ops"] if at in o["ins"]}
    if fault == "second_max":
        only = {at}
    bad = GA.audit(snap, fault=(at, fault), only=only)
    b, c = GA.find(bad, *key), GA.find(clean, *key)
    print("  fault %-16s at %-28s %s: err %.3e l2 %.3e (clean %.3e / %.3e)" % (fault, ops.get(at, {}).get("name", at), key[1], b["err"], b["l2"],
                                                                             c["err"], c["l2"]))
    assert b["err"] > 100 * GA.LARGEST_SINGLE_KERNEL_BAR and b["l2"] >= GA.MIN_FAULT_L2, (fault, at, b)
    cls = dict(zip([(r["op"], r["what"]) for r in clean], classes))[key]
    assert b["err"] >= 25 * BARS["bf16"][cls][0] and b["l2"] >= 25 * BARS["bf16"][cls][1], (fault, at, cls, b)
    for r in bad:                                             # and whatever else was recomputed next to it is where it was
        if (r["op"], r["what"]) != key:
            c2 = GA.find(clean, r["op"], r["what"])
            assert (r["err"], r["l2"]) == (c2["err"], c2["l2"]), (fault, r["op"], r["what"])


def test_largest_stored_bar_is_what_the_detection_threshold_assumes():
    stored = [BARS["bf16"][c][0] for c in SINGLE_KERNEL if c in BARS["bf16"]]
    assert len(stored) >= 8 and max(stored) <= GA.LARGEST_SINGLE_KERNEL_BAR
    for mode in BARS:                                         # and every bar respects the caps
        for c, (atol, l2) in BARS[mode].items():
            if c.startswith(("fwd.", "tgrad.", "dlogits")):
                assert l2 <= CAP_STORED_L2, (mode, c)
            elif c != "stats":
                assert atol <= CAP_PARAM and l2 <= CAP_PARAM, (mode, c)


# ------------------------------------------------------------------------------------------------ A - D: isensee2017_model_3d
def _isensee(base, N=2, sp=(16, 32, 64)):
    import fetal_net.model as fmodel
    from oracle import isensee_oracle as I, unet_oracle as O
    kw = dict(input_shape=(1,) + sp, depth=3, n_base_filters=base, n_segmentation_levels=2, dropout_rate=0.3)
    model, spec = fmodel.isensee2017_model_3d(**kw), I.IsenseeSpec(**kw)
    W = _perturb(spec.init_weights(31))
    x, y = O.synthetic_batch((N, 1) + sp)
    rs = np.random.RandomState(8)
    masks = {"spatial_dropout3d_%d" % (lv + 1): torch.tensor((rs.rand(N, spec.levels[lv]["filters"]) < 0.7).astype(np.float32) / 0.7).cuda()
             for lv in range(3)}
    return model, W, x.reshape(N, *sp, 1), torch.from_numpy(y).cuda().reshape(-1).contiguous(), masks


def _isensee_engine(base, dtype=torch.bfloat16):
    from fmri_hip.graph_engine import LayerGraphEngine
    model, W, x, yd, masks = _isensee(base)
    eng = LayerGraphEngine(model.layers, x.shape[0], dtype=dtype)
    eng.load_keras_weights(W)
    eng.set_dropout_masks(masks)
    return eng, torch.from_numpy(x).cuda().to(dtype).contiguous(), yd


def _padded_routes(eng):
    """(Ws2 entries with / without the parity-form weight gradient, the same of Wup)"""
    assert eng.pad and not any(eng._c32.values())            # (the `_c32` route is out of reach at these sizes: module docstring)
    s2 = sorted(n for n, w in eng.Ws2.items() if w["wgrad"]), sorted(n for n, w in eng.Ws2.items() if not w["wgrad"])
    up = sorted(n for n, w in eng.Wup.items() if w["wgrad"]), sorted(n for n, w in eng.Wup.items() if not w["wgrad"])
    return s2, up


def _phys(eng, name):
    return eng.shape[name][0]


def _assert_case_a_routes(eng):
    (s2w, s2n), (upw, upn) = _padded_routes(eng)
    assert len(s2w) == 1 and len(s2n) == 1 and len(upw) == 1 and len(upn) == 1, (s2w, s2n, upw, upn)
    # real padding: 24 -> 32, 48 -> 64, and a concat both of whose halves carry holes
    assert sorted(set((eng.clog[n], _phys(eng, n)) for n in eng.convs)) == [(1, 32), (24, 32), (48, 64), (96, 96)]
    holes = [n for n, o in eng.convs.items() if len(o["ins"]) == 2 and all(eng.clog[i] < _phys(eng, i) for i in o["ins"])]
    assert holes and all(len(eng.cin_map[n]) < eng.Wp32[n].shape[2] for n in holes)
    # the 32-wide channel blocks (CIB 32) of the parity-form weight gradient: 96 channels on the blocked side of both launches
    assert _phys(eng, s2w[0]) == 96 and eng.Wp32[upw[0]].shape[2] == 96
    return s2w, s2n, upw, upn


def test_case_a_isensee_base24_padded_bf16():
    """A: 24 -> 32 and 48 -> 64 padding, holes in both halves of a concat, Ws2 and Wup each with one parity-form weight gradient (96 channels: the
    32-wide blocks) and one without (stride-1 wgrad on `gfull` / fused-up0 27-tap wgrad)"""
    eng, xd, yd = _isensee_engine(24)
    s2w, s2n, upw, upn = _assert_case_a_routes(eng)
    snap = _step(eng, xd, yd)
    recs = GA.audit(snap)
    cls = _judge("A", eng, snap, recs)
    out_of = {o["name"]: o["out"] for o in snap["ops"]}
    one = [o for o in snap["ops"] if o["kind"] == "conv" and o["k"] == 1 and eng.clog[o["out"]] > 1][0]
    cat = [o for o in snap["ops"] if o["kind"] == "conv" and len(o["ins"]) == 2][0]
    two = [r for r in recs if r["what"] == "tgrad" and r["k"] == 2][0]
    _detect(snap, recs, cls, out_of[s2w[0]], "drop_tap13", (out_of[s2w[0]], "fwd"))
    _detect(snap, recs, cls, out_of[upw[0]], "drop_tap13", (out_of[upw[0]], "fwd"))
    _detect(snap, recs, cls, one["out"], "tap12", (one["out"], "fwd"))
    _detect(snap, recs, cls, cat["out"], "swap_concat", (cat["out"], "fwd"))
    _detect(snap, recs, cls, out_of[s2n[0]], "phase", (out_of[s2n[0]], "fwd"))
    _detect(snap, recs, cls, two["tensor"], "missing_consumer", (two["op"], "tgrad"))


def test_case_b_isensee_base32_padded_bf16():
    """B: no padding but at the ends (32 / 64 / 128 wide): the parity-form weight gradients with 64-multiple channel counts on both sides
    (the kd'-sharing kernel)"""
    eng, xd, yd = _isensee_engine(32)
    (s2w, s2n), (upw, upn) = _padded_routes(eng)
    assert s2w and upw
    assert all(_phys(eng, n) % 64 == 0 and eng.Wp32[n].shape[2] % 64 == 0 for n in s2w + upw)
    assert sorted(set(_phys(eng, n) for n in eng.convs)) == [32, 64, 128]
    snap = _step(eng, xd, yd)
    _judge("B", eng, snap, GA.audit(snap))


def test_case_c_isensee_base24_deterministic(monkeypatch):
    """C: FMRI_DETERMINISTIC=1 gives up the parity-form weight gradients: the stride-2 convs run sampled at stride 1 with the `gfull`
    scatter, the up-sampling convs keep the parity form forward / input gradient and take the fused-up0 27-tap weight gradient"""
    monkeypatch.setenv("FMRI_DETERMINISTIC", "1")
    eng, xd, yd = _isensee_engine(24)
    try:
        assert eng.deterministic and eng.pad and not eng.Ws2 and eng.Wup and not any(w["wgrad"] for w in eng.Wup.values())
        assert sum(1 for o in eng.ops if o["kind"] == "conv" and o["sub"] == (2, 2, 2)) == 2 and len(eng.gfull) == 2
        snap = _step(eng, xd, yd)
        _judge("C", eng, snap, GA.audit(snap))
    finally:
        eng.close()                                           # one deterministic registration per process
        del eng
        gc.collect()


@pytest.mark.parametrize("dtype,tag", [(torch.float32, "fp32"), (torch.bfloat16, "bf16_nopad")])
def test_case_d_isensee_base24_exact_size_engines(monkeypatch, dtype, tag):
    """D: the exact-size engines (fp32, and bf16 with FMRI_GRAPH_PAD=0): the direct 1x1x1 / stride-2 kernels"""
    monkeypatch.setenv("FMRI_GRAPH_PAD", "0")
    eng, xd, yd = _isensee_engine(24, dtype)
    assert not eng.pad and not eng.Ws2 and not eng.Wup
    assert any(o["kind"] == "conv" and o["s"] == 2 and o["sub"] is None for o in eng.ops) and any(o["kind"] == "conv" and o["k"] == 1 for o in eng.ops)
    snap = _step(eng, xd, yd)
    _judge("D " + tag, eng, snap, GA.audit(snap))


# ------------------------------------------------------------------------------------------------ E: 2-D Isensee
def test_case_e_isensee2d_padded_bf16():
    """E: planar (the slices ride the kernels' D axis); strides through `_sub`; fused-upsample 9-tap convs (no parity routes in 2-D)"""
    import fetal_net.model as fmodel
    from fmri_hip.graph_engine import LayerGraphEngine
    from oracle import isensee_oracle as I
    N, X, Y, C = 8, 64, 64, 5
    kw = dict(input_shape=(X, Y, C), depth=3, n_base_filters=16, n_segmentation_levels=2, dropout_rate=0.3)
    model, spec = fmodel.isensee2017_model(**kw), I.IsenseeSpec(ndim=2, **kw)
    W = _perturb(spec.init_weights(4))
    rs = np.random.RandomState(2)
    x = rs.randn(N, X, Y, C).astype(np.float32)
    yd = torch.from_numpy((rs.rand(N, X, Y, 1) > 0.7).astype(np.uint8)).cuda().reshape(-1).contiguous()
    masks = {"spatial_dropout2d_%d" % (lv + 1): torch.tensor((rs.rand(N, spec.levels[lv]["filters"]) < 0.7).astype(np.float32) / 0.7).cuda()
             for lv in range(3)}
    eng = LayerGraphEngine(model.layers, N, dtype=torch.bfloat16)
    eng.load_keras_weights(W)
    eng.set_dropout_masks(masks)
    assert eng.pad and eng.planar and not eng.Ws2 and not eng.Wup
    assert sum(1 for o in eng.ops if o["kind"] == "conv" and o["sub"] == (2, 2)) == 2 and len(eng.full) == 2 and len(eng.gfull) == 2
    assert any(o["kind"] == "conv" and o["up0"] for o in eng.ops)
    snap = _step(eng, torch.from_numpy(x).cuda().unsqueeze(0).to(torch.bfloat16).contiguous(), yd)
    _judge("E", eng, snap, GA.audit(snap))


# ------------------------------------------------------------------------------------------------ F: unet_model_3d on the layer-graph engine
def test_case_f_unet3d_on_the_graph_engine_bf16():
    """F: max-pool (ties among the ReLU's zeros: first maximum in scan order), the two-source conv on [up-sampled, skip] - the engine fuses the
    concatenation, the up-sampling in front of a concatenation is materialised - with the concat split of its input gradient into
    `upsample_bwd` and the skip (which the max-pool's gradient is accumulated onto), fused-ReLU convs (Gt holds dz)"""
    import fetal_net.model as fmodel
    from fmri_hip.graph_engine import LayerGraphEngine
    from oracle import unet_oracle as O
    sp, N = (8, 16, 32), 2
    model = fmodel.unet_model_3d(input_shape=(1,) + sp, depth=2, n_base_filters=32)
    W = _perturb(O.Spec((1,) + sp, depth=2, n_base_filters=32).init_weights(4))
    eng = LayerGraphEngine(model.layers, N, dtype=torch.bfloat16)
    eng.load_keras_weights(W)
    assert eng.pad and any(o["kind"] == "maxpool" for o in eng.ops)
    cat = [o for o in eng.ops if o["kind"] == "conv" and len(o["ins"]) == 2]
    assert len(cat) == 1 and [o["out"] for o in eng.ops if o["kind"] == "upsample"] == [cat[0]["ins"][0]]
    assert len(eng.consumers[cat[0]["ins"][1]]) == 2                                       # the skip: max-pool + concatenation
    assert sum(1 for o in eng.ops if o["kind"] == "conv" and o["act"] != 0) >= 4
    x, y = O.synthetic_batch((N, 1) + sp)
    snap = _step(eng, torch.from_numpy(x).cuda().reshape(N, *sp, 1).to(torch.bfloat16).contiguous(), torch.from_numpy(y).cuda().reshape(-1).contiguous())
    pool_src = [o["ins"][0] for o in snap["ops"] if o["kind"] == "maxpool"][0]
    w = GA._windows(snap["T"][pool_src], (2, 2, 2))
    assert int(((w == w.max(-1, keepdim=True).values).sum(-1) >= 2).sum()) > 0            # the first-max rule is exercised
    recs = GA.audit(snap)
    _judge("F", eng, snap, recs)


# ------------------------------------------------------------------------------------------------ G: PatchGAN discriminator
@pytest.mark.parametrize("base", [8, 4])
def test_case_g_discriminator_padded_bf16_with_input_gradient(base):
    """G: dense head, padded 2-channel input, (2, 2, 1) strides through `_sub`, average pooling, global average pooling; the input gradient is
    audited too.  At 8 base filters the last block is 32 wide - no padding in front of the dense head; 4 base filters (16 -> 32) add the
    dense layer that reads, and hands its gradient to, a channel-padded source."""
    from fmri_hip.graph_engine import LayerGraphEngine
    from test_gpu_adversarial import _dev_x, _dis_setup, _engine_masks
    N = 4
    model, spec, W, x, t, masks = _dis_setup((2, 32, 32, 16), N, 4, base)
    eng = LayerGraphEngine(model.layers, N, dtype=torch.bfloat16, input_grad=True)
    eng.load_keras_weights(W)
    eng.set_dropout_masks(_engine_masks(masks))
    assert eng.pad and eng.head == "dense" and eng.shape[eng.input_name][0] == 32 and eng.clog[eng.input_name] == 2
    assert any(o["kind"] == "conv" and o["sub"] == (2, 2, 1) for o in eng.ops)
    assert {"avgpool", "gap", "dense"} <= {o["kind"] for o in eng.ops}
    dense0 = [o for o in eng.ops if o["kind"] == "dense"][0]
    assert (eng.T[dense0["ins"][0]].shape[1] > eng.layout[dense0["name"]]["K"]) == (base == 4)      # a channel-padded source
    snap = _step(eng, _dev_x(eng, x, torch.bfloat16), torch.from_numpy(t.astype(np.float32)).cuda().reshape(-1))
    recs = GA.audit(snap)
    assert any(r["what"] == "tgrad" and r["tensor"] == eng.input_name for r in recs)
    cls = _judge("G base %d" % base, eng, snap, recs)
    if base != 8:
        return
    strided = [o for o in snap["ops"] if o["kind"] == "conv" and o["sub"] == (2, 2, 1)][0]
    widest = max((o for o in snap["ops"] if o["kind"] == "conv"), key=lambda o: sum(eng.clog[i] for i in o["ins"]))
    inorm = [o for o in snap["ops"] if o["kind"] == "norm" and o["instance"]][-1]
    _detect(snap, recs, cls, strided["out"], "phase", (strided["out"], "fwd"))
    _detect(snap, recs, cls, widest["out"], "zero_cin", (widest["out"], "fwd"))
    _detect(snap, recs, cls, inorm["out"], "batch_stats", (inorm["out"], "fwd"))
