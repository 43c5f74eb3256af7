"""tests/graph_audit.py audits itself on the CPU: a hand-written op list with every op kind, its snapshot made by an independent float64
forward and torch AUTOGRAD backward of the whole graph (no rounding anywhere).  The clean snapshot must audit to ~0 everywhere, and each
known mistake injected into the reference of one op must be flagged at that op's record and nowhere else: > 100x the largest bar a bf16
tensor written by one kernel has in tests/test_gpu_graph_audit.py, and >= 9x its cap on any stored tensor (graph_audit.MIN_FAULT_L2) in both
metrics.  (The mistake sits in the reference, not in the stored tensors: a corrupted stored tensor would also be the input of the next op.)"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import graph_audit as GA

N = 2


def _op(kind, out, ins, name=None, k=None, strides=None, up0=False, act="none", pool=None, instance=None, rate=None, units=None):
    sub = strides if (strides is not None and strides != (1, 1, 1) and len(set(strides)) != 1) else None
    return dict(kind=kind, name=name or out, ins=ins, out=out, k=k, strides=strides, sub=sub, up0=up0, act=act, pool=pool, instance=instance,
                rate=rate, units=units)


OPS = [
    _op("conv", "a1", ["input"], name="c1", k=3, strides=(1, 1, 1), act="relu"),          # fused ReLU; a1 has two consumers
    _op("conv", "c2", ["a1"], k=3, strides=(2, 2, 2)),                                    # stride 2 on the odd extent 9
    _op("norm", "l2", ["c2"], name="n2", instance=True, act="leaky"),
    _op("conv", "c3", ["a1"], k=3, strides=(2, 2, 1)),                                    # (2, 2, 1) on the odd extent
    _op("dropout", "dr", ["c3"], rate=0.3),                                               # dropped channels = ties for the max-pool
    _op("maxpool", "mp", ["dr"], pool=(1, 1, 2)),
    _op("add", "ad", ["l2", "mp"]),
    _op("avgpool", "ap", ["ad"]),                                                         # (5, 4, 3) -> (2, 2, 1): cropped; two consumers
    _op("upsample", "us", ["ap"], pool=None),
    _op("conv", "c6", ["us"], k=1, strides=(1, 1, 1)),                                    # 1x1x1
    _op("conv", "c5", ["ap", "c6"], k=3, strides=(1, 1, 1), up0=True),                    # two sources, fused nearest x2 on the first; the widest
    _op("norm", "r5", ["c5"], name="n5", instance=False, act="relu"),
    _op("gap", "gp", ["r5"]),
    _op("dense", "d1", ["gp"], units=4, act="leaky"),
    _op("dense", "d2", ["d1"], units=1),
]
CH = dict(input=3, a1=8, c2=8, c3=8, c6=5, c5=7)


def _weights():
    rs = np.random.RandomState(3)
    t = lambda *s: torch.from_numpy(rs.randn(*s)).double()
    W = {}
    for name, cin, cout, k in (("c1", 3, 8, 3), ("c2", 8, 8, 3), ("c3", 8, 8, 3), ("c6", 8, 5, 1), ("c5", 13, 7, 3)):
        W[name + "/kernel"] = t(k, k, k, cin, cout) / np.sqrt(k ** 3 * cin)
        W[name + "/bias"] = t(cout) * 0.1
    for name, c in (("n2", 8), ("n5", 7)):
        W[name + "/gamma"] = 1 + 0.1 * t(c)
        W[name + "/beta"] = 0.1 * t(c)
    for name, K, M in (("d1", 7, 4), ("d2", 4, 1)):
        W[name + "/kernel"] = t(K, M) / np.sqrt(K)
        W[name + "/bias"] = t(M) * 0.1
    return W


def _tf_conv(x, kernel, bias, strides):
    """the stride-1 'same' result sampled where TensorFlow's strided 'same' convolution sits: at 2o for an odd extent, at 2o + 1 for an even one"""
    y = F.conv3d(x, kernel.permute(4, 3, 0, 1, 2), bias, padding=kernel.shape[0] // 2)
    sl = [slice(None), slice(None)]
    for n, s in zip(x.shape[2:], strides):
        sl.append(slice(None) if s == 1 else slice(0 if n % 2 else 1, None, 2))
    return y[tuple(sl)]


@pytest.fixture(scope="module")
def snap():
    """independent forward (other formulations than graph_audit's) + autograd backward of the whole graph"""
    rs = np.random.RandomState(11)
    W = {k: v.clone().requires_grad_(True) for k, v in _weights().items()}
    x = torch.from_numpy(rs.randn(N, 3, 9, 8, 6)).double()
    x[1] = 3 * x[1] + 1                                       # (two samples of unlike statistics: batch statistics are not the instance's)
    x.requires_grad_(True)
    drop = torch.tensor([[1, 0, 1, 1, 0, 1, 1, 1], [0, 1, 1, 0, 1, 1, 1, 1]], dtype=torch.float64) / 0.7
    T, pre = {"input": x}, {}

    def keep(name, t, z=None):
        t.retain_grad()
        T[name] = t
        if z is not None:
            z.retain_grad()
            pre[name] = z
        return t

    z = _tf_conv(x, W["c1/kernel"], W["c1/bias"], (1, 1, 1))
    a1 = keep("a1", torch.clamp(z, min=0), z)
    c2 = keep("c2", _tf_conv(a1, W["c2/kernel"], W["c2/bias"], (2, 2, 2)))
    xh = (c2 - c2.mean((2, 3, 4), keepdim=True)) / (c2.std((2, 3, 4), unbiased=False, keepdim=True) + 1e-3)
    v = xh * W["n2/gamma"].view(1, -1, 1, 1, 1) + W["n2/beta"].view(1, -1, 1, 1, 1)
    l2 = keep("l2", torch.where(v > 0, v, 0.3 * v))
    c3 = keep("c3", _tf_conv(a1, W["c3/kernel"], W["c3/bias"], (2, 2, 1)))
    dr = keep("dr", c3 * drop.view(N, 8, 1, 1, 1))
    mp = keep("mp", F.max_pool3d(dr, (1, 1, 2)))
    ad = keep("ad", l2 + mp)
    ap = keep("ap", F.avg_pool3d(ad, 2))
    us = keep("us", F.interpolate(ap, scale_factor=2, mode="nearest"))
    c6 = keep("c6", torch.einsum("ncdhw,co->nodhw", us, W["c6/kernel"][0, 0, 0]) + W["c6/bias"].view(1, -1, 1, 1, 1))
    cat = torch.cat([F.interpolate(ap, scale_factor=2, mode="nearest"), c6], 1)
    c5 = keep("c5", _tf_conv(cat, W["c5/kernel"], W["c5/bias"], (1, 1, 1)))
    v = F.batch_norm(c5, None, None, W["n5/gamma"], W["n5/beta"], training=True, eps=1e-3)
    r5 = keep("r5", torch.relu(v))
    gp = keep("gp", r5.mean((2, 3, 4)))
    d1 = keep("d1", F.leaky_relu(gp @ W["d1/kernel"] + W["d1/bias"], 0.3))
    d2 = keep("d2", d1 @ W["d2/kernel"] + W["d2/bias"])
    loss = (torch.sigmoid(d2) * torch.tensor([[0.7], [-1.3]], dtype=torch.float64)).sum()
    loss.backward()
    G = {n: t.grad.detach().clone() for n, t in T.items()}
    for n, z in pre.items():
        G[n] = z.grad.detach().clone()               # a conv with a fused ReLU: the engine leaves dz in Gt[out]
    return dict(nd=3, dtype=torch.float64, input_name="input", logits_src="d2", n_labels=1, head="dense", pad=False, ops=OPS,
                T={n: t.detach().clone() for n, t in T.items()}, G=G, drop={"dr": drop}, stats={}, dlogits=G["d2"].clone(),
                W={k: v.detach().clone() for k, v in W.items()}, dW={k: v.grad.detach().clone() for k, v in W.items()})


def test_op_list_uses_every_kind(snap):
    assert {o["kind"] for o in OPS} == {"conv", "norm", "add", "dropout", "upsample", "maxpool", "avgpool", "gap", "dense"}
    assert any(o["up0"] and len(o["ins"]) == 2 for o in OPS) and any(o["k"] == 1 for o in OPS)
    assert any(o["strides"] == (2, 2, 2) for o in OPS) and any(o["strides"] == (2, 2, 1) for o in OPS) and snap["T"]["a1"].shape[2] % 2 == 1
    assert any(o["kind"] == "norm" and o["instance"] and o["act"] == "leaky" for o in OPS)


def test_clean_snapshot_audits_to_zero(snap):
    recs = GA.audit(snap)
    whats = {(r["op"], r["what"]) for r in recs}
    for o in OPS:                                            # every op: forward; every parameter: its gradient; every tensor: its gradient
        assert (o["out"], "fwd") in whats
        if o["kind"] in ("conv", "dense"):
            assert (o["out"], "dW") in whats and (o["out"], "db") in whats
        if o["kind"] == "norm":
            assert (o["out"], "dgamma") in whats and (o["out"], "dbeta") in whats
        assert (o["out"], "tgrad" if o["out"] != "d2" else "dlogits") in whats
    assert ("input", "tgrad") in whats
    assert GA.find(recs, "a1", "tgrad")["k"] == 2 and GA.find(recs, "ap", "tgrad")["k"] == 2
    assert GA.find(recs, "c2", "db")["cancel"] and GA.find(recs, "c5", "db")["cancel"] and not GA.find(recs, "a1", "db")["cancel"]
    for r in recs:
        assert r["rtol"] == 0.0
        assert max(r["err"], r["linf"], r["l2"]) < 1e-11, (r["op"], r["what"], r["err"], r["l2"])


# fault -> (op it is injected at, the records that must leave their bar; everything else must stay where it was)
CORRUPTIONS = {
    "drop_tap13": ("c2", [("c2", "fwd")]),                   # tap 13 of a 3x3x3 output dropped
    "tap12": ("c6", [("c6", "fwd")]),                        # a 1x1x1 kernel placed at tap 12
    "swap_concat": ("c5", [("c5", "fwd")]),                  # the two halves of a concat swapped
    "zero_cin": ("c5", [("c5", "fwd")]),                     # one input channel of the widest conv zeroed
    "phase": ("c2", [("c2", "fwd")]),                        # stride-2 sampling phase off by one voxel on one axis
    "missing_consumer": ("a1", [("a1", "tgrad")]),           # one of two consumers missing from a tensor gradient
    "second_max": ("mp", [("dr", "tgrad")]),                 # first-max tie of the max-pool routed to the second maximum: its source's gradient
    "batch_stats": ("l2", [("l2", "fwd")]),                  # instance statistics taken over the batch
}


def test_the_widest_conv_is_the_one_corrupted():
    cin = {o["out"]: sum(CH.get(i, 8) for i in o["ins"]) for o in OPS if o["kind"] == "conv"}
    assert max(cin, key=cin.get) == "c5"


@pytest.mark.parametrize("fault", sorted(CORRUPTIONS))
def test_corruption_is_flagged_at_its_op_and_nowhere_else(snap, fault):
    assert set(CORRUPTIONS) == set(GA.FAULTS)
    at, expect = CORRUPTIONS[fault]
    clean, bad = GA.audit(snap), GA.audit(snap, fault=(at, fault))
    for c, b in zip(clean, bad):
        key = (b["op"], b["what"])
        assert (c["op"], c["what"]) == key
        if key in expect:
            assert b["err"] > 100 * GA.LARGEST_SINGLE_KERNEL_BAR and min(b["err"], b["l2"]) >= GA.MIN_FAULT_L2, (fault, b)
        else:
            assert (b["err"], b["linf"], b["l2"]) == (c["err"], c["linf"], c["l2"]), (fault, b, c)
    assert GA.faulted_records(clean, bad) == expect
