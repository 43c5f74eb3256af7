"""Op-by-op audit of a LayerGraphEngine step against plain float64 torch on the CPU (helper module, like gpu_util.py).

After forward / loss / backward the engine still holds every activation (eng.T) and every tensor gradient (eng.Gt).  `snapshot` copies them
out; `audit` then recomputes, for every op, its output, its parameter gradients and its share of its sources' gradients FROM THE OP'S OWN
STORED INPUTS, so that the error of a record is that of one op (one rounding of the storage type plus fp32 accumulation), not the bf16 noise
of the network, and a structural mistake - a tap, a channel, a parity slot, a sampling phase, a lost consumer - stands orders of magnitude
above it.  Only `snapshot` touches the engine; nothing here calls one of the project's kernels or reads a packed weight image
(Wf / Wd / Wup / Ws2: the packing is part of what is under test).

Layout of a snapshot: tensors are float64, channels first, (N, C, *spatial) with the logical channels only (2-D graphs: N = the slices);
GlobalAveragePooling / Dense outputs are (N, C).  Parameters and parameter gradients are in Keras layout (`flat_to_keras`).

`audit(snap, fault=(op_out, kind))` injects one known mistake into the REFERENCE of one op (FAULTS below): the auditor's own test, and the GPU
cases, use it to show that the record of that op - and no other - leaves its bar by orders of magnitude.
"""
import numpy as np
import torch
import torch.nn.functional as F

LEAKY_ALPHA = 0.3        # keras.layers.LeakyReLU default (oracle/isensee_oracle.py)
IN_EPS = 1e-3            # keras-contrib InstanceNormalization: (x - mean) / (std + eps)
BN_EPS = 1e-3            # Keras BatchNormalization: (x - mean) / sqrt(var + eps)
ACTS = {0: "none", 1: "relu", 2: "leaky"}
ULP = 2.0 ** -8          # one bf16 ulp relative to the value = twice the round-to-nearest bound
# No measured atol bar of a bf16 tensor written by ONE kernel in one rounding (tests/test_gpu_graph_audit.py: SINGLE_KERNEL, asserted there) is
# above this.  A known mistake must be flagged at > 100x this, in the GPU cases and in the auditor's own CPU test - and, in l2, at >= 9x the
# cap on any stored tensor (MIN_FAULT_L2 = 9 x 1e-2: one tap of 27 is ~0.19, one channel of 128 ~0.09).
LARGEST_SINGLE_KERNEL_BAR = 1e-6
MIN_FAULT_L2 = 9e-2
FAULTS = ("drop_tap13", "tap12", "swap_concat", "zero_cin", "phase", "missing_consumer", "second_max", "batch_stats")


# ------------------------------------------------------------------------------------------------ snapshot (the only part that touches the engine)
def _cf(t, planar):
    """engine tensor (channels last; 2-D: [1][slices][H][W][C]) -> float64 CPU, channels first"""
    t = t.detach().to("cpu").to(torch.float64)
    if t.dim() == 2:
        return t.clone()
    if planar:
        t = t.reshape(tuple(t.shape[1:]))
    return t.movedim(-1, 1).contiguous()


def _padmax(t, c):
    return float(t[..., c:].abs().max()) if t.shape[-1] > c else 0.0


def snapshot(eng, x, with_grads=True):
    """x: the tensor handed to eng.forward.  Call after forward / loss / backward / synchronize."""
    planar = eng.planar
    snap = dict(nd=eng.nd, dtype=eng.dtype, input_name=eng.input_name, logits_src=eng.logits_src, n_labels=eng.plan.n_labels, head=eng.head,
                pad=bool(eng.pad), ops=[], T={}, G={}, pad_max={}, gpad_max={}, drop={}, stats={}, grad_pad={})
    for o in eng.ops:
        s = o.get("sub") or ((o["s"],) * eng.nd if "s" in o else None)
        snap["ops"].append(dict(kind=o["kind"], name=o.get("name", o["out"]), ins=list(o["ins"]), out=o["out"], k=o.get("k"),
                                strides=None if s is None else tuple(int(v) for v in s), sub=o.get("sub"), up0=bool(o.get("up0", False)),
                                act=ACTS[o.get("act", 0)], pool=o.get("pool"), instance=o.get("instance"), rate=o.get("rate"), units=o.get("units")))
    clog = eng.clog
    snap["T"][eng.input_name] = _cf(x[..., :clog[eng.input_name]], planar)
    snap["pad_max"][eng.input_name] = _padmax(x, clog[eng.input_name])
    for name, t in eng.T.items():
        snap["T"][name] = _cf(t[..., :clog[name]], planar)
        snap["pad_max"][name] = _padmax(t, clog[name])
    if with_grads:
        for name in eng._has_grad:
            g = eng.Gt[name]
            snap["G"][name] = _cf(g[..., :clog[name]], planar)
            snap["gpad_max"][name] = _padmax(g, clog[name])
    for name, sc in eng.drop.items():
        snap["drop"][name] = None if sc is None else sc.detach().cpu().double()[:, :clog[name]].clone()
    for name, st in eng.stats.items():
        snap["stats"][name] = st.detach().cpu().double()[:, :clog[name]].clone()
    for key in ("logits", "probs", "dlogits"):
        snap[key] = getattr(eng, key).detach().cpu().double().clone()
    to64 = lambda W: {k: torch.from_numpy(np.ascontiguousarray(v)).double() for k, v in W.items()}
    snap["W"] = to64(eng.flat_to_keras(eng.P.detach().cpu().numpy()))
    if with_grads:
        Gh = eng.G.detach().cpu().numpy()
        snap["dW"] = to64(eng.flat_to_keras(Gh))
        # gradient entries outside the logical parameters: alignment holes of the flat buffer, the kd != centre planes of a 2-D filter's
        # image, and - channel-padded engines - the padding rows / columns of the taps that map_g gathers from
        cover = np.zeros(eng.n_flat, bool)
        off_plane = 0.0
        for name, L in eng.layout.items():
            for key in ("w", "b", "gamma", "beta"):
                if key in L:
                    cover[L[key][0]:L[key][0] + L[key][1]] = True
            if L["kind"] == "conv" and planar and L["k"] == 3:
                w = Gh[L["w"][0]:L["w"][0] + L["w"][1]].reshape(3, -1)
                off_plane = max(off_plane, float(np.abs(w[[0, 2]]).max()))
        snap["grad_pad"]["flat_holes"] = float(np.abs(Gh[~cover]).max()) if (~cover).any() else 0.0
        snap["grad_pad"]["planar_off_centre_planes"] = off_plane
        if eng.pad:
            for name in eng.convs:
                L = eng.layout[name]
                taps = list(range(27)) if L["k"] == 3 else [13]
                if planar and L["k"] == 3:
                    taps = list(range(9, 18))
                w = eng.dWp[name][taps].clone()
                w[:, :L["cout"]].index_fill_(2, eng.cin_map[name], 0.0)
                snap["grad_pad"][name + "/kernel"] = float(w.abs().max())
                snap["grad_pad"][name + "/bias"] = _padmax(eng.dbp[name], L["cout"])
            for name in eng.norms:
                c = eng.layout[name]["c"]
                snap["grad_pad"][name + "/gamma"] = _padmax(eng.dgp[name], c)
                snap["grad_pad"][name + "/beta"] = _padmax(eng.dbetap[name], c)
    return snap


# ------------------------------------------------------------------------------------------------ the ops, restated
def _same_pads(sp, k, strides):
    """TensorFlow 'same': F.pad list (last axis first)"""
    pads = []
    for n, s in reversed(list(zip(sp, strides))):
        out = -(-n // s)
        tot = max((out - 1) * s + k - n, 0)
        pads += [tot // 2, tot - tot // 2]
    return pads


def _up(x, factors):
    for a, f in enumerate(factors):
        if f != 1:
            x = torch.repeat_interleave(x, f, dim=2 + a)
    return x


def _convnd(x, kernel, bias, strides):
    """x (N, C, *sp); kernel in Keras layout (k,) * nd + (Cin, Cout)"""
    nd = x.dim() - 2
    w = kernel.permute(nd + 1, nd, *range(nd))
    x = F.pad(x, _same_pads(x.shape[2:], kernel.shape[0], strides))
    return (F.conv2d if nd == 2 else F.conv3d)(x, w, bias, stride=tuple(strides))


def conv_ref(xs, op, kernel, bias, fault=None):
    nd = xs[0].dim() - 2
    a = _up(xs[0], (2,) * nd) if op["up0"] else xs[0]
    parts = [a] + list(xs[1:])
    if fault == "swap_concat":
        assert len(parts) == 2
        parts = parts[::-1]
    x = torch.cat(parts, 1) if len(parts) > 1 else a
    if fault == "zero_cin":
        keep = torch.ones(x.shape[1], dtype=x.dtype)
        keep[x.shape[1] // 2] = 0
        x = x * keep.view((1, -1) + (1,) * nd)
    if fault == "phase":
        ax = [i for i, s in enumerate(op["strides"]) if s == 2][0]
        x = torch.roll(x, 1, dims=2 + ax)
    if fault == "drop_tap13":
        assert op["k"] == 3
        kernel = kernel.clone()
        kernel[(1,) * nd] = 0
    if fault == "tap12":
        assert op["k"] == 1 and nd == 3                       # the 1x1x1 filter one tap early in the 27-tap image: (kd, kh, kw) = (1, 1, 0)
        k3 = kernel.new_zeros((3, 3, 3) + tuple(kernel.shape[-2:]))
        k3[1, 1, 0] = kernel[0, 0, 0]
        kernel = k3
    return _convnd(x, kernel, bias, op["strides"])


def norm_ref(x, gamma, beta, instance, fault=None):
    sp = tuple(range(2, x.dim()))
    ax = sp if (instance and fault != "batch_stats") else (0,) + sp
    mean = x.mean(dim=ax, keepdim=True)
    var = x.var(dim=ax, unbiased=False, keepdim=True)
    s = (var.sqrt() + IN_EPS) if instance else (var + BN_EPS).sqrt()
    shp = (1, -1) + (1,) * (x.dim() - 2)
    return (x - mean) / s * gamma.view(shp) + beta.view(shp)


def _windows(x, pool):
    """(N, C, *sp) -> (N, C, *sp // pool, prod(pool)), the window's voxels in scan order (first axis slowest); trailing voxels cropped"""
    nd = x.dim() - 2
    out = [n // p for n, p in zip(x.shape[2:], pool)]
    x = x[(slice(None), slice(None)) + tuple(slice(0, o * p) for o, p in zip(out, pool))]
    shp = list(x.shape[:2])
    for o, p in zip(out, pool):
        shp += [o, p]
    x = x.reshape(shp)
    perm = [0, 1] + [2 + 2 * a for a in range(nd)] + [3 + 2 * a for a in range(nd)]
    return x.permute(perm).reshape(tuple(x.shape[:2]) + tuple(out) + (-1,))


def maxpool_ref(x, pool, fault=None):
    """differentiable in x with the gradient routed to the FIRST maximum of a window in scan order (`second_max`: to the second of a tie)"""
    w = _windows(x, pool)
    eq = w.detach() == w.detach().max(dim=-1, keepdim=True).values
    rank = eq.cumsum(-1)
    pick = eq & (rank == 1)
    if fault == "second_max":
        tied = eq.sum(-1, keepdim=True) >= 2
        pick = torch.where(tied, eq & (rank == 2), pick)
    return (w * pick.to(w.dtype)).sum(-1)


def avgpool_ref(x):
    return _windows(x, (2,) * (x.dim() - 2)).mean(-1)


def act_ref(z, act):
    return F.relu(z) if act == "relu" else (F.leaky_relu(z, LEAKY_ALPHA) if act == "leaky" else z)


def _act_slope(y_stored, act):
    """d act / dz from the STORED output: the branch the forward pass took (the kernels recompute or re-read exactly that sign)"""
    if act == "relu":
        return (y_stored > 0).to(torch.float64)
    if act == "leaky":
        y = y_stored.to(torch.float64)
        return torch.where(y > 0, torch.ones_like(y), torch.full_like(y, LEAKY_ALPHA))
    return None


def _pool_of(op, nd):
    return tuple(op["pool"]) if op["pool"] is not None else (2,) * nd


# ------------------------------------------------------------------------------------------------ audit
def _record(recs, op, what, got, ref, rtol=0.0, k=1, tensor=None, scale_by=None):
    got, ref = got.double(), ref.double()
    assert got.shape == ref.shape, (op["out"], what, tuple(got.shape), tuple(ref.shape))
    err = (got - ref).abs()
    if scale_by is None:
        scale = float(ref.abs().max())
        l2den = float(ref.norm())
    else:                                                     # a sum that cancels: judged on the scale of its terms
        scale = float(scale_by.abs().max())
        l2den = float(scale_by.norm())
    tiny = 1e-300
    finite = bool(torch.isfinite(got).all())
    linf = float(err.max()) / (scale + tiny) if finite else float("inf")
    atol = float((err - rtol * ref.abs()).clamp_min(0).max()) / (scale + tiny) if finite else float("inf")
    l2 = float(err.norm()) / (l2den + tiny) if finite else float("inf")
    if scale == 0.0 and float(err.max()) == 0.0:
        linf = atol = l2 = 0.0
    recs.append(dict(op=op["out"], name=op.get("name", op["out"]), kind=op["kind"], what=what, tensor=tensor, err=atol, linf=linf, l2=l2,
                     scale=scale, rtol=rtol, k=k, n=got.numel(), cancel=scale_by is not None))


def audit(snap, fault=None, only=None):
    """-> list of records {op, kind, what, err, linf, l2, scale, rtol, k, ...}.
    err = the atol_rel that gpu_util.assert_close(got, ref, rtol, atol_rel) would need (|got - ref| <= rtol |ref| + err max|ref| everywhere),
    linf = the same with rtol = 0, l2 = |got - ref|_2 / |ref|_2.  rtol is derived, not measured: k * 2^-8 for a tensor stored in bf16 that
    k kernels wrote / accumulated into (one rounding each), 0 for fp32 tensors and for every parameter gradient.
    only: a set of op outputs - only these ops are recomputed (and only the gradients of tensors ALL of whose consumers are among them).
    what: 'fwd' | 'dW' | 'db' | 'dgamma' | 'dbeta' | 'stats' | 'tgrad' (gradient of tensor `tensor`: the sum over all its consumers) | 'dlogits'.
    Runs on at most 16 CPU threads (the setting is restored afterwards)."""
    n = torch.get_num_threads()
    torch.set_num_threads(min(16, n))
    try:
        return _audit(snap, fault, only)
    finally:
        torch.set_num_threads(n)


def _audit(snap, fault=None, only=None):
    T, G, W, dWs = snap["T"], snap["G"], snap["W"], snap.get("dW", {})
    nd, dtype = snap["nd"], snap["dtype"]
    lowp = dtype == torch.bfloat16
    ulp = ULP if lowp else 0.0
    rq = (lambda w: w.to(dtype).double()) if dtype != torch.float64 else (lambda w: w)       # the conv filters are cast to the compute type
    stored_rtol = lambda t: ulp if (lowp and t.dim() > 2) else 0.0                           # (N, C) tensors are fp32
    f_op, f_kind = fault if fault is not None else (None, None)
    assert f_kind is None or f_kind in FAULTS
    recs, contrib = [], {}
    producer = {o["out"]: o for o in snap["ops"]}
    feeds_norm = {}
    for o in snap["ops"]:
        for i in o["ins"]:
            feeds_norm.setdefault(i, []).append(o["kind"] == "norm")
    for op in snap["ops"]:
        kind, out, name = op["kind"], op["out"], op["name"]
        if only is not None and out not in only:
            continue
        flt = f_kind if (f_op == out and f_kind not in ("missing_consumer", "second_max")) else None
        flt_b = f_kind if (f_op == out and f_kind == "second_max") else None
        xs = [T[i].clone().requires_grad_(True) for i in op["ins"]]
        params = {}
        if kind == "conv":
            params = dict(kernel=rq(W[name + "/kernel"]).requires_grad_(True), bias=W[name + "/bias"].clone().requires_grad_(True))
            f = lambda fl: conv_ref(xs, op, params["kernel"], params["bias"], fl)
        elif kind == "norm":
            params = dict(gamma=W[name + "/gamma"].clone().requires_grad_(True), beta=W[name + "/beta"].clone().requires_grad_(True))
            f = lambda fl: norm_ref(xs[0], params["gamma"], params["beta"], op["instance"], fl)
        elif kind == "add":
            f = lambda fl: xs[0] + xs[1]
        elif kind == "dropout":
            sc = snap["drop"].get(out)
            f = lambda fl: xs[0] * 1.0 if sc is None else xs[0] * sc.view(tuple(sc.shape) + (1,) * nd)
        elif kind == "upsample":
            f = lambda fl: _up(xs[0], _pool_of(op, nd))
        elif kind == "maxpool":
            f = lambda fl: maxpool_ref(xs[0], _pool_of(op, nd), fl)
        elif kind == "avgpool":
            f = lambda fl: avgpool_ref(xs[0])
        elif kind == "gap":
            f = lambda fl: xs[0].mean(dim=tuple(range(2, xs[0].dim())))
        elif kind == "dense":
            params = dict(kernel=W[name + "/kernel"].clone().requires_grad_(True), bias=W[name + "/bias"].clone().requires_grad_(True))
            f = lambda fl: xs[0] @ params["kernel"] + params["bias"]
        else:
            raise NotImplementedError(kind)
        z = f(flt_b)
        zf = f(flt) if flt is not None else z
        _record(recs, op, "fwd", T[out], act_ref(zf.detach(), op["act"]), rtol=stored_rtol(T[out]))
        if kind == "norm" and name in snap["stats"]:
            x = T[op["ins"][0]]
            ax = tuple(range(2, x.dim())) if op["instance"] else (0,) + tuple(range(2, x.dim()))
            mean, var = x.mean(dim=ax), x.var(dim=ax, unbiased=False)
            s = (var.sqrt() + IN_EPS) if op["instance"] else (var + BN_EPS).sqrt()
            st = snap["stats"][name]
            _record(recs, op, "stats", st[..., :2], torch.stack([mean, 1.0 / s], -1).reshape(st.shape[0], -1, 2))
        if out not in G:
            continue
        gz = G[out]
        if kind in ("norm", "dense") and op["act"] != "none":
            gz = gz * _act_slope(T[out], op["act"])            # (a conv with a fused ReLU: Gt[out] holds dz after backward)
        leaves = xs + list(params.values())
        grads = torch.autograd.grad(z, leaves, gz, allow_unused=True)
        for i, g in zip(op["ins"], grads[:len(xs)]):
            contrib.setdefault(i, []).append((out, torch.zeros_like(T[i]) if g is None else g))
        for (key, p), g in zip(params.items(), grads[len(xs):]):
            if name + "/" + key not in dWs:
                continue
            what = dict(kernel="dW", bias="db", gamma="dgamma", beta="dbeta")[key]
            scale_by = None
            if kind == "conv" and key == "bias" and feeds_norm.get(out) == [True]:
                # the bias of a conv that feeds a normalisation: the gradient is a sum that cancels to ~0 - judged on sum |dz| per channel
                scale_by = gz.abs().sum(dim=(0,) + tuple(range(2, gz.dim())))
            _record(recs, op, what, dWs[name + "/" + key], g, scale_by=scale_by)
    # tensor gradients: the sum over ALL consumers, each from that consumer's stored output gradient
    for tname, got in G.items():
        cs = contrib.get(tname, [])
        op = producer.get(tname, dict(out=tname, name=tname, kind="input", act="none"))
        if tname == snap["logits_src"]:
            if only is not None:
                continue
            assert not cs, "the logits' source has consumers"
            dl = snap["dlogits"]
            want = rq(dl) if got.dim() > 2 else dl
            g2 = got.movedim(1, -1).reshape(-1, got.shape[1]) if got.dim() > 2 else got
            _record(recs, op, "dlogits", g2[:, :snap["n_labels"]], want.reshape(g2.shape[0], -1), tensor=tname)
            continue
        if not cs or (only is not None and not all(o["out"] in only for o in snap["ops"] if tname in o["ins"])):
            continue
        if f_kind == "missing_consumer" and f_op == tname:
            assert len(cs) >= 2
            cs = cs[:-1]
        ref = sum(g for _, g in cs)
        if op["kind"] == "conv" and op["act"] != "none":
            ref = ref * _act_slope(T[tname], op["act"])
        _record(recs, op, "tgrad", got, ref, rtol=len(contrib[tname]) * stored_rtol(got), k=len(contrib[tname]), tensor=tname)
    return recs


# ------------------------------------------------------------------------------------------------ reading the records
def worst(recs, what=None, pred=None):
    sel = [r for r in recs if (what is None or r["what"] == what) and (pred is None or pred(r))]
    return max(sel, key=lambda r: max(r["err"], r["l2"])) if sel else None


def find(recs, op, what):
    sel = [r for r in recs if r["op"] == op and r["what"] == what]
    assert len(sel) == 1, (op, what, len(sel))
    return sel[0]


def faulted_records(clean, bad, factor=4.0, floor=1e-9):
    """the records of `bad` (an audit with a fault) whose error left that of the clean audit: [(op, what)]"""
    assert [(r["op"], r["what"]) for r in clean] == [(r["op"], r["what"]) for r in bad]
    return [(b["op"], b["what"]) for c, b in zip(clean, bad) if max(b["err"], b["l2"]) > factor * max(c["err"], c["l2"]) + floor]
