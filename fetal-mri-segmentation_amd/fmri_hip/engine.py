"""Execution engine for the reference's U-Net topology on the C ABI (explicit forward + backward, no autograd).

Mirrors the graph built by reference fetal_net/model/unet3d/unet.py:17-86 (and the 2-D twin model/unet/unet.py:22-88,
run as D == 1 volumes): per level two Conv(3x3x3,'same')+ReLU blocks, MaxPooling(2), then per decoder level
UpSampling(2) -> concatenate([up, skip]) -> two conv blocks, final 1x1x1 conv + sigmoid; loss = -Dice
(metrics.py:11-32); optimizer = Keras Adam (unet.py:85).

MI355X layout decisions
  * activations channels-last [N][D][H][W][C] in the compute dtype (bf16 for speed, fp32 for parity);
  * all parameters live in ONE flat fp32 buffer ordered in BACKWARD-completion order (final layer first, first
    encoder conv last) so that gradient buckets for the RCCL all-reduce are contiguous prefixes, Adam is one launch
    and gradient zeroing is one memset;
  * the up-sampled tensor and the concat are never materialised (the conv kernels read two sources);
  * every tensor is allocated once at build time (288 GB HBM: no re-computation, no allocator traffic in the step).
"""
from collections import OrderedDict

import numpy as np
import torch

from . import ops
from ._lib import ACT_NONE, ACT_RELU, IMPL_AUTO
from .engine_base import EngineBase, flat_to_kernel, glorot_uniform, kernel_to_flat
from .up_routes import D2s, Fold, Onetap, Upcat, candidates


class UNetPlan:
    """Topology in Keras creation order (names match Keras auto-naming)."""

    def __init__(self, in_channels, spatial, depth=4, n_base_filters=32, n_labels=1, ndim=3, norm=None, deconvolution=False):
        """norm: None | 'batch' | 'instance' (reference create_convolution_block options); deconvolution: Conv*DTranspose(k=2,s=2)
        instead of nearest up-sampling (reference get_up_convolution)."""
        self.in_channels, self.spatial = in_channels, tuple(spatial)
        self.depth, self.n_base_filters, self.n_labels, self.ndim = depth, n_base_filters, n_labels, ndim
        self.norm, self.deconvolution = norm, deconvolution
        d = "3d" if ndim == 3 else "2d"
        k = 0
        nk = 0
        tk = 0

        def conv_name():
            nonlocal k
            k += 1
            return "conv%s_%d" % (d, k)

        def norm_name():
            nonlocal nk
            nk += 1
            return "%s_%d" % ("batch_normalization" if norm == "batch" else "instance_normalization", nk)

        self.enc = []
        cin = in_channels
        for ld in range(depth):
            lv = []
            for mult in (1, 2):
                cout = n_base_filters * (2 ** ld) * mult
                lv.append(dict(name=conv_name(), cin=cin, cout=cout, level=ld, norm=norm_name() if norm else None))
                cin = cout
            self.enc.append(lv)
        self.dec = []
        self.up = {}          # decoder level -> transposed-conv descriptor (only with deconvolution=True)
        for ld in range(depth - 2, -1, -1):
            skip_c = self.enc[ld][1]["cout"]
            if deconvolution:
                tk += 1
                self.up[ld] = dict(name="conv%s_transpose_%d" % (d, tk), cin=cin, cout=cin, level=ld)
            a = dict(name=conv_name(), cin=cin + skip_c, cout=skip_c, level=ld, c_up=cin, c_skip=skip_c,
                     norm=norm_name() if norm else None)
            b = dict(name=conv_name(), cin=skip_c, cout=skip_c, level=ld, norm=norm_name() if norm else None)
            self.dec.append([a, b])
            cin = skip_c
        self.final = dict(name=conv_name(), cin=cin, cout=n_labels)
        for s in self.spatial:
            if s % (2 ** (depth - 1)):
                raise ValueError("spatial dims %s must be divisible by 2^(depth-1)" % (self.spatial,))

    def convs_forward_order(self):
        out = []
        for lv in self.enc:
            out += lv
        for lv in self.dec:
            out += lv
        return out

    def level_dims(self, level, slices=1):
        """(D,H,W) of the activations at `level`.  2-D plans are planar: D = number of slices in the batch, never pooled."""
        if self.ndim == 3:
            return tuple(s >> level for s in self.spatial)
        return (slices,) + tuple(s >> level for s in self.spatial)


class UNetEngine(EngineBase):
    def __init__(self, plan, batch, dtype=torch.bfloat16, device="cuda", seed=42, training=True, dist_ctx=None, input_grad=False, frozen=False):
        """input_grad: backward() also delivers dL/d(input) (input_gradient()) - the gradient a network in front of this one is trained
        with while this one stays frozen (backward(params=False); reference fetal_net/model/norm/NormNet.py).  frozen: EngineBase."""
        # every switch of this engine, read here and nowhere else; what each one does stands where self.sw[...] is used
        super().__init__(dtype, device, training, dist_ctx, frozen=frozen, DECONV_FOLD=True, FWD_WS=True, UPCAT=True, TAIL_FUSE=True,
                         TAIL_FUSE_2D=True, NORM_FUSE=1, NORM_FUSE_MAXLEVEL=1 if plan.norm == "batch" else 0, FIRST_DGRAD=True)
        self.plan, self.N = plan, batch
        self.input_grad = bool(input_grad and training)
        self.planar = plan.ndim == 2      # 2-D: tensors are [1][slices][H][W][C], every op is planar (no coupling along D)
        if self.deterministic:
            # FMRI_DETERMINISTIC=1 (EngineBase) keeps to routes whose sums are ordered: the decoder routes that say so of themselves
            # (up_routes: `ordered`), and not the statistics a conv launch forms in its epilogue (the four producer waves of a workgroup
            # meet in its slot with fp64 atomics) but the separate reductions, which add their workgroups' partials in block order - the
            # FMRI_NORM_FUSE=0 path
            self.sw["NORM_FUSE"] = 0
        self._bufsets = {}
        self._build_params(seed)
        self.set_batch(batch)

    # ------------------------------------------------------------------------------------------------ parameters
    def _build_params(self, seed):
        p = self.plan
        # backward-completion order: final, dec (shallowest level first: b, a, transposed conv), enc (deepest first, b before a)
        order = [("final", p.final)]
        for lv in reversed(p.dec):
            order += [("conv", lv[1]), ("conv", lv[0])]
            if lv[0]["level"] in p.up:
                order.append(("deconv", p.up[lv[0]["level"]]))
        for lv in reversed(p.enc):
            order += [("conv", lv[1]), ("conv", lv[0])]
        self.layout = OrderedDict()
        off = 0
        ntap = {"conv": 27, "final": 1, "deconv": 8}
        for kind, c in order:
            nw = ntap[kind] * c["cout"] * c["cin"]
            off = (off + 3) & ~3
            L = dict(kind=kind, w=(off, nw), b=(((off + nw + 3) & ~3), c["cout"]), cin=c["cin"], cout=c["cout"], norm=c.get("norm"))
            off = ((off + nw + 3) & ~3) + c["cout"]
            if c.get("norm"):          # gamma, beta of the block's normalisation layer right behind the bias
                off = (off + 3) & ~3
                L["gamma"] = (off, c["cout"])
                L["beta"] = (off + ((c["cout"] + 3) & ~3), c["cout"])
                off = L["beta"][0] + c["cout"]
            self.layout[c["name"]] = L
        self.n_flat = (off + 3) & ~3
        dev = self.dev
        self._alloc_params()
        if self.deterministic:
            cf = p.final["cin"]
            if cf % 8 or (cf // 8) & (cf // 8 - 1) or cf // 8 > 64 or p.n_labels > 4:
                raise NotImplementedError("FMRI_DETERMINISTIC=1: the final 1x1x1 convolution over %d channels / %d labels takes the generic "
                                          "fmri_conv1x1_bwd kernel, whose waves meet in LDS with floating-point atomics (reproducible: "
                                          "8 x 2^k <= 512 channels, at most 4 labels)" % (cf, p.n_labels))
        if self.training:
            self._det_register(self.G)
        # the candidate routes of every decoder level (up_routes.candidates), keyed by block a's name, deepest level first
        self.fold = None                  # the index tables of deconv_fold, shared by the folded levels
        self.up_routes = OrderedDict((lv[0]["name"], candidates(self, lv[0], p.up.get(lv[0]["level"]))) for lv in p.dec)
        # compute-dtype copies of the 3x3x3 filters (and no pack table yet: it holds their addresses)
        self.Wf, self.Wd, self._ptab = {}, {}, None
        self.moving = {}                  # batch-norm moving mean / variance (inference statistics), fp32 [2][C]
        first = p.enc[0][0]["name"]
        for name, L in self.layout.items():
            if L.get("norm") and p.norm == "batch":
                mv = torch.zeros((2, L["cout"]), dtype=torch.float32, device=dev)
                mv[1].fill_(1.0)
                self.moving[name] = mv
            if L["kind"] != "conv" or (name in self.up_routes and not self.up_routes[name][0].plain_a):
                continue
            self.Wf[name] = torch.empty((27, L["cout"], L["cin"]), dtype=self.dtype, device=dev)
            # (the first conv's input-gradient image: only with input_grad, and only where fmri_conv3d_first_dgrad - which reads the forward
            # image - does not take the shape)
            if self.training and (name != first or (self.input_grad and not self._first_dgrad_ok())):
                self.Wd[name] = torch.empty((27, L["cin"], L["cout"]), dtype=self.dtype, device=dev)
        need = [r.scratch() for cands in self.up_routes.values() for r in cands]
        self.dwc_scratch = torch.empty(max(need), dtype=torch.float32, device=dev) if self.training and any(need) else None
        self.init_glorot(seed)

    def w_view(self, name, buf=None):
        L = self.layout[name]
        buf = self.P if buf is None else buf
        o, n = L["w"]
        shape = {"conv": (27, L["cout"], L["cin"]), "deconv": (8, L["cout"], L["cin"]), "final": (L["cout"], L["cin"])}[L["kind"]]
        return buf[o:o + n].view(shape)

    def gb_view(self, name, which, buf=None):
        """gamma / beta of the normalisation layer of conv block `name`"""
        buf = self.P if buf is None else buf
        o, n = self.layout[name][which]
        return buf[o:o + n]

    def b_view(self, name, buf=None):
        L = self.layout[name]
        buf = self.P if buf is None else buf
        o, n = L["b"]
        return buf[o:o + n]

    def init_glorot(self, seed):
        """Keras defaults (glorot_uniform kernels, zero bias), drawn in Keras layer-creation order."""
        rs = np.random.RandomState(seed)
        W = OrderedDict()
        k3, k1 = ((3, 3, 3), (1, 1, 1)) if self.plan.ndim == 3 else ((3, 3), (1, 1))
        k2 = (2, 2, 2) if self.plan.ndim == 3 else (2, 2)
        p = self.plan
        seq = [c for lv in p.enc for c in lv]
        for lv in p.dec:                                  # Keras creation order: the transposed conv precedes its level's blocks
            if lv[0]["level"] in p.up:
                seq.append(dict(p.up[lv[0]["level"]], transpose=True))
            seq += lv
        for c in seq:
            if c.get("transpose"):
                W[c["name"] + "/kernel"] = glorot_uniform(rs, k2 + (c["cout"], c["cin"]))      # Keras: (k,k,k,Cout,Cin)
                W[c["name"] + "/bias"] = np.zeros(c["cout"], np.float32)
                continue
            W[c["name"] + "/kernel"] = glorot_uniform(rs, k3 + (c["cin"], c["cout"]))
            W[c["name"] + "/bias"] = np.zeros(c["cout"], np.float32)
            if c.get("norm"):
                W[c["norm"] + "/gamma"] = np.ones(c["cout"], np.float32)
                W[c["norm"] + "/beta"] = np.zeros(c["cout"], np.float32)
        f = self.plan.final
        W[f["name"] + "/kernel"] = glorot_uniform(rs, k1 + (f["cin"], f["cout"]))
        W[f["name"] + "/bias"] = np.zeros(f["cout"], np.float32)
        self.load_keras_weights(W)

    def keras_to_flat(self, W):
        """W: {'<layer>/kernel': (kD,kH,kW,Cin,Cout) ndarray, '<layer>/bias': (Cout,), '<norm>/gamma' ...} in Keras layout -> the flat
        fp32 parameter vector of this engine (also the layout of the Adam moments)."""
        host = np.zeros(self.n_flat, np.float32)
        for name, L in self.layout.items():
            k = np.asarray(W[name + "/kernel"], np.float32)
            o, n = L["w"]
            cio = (L["cin"], L["cout"])
            if L["kind"] == "deconv":
                if k.ndim == 4:                                               # (2,2,Cout,Cin) -> taps 0..3 of the 8
                    k = np.concatenate([k.reshape(4, L["cout"], L["cin"]), np.zeros((4, L["cout"], L["cin"]), np.float32)])
                host[o:o + n] = k.reshape(8, L["cout"], L["cin"]).reshape(-1)
            elif L["kind"] == "conv":                                         # 2-D kernels (kH,kW,Cin,Cout) fill the centre kd plane
                assert k.shape in ((3, 3, 3) + cio, (3, 3) + cio), (name, k.shape)
                host[o:o + n] = kernel_to_flat(k, 3)                          # -> [27][Cout][Cin]
            else:
                assert k.shape[-2:] == cio, (name, k.shape)
                host[o:o + n] = kernel_to_flat(k, 1)                          # -> [L][C]
            ob, nb = L["b"]
            host[ob:ob + nb] = np.asarray(W[name + "/bias"], np.float32)
            if L.get("norm"):
                host[L["gamma"][0]:L["gamma"][0] + nb] = np.asarray(W[L["norm"] + "/gamma"], np.float32)
                host[L["beta"][0]:L["beta"][0] + nb] = np.asarray(W[L["norm"] + "/beta"], np.float32)
        return host

    def load_keras_weights(self, W):
        """the Keras weights into P (EngineBase.load_keras_weights), then the batch-norm moving statistics where W has them"""
        super().load_keras_weights(W)
        for name, L in self.layout.items():
            if L.get("norm") and name in self.moving and (L["norm"] + "/moving_mean") in W:
                self.moving[name][0].copy_(torch.from_numpy(np.asarray(W[L["norm"] + "/moving_mean"], np.float32)))
                self.moving[name][1].copy_(torch.from_numpy(np.asarray(W[L["norm"] + "/moving_variance"], np.float32)))

    def flat_to_keras(self, host, moving=True):
        """inverse of keras_to_flat for any vector in the parameter layout (weights, Adam m, Adam v)"""
        W = OrderedDict()
        order = [c["name"] for c in self.plan.convs_forward_order()] + [u["name"] for u in self.plan.up.values()] + [self.plan.final["name"]]
        for name in order:
            L = self.layout[name]
            o, n = L["w"]
            if L["kind"] == "deconv":
                k = host[o:o + n].reshape(8, L["cout"], L["cin"])
                W[name + "/kernel"] = (k.reshape(2, 2, 2, L["cout"], L["cin"]) if self.plan.ndim == 3
                                       else k[:4].reshape(2, 2, L["cout"], L["cin"])).copy()
            else:
                W[name + "/kernel"] = flat_to_kernel(host[o:o + n], 3 if L["kind"] == "conv" else 1, L["cin"], L["cout"], self.plan.ndim)
            ob, nb = L["b"]
            W[name + "/bias"] = host[ob:ob + nb].copy()
            if L.get("norm"):
                W[L["norm"] + "/gamma"] = host[L["gamma"][0]:L["gamma"][0] + nb].copy()
                W[L["norm"] + "/beta"] = host[L["beta"][0]:L["beta"][0] + nb].copy()
                if moving and name in self.moving:
                    mv = self.moving[name].cpu().numpy()
                    W[L["norm"] + "/moving_mean"], W[L["norm"] + "/moving_variance"] = mv[0].copy(), mv[1].copy()
        return W

    # What the decoder levels were built with, whichever batch size is current - read by the tests and by the benchmark's FLOP count.
    def _built(self, cls):
        """the candidate routes of class cls, shallowest level first"""
        return [r for cands in reversed(self.up_routes.values()) for r in cands if type(r) is cls]

    @property
    def upcat(self):
        """decoder 'a' convs that can take the parity form: name -> (up-sampled channels, skip channels)"""
        return OrderedDict((r.a["name"], (r.a["c_up"], r.a["c_skip"])) for r in self._built(Upcat))

    @property
    def upcat_wgrad(self):
        """... of which the weight gradient takes the parity form too (never in deterministic mode)"""
        return set(r.a["name"] for r in self._built(Upcat) if r.wgrad)

    # the weight images of the parity-form and folded levels by block a's name, of the one-tap and 2-D transposed convs by their own
    Wup = property(lambda self: OrderedDict((r.a["name"], r.W) for r in self._built(Upcat)))
    Wfd = property(lambda self: OrderedDict((r.a["name"], r.W) for r in self._built(Fold)))
    Wdc = property(lambda self: OrderedDict((r.u["name"], r.W) for r in self._built(Onetap)))
    Wd2 = property(lambda self: OrderedDict((r.u["name"], r.W) for r in self._built(D2s)))

    def _first_dgrad_ok(self):
        """does fmri_conv3d_first_dgrad take the first convolution's input gradient? (3-D bf16 shapes of ops.conv3d_first_dgrad_ok; it does
        not depend on the batch size).  FMRI_FIRST_DGRAD=0 keeps the generic route (A/B switch, tools/bench_norm_net.py)."""
        c = self.plan.enc[0][0]
        return (self.sw["FIRST_DGRAD"] and not self.planar and self.dtype == torch.bfloat16 and
                ops.conv3d_first_dgrad_ok(c["cin"], c["cout"], *self.plan.level_dims(0), self.dtype))

    def _use_upcat(self, name):
        """parity form for this layer at the CURRENT batch size (2-D: the slice count must be a multiple of the 4-slice tile)"""
        return type(self.up.get(name)) is Upcat

    def _pack_table(self):
        """the plain and the parity-form images as one table for ops.pack_weights_batched: (table, blocks, the tensors whose raw addresses the
        table holds, P's address when it was built) - rebuilt when P has moved since, dropped wherever the images are allocated"""
        if self._ptab is None or self._ptab[3] != self.P.data_ptr():
            ent = [("plain", self.w_view(n), self.Wf[n], self.Wd.get(n)) for n in self.Wf]
            for cands in reversed(self.up_routes.values()):
                ent += [e for r in cands for e in r.pack_entries()]
            self._ptab = (ops.pack_table(ent, self.dev) if ent else (None, 0)) + (ent, self.P.data_ptr())
        return self._ptab

    def refresh_weight_copies(self):
        """compute-dtype images of the fp32 parameters (forward filters, tap-flipped transposed filters for the input gradients, parity
        filters), on the current stream.  Every plain / parity-form image in ONE launch: per-layer launches are launch-bound - 14 of them
        cost the configs[1] step 0.12 ms wherever they run, also on a side stream under the next step's first convolutions (rounds 2-5,
        retired: profiles/r06_pack_batched_ab.log, tools/r06/pack_cost.py).  The images of a level's preferred route that are not in the
        table (folded layers, transposed convs): per layer, shallowest level first."""
        tab, nb = self._pack_table()[:2]
        if tab is not None:
            ops.pack_weights_batched(tab, nb, self.dtype)
        for cands in reversed(self.up_routes.values()):
            cands[0].refresh()

    # ------------------------------------------------------------------------------------------------ buffers
    def set_batch(self, N):
        """switch to (and lazily allocate) the activation / gradient buffer set for batch size N"""
        key = (N, self.training)
        if key not in self._bufsets:
            self.N = N
            self._build_buffers()
            self._bufsets[key] = dict(act=self.act, grad=getattr(self, "grad", None), logits=self.logits, probs=self.probs,
                                      dlogits=getattr(self, "dlogits", None), pre=self.pre, nstats=self.nstats, nss=self.nss, norm_ws=self.norm_ws,
                                      wgrad_ws=getattr(self, "wgrad_ws", None), route=self.route, up=self.up, dx_in=self.dx_in, dx_tmp=self.dx_tmp,
                                      dummy_y=torch.zeros(self.logits.numel(), dtype=torch.uint8, device=self.dev))
        b = self._bufsets[key]
        self.N, self.act, self.grad, self.logits, self.probs, self.dlogits = N, b["act"], b["grad"], b["logits"], b["probs"], b["dlogits"]
        self.pre, self.nstats, self.nss, self.norm_ws, self.wgrad_ws = b["pre"], b["nstats"], b["nss"], b["norm_ws"], b["wgrad_ws"]
        self.route, self.up, self.dx_in, self.dx_tmp = b["route"], b["up"], b["dx_in"], b["dx_tmp"]
        self._dummy_y = b["dummy_y"]       # per buffer set and never freed: captured hipGraphs keep raw pointers to it

    def _dims(self, level):
        """leading (N, D, H, W) of an activation at `level` for the current batch"""
        if self.planar:
            return (1,) + self.plan.level_dims(level, self.N)
        return (self.N,) + self.plan.level_dims(level)

    def _plan_routes(self):
        """Which kernel form every launch of a step takes at the CURRENT batch size, decided once per buffer set: the buffers are sized from
        it, and forward and backward dispatch on it and on nothing else.
          tail[block]   bits of ops.conv3d_fwd_tail_ok: what the epilogue of a plain single-source bf16 block without a normalisation layer
                        produces besides its output (1: MaxPooling, 2: the final 1x1x1 conv's logits).  FMRI_TAIL_FUSE=0 switches it off,
                        FMRI_TAIL_FUSE_2D=0 the same for the 2-D models only (A/B).
          stats[block]  the block's forward launch sums its own output for the statistics of its normalisation layer;
          dz[block]     the input-gradient launch that writes the block's gradient forms the reductions of its normalisation backward -
                        both in the asynchronous epilogue of the 3-D bf16 MFMA launch (ops.conv3d_fwd_ntail_ok).  FMRI_NORM_FUSE = bit mask
                        (1: stats, 2: dz), FMRI_NORM_FUSE_MAXLEVEL = deepest level that uses them.  Defaults from the interleaved A/B inside
                        the configs[1] step (tools/ab_norm_tails.py, profiles/r03_norm_tails_ab.log): the statistics tail down to level 1
                        (batch norm: 19.91 -> 19.55 ms) or on level 0 only (instance norm: a workgroup's sums are flushed whenever the sample
                        changes; 20.65 -> 20.47 ms); the backward tail is built and tested but off: it saves 170-340 us of reduction passes
                        per full-resolution layer and costs the input-gradient launch 100-180 us (tools/bench_ntail.py) - a launch that
                        shares the chip with the weight-gradient stream, under which the HBM-bound reduction passes were already hidden
                        (step +0.2 ... 0.5 ms with it).
          up[a]         how decoder block `a` gets its up-sampled input: "fold" (transposed conv folded into a), "d2s" (2-D transposed conv as
                        planar conv + depth-to-space; the slices must tile by 4), "onetap" (one-tap parity transposed conv), "deconv" (direct
                        k2s2 transposed conv), "upcat" (parity-form up-sample + concat; 2-D: the slices must tile by 4) or "upsample" (the
                        fused-upsample 27- / 9-tap conv);
          upcat_wgrad[a]  a's weight gradient takes the parity form too;
          first_dgrad   engines built with input_grad: "first" (fmri_conv3d_first_dgrad: fp32 straight from the forward filter image) or
                        "generic" (fmri_conv3d_dgrad in the compute dtype on a [27][Cin][Cout] image, then a cast: fp32, 2-D, other shapes)."""
        p, sw = self.plan, self.sw
        r = dict(tail={}, stats={}, dz={}, up={}, upcat_wgrad={})
        if self.input_grad:
            r["first_dgrad"] = "first" if self._first_dgrad_ok() else "generic"

        def ntail(c0, c1, cout, level, kind):
            if p.norm is None or self.planar or self.dtype != torch.bfloat16 or not (sw["NORM_FUSE"] & kind) or level > sw["NORM_FUSE_MAXLEVEL"]:
                return False
            return ops.conv3d_fwd_ntail_ok(c0, c1, cout, *self._dims(level), self.dtype)

        self.up = OrderedDict()                             # block a -> the route object behind route["up"][a]
        for name, cands in self.up_routes.items():
            self.up[name] = next(c for c in cands if c.takes(self.N))
            r["up"][name] = self.up[name].name
            r["upcat_wgrad"][name] = self.up[name].wgrad
        tails = self.dtype == torch.bfloat16 and sw["TAIL_FUSE"] and (sw["TAIL_FUSE_2D"] or not self.planar)
        for lv in p.enc + p.dec:
            a, b = lv
            for c in lv:
                r["tail"][c["name"]] = (ops.conv3d_fwd_tail_ok(c["cin"], c["cout"], *self._dims(c["level"]), self.dtype, planar=self.planar)
                                        if tails and not c.get("norm") else 0)
                c0, c1 = self.up[c["name"]].writer() if c["name"] in self.up else (c["cin"], 0)
                r["stats"][c["name"]] = ntail(c0, c1, c["cout"], c["level"], 1)
            r["dz"][a["name"]] = ntail(b["cout"], 0, a["cout"], a["level"], 2)
            r["dz"][b["name"]] = False                      # its gradient comes from a pooling / up-sampling / 1x1x1 backward, not from a conv launch
        return r

    def _build_buffers(self):
        p, N, dt, dev = self.plan, self.N, self.dtype, self.dev
        self.route = self._plan_routes()
        A = self.act = {}
        self.pre, self.nstats = {}, {}            # conv outputs before normalisation; saved statistics {mean, 1/s, 1/sigma}
        self.nss = {}                             # {scale, shift} of the apply pass, for the normalisation tail of the input-gradient launches
        G = N if (p.norm == "instance" and not self.planar) else 1
        if p.norm == "instance" and self.planar:
            G = N                                  # 2-D: every slice is a sample

        def block_bufs(c):
            A[c["name"]] = torch.empty(self._dims(c["level"]) + (c["cout"],), dtype=dt, device=dev)
            if c.get("norm"):
                self.pre[c["name"]] = torch.empty_like(A[c["name"]])
                self.nstats[c["name"]] = torch.zeros((G, c["cout"], 3), dtype=torch.float32, device=dev)
                self.nss[c["name"]] = torch.zeros((G, c["cout"], 2), dtype=torch.float32, device=dev)

        for lv in p.enc:
            for c in lv:
                block_bufs(c)
        for ld in range(p.depth - 1):
            A["pool_%d" % ld] = torch.empty(self._dims(ld + 1) + (p.enc[ld][1]["cout"],), dtype=dt, device=dev)
        for lv in p.dec:
            if self.up[lv[0]["name"]].up_output:
                u = p.up[lv[0]["level"]]
                A[u["name"]] = torch.empty(self._dims(u["level"]) + (u["cout"],), dtype=dt, device=dev)
            for c in lv:
                block_bufs(c)
        cmax = max(c["cout"] for c in p.convs_forward_order())
        # scratch of the normalisation sums: [G][C][2] doubles - and, behind them, the per-workgroup blocks of the conv launches' tails
        self.norm_ws = torch.zeros(max(max(G, 1) * cmax * 2, ops.norm_tail_ws_doubles(max(G, 1), cmax) if dev.type == "cuda" else 0),
                                   dtype=torch.float64, device=dev) if p.norm else None
        if p.norm:
            self._det_reserve_norm([(N, int(np.prod(self._dims(c["level"])[1:])) // (N if self.planar else 1), c["cout"], self._norm_mode()[0])
                                    for c in p.convs_forward_order()])
        nvox0 = int(np.prod(self._dims(0)))
        self.logits = torch.empty((nvox0, p.n_labels), dtype=torch.float32, device=dev)
        self.probs = torch.empty_like(self.logits)
        # dL/d(input) in fp32 (what the network in front takes as the gradient on its output); the generic route in bf16 goes through dx_tmp
        self.dx_in = torch.empty(self._dims(0) + (p.in_channels,), dtype=torch.float32, device=dev) if self.input_grad else None
        self.dx_tmp = torch.empty_like(self.dx_in, dtype=dt) if (self.input_grad and dt != torch.float32 and
                                                                 self.route["first_dgrad"] == "generic") else None
        if not self.training:
            self.grad, self.dlogits, self.wgrad_ws = None, None, None
            return
        Gd = self.grad = {}
        for name, t in A.items():
            Gd[name] = torch.empty_like(t)            # gradient w.r.t. the tensor (conv blocks: w.r.t. the pre-activation)
        for lv in p.dec:
            a = lv[0]
            # gradient of the concatenated conv input; the parity forms write the up-sampled part straight at low resolution,
            # so only the skip channels remain
            ccat = a["c_skip"] if self.up[a["name"]].cat_skip_only else a["cin"]
            Gd["cat_%d" % a["level"]] = torch.empty(self._dims(a["level"]) + (ccat,), dtype=dt, device=dev)
        self.dlogits = torch.empty_like(self.logits)
        # scratch for the slab flush of the MFMA weight-gradient kernel (max over the layers of this plan)
        need = 0
        for c in p.convs_forward_order():
            dims = self._dims(c["level"])
            c0, c1 = (c["c_up"], c["c_skip"]) if "c_up" in c else (c["cin"], 0)
            need = max(need, ops.conv3d_wgrad_workspace_bytes(c0, c1, c["cout"], dims[0], dims[1], dims[2], dims[3], dt, self.planar))
            if c["name"] in self.upcat_wgrad:             # parity form: the plain kernel only sees the skip channels
                need = max(need, ops.conv3d_wgrad_workspace_bytes(c1, 0, c["cout"], dims[0], dims[1], dims[2], dims[3], dt, self.planar))
        self.wgrad_ws = torch.empty(max(need // 4, 1), dtype=torch.float32, device=dev) if need else None

    # ------------------------------------------------------------------------------------------------ forward
    def _norm_mode(self):
        """(per_instance, eps_on_std) of fmri_norm_act_fwd for this plan"""
        return (1, True) if self.plan.norm == "instance" else (0, False)

    def _as_samples(self, t):
        """view [N][D][H][W][C] as [samples][voxels...][C] for the normalisation kernels (2-D: slices are the samples)"""
        return t.reshape((t.shape[1],) + tuple(t.shape[2:])) if self.planar else t

    def _tail_ok(self, c):
        """what the epilogue of conv block `c` produces besides its output (_plan_routes)"""
        return self.route["tail"][c["name"]]

    def _block_fwd(self, c, src0, src1, up0, bn_training, pool=None, final=None, conv=None):
        """one [conv -> (norm) -> ReLU] block (reference create_convolution_block, unet.py:89-115).  pool: tensor that receives
        MaxPooling3D(2) of the block's output; final: the final 1x1x1 conv descriptor whose logits the epilogue computes - both only
        when the route plan's tail bits say so (the caller checks); conv(src0, src1, out, act, summed, per_instance): the launch of a
        decoder route that runs the block's convolution in a form of its own."""
        name = c["name"]
        out, act = (self.pre[name], ACT_NONE) if c.get("norm") else (self.act[name], ACT_RELU)
        if pool is not None or final is not None:
            w1 = self.w_view(final["name"]).reshape(-1) if final is not None else None
            ops.conv3d_fwd_tail(src0, self.Wf[name], self.b_view(name), out, pool=pool, w1=w1,
                                b1=self.b_view(final["name"]) if final is not None else None,
                                logits=self.logits.reshape(-1) if final is not None else None, act=act, planar=self.planar)
            return self.act[name]
        # normalised block with training statistics: the conv sums its own output in its epilogue where the launch allows it
        per, eos = self._norm_mode()
        want_sums = bool(c.get("norm")) and not (self.plan.norm == "batch" and not bn_training)
        summed = want_sums and self.route["stats"][name]
        if conv is not None:
            conv(src0, src1, out, act, summed, per)
        elif summed:
            ops.conv3d_fwd_stats(src0, src1, self.Wf[name], self.b_view(name), out, self.norm_ws, per, up0=up0, act=act)
        else:
            ops.conv3d_fwd(src0, src1, self.Wf[name], self.b_view(name), out, up0=up0, act=act, planar=self.planar)
        if not c.get("norm"):
            return self.act[name]
        st = self.nstats[name]
        if self.plan.norm == "batch" and not bn_training:
            mv = self.moving[name]                                            # inference: moving averages (Keras learning_phase 0)
            st[0, :, 0] = mv[0]
            st[0, :, 1] = torch.rsqrt(mv[1] + 1e-3)
            st[0, :, 2] = st[0, :, 1]
            per = -1
        (ops.norm_act_fwd_pre if summed else ops.norm_act_fwd)(
            self._as_samples(self.pre[name]), self.gb_view(name, "gamma"), self.gb_view(name, "beta"),
            self._as_samples(self.act[name]), st, self.norm_ws, per, eps=1e-3, eps_on_std=eos, act=ACT_RELU)
        if self.plan.norm == "batch" and bn_training and self._update_moving:
            # Keras moving statistics (momentum 0.99); the variance fed to the moving average is sample-size corrected
            M = float(self.pre[name].numel() // c["cout"])
            mv = self.moving[name]
            if st.is_cuda:
                ops.norm_moving_update(st, mv[0], mv[1], M)
            else:
                var = (1.0 / (st[0, :, 1] * st[0, :, 1]) - 1e-3) * (M / max(M - (1.0 + 1e-3), 1.0))
                mv[0].mul_(0.99).add_(st[0, :, 0], alpha=0.01)
                mv[1].mul_(0.99).add_(var, alpha=0.01)
        return self.act[name]

    def forward(self, x, bn_training=None, update_moving=True):
        """x: [N,D,H,W,Cin] compute dtype, device.  Leaves logits (fp32 [nvox, L]) in self.logits.  update_moving=False: a training-mode pass
        of a FROZEN network - BatchNormalization normalises with the batch statistics but leaves its moving averages alone."""
        p, A = self.plan, self.act
        assert tuple(x.shape) == self._dims(0) + (p.in_channels,), (x.shape,)
        bn_training = self.training if bn_training is None else bn_training
        self._update_moving = update_moving
        self.x_in = x
        h = x
        for ld, lv in enumerate(p.enc):
            h = self._block_fwd(lv[0], h, None, False, bn_training)
            # MaxPooling3D behind the level's second block comes out of that conv's epilogue when the kernel can do it
            fuse_pool = ld < p.depth - 1 and (self.route["tail"][lv[1]["name"]] & 1)
            h = self._block_fwd(lv[1], h, None, False, bn_training, pool=A["pool_%d" % ld] if fuse_pool else None)
            if ld < p.depth - 1:
                h = A["pool_%d" % ld] if fuse_pool else ops.maxpool_fwd(h, A["pool_%d" % ld], planar=self.planar)
        for lv in p.dec:
            a, b = lv
            skip = A[p.enc[a["level"]][1]["name"]]
            self.up[a["name"]].forward(h, skip, bn_training)
            # the last block also produces the logits of the final 1x1x1 conv (one label) in its epilogue when the kernel can do it
            fuse_final = lv is p.dec[-1] and p.n_labels == 1 and (self.route["tail"][b["name"]] & 2)
            h = self._block_fwd(b, A[a["name"]], None, False, bn_training, final=p.final if fuse_final else None)
        f = p.final
        if not (p.dec and fuse_final):
            ops.conv1x1_fwd(h, self.w_view(f["name"]), self.b_view(f["name"]), self.logits)
        return self.logits

    # ------------------------------------------------------------------------------------------------ backward
    def _block_bwd(self, c, src0, src1, up0, wgrad=None):
        """G[c] holds dL/d(output of the block) (already ReLU-masked when the block has no norm).  Leaves dL/d(conv output) in
        G[c] and accumulates the block's parameter gradients - with wgrad(src0, src1, dy) where a decoder route brings a weight-gradient
        launch of its own."""
        name = c["name"]
        g = self.grad[name]
        if c.get("norm") and name in self._dz_ready:
            # the input-gradient launch that produced g already applied the ReLU mask and left the two reductions in norm_ws (_dgrad_into)
            self._dz_ready.discard(name)
            ops.norm_act_bwd_pre(self.pre[name], g, self.gb_view(name, "gamma"), self.nstats[name], g, self.gb_view(name, "gamma", self.G),
                                 self.gb_view(name, "beta", self.G), self.norm_ws, self._norm_mode()[0])
        elif c.get("norm"):
            per, _ = self._norm_mode()
            # (beta given: the ReLU mask is recomputed from the pre-normalisation tensor, the block's output is not read)
            ops.norm_act_bwd(self._as_samples(self.pre[name]), None, self._as_samples(g),
                             self.gb_view(name, "gamma"), self.nstats[name], self._as_samples(g), self.gb_view(name, "gamma", self.G),
                             self.gb_view(name, "beta", self.G), self.norm_ws, per, act=ACT_RELU, beta=self.gb_view(name, "beta"))
        def launch():
            if wgrad is not None:
                wgrad(src0, src1, g)
            else:
                ops.conv3d_wgrad(src0, src1, g, self.w_view(name, self.G), self.b_view(name, self.G), up0=up0, planar=self.planar,
                                 workspace=self.wgrad_ws)
            self._grad_ready(name)

        if self._params:
            self._wgrad(launch)             # behind the event "dL/d(conv output) is final"

    def _dgrad_into(self, b, a):
        """dL/d(output of block a) from block b's conv (whose only input is a's output) -> grad[a].  a normalised: the launch's epilogue
        applies a's ReLU mask (recomputed from a's conv output) and sums dz and dz * x for a's normalisation backward where it can."""
        Gd = self.grad
        an, bn = a["name"], b["name"]
        if self.route["dz"][an]:
            per = self._norm_mode()[0]
            ops.norm_scale_shift(self.nstats[an], self.gb_view(an, "gamma"), self.gb_view(an, "beta"), self.nss[an])
            ops.conv3d_dgrad_norm(Gd[bn], self.Wd[bn], self.pre[an], self.nss[an], Gd[an], self.norm_ws, per, act=ACT_RELU)
            self._dz_ready.add(an)
        else:
            ops.conv3d_dgrad(Gd[bn], self.Wd[bn], Gd[an], mask=self._mask_of(an), planar=self.planar)

    def _mask_of(self, name):
        """ReLU mask tensor a consumer applies to the gradient of `name`'s output, or None when the block is normalised (its
        norm backward applies the activation derivative itself) or `name` is not a conv block."""
        if name in self.pre:
            return None
        return self.act.get(name)

    def backward(self, y_true, grad_scale=1.0, weight=None, dprobs=None, dprobs_scale=1.0, seg_loss=True, params=True):
        """`dprobs` ([..., ld >= n_labels], optional): a gradient that arrives on the probabilities from outside - the adversarial term of
        reference fetal/experiments/train_adv.py:177-180 (the frozen discriminator's input gradient); `seg_loss=False` leaves only that
        term (the unlabelled pass of train_semi.py:176-183).
        params=False: the pass of a FROZEN network, of which only input_gradient() is wanted (engines built with input_grad=True): no
        weight-gradient launch (the side stream stays idle), no data-parallel bucket, and no adam_step is to follow.  The kernels that form
        a parameter gradient next to an input gradient (1x1x1 conv, transposed conv, normalisation backward) still write theirs into G,
        which nobody applies; P, M, V, t and the moving statistics are untouched."""
        p, A, Gd = self.plan, self.act, self.grad
        normed = p.norm is not None
        self._params = bool(params)
        self._det_check_backward(params)
        self._main_stream = torch.cuda.current_stream(self.dev) if self.dev.type == "cuda" else None
        self._dz_ready = set()
        self.G.zero_()
        self._seg_loss_bwd(y_true, grad_scale, weight, dprobs, dprobs_scale, seg_loss)
        f = p.final
        last = p.dec[-1][1] if p.dec else p.enc[-1][1]
        ops.conv1x1_bwd(A[last["name"]], self.w_view(f["name"]), self.dlogits, Gd[last["name"]], self.w_view(f["name"], self.G),
                        self.b_view(f["name"], self.G), relu_mask=not normed)
        self._grad_ready(f["name"])
        # decoder, shallowest level first
        for lv in reversed(p.dec):
            a, b = lv
            ld = a["level"]
            low = self._dec_input_name(ld)
            skip = A[p.enc[ld][1]["name"]]
            self._block_bwd(b, A[a["name"]], None, False)
            self._dgrad_into(b, a)
            self.up[a["name"]].backward(low, skip, Gd["cat_%d" % ld])
        # encoder, deepest level first
        for ld in range(p.depth - 1, -1, -1):
            ca, cb = p.enc[ld]
            if ld < p.depth - 1:
                # gradient of enc[ld].b output = pooled path + skip path, masked by its ReLU
                cat = Gd["cat_%d" % ld]
                ops.maxpool_bwd(A[cb["name"]], Gd["pool_%d" % ld], Gd[cb["name"]], add=cat, add_off=cat.shape[-1] - cb["cout"],
                                relu_mask=not normed, planar=self.planar)
            self._block_bwd(cb, A[ca["name"]], None, False)
            self._dgrad_into(cb, ca)
            xin = self.x_in if ld == 0 else A["pool_%d" % (ld - 1)]
            self._block_bwd(ca, xin, None, False)
            if ld > 0:
                ops.conv3d_dgrad(Gd[ca["name"]], self.Wd[ca["name"]], Gd["pool_%d" % (ld - 1)], planar=self.planar)
            elif self.input_grad:
                # dL/d(input), fp32: the first conv's input gradient on the route planned in _plan_routes
                if self.route["first_dgrad"] == "first":
                    ops.conv3d_first_dgrad(Gd[ca["name"]], self.Wf[ca["name"]], self.dx_in)
                else:
                    ops.conv3d_dgrad(Gd[ca["name"]], self.Wd[ca["name"]], self.dx_in if self.dx_tmp is None else self.dx_tmp, planar=self.planar)
                    if self.dx_tmp is not None:
                        ops.cast(self.dx_tmp, self.dx_in)
        if params:
            self._join_wgrad()
        if self.deterministic:
            self._det_finish()                               # G += the fixed-point sums of every gradient kernel of this pass
            if self.dist is not None and params:
                self.dist.begin()                            # nothing was reduced during this backward: one range, the whole buffer
        if self.dist is not None and params:
            self.dist.finish(self)

    def input_gradient(self):
        """dL/d(input) of the last backward pass, [N][D][H][W][Cin] fp32 (engines built with input_grad=True)"""
        if not self.input_grad:
            raise RuntimeError("this engine was built without input_grad=True")
        return self.dx_in

    def _dec_input_name(self, ld):
        """name of the activation that is up-sampled into decoder level ld"""
        p = self.plan
        if ld == p.depth - 2:
            return p.enc[-1][1]["name"]
        for lv in p.dec:
            if lv[0]["level"] == ld + 1:
                return lv[1]["name"]
        raise KeyError(ld)

    def _grad_ready(self, name):
        # deterministic mode: the gradients sit in the int64 shadow until deterministic_finish at the end of backward(), so no bucket of
        # G may be reduced before that - the whole buffer goes in dist.finish (early buckets all-reduced zeros)
        if self.dist is not None and not self.deterministic and self._params:
            self.dist.grad_ready(self, name)

