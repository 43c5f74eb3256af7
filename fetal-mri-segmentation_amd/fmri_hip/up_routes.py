"""How a decoder level of UNetEngine gets its up-sampled input: six routes, one class each.

A route object belongs to one decoder level (block `a`, its transposed conv `u` when the plan has one).  `candidates` builds, per level,
every route that exists for the plan and dtype, in priority order; UNetEngine._plan_routes takes the first that accepts the batch size.
The first candidate is the level's preferred route: its per-layer images are the ones refresh_weight_copies keeps current, the ones behind
it are fall-backs on the engine's plain [27][Cout][Cin] images of block `a`.

A route
  * decides in `build` whether it exists (None: it does not), and with `ordered` whether FMRI_DETERMINISTIC=1 may run it;
  * owns its weight images (`W`) and says how much of the engine's dwc_scratch it needs (`scratch`);
  * gives its entries of the batched pack table (`pack_entries`) and refreshes the rest of its images (`refresh`);
  * says whether it takes a batch size (`takes`);
  * says what it needs from a buffer set: `up_output` (the transposed conv's output exists), `cat_skip_only` (cat_<level> holds the skip
    channels only: the up-sampled part of the gradient is written straight at low resolution), `writer` (the source channels of the launch
    that writes block a's output, for the statistics tail), `plain_a` (block a runs as a plain conv on eng.Wf / eng.Wd - on this route or
    on the one it falls back to);
  * runs its `forward` and `backward`.
"""
import torch

from . import ops
from ._lib import lib, ACT_NONE, ACT_RELU


class UpRoute(object):
    name = None                # the value of route["up"]
    ordered = True             # every sum of the route is formed in a fixed order: FMRI_DETERMINISTIC=1 may run it
    up_output = False
    cat_skip_only = False
    plain_a = True
    wgrad = False              # block a's weight gradient takes the parity form too (Upcat)

    def __init__(self, eng, a, u, W=None):
        self.eng, self.a, self.u, self.W = eng, a, u, W

    def scratch(self):
        return 0

    def pack_entries(self):
        return []

    def refresh(self):
        pass

    def takes(self, N):
        return True

    def writer(self):
        return self.a["c_up"], self.a["c_skip"]

    def _img(self, *shape, **kw):
        return torch.empty(shape, dtype=kw.get("dtype", self.eng.dtype), device=self.eng.dev)

    def _zeros(self, *shape, **kw):
        return torch.zeros(shape, dtype=kw.get("dtype", self.eng.dtype), device=self.eng.dev)


class Upsample(UpRoute):
    """UpSampling -> concatenate -> conv as the fused-upsample 27- / 9-tap conv: the up-sampled tensor and the concat are never
    materialised (the conv kernels read two sources, the first at half resolution)."""
    name = "upsample"

    @classmethod
    def build(cls, eng, a, u):
        return cls(eng, a, u) if u is None else None

    def forward(self, h, skip, bn_training):
        self.eng._block_fwd(self.a, h, skip, True, bn_training)

    def backward(self, low, skip, cat):
        eng, an = self.eng, self.a["name"]
        eng._block_bwd(self.a, eng.act[low], skip, True)
        ops.conv3d_dgrad(eng.grad[an], eng.Wd[an], cat, planar=eng.planar)
        ops.upsample_bwd(cat, eng.grad[low], dy_off=0, xmask=eng._mask_of(low), planar=eng.planar)


class Upcat(UpRoute):
    """UpSampling -> concatenate -> conv (reference unet.py:132-138,61,102) in parity form (fmri_conv3d_upcat_*): pre-summed 2x2x2 filters
    per output parity for the up-sampled channels, plain 27-tap filters for the skip channels.  FMRI_UPCAT=0 keeps the fused-upsample conv
    (A/B switch).  fp32 (round 6): the parity form runs on the fp32 instantiation of the same MFMA kernels where fmri_conv3d_upcat_ok says
    so - 3-D, channels in multiples of 16; FMRI_F32_MFMA=0 keeps fp32 on the VALU kernels and with them on the fused-upsample form.
    2-D: the slices ride the kernels' D axis, so the slice count must be a multiple of the 4-slice tile; other batches fall back to the
    fused-upsample conv, for which the level keeps its plain 9-tap images too.
    `wgrad`: the weight gradient takes the parity form as well.  Its scratch is filled by fp32 atomics, so deterministic mode keeps the
    fused-upsample 27-tap weight gradient."""
    name = "upcat"
    cat_skip_only = True

    @classmethod
    def build(cls, eng, a, u):
        if u is not None or (eng.dtype != torch.bfloat16 and eng.planar) or not eng.sw["UPCAT"]:
            return None
        c0, c1, cout = a["c_up"], a["c_skip"], a["cout"]
        # (2-D: 4 slices, one tile, stand in for "a batch that tiles")
        D, H, W = eng.plan.level_dims(a["level"], 4) if eng.planar else eng.plan.level_dims(a["level"])
        ok = ops.conv3d_upcat_ok(c0, c1, cout, D, H, W, eng.dtype, planar=eng.planar)
        if not ok & 1:
            return None
        self = cls(eng, a, u)
        npar = 4 if eng.planar else 8           # parity classes = pre-summed taps per class (2-D: (ph,pw) x 2x2 taps)
        self.W = dict(up_f=self._img(npar, npar, cout, c0), sk_f=self._img(27, cout, c1), up_d=None, sk_d=None)
        if eng.training:
            self.W["up_d"], self.W["sk_d"] = self._img(npar, npar, c0, cout), self._img(27, c1, cout)
        self.wgrad = bool(ok & 2) and not eng.deterministic
        self.plain_a = eng.planar
        return self

    def scratch(self):
        return 64 * self.a["cout"] * self.a["c_up"] if self.wgrad else 0

    def pack_entries(self):
        W = self.W
        return [("up", self.eng.w_view(self.a["name"]), self.a["c_up"], self.a["c_skip"], W["up_f"], W["up_d"], W["sk_f"], W["sk_d"],
                 self.eng.planar)]

    def takes(self, N):
        return not self.eng.planar or N % 4 == 0

    def writer(self):
        return self.a["c_skip"], 0              # the parity form's skip launch writes the output

    def _conv(self, src0, src1, out, act, summed, per):
        eng, W, b = self.eng, self.W, self.eng.b_view(self.a["name"])
        if summed:
            ops.conv3d_upcat_fwd_stats(src0, src1, W["up_f"], W["sk_f"], b, out, eng.norm_ws, per, act=act)
        else:
            ops.conv3d_upcat_fwd(src0, src1, W["up_f"], W["sk_f"], b, out, act=act, planar=eng.planar)

    def _wgrad_launch(self, src0, src1, g):
        eng, an = self.eng, self.a["name"]
        ops.conv3d_upcat_wgrad(src0, src1, g, eng.w_view(an, eng.G), eng.b_view(an, eng.G), eng.dwc_scratch, workspace=eng.wgrad_ws,
                               planar=eng.planar)

    def forward(self, h, skip, bn_training):
        self.eng._block_fwd(self.a, h, skip, True, bn_training, conv=self._conv)

    def backward(self, low, skip, cat):
        eng, W = self.eng, self.W
        eng._block_bwd(self.a, eng.act[low], skip, True, wgrad=self._wgrad_launch if self.wgrad else None)
        ops.conv3d_upcat_dgrad(eng.grad[self.a["name"]], W["up_d"], W["sk_d"], eng._mask_of(low), None, eng.grad[low], cat, planar=eng.planar)


class Deconv(UpRoute):
    """Deconvolution(k = 2, s = 2) (reference unet.py:135) on the direct k2s2 kernels into its own tensor, then block a as a plain
    two-source conv.  The base of the other materialising routes, which replace `up_fwd` / `up_bwd` / `refresh`."""
    name = "deconv"
    up_output = True

    @classmethod
    def build(cls, eng, a, u):
        if u is None:
            return None
        self = cls(eng, a, u)
        self.wt = self._img(8, u["cout"], u["cin"])          # compute-dtype copy of the transposed-conv filter [8][Cout][Cin]
        return self

    def refresh(self):
        ops.cast(self.eng.w_view(self.u["name"]), self.wt)

    def up_fwd(self, h, y):
        ops.deconv_fwd(h, self.wt, self.eng.b_view(self.u["name"]), y, planar=self.eng.planar)

    def up_bwd(self, low, cat):
        eng, un = self.eng, self.u["name"]
        ops.deconv_bwd(eng.act[low], self.wt, cat, eng.grad[low], eng.w_view(un, eng.G), eng.b_view(un, eng.G), dy_off=0,
                       xmask=eng._mask_of(low), planar=eng.planar)

    def forward(self, h, skip, bn_training):
        y = self.eng.act[self.u["name"]]
        self.up_fwd(h, y)
        self.eng._block_fwd(self.a, y, skip, False, bn_training)

    def backward(self, low, skip, cat):
        eng, an = self.eng, self.a["name"]
        eng._block_bwd(self.a, eng.act[self.u["name"]], skip, False)
        ops.conv3d_dgrad(eng.grad[an], eng.Wd[an], cat, planar=eng.planar)
        self.up_bwd(low, cat)
        eng._grad_ready(self.u["name"])


class Onetap(Deconv):
    """Deconvolution3D as the parity form with ONE non-zero tap per parity class: output voxel 2g+p = W[p] . x[g] + b, so the transposed
    conv rides the MFMA kernels of the up-sampling parity form (fmri_conv3d_upcat_* with C1 = 0).  Parity p reads low-res offset 0, which is
    combined tap 7 - p of the forward image and (mirrored) tap p of the input-gradient image; the other taps stay zero.
    Not ordered: its weight gradient is the parity-form one, whose scratch is filled by fp32 atomics."""
    name = "onetap"
    ordered = False

    @classmethod
    def build(cls, eng, a, u):
        if u is None or eng.planar or eng.dtype != torch.bfloat16:
            return None
        cin, cout = u["cin"], u["cout"]
        if ops.conv3d_upcat_ok(cin, 0, cout, *eng.plan.level_dims(a["level"]), eng.dtype) != 3:
            return None
        self = cls(eng, a, u)
        self.W = dict(up_f=self._zeros(8, 8, cout, cin), up_d=None, dw27=None)
        if eng.training:
            self.W["up_d"] = self._zeros(8, 8, cin, cout)
            self.W["dw27"] = self._zeros(27, cout, cin, dtype=torch.float32)   # never read
        self.par8 = torch.arange(8, device=eng.dev)
        return self

    def scratch(self):
        return 64 * self.u["cout"] * self.u["cin"]

    def refresh(self):
        W, p8, w8 = self.W, self.par8, self.eng.w_view(self.u["name"])
        W["up_f"][p8, 7 - p8] = w8.to(self.eng.dtype)
        if W["up_d"] is not None:
            W["up_d"][p8, p8] = w8.transpose(1, 2).to(self.eng.dtype)

    def up_fwd(self, h, y):
        ops.conv3d_upcat_fwd(h, None, self.W["up_f"], None, self.eng.b_view(self.u["name"]), y, act=ACT_NONE)

    def up_bwd(self, low, cat):
        eng, un, W = self.eng, self.u["name"], self.W
        dyc = ops.slice_channels(cat, 0, eng.grad[un])          # the transposed conv's own slice of the concat gradient
        ops.conv3d_upcat_dgrad(dyc, W["up_d"], None, eng._mask_of(low), None, eng.grad[low], None)
        if eng._params:
            ops.conv3d_upcat_wgrad(eng.act[low], None, dyc, W["dw27"], eng.b_view(un, eng.G), eng.dwc_scratch)
            cin, cout = self.u["cin"], self.u["cout"]
            dwc = eng.dwc_scratch[:64 * cout * cin].view(8, 8, cout, cin)
            eng.w_view(un, eng.G).add_(dwc[self.par8, 7 - self.par8])


class D2s(Deconv):
    """Deconvolution2D (reference unet/unet.py get_up_convolution): the 4 taps are 4 independent 1x1 convs, run as ONE planar 3x3 MFMA conv
    to 4*Cout channels whose only non-zero tap is the centre one, followed by a depth-to-space copy.  The slices must tile by 4; other
    batches fall back to the direct kernels.
    Not ordered: the filter and bias gradients are formed in buffers of the route's own and added to G by torch, outside the fixed-point
    shadow of deterministic mode.
    The (1, S, H, W, 4*Cout) scratch is allocated once per slice count and never replaced: captured hipGraphs keep its address.
    Kept as found: only a level's preferred route is refreshed, so the direct kernels that run behind this route on a slice count that
    does not tile read a filter copy no launch has filled.  Filling it is one more cast launch per step, a change of the pinned schedule."""
    name = "d2s"
    ordered = False

    @classmethod
    def build(cls, eng, a, u):
        if u is None or not eng.planar or eng.dtype != torch.bfloat16:
            return None
        cin, c4 = u["cin"], 4 * u["cout"]
        _, H, W = eng.plan.level_dims(a["level"] + 1, 4)          # low-res dims (the slice count does not matter here)
        if not lib().fmri_conv3d_uses_mfma(cin, 0, c4, 4, H, W, 1) & 1:
            return None
        self = cls(eng, a, u)
        f32 = torch.float32
        self.W = dict(w32=self._zeros(27, c4, cin, dtype=f32), wf=self._img(27, c4, cin), wd=None, b4=self._zeros(c4, dtype=f32))
        if eng.training:
            self.W.update(wd=self._img(27, cin, c4), dw=self._zeros(27, c4, cin, dtype=f32), db=self._zeros(c4, dtype=f32))
        self.t4 = {}
        return self

    def takes(self, N):
        return N % 4 == 0

    def refresh(self):
        eng, W, un = self.eng, self.W, self.u["name"]
        W["w32"][13] = eng.w_view(un)[:4].reshape(4 * self.u["cout"], self.u["cin"])
        W["b4"].copy_(eng.b_view(un).repeat(4))
        ops.pack_weights(W["w32"], W["wf"], W["wd"])

    def _tmp(self, x_low):
        S = x_low.shape[1]
        if S not in self.t4:
            self.t4[S] = self._img(*(tuple(x_low.shape[:-1]) + (4 * self.u["cout"],)))
        return self.t4[S]

    @staticmethod
    def _views(y, t4):
        """matching 6-D views (S, H, ah, W, aw, Cout) of the full-resolution tensor y (1,S,2H,2W,Cout) and of t4 (1,S,H,W,4*Cout)"""
        _, S, H, W, C4 = t4.shape
        C = C4 // 4
        return y.view(S, H, 2, W, 2, C), t4.view(S, H, W, 2, 2, C).permute(0, 1, 3, 2, 4, 5)

    def up_fwd(self, h, y):
        t4 = self._tmp(h)
        ops.conv3d_fwd(h, None, self.W["wf"], self.W["b4"], t4, act=ACT_NONE, planar=True)
        yv, tv = self._views(y, t4)
        yv.copy_(tv)

    def up_bwd(self, low, cat):
        eng, un, W = self.eng, self.u["name"], self.W
        dyc = ops.slice_channels(cat, 0, eng.grad[un])
        t4 = self._tmp(eng.act[low])
        yv, tv = self._views(dyc, t4)
        tv.copy_(yv)                                               # space-to-depth of the gradient
        ops.conv3d_dgrad(t4, W["wd"], eng.grad[low], mask=eng._mask_of(low), planar=True)
        if eng._params:
            W["dw"].zero_()
            W["db"].zero_()
            ops.conv3d_wgrad(eng.act[low], None, t4, W["dw"], W["db"], planar=True)
            eng.w_view(un, eng.G)[:4].add_(W["dw"][13].view(4, self.u["cout"], self.u["cin"]))
            eng.b_view(un, eng.G).add_(W["db"].view(4, self.u["cout"]).sum(0))


class Fold(UpRoute):
    """Deconvolution3D -> concatenate -> Conv3D FOLDED into one parity-form convolution of the low-res tensor (round 3; fmri_hip/deconv_fold.py,
    fmri_conv3d_upcat_fwd_bias27): the transposed conv's output is never materialised and block a does 8 instead of 27 taps on its
    up-sampled channels, exactly as in the UpSampling3D variant - with pre-MULTIPLIED instead of pre-summed filters.  The level has no
    plain images of block a.  FMRI_DECONV_FOLD=0 keeps the two-step form (A/B switch).
    Backward: the parity-filter gradients come from the MFMA kernel and are chained through the transposed conv's weights by deconv_fold
    (with the sums of dy over the 26 border classes for the bias classes); the input gradients w.r.t. the low-res tensor (parity-form
    launch over the space-to-depth view of dy) and the skip tensor come from one launch.
    Not ordered: the border classes are summed with fp32 atomics, and the weight gradient is the parity-form one."""
    name = "fold"
    ordered = False
    cat_skip_only = True
    plain_a = False

    @classmethod
    def build(cls, eng, a, u):
        sw = eng.sw
        if u is None or eng.planar or eng.dtype != torch.bfloat16 or eng.plan.norm is not None or not (sw["DECONV_FOLD"] and sw["FWD_WS"]):
            return None
        cin, cmid, cs, cout = u["cin"], u["cout"], a["c_skip"], a["cout"]
        if cmid != a["c_up"] or ops.conv3d_upcat_ok(cin, cs, cout, *eng.plan.level_dims(a["level"]), eng.dtype) != 3:
            return None
        if eng.fold is None:
            from .deconv_fold import DeconvFold
            eng.fold = DeconvFold(eng.dev)
        self = cls(eng, a, u)
        # weight GEMMs of the largest levels with bf16 operands (fp32 accumulation): 0.3 % relative error on filters that are rounded to
        # bf16 for the MFMA kernels anyway, 2.3x faster at 256 x 512 x 512 (tools/bench_fold.py); below 2^25 multiply-adds per block fp32
        # is as fast
        self.gd = torch.bfloat16 if cout * cmid * cin >= (1 << 25) else None
        f32 = torch.float32
        self.W = dict(up_f=self._img(8, 8, cout, cin), sk_f=self._img(27, cout, cs), up_d=None, sk_d=None,
                      bias27=self._zeros(27, cout, dtype=f32))
        if eng.training:
            self.W.update(up_d=self._img(8, 8, cin, cout), sk_d=self._img(27, cs, cout), s27=self._zeros(27, cout, dtype=f32))
        return self

    def scratch(self):
        return 64 * self.a["cout"] * self.u["cin"]

    def refresh(self):
        eng, W, an, un, cmid = self.eng, self.W, self.a["name"], self.u["name"], self.u["cout"]
        w3 = eng.w_view(an)
        weff, b27 = eng.fold.effective(w3, eng.w_view(un), eng.b_view(an), eng.b_view(un), cmid, gemm_dtype=self.gd)
        W["up_f"].copy_(weff)
        W["bias27"].copy_(b27)
        W["sk_f"].copy_(w3[:, :, cmid:])
        if W["up_d"] is not None:
            W["up_d"].copy_(weff[:, eng.fold.mirror].transpose(-1, -2))            # Wc[p][1 - t']^T (fmri_conv3d_pack_up_weights' w_up_dgrad)
            W["sk_d"].copy_(w3[:, :, cmid:].flip(0).transpose(1, 2))               # tap-flipped transposed skip filters

    def forward(self, h, skip, bn_training):
        W = self.W
        ops.conv3d_upcat_fwd_bias27(h, skip, W["up_f"], W["sk_f"], W["bias27"], self.eng.act[self.a["name"]], act=ACT_RELU)

    def backward(self, low, skip, cat):
        """G[a] holds dL/d(conv output)"""
        eng, W, an, un, cmid = self.eng, self.W, self.a["name"], self.u["name"], self.u["cout"]
        cout, cin = self.a["cout"], self.u["cin"]
        g, x_low = eng.grad[an], eng.act[low]

        def wgrad():
            dwc = eng.dwc_scratch[:64 * cout * cin]
            ops.conv3d_upcat_wgrad_parts(x_low, skip, g, eng.w_view(an, eng.G), eng.b_view(an, eng.G), dwc, workspace=eng.wgrad_ws)
            s27 = W["s27"]
            s27.zero_()
            ops.border_class_sums(g, s27)
            s27[13] = eng.b_view(an, eng.G) - s27.sum(0)        # interior class = all voxels (the conv's bias gradient) - the 26 border classes
            dw3u, dwt, dbt = eng.fold.chain(dwc.view(8, 8, cout, cin), eng.w_view(an), eng.w_view(un), eng.b_view(un), cmid, s27,
                                            gemm_dtype=self.gd)
            eng.w_view(an, eng.G)[:, :, :cmid].add_(dw3u)
            eng.w_view(un, eng.G).add_(dwt)
            eng.b_view(un, eng.G).add_(dbt)
            eng._grad_ready(an)
            eng._grad_ready(un)

        if eng._params:
            eng._wgrad(wgrad)
        ops.conv3d_upcat_dgrad(g, W["up_d"], W["sk_d"], eng._mask_of(low), None, eng.grad[low], cat)


ORDER = (Fold, D2s, Onetap, Deconv, Upcat, Upsample)


def candidates(eng, a, u):
    """the routes of one decoder level in priority order; deterministic mode keeps the ordered ones"""
    built = [cls.build(eng, a, u) for cls in ORDER if cls.ordered or not eng.deterministic]
    return [r for r in built if r is not None]
