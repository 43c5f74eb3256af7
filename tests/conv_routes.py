"""The dispatch rule of the forward / input-gradient conv launchers (csrc/conv3d_mfma.hip: conv3d_fwd_mfma_launch and
conv3d_fwd_mfma_launch_f32), restated in plain Python, and a table of tensors (ROWS) that reaches every kernel instantiation behind the
FMRI_FWD(...) launch sites on both sides of the thresholds that select it.  Test infrastructure, like tests/philox_ref.py: nothing here
touches a device.  tests/test_host_conv_routes.py proves the table against the source text, tests/test_gpu_conv_routes.py runs it.

The rule.  A launch works on `ntile` output tiles (4 x 8 x 16 voxels, or 8 x 8 x 8 when only that tiling fits: "cube") and on Cout blocks
of 32 or 64 channels; np = ntile * blocks [* 8 | * 4 parity classes in the up-forward mode] (tile, block) pairs go to
grid = min(np, ncu) persistent workgroups, workgroup b taking the pairs b, b + grid, ... (after the XCD renumbering of b).
  wide   64-wide blocks:  Cout % 64 == 0  and  ntile * (Cout / 64) * f >= ncu   (f = 8 / 4 / 1 as above)
  drain  the asynchronous epilogues of the warp-specialised kernel:  np > ncu  (3-D, FMRI_FWD_WS on, one epilogue kind)
  fh     fast halo addressing:  one plain source on the 4 x 8 x 16 tiling
fp32 launches: 32-wide blocks and the asynchronous epilogue throughout."""
import collections
import itertools

TD, TH, TW = 4, 8, 16
CHANNELS = (32, 64, 96, 128, 256)            # the generator's channel counts; fp32 rows may also take 16
CHANNELS_F32 = (16,) + CHANNELS

Route = collections.namedtuple("Route", "inst ntile np grid compact wide drain cube tile")


class Refused(ValueError):
    """the launcher (or the entry point in front of it) answers FMRI_E_SHAPE"""


def needs_cube(D, H, W):
    return bool((D % TD) or (H % TH) or (W % TW))


def mfma_ok(C0, C1, Cout, D, H, W, f32, f32_mfma=True):
    """conv3d_fwd_mfma_ok"""
    if f32:
        if not f32_mfma or (C0 % 16) or (C1 % 16) or C0 + C1 < 16 or (Cout % 32):
            return False
        if needs_cube(D, H, W):
            return False
        C0, C1 = 2 * C0, 2 * C1
    if (C0 % 32) or (C1 % 32) or C0 + C1 < 32 or (Cout % 32):
        return False
    if C0 + C1 > 4096:
        return False
    if (min(D, TD) + 2) * 2 * H * W * max(C0, C1) * 2 >= 1 << 31:
        return False
    if needs_cube(D, H, W):
        return not ((D % 8) or (H % 8) or (W % 8))
    return True


def first_layer(C0, C1):
    """conv3d_first_ok takes the launches with 1-4 input channels away from fmri_conv3d_fwd: none of this table's (>= 16)"""
    return C1 == 0 and C0 <= 4


def fwd_wide(mode, planar, ntile, Cout, ncu):
    return Cout % 64 == 0 and ntile * (Cout // 64) * ((4 if planar else 8) if mode == 1 else 1) >= ncu


def upcat_ok(C0, C1, Cout, D, H, W, f32, planar=False, f32_mfma=True):
    """bit 0 of conv3d_api.hip upcat_ok (D, H, W: the full-resolution output)"""
    if ((0 if planar else D) | H | W) & 1:
        return False
    if planar and f32:
        return False
    Dl = D if planar else D // 2
    if C0 <= 0 or C1 < 0 or Cout * (4 if planar else 8) * (2 if f32 else 1) > 4096:
        return False
    if needs_cube(Dl, H // 2, W // 2) or needs_cube(D, H, W):
        return False
    ok = lambda a, o, d, h, w: mfma_ok(a, 0, o, d, h, w, f32, f32_mfma)
    return (ok(C0, Cout, Dl, H // 2, W // 2) and ok(Cout, C0, Dl, H // 2, W // 2)
            and (C1 == 0 or (ok(C1, Cout, D, H, W) and ok(Cout, C1, D, H, W))))


def _b(v):
    return "true" if v else "false"


def route(launcher, mode, planar, N, D, H, W, C0, C1, up0, Cout, mask, residual, tail, ncu, use_ws=True, res_async=True):
    """The kernel instantiation one launch runs, as written at its FMRI_FWD(...) site, and its work split.
    launcher 'bf16' | 'f32'; mode 0 plain, 1 up-forward, 2 up-backward (D, H, W: the launch's own grid, low resolution in the parity
    modes); tail: the FwdTail members that are set, a subset of {'pool', 'logits', 'bias27', 'nws', 'nss'}; use_ws / res_async: the
    process's FMRI_FWD_WS / FMRI_RES_ASYNC.  Raises Refused where the launcher returns FMRI_E_SHAPE."""
    tail = frozenset(tail or ())
    planar, up0, mask, residual = bool(planar), bool(up0), bool(mask), bool(residual)
    if launcher == "f32":
        if planar or needs_cube(D, H, W) or "logits" in tail or "nws" in tail:
            raise Refused("fp32: 3-D launches on the 4x8x16 tiling, no logits / normalisation tails")
        if mode != 0 and (C1 or up0):
            raise Refused("parity modes: one plain source")
        ntile = N * (D // TD) * (H // TH) * (W // TW)
        np_ = ntile * (Cout // 32) * (8 if mode == 1 else 1)
        fh = C1 == 0 and not up0
        if mode == 1:
            if mask or residual or "pool" in tail:
                raise Refused("up-forward: plain store only")
            inst = "k_conv_fwd_ws<1, 1, false, false, -1, true, true>"
        elif mode == 2:
            if residual or "pool" in tail:
                raise Refused("up-backward: store or mask")
            inst = "k_conv_fwd_ws<1, 2, false, false, -1, true, true>"
        else:
            if (residual and (mask or "pool" in tail)) or (mask and "pool" in tail):
                raise Refused("one epilogue kind per launch")
            inst = "k_conv_fwd_ws<1, 0, false, true, %d, %s, true>" % (3 if residual else (1 if mask else 0), _b(fh))
        return Route(inst, ntile, np_, min(np_, ncu), _compact(D // TD, H // TH, W // TW), False, True, False, (TD, TH, TW))
    assert launcher == "bf16"
    if mode != 0 and (C1 or up0):
        raise Refused("parity modes: one plain source")
    cube = needs_cube(D, H, W)
    tile = (8, 8, 8) if cube else (TD, TH, TW)
    tdn, thn, twn = D // tile[0], H // tile[1], W // tile[2]
    ntile = N * tdn * thn * twn
    fh = not cube and C1 == 0 and not up0
    wide = fwd_wide(mode, planar, ntile, Cout, ncu)
    np_ = ntile * (Cout // (64 if wide else 32)) * ((4 if planar else 8) if mode == 1 else 1)
    nt = 2 if wide else 1
    pool, logits = "pool" in tail, "logits" in tail
    drain = False
    if "nws" in tail:
        if cube or mode != 0 or planar or not use_ws or np_ <= ncu or pool or logits or "bias27" in tail:
            raise Refused("normalisation tails: the asynchronous epilogue only")
        if ((not mask or residual) if "nss" in tail else mask):
            raise Refused("normalisation tails: lines")
        drain = True
        inst = "k_conv_fwd_ws<%d, 0, false, true, %d>" % (nt, 5 if "nss" in tail else (6 if residual else 4))
    elif planar and (pool or logits):
        if cube or mode != 0 or residual or mask or C1 or up0 or (logits and Cout != (64 if wide else 32)):
            raise Refused("planar tails")
        inst = "k_conv_fwd_mfma<%d, true, 0, false, false, true, true>" % nt
    elif cube:
        if mode != 0 or residual or planar:
            raise Refused("8x8x8 tiling: plain 3-D launches")
        inst = "k_conv_fwd_mfma<%d, false, 0, false, true>" % nt
    elif mode != 0:
        if planar:
            inst = "k_conv_fwd_mfma<%d, true, %d, false>" % (nt, mode)
        elif use_ws:
            inst = "k_conv_fwd_ws<%d, %d, false, false, -1, true>" % (nt, mode)
        else:
            inst = "k_conv_fwd_mfma<%d, false, %d, false>" % (nt, mode)
    elif residual:
        drain = res_async and not planar and use_ws and np_ > ncu and not mask and not pool and not logits
        if planar:
            inst = "k_conv_fwd_mfma<%d, true, 0, true, false, %s>" % (nt, _b(fh))
        elif drain:
            inst = "k_conv_fwd_ws<%d, 0, false, true, 3, %s>" % (nt, _b(fh))
        elif use_ws:
            inst = "k_conv_fwd_ws<%d, 0, true, false, -1, %s>" % (nt, _b(fh))
        else:
            inst = "k_conv_fwd_mfma<%d, false, 0, true, false, %s>" % (nt, _b(fh))
    else:
        epi = (-1 if (pool or logits) else 1) if mask else ((-1 if pool else 2) if logits else 0)
        drain = not planar and use_ws and np_ > ncu and epi >= 0
        if drain:
            inst = "k_conv_fwd_ws<%d, 0, false, true, %d, %s>" % (nt, epi, _b(fh))
        elif use_ws and not planar:
            inst = "k_conv_fwd_ws<%d, 0, false, false, -1, %s>" % (nt, _b(fh))
        elif planar:
            inst = "k_conv_fwd_mfma<%d, true, 0, false, false, %s>" % (nt, _b(fh))
        else:
            inst = "k_conv_fwd_mfma<%d, false, 0, false, false, %s>" % (nt, _b(fh))
    return Route(inst, ntile, np_, min(np_, ncu), _compact(tdn, thn, twn), wide, drain, cube, tile)


def _compact(tdn, thn, twn):
    """tiles numbered in compact 2 x 4 x 4 blocks (the kernels' decode()) instead of linearly"""
    return ((twn | thn) & 3) == 0 and (tdn & 1) == 0


def tile_of_pair(r, pair, mode, planar, N, D, H, W, Cout):
    """decode() of the kernels: (n, d0, h0, w0, co0, parity) of pair number `pair` of a launch with route r"""
    bn = 64 if r.wide else 32
    cbn = Cout // bn
    ncb = ((4 if planar else 8) if mode == 1 else 1) * cbn
    cb, q = pair % ncb, pair // ncb
    par, co0 = (cb // cbn, (cb % cbn) * bn) if mode == 1 else (0, cb * bn)
    tdn, thn, twn = D // r.tile[0], H // r.tile[1], W // r.tile[2]
    if r.compact:
        i, blk = q & 31, q >> 5
        bw, blk = blk % (twn >> 2), blk // (twn >> 2)
        bh, blk = blk % (thn >> 2), blk // (thn >> 2)
        return (blk // (tdn >> 1), ((blk % (tdn >> 1)) * 2 + (i >> 4)) * r.tile[0], (bh * 4 + ((i >> 2) & 3)) * r.tile[1],
                (bw * 4 + (i & 3)) * r.tile[2], co0, par)
    w0, q = (q % twn) * r.tile[2], q // twn
    h0, q = (q % thn) * r.tile[1], q // thn
    return (q // tdn, (q % tdn) * r.tile[0], h0, w0, co0, par)


# ------------------------------------------------------------------------------------------------ public wrappers -> launches
# An op is the public wrapper a row goes through.  A shape is (N, D, H, W, C0, C1, Cout) in the wrapper's own terms: D, H, W the
# full-resolution grid, C0 the channels of the first (or low-resolution, or dy) tensor, C1 of the skip tensor, Cout of the result
# (upcat_dgrad*: C0 / C1 are the channels of the two gradients, Cout those of dy; stride2: D, H, W is the input grid).
L = collections.namedtuple("Launch", "mode planar N D H W C0 C1 up0 Cout mask residual tail")
OPS = ("fwd", "fwd_up", "fwd_mask", "dgrad", "dgrad_mask", "tail_pool", "tail_logits", "tail_both", "stats", "dgrad_norm", "upcat",
       "upcat_stats", "bias27", "upcat_dgrad", "upcat_dgrad_mask", "stride2")


def launches(op, f32, planar, N, D, H, W, C0, C1, Cout, ncu, use_ws=True, f32_mfma=True):
    """the forward-launcher calls wrapper `op` makes, in order (Refused where the entry point refuses before any launch)"""
    p = bool(planar)
    Dl = D if p else D // 2
    if op in ("fwd", "fwd_up", "fwd_mask", "dgrad", "dgrad_mask"):
        up0 = op == "fwd_up"
        if op.startswith("dgrad") and C1:
            raise Refused("input gradient: one source")
        if up0 and (((0 if p else D) | H | W) & 1):
            raise Refused("odd dims under an up-sampled source")
        if first_layer(C0, C1) or not mfma_ok(C0, C1, Cout, D, H, W, f32, f32_mfma) or (p and (f32 or needs_cube(D, H, W))):
            raise Refused("not on the MFMA forward launchers")
        return [L(0, p, N, D, H, W, C0, C1, up0, Cout, op.endswith("mask"), False, ())]
    if op in ("tail_pool", "tail_logits", "tail_both"):
        t = {"tail_pool": ("pool",), "tail_logits": ("logits",), "tail_both": ("pool", "logits")}[op]
        if C1 or not mfma_ok(C0, 0, Cout, D, H, W, f32, f32_mfma) or needs_cube(D, H, W) or (p and f32) or (f32 and "logits" in t):
            raise Refused("fmri_conv3d_fwd_tail_ok")
        if not p and not use_ws:
            raise Refused("fmri_conv3d_fwd_tail_ok: the 3-D tails are the warp-specialised kernel's")
        ntile = N * (D // TD) * (H // TH) * (W // TW)
        if "logits" in t and Cout != (64 if fwd_wide(0, p, ntile, Cout, ncu) else 32):
            raise Refused("fmri_conv3d_fwd_tail_ok bit 1: the logits need the whole channel range in one block")
        return [L(0, p, N, D, H, W, C0, 0, False, Cout, False, False, t)]
    if op == "stats":
        if f32 or p or not mfma_ok(C0, C1, Cout, D, H, W, False) or needs_cube(D, H, W):
            raise Refused("fmri_conv3d_fwd_ntail_ok")
        return [L(0, False, N, D, H, W, C0, C1, False, Cout, False, False, ("nws",))]
    if op == "dgrad_norm":
        if f32 or p or C1 or not mfma_ok(C0, 0, Cout, D, H, W, False) or needs_cube(D, H, W):
            raise Refused("fmri_conv3d_fwd_ntail_ok")
        return [L(0, False, N, D, H, W, C0, 0, False, Cout, True, False, ("nws", "nss"))]
    if op in ("upcat", "upcat_stats", "bias27"):
        if not upcat_ok(C0, C1, Cout, D, H, W, f32, p, f32_mfma) or (op != "upcat" and (p or not C1)) or (op == "upcat_stats" and f32):
            raise Refused("fmri_conv3d_upcat_ok")
        out = [L(1, p, N, Dl, H // 2, W // 2, C0, 0, False, Cout, False, False, ())]
        if C1:
            out.append(L(0, p, N, D, H, W, C1, 0, False, Cout, False, True, {"upcat": (), "upcat_stats": ("nws",), "bias27": ("bias27",)}[op]))
        return out
    if op in ("upcat_dgrad", "upcat_dgrad_mask"):
        if not upcat_ok(C0, C1, Cout, D, H, W, f32, p, f32_mfma):
            raise Refused("fmri_conv3d_upcat_ok")
        m = op.endswith("mask")
        out = [L(2, p, N, Dl, H // 2, W // 2, Cout, 0, False, C0, m, False, ())]
        if C1:
            out.append(L(0, p, N, D, H, W, Cout, 0, False, C1, m, False, ()))
        return out
    if op == "stride2":
        if p or C1 or not upcat_ok(Cout, 0, C0, D, H, W, f32, False, f32_mfma):
            raise Refused("fmri_conv3d_upcat_ok")
        return [L(2, False, N, D // 2, H // 2, W // 2, C0, 0, False, Cout, False, False, ())]
    raise KeyError(op)


def route_of(launch, f32, ncu, use_ws=True, res_async=True):
    return route("f32" if f32 else "bf16", *launch, ncu=ncu, use_ws=use_ws, res_async=res_async)


# ------------------------------------------------------------------------------------------------ targets and the row generator
# rel: which side of which threshold the row sits on (k = ntile * (Cout / 64) * f, the left side of fwd_wide)
#   np_eq    np == ncu                      the last launch without a second item per workgroup
#   np_gt    the smallest reachable np > ncu
#   np_gt2   the smallest reachable np > 2 * ncu: some workgroup handles a third item
#   np_lt    np < ncu, the largest reachable (with grid % 8 != 0 asked for in `where`)
#   wide_eq  k == ncu: wide by the >=
#   wide_lt  the largest reachable k < ncu with Cout % 64 == 0: narrow by one step
#   any      the cheapest tensor on the route
Target = collections.namedtuple("Target", "name op f32 planar which inst rel where")


def T(name, op, inst, rel, f32=False, planar=False, which=0, **where):
    return Target(name, op, f32, planar, which, inst, rel, tuple(sorted(where.items())))


Row = collections.namedtuple("Row", "target shape launch route")


def _grids(planar, cube, f32):
    """(N, D, H, W, tiles per sample, compact numbering) of the TARGET launch in the fixed search order: tile counts first, then the batch"""
    t = (8, 8, 8) if cube else (TD, TH, TW)
    out = []
    for tdn, thn, twn, N in itertools.product(range(1, 9), range(1, 21), range(1, 9), (1, 2, 3)):
        if planar and N != 1:
            continue
        D, H, W = tdn * t[0], thn * t[1], twn * t[2]
        if cube and not needs_cube(D, H, W):
            continue
        if N * D * H * W <= MAX_VOXELS:
            out.append((N, D, H, W, tdn * thn * twn, _compact(tdn, thn, twn)))
    return out


MAX_VOXELS = 330000
_GRID_CACHE = {}
_LOW_OPS = ("upcat", "upcat_stats", "bias27", "upcat_dgrad", "upcat_dgrad_mask", "stride2")


def _shape(target, where, chans, N, D, H, W, Cout, C1):
    """the wrapper's shape whose TARGET launch has grid (N, D, H, W) and Cout output channels"""
    cmin = 32 if target.op in _LOW_OPS else chans[0]            # the parity form runs both directions: every channel count is a Cout too
    c_in = where.get("C0", cmin)
    low = target.op in _LOW_OPS and target.which == 0            # the target launch runs on the half-resolution grid
    full = (N, D if (target.planar or not low) else 2 * D, 2 * H if low else H, 2 * W if low else W)
    if target.op == "stride2":
        return full + (c_in, 0, Cout)
    if target.op.startswith("upcat_dgrad"):
        # which 0: the launch's Cout is the low tensor's C0, its input channels those of dy; which 1: its Cout is the skip tensor's C1
        return full + ((Cout, C1, c_in) if target.which == 0 else (cmin, Cout, c_in))
    if target.op in ("upcat", "upcat_stats", "bias27") and target.which == 1:
        return full + (cmin, c_in, Cout)
    return full + (c_in, C1, Cout)


def _place(target, shape, ncu):
    ls = launches(target.op, target.f32, target.planar, *shape, ncu=ncu)
    if target.which >= len(ls):
        raise Refused("no such launch")
    return ls[target.which], route_of(ls[target.which], target.f32, ncu)


def _primary(rel, r, lc, ncu):
    """the search key of `rel` (smaller is better), or None where the launch is on the wrong side"""
    k = r.ntile * (lc.Cout // 64) * ((4 if lc.planar else 8) if lc.mode == 1 else 1)
    if rel == "np_eq":
        return 0 if r.np == ncu else None
    if rel == "np_gt":
        return r.np if r.np > ncu else None
    if rel == "np_gt2":
        return r.np if r.np > 2 * ncu else None
    if rel == "np_lt":
        return -r.np if r.np < ncu else None
    if rel == "wide_eq":
        return 0 if lc.Cout % 64 == 0 and k == ncu else None
    if rel == "wide_lt":
        return -k if lc.Cout % 64 == 0 and k < ncu else None
    assert rel == "any"
    return 0


def generate(target, ncu):
    """the smallest tensor that reaches the target at this CU count, or None.  Search order: the primary key of `rel`, then the cost
    voxels x input channels x output channels of the wrapper's plain definition, then the fixed order of _grids() and of the channel
    counts: the same row on every machine."""
    where = dict(target.where)
    key = (target.planar, bool(where.get("cube")), target.f32)
    if key not in _GRID_CACHE:
        _GRID_CACHE[key] = _grids(*key)
    chans = CHANNELS_F32 if target.f32 else CHANNELS
    c1s = (where["C1"],) if "C1" in where else (0,)
    memo, cand = {}, []
    for order, ((N, D, H, W, tps, compact), Cout, C1) in enumerate(itertools.product(_GRID_CACHE[key], chans, c1s)):
        if "N" in where and N != where["N"]:
            continue
        if "compact" in where and compact != where["compact"]:
            continue
        if where.get("odd_ntile") and not tps & 1:
            continue
        shape = _shape(target, where, chans, N, D, H, W, Cout, C1)
        if shape[0] * shape[1] * shape[2] * shape[3] > MAX_VOXELS:
            continue
        mk = (N * tps, compact, Cout)              # what a target's route depends on
        if mk not in memo:
            try:
                lc, r = _place(target, shape, ncu)
            except Refused:
                continue
            memo[mk] = None if r.inst != target.inst or (where.get("odd_grid") and r.grid % 8 == 0) else _primary(target.rel, r, lc, ncu)
        if memo[mk] is None:
            continue
        cand.append((memo[mk], shape[0] * shape[1] * shape[2] * shape[3] * (shape[4] + shape[5]) * shape[6], order, shape))
    for prim, cost, order, shape in sorted(cand):
        try:
            lc, r = _place(target, shape, ncu)
        except Refused:
            continue
        if r.inst == target.inst and _primary(target.rel, r, lc, ncu) == prim:
            return Row(target, shape, lc, r)
    return None


def _ws(nt, mode=0, res=False, asy=False, epi=-1, fh=None):
    s = "k_conv_fwd_ws<%d, %d, %s, %s, %d" % (nt, mode, _b(res), _b(asy), epi)
    return s + (">" if fh is None else ", %s>" % _b(fh))


def _sym(nt, pl, mode, res, fh=None):
    s = "k_conv_fwd_mfma<%d, %s, %d, %s" % (nt, _b(pl), mode, _b(res))
    return s + (">" if fh is None else ", false, %s>" % _b(fh))


def _targets():
    t = []
    for nt in (1, 2):
        w = "n%d" % nt
        thr = "wide_eq" if nt == 2 else "np_eq"           # a wide launch at k == ncu has np == ncu as well
        # ---- plain launches, 3-D, one source (fast halo)
        t += [T("plain-%s-%s" % (w, thr), "fwd", _ws(nt, fh=True), thr),
              T("mask-%s-%s" % (w, thr), "dgrad_mask", _ws(nt, fh=True), thr),
              T("logits-%s-%s" % (w, thr), "tail_logits", _ws(nt, fh=True), thr),
              T("pool-%s-%s" % (w, thr), "tail_pool", _ws(nt, fh=True), thr),
              T("pool+logits-%s-np_gt" % w, "tail_both", _ws(nt, fh=True), "np_gt"),          # both tails: no drain at any np
              T("pool+logits-%s-np_gt2" % w, "tail_both", _ws(nt, fh=True), "np_gt2")]
        for rel in ("np_gt", "np_gt2"):
            t += [T("plain-drain-%s-%s" % (w, rel), "fwd", _ws(nt, 0, False, True, 0, True), rel),
                  T("pool-drain-%s-%s" % (w, rel), "tail_pool", _ws(nt, 0, False, True, 0, True), rel),
                  T("mask-drain-%s-%s" % (w, rel), "dgrad_mask", _ws(nt, 0, False, True, 1, True), rel),
                  T("logits-drain-%s-%s" % (w, rel), "tail_logits", _ws(nt, 0, False, True, 2, True), rel)]
        # ---- plain launches with two sources / a fused up-sampled source (FH = false)
        t += [T("plain-2src-%s-%s" % (w, thr), "fwd", _ws(nt, fh=False), thr, C0=64, C1=32),
              T("plain-up-%s-%s" % (w, thr), "fwd_up", _ws(nt, fh=False), thr),
              T("mask-2src-%s-%s" % (w, thr), "fwd_mask", _ws(nt, fh=False), thr, C1=32)]
        for rel in ("np_gt", "np_gt2"):
            t += [T("plain-2src-drain-%s-%s" % (w, rel), "fwd", _ws(nt, 0, False, True, 0, False), rel, C0=64, C1=32),
                  T("plain-up-drain-%s-%s" % (w, rel), "fwd_up", _ws(nt, 0, False, True, 0, False), rel),
                  T("mask-2src-drain-%s-%s" % (w, rel), "fwd_mask", _ws(nt, 0, False, True, 1, False), rel, C1=32)]
        # ---- the residual (skip) launch of the parity form
        t += [T("res-%s-%s" % (w, thr), "upcat", _ws(nt, 0, True, False, -1, True), thr, which=1),
              T("res-b27-%s-%s" % (w, thr), "bias27", _ws(nt, 0, True, False, -1, True), thr, which=1)]
        for rel in ("np_gt", "np_gt2"):
            t += [T("res-drain-%s-%s" % (w, rel), "upcat", _ws(nt, 0, False, True, 3, True), rel, which=1),
                  T("res-b27-drain-%s-%s" % (w, rel), "bias27", _ws(nt, 0, False, True, 3, True), rel, which=1)]
        # ---- normalisation tails (drain only)
        for rel in ("np_gt", "np_gt2"):
            t += [T("stats-%s-%s" % (w, rel), "stats", _ws(nt, 0, False, True, 4), rel),
                  T("res-stats-%s-%s" % (w, rel), "upcat_stats", _ws(nt, 0, False, True, 6), rel, which=1),
                  T("dgrad-norm-%s-%s" % (w, rel), "dgrad_norm", _ws(nt, 0, False, True, 5), rel)]
        # ---- the parity modes: not split by np; the wide threshold, and one launch with several items per workgroup
        wthr = "wide_eq" if nt == 2 else "wide_lt"
        t += [T("upfwd-%s-%s" % (w, wthr), "upcat", _ws(nt, 1, False, False, -1, True), wthr),
              T("upfwd-%s-np_gt2" % w, "upcat", _ws(nt, 1, False, False, -1, True), "np_gt2"),
              T("upbwd-%s-%s" % (w, wthr), "upcat_dgrad", _ws(nt, 2, False, False, -1, True), wthr),
              T("upbwd-mask-%s-np_gt" % w, "upcat_dgrad_mask", _ws(nt, 2, False, False, -1, True), "np_gt"),
              T("stride2-%s-%s" % (w, wthr), "stride2", _ws(nt, 2, False, False, -1, True), wthr)]
        # ---- the 8x8x8 tiling
        t += [T("cube-%s-%s" % (w, wthr), "fwd", "k_conv_fwd_mfma<%d, false, 0, false, true>" % nt, wthr, cube=True),
              T("cube-2src-%s-np_gt" % w, "fwd", "k_conv_fwd_mfma<%d, false, 0, false, true>" % nt, "np_gt", cube=True, C1=32)]
        # ---- 2-D slices
        t += [T("2d-plain-%s-%s" % (w, wthr), "fwd", _sym(nt, True, 0, False, True), wthr, planar=True),
              T("2d-plain-2src-%s-%s" % (w, wthr), "fwd", _sym(nt, True, 0, False, False), wthr, planar=True, C1=32),
              T("2d-mask-%s-np_gt" % w, "dgrad_mask", _sym(nt, True, 0, False, True), "np_gt", planar=True),
              T("2d-pool-%s-%s" % (w, wthr), "tail_pool", "k_conv_fwd_mfma<%d, true, 0, false, false, true, true>" % nt, wthr, planar=True),
              T("2d-pool+logits-%s-np_gt" % w, "tail_both", "k_conv_fwd_mfma<%d, true, 0, false, false, true, true>" % nt, "np_gt", planar=True),
              T("2d-res-%s-%s" % (w, wthr), "upcat", _sym(nt, True, 0, True, True), wthr, planar=True, which=1),
              T("2d-upfwd-%s-%s" % (w, wthr), "upcat", _sym(nt, True, 1, False), wthr, planar=True),
              T("2d-upbwd-%s-%s" % (w, wthr), "upcat_dgrad_mask", _sym(nt, True, 2, False), wthr, planar=True)]
    # ---- just below the wide threshold on the routes split by np as well: Cout % 64 == 0 on 32-wide blocks (np = 2k > ncu: the drains)
    t += [T("plain-drain-n1-wide_lt", "fwd", _ws(1, 0, False, True, 0, True), "wide_lt"),
          T("mask-drain-n1-wide_lt", "dgrad_mask", _ws(1, 0, False, True, 1, True), "wide_lt"),
          T("plain-2src-drain-n1-wide_lt", "fwd", _ws(1, 0, False, True, 0, False), "wide_lt", C1=32),
          T("mask-2src-drain-n1-wide_lt", "fwd_mask", _ws(1, 0, False, True, 1, False), "wide_lt", C1=32),
          T("res-drain-n1-wide_lt", "upcat", _ws(1, 0, False, True, 3, True), "wide_lt", which=1),
          T("stats-n1-wide_lt", "stats", _ws(1, 0, False, True, 4), "wide_lt"),
          T("res-stats-n1-wide_lt", "upcat_stats", _ws(1, 0, False, True, 6), "wide_lt", which=1),
          T("dgrad-norm-n1-wide_lt", "dgrad_norm", _ws(1, 0, False, True, 5), "wide_lt")]
    # ---- the item-to-item carry, across the table
    t += [T("plain-n1-odd-grid", "fwd", _ws(1, fh=True), "np_lt", odd_grid=True),              # grid % 8 != 0 needs np < ncu: no drain there
          T("plain-2src-n1-odd-grid", "fwd", _ws(1, fh=False), "np_lt", odd_grid=True, C1=32),
          T("plain-drain-n2-compact-N3", "fwd", _ws(2, 0, False, True, 0, True), "np_gt", N=3, compact=True),
          T("stats-n1-compact-N3", "stats", _ws(1, 0, False, True, 4), "np_gt2", N=3, compact=True),
          T("dgrad-norm-n2-compact-N3", "dgrad_norm", _ws(2, 0, False, True, 5), "np_gt", N=3, compact=True),
          T("res-drain-n1-compact-N3", "upcat", _ws(1, 0, False, True, 3, True), "np_gt", which=1, N=3, compact=True),
          T("mask-drain-n2-linear-odd-N3", "dgrad_mask", _ws(2, 0, False, True, 1, True), "np_gt", N=3, compact=False, odd_ntile=True),
          T("plain-2src-drain-n1-linear-odd-N3", "fwd", _ws(1, 0, False, True, 0, False), "np_gt2", N=3, compact=False, odd_ntile=True,
            C0=96, C1=32),
          T("plain-up-drain-n2-compact-N3", "fwd_up", _ws(2, 0, False, True, 0, False), "np_gt", N=3, compact=True),
          T("upfwd-n1-linear-odd-N3", "upcat", _ws(1, 1, False, False, -1, True), "np_gt", N=3, compact=False, odd_ntile=True)]
    # ---- fp32: every site at np <= ncu (np == ncu) and at np > ncu
    f = lambda mode, epi, fh: "k_conv_fwd_ws<1, %d, false, %s, %d, %s, true>" % (mode, _b(mode == 0), epi, _b(fh))
    for rel in ("np_eq", "np_gt"):
        t += [T("f32-plain-%s" % rel, "fwd", f(0, 0, True), rel, f32=True),
              T("f32-plain-2src-%s" % rel, "fwd", f(0, 0, False), rel, f32=True, C1=16),
              T("f32-plain-up-%s" % rel, "fwd_up", f(0, 0, False), rel, f32=True),
              T("f32-pool-%s" % rel, "tail_pool", f(0, 0, True), rel, f32=True),
              T("f32-mask-%s" % rel, "dgrad_mask", f(0, 1, True), rel, f32=True),
              T("f32-mask-2src-%s" % rel, "fwd_mask", f(0, 1, False), rel, f32=True, C1=16),
              T("f32-res-%s" % rel, "upcat", f(0, 3, True), rel, f32=True, which=1),
              T("f32-res-b27-%s" % rel, "bias27", f(0, 3, True), rel, f32=True, which=1),
              T("f32-upfwd-%s" % rel, "upcat", f(1, -1, True), rel, f32=True),
              T("f32-upbwd-%s" % rel, "upcat_dgrad_mask", f(2, -1, True), rel, f32=True),
              T("f32-stride2-%s" % rel, "stride2", f(2, -1, True), rel, f32=True)]
    t += [T("f32-plain-np_gt2-compact-N3", "fwd", f(0, 0, True), "np_gt2", f32=True, N=3, compact=True),
          T("f32-res-np_gt2", "upcat", f(0, 3, True), "np_gt2", f32=True, which=1)]
    names = [x.name for x in t]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
    return t


TARGETS = _targets()


def rows(ncu):
    """[(target, Row or None)] at this CU count"""
    return [(t, generate(t, ncu)) for t in TARGETS]


_ROWS = {}


def rows_cached(ncu):
    if ncu not in _ROWS:
        _ROWS[ncu] = rows(ncu)
    return _ROWS[ncu]


ROWS = TARGETS          # the table: one target per row; generate(target, ncu) places it on a device

# Environment-switched arms (read once per process): the switch, and the route() keywords it stands for
ARMS = {"FMRI_FWD_WS": {"use_ws": False}, "FMRI_RES_ASYNC": {"res_async": False}, "FMRI_F32_MFMA": {"f32_mfma": False}}

# Instantiations behind a launch site that no public entry point reaches, with the line of the API that excludes them
_RES_ONE_SOURCE = ("conv3d_api.hip upcat_fwd / fmri_conv3d_upcat_fwd_bias27 / fmri_conv3d_upcat_fwd_stats: every residual launch is "
                   "conv3d_fwd_mfma_ex(0, src1, C1, 0, planar, nullptr, 0, ...) - one plain source, so FH is true")
UNREACHABLE = {}
for _nt in (1, 2):
    UNREACHABLE[("bf16", _ws(_nt, 0, False, True, 3, False))] = _RES_ONE_SOURCE
    UNREACHABLE[("bf16", _ws(_nt, 0, True, False, -1, False))] = _RES_ONE_SOURCE
    UNREACHABLE[("bf16", _sym(_nt, True, 0, True, False))] = _RES_ONE_SOURCE
    UNREACHABLE[("bf16", _sym(_nt, False, 0, True, False))] = _RES_ONE_SOURCE
    UNREACHABLE[("bf16", _ws(_nt, 0, False, True, 2, False))] = (
        "conv3d_mfma.hip conv3d_fwd_mfma_tail: the only caller that sets FwdTail::logits launches (0, src0, C0, 0, planar, nullptr, 0, ...) - "
        "one plain source, so FH is true")
UNREACHABLE[("f32", "k_conv_fwd_ws<1, 0, false, true, 3, false, true>")] = _RES_ONE_SOURCE
