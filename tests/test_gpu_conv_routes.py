"""Every forward / input-gradient conv route at its dispatch thresholds (csrc/conv3d_mfma.hip: seventy kernel instantiations behind 26
FMRI_FWD launch sites).  tests/conv_routes.py restates the dispatch rule and lists, per instantiation, tensors on both sides of the
thresholds that select it (np == ncu against np > ncu, 64-wide blocks at k == ncu against just below, a third item per workgroup, grids that
are no multiple of 8, compact and linear tile numbering, items that cross samples).  Each row here

  1. is placed for the CU count of THIS device, and the restatement is checked against the library's own predicates before it is trusted;
  2. goes through the public wrapper that reaches it, with the outputs pre-filled with NaN;
  3. must equal the plain definition BIT FOR BIT: the data are small dyadic numbers (activations k/4, weights k/8, gradients k/2, biases
     k/4), every product and partial sum is exact in fp32, so neither the order of summation nor the route can change a result.  bf16
     outputs are the definition rounded once; the parity form with a skip source has its two documented intermediate roundings; logits,
     pooled copies, the normalisation sums and fp32 outputs are exact.  There is no tolerance in this file.

A failing row names the restated instantiation, ntile, np, grid and the first differing element with its tile and item number."""
import json
import os
import subprocess
import sys

import pytest
import torch

import conv_routes as CR
import conv_routes_gpu as RG

pytestmark = pytest.mark.gpu

_FAULT = []          # the row at which the device reported an error, if any
_DIGESTS = {}        # row name -> {output: sha256}: the default arm, for the environment-switched arms below


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the GPU box"
    from fmri_hip import ops as o
    return o


def cross_check(ops, row, ncu):
    """the restatement against the library's predicates, for every launch of the row's wrapper; a disagreement is a failure of the row"""
    from fmri_hip._lib import lib, BF16, F32
    t = row.target
    dt = torch.float32 if t.f32 else torch.bfloat16
    N, D, H, W, C0, C1, Cout = row.shape
    for lc in CR.launches(t.op, t.f32, t.planar, *row.shape, ncu=ncu):
        r = CR.route_of(lc, t.f32, ncu)
        uses = lib().fmri_conv3d_uses_mfma(lc.C0, lc.C1, lc.Cout, lc.D, lc.H, lc.W, F32 if t.f32 else BF16)
        assert uses & 1, "%s: the library keeps launch %s off the MFMA forward kernels" % (t.name, (lc,))
        assert not uses & 4 and not CR.first_layer(lc.C0, lc.C1), "%s: a first-layer launch" % t.name
        if lc.mode == 0 and not lc.planar and not t.f32 and not r.cube:
            plain = CR.route("bf16", 0, False, lc.N, lc.D, lc.H, lc.W, lc.C0, lc.C1, lc.up0, lc.Cout, False, False, (), ncu)
            got = ops.conv3d_fwd_ntail_ok(lc.C0, lc.C1, lc.Cout, lc.N, lc.D, lc.H, lc.W, dt)
            assert got == (plain.np > ncu), "%s: fmri_conv3d_fwd_ntail_ok says %s, the restatement np = %d against %d CUs" % (t.name, got, plain.np, ncu)
        if lc.mode == 0 and lc.Cout == 64 and lc.C1 == 0 and not lc.up0 and not t.f32 and not r.cube:
            bits = ops.conv3d_fwd_tail_ok(lc.C0, 64, lc.N, lc.D, lc.H, lc.W, dt, planar=lc.planar)
            wide = CR.fwd_wide(0, lc.planar, r.ntile, 64, ncu)
            assert bool(bits & 2) == wide, "%s: fmri_conv3d_fwd_tail_ok = %d, the restatement wide = %s (ntile %d)" % (t.name, bits, wide, r.ntile)
    if t.op in ("upcat", "upcat_stats", "bias27", "upcat_dgrad", "upcat_dgrad_mask"):
        assert ops.conv3d_upcat_ok(C0, C1, Cout, D, H, W, dt, planar=bool(t.planar)) & 1, "%s: fmri_conv3d_upcat_ok denies the row" % t.name
    if t.op == "stride2":
        assert ops.conv3d_upcat_ok(Cout, 0, C0, D, H, W, dt) & 1, "%s: fmri_conv3d_upcat_ok denies the row" % t.name
    if t.op in ("tail_pool", "tail_logits", "tail_both"):
        bits = ops.conv3d_fwd_tail_ok(C0, Cout, N, D, H, W, dt, planar=bool(t.planar))
        assert bits & 1 and (t.op == "tail_pool" or bits & 2), "%s: fmri_conv3d_fwd_tail_ok = %d denies the row" % (t.name, bits)


def describe(row, name, idx):
    """where the first differing element was computed: launch coordinates, pair, tile, item number of its workgroup"""
    r, lc = row.route, row.launch
    s = "%s  ntile %d np %d grid %d %s numbering, shape %s; first difference: %s%s" % (
        r.inst, r.ntile, r.np, r.grid, "compact" if r.compact else "linear", (row.shape,), name, (idx,))
    out_of_target = {"y": True, "dx": True, "pool": False, "logits": False, "sums": False, "slots": False,
                     "dx_low": row.target.which == 0, "dx_skip": row.target.which == 1}[name]
    if not out_of_target or len(idx) != 5:
        return s
    n, d, h, w, c = idx
    par = 0
    if lc.mode == 1:                  # the scatter: output voxel 2g + p belongs to low-resolution voxel g, parity class p
        par = ((0 if lc.planar else d % 2) * 2 + h % 2) * 2 + w % 2
        d, h, w = (d if lc.planar else d // 2), h // 2, w // 2
    bn = 64 if r.wide else 32
    for pair in range(r.np):
        tn, d0, h0, w0, co0, p = CR.tile_of_pair(r, pair, lc.mode, lc.planar, lc.N, lc.D, lc.H, lc.W, lc.Cout)
        if tn == n and d0 <= d < d0 + r.tile[0] and h0 <= h < h0 + r.tile[1] and w0 <= w < w0 + r.tile[2] and co0 <= c < co0 + bn and p == par:
            return s + "; tile (n %d, d0 %d, h0 %d, w0 %d, co0 %d, parity %d) = pair %d: item %d of its workgroup" % (tn, d0, h0, w0, co0, p, pair, pair // r.grid)
    return s


def compare(row, out, ref):
    assert set(out) == set(ref), (sorted(out), sorted(ref))
    for name in sorted(out):
        idx, n = RG.first_difference(out[name], ref[name])
        if idx is not None:
            raise AssertionError("%s: %d of %d elements of %s differ (got %r, want %r)\n%s" % (
                row.target.name, n, out[name].numel(), name, float(out[name][idx]), float(ref[name][idx]), describe(row, name, idx)))


@pytest.mark.parametrize("target", CR.ROWS, ids=[t.name for t in CR.ROWS])
def test_conv_route_is_exact_on_dyadic_data(ops, target):
    ncu = RG.ncu_of_device()
    row = {t.name: r for t, r in CR.rows_cached(ncu)}[target.name]
    if row is None:
        assert ncu != 256, "%s: no tensor reaches the route on a 256-CU device" % target.name
        pytest.skip("%s: the generator cannot place this row on %d CUs" % (target.name, ncu))
    assert row.route.inst == target.inst
    assert not _FAULT, "an earlier row left the device in an error state (%s): no further row is started" % _FAULT[0]
    cross_check(ops, row, ncu)
    try:
        out, ref = RG.run_row(ops, row)
    except RuntimeError as e:
        if "HIP error" in str(e) or "hipError" in str(e) or "illegal memory access" in str(e):
            _FAULT.append(target.name)
        raise
    _DIGESTS[target.name] = {k: RG.digest(v) for k, v in out.items() if k not in ("sums", "slots")}
    if "sums" in out:
        # dense filters: the sums exceed what fp32 partial sums hold exactly - the tensor is checked here, the sums in the sparse run below
        out = {k: v for k, v in out.items() if k not in ("sums", "slots")}
        ref = {k: v for k, v in ref.items() if k not in ("sums", "slots")}
    compare(row, out, ref)
    if target.op in ("stats", "upcat_stats", "dgrad_norm"):
        assert RG.sums_exact_bound(row) < 1 << 24
        out, ref = RG.run_row(ops, row, sparse=True)
        compare(row, out, ref)


def test_few_rows_are_skipped_on_this_device():
    ncu = RG.ncu_of_device()
    missing = [t.name for t, r in CR.rows_cached(ncu) if r is None]
    assert len(missing) * 10 <= len(CR.ROWS) and (ncu != 256 or not missing), (ncu, missing)


def _arm_rows(arm, ncu):
    """the rows whose route the switch changes, and that the switched library still takes"""
    kw = CR.ARMS[arm]
    names = []
    for t, row in CR.rows_cached(ncu):
        if row is None:
            continue
        if arm == "FMRI_F32_MFMA":
            # fmri_conv3d_fwd / _dgrad fall back to the VALU kernels of conv3d_generic.hip; the tails and the parity form have no fp32 form
            # without the MFMA kernels (fmri_conv3d_fwd_tail_ok / fmri_conv3d_upcat_ok answer 0 there)
            if t.f32 and t.op in ("fwd", "fwd_up", "fwd_mask", "dgrad", "dgrad_mask"):
                names.append(t.name)
            continue
        if t.f32:
            continue
        try:
            ls = CR.launches(t.op, False, t.planar, *row.shape, ncu=ncu, use_ws=kw.get("use_ws", True))
            if t.op == "bias27" and not kw.get("use_ws", True):
                continue                       # conv3d_fwd_mfma_res_b27: only the warp-specialised kernel implements it
            changed = [CR.route_of(l, False, ncu, **kw).inst != CR.route_of(l, False, ncu).inst for l in ls]
        except CR.Refused:
            continue
        if any(changed):
            names.append(t.name)
    return names


def test_environment_switched_arms_are_bit_identical(ops, tmp_path):
    """FMRI_FWD_WS=0 (the symmetric kernel), FMRI_RES_ASYNC=0 (the residual added by the MFMA waves) and FMRI_F32_MFMA=0 (fp32 on the VALU
    kernels): the library reads these once per process, so each arm is a fresh child, one after another.  A child runs the rows whose
    route its switch changes; every output must equal the default arm's bit for bit (compared through sha256 digests)."""
    assert not _FAULT, "an earlier row left the device in an error state (%s)" % _FAULT[0]
    ncu = RG.ncu_of_device()
    rows = {t.name: r for t, r in CR.rows_cached(ncu) if r is not None}
    here = os.path.dirname(os.path.abspath(__file__))
    for arm in ("FMRI_FWD_WS", "FMRI_RES_ASYNC", "FMRI_F32_MFMA"):
        names = _arm_rows(arm, ncu)
        assert len(names) >= 4, (arm, names)
        for n in names:
            if n not in _DIGESTS:
                out, _ = RG.run_row(ops, rows[n], with_ref=False)
                _DIGESTS[n] = {k: RG.digest(v) for k, v in out.items() if k not in ("sums", "slots")}
        fin, fout = tmp_path / (arm + "_rows.json"), tmp_path / (arm + "_out.json")
        fin.write_text(json.dumps(names))
        r = subprocess.run([sys.executable, os.path.join(here, "conv_routes_gpu.py"), str(fin), str(fout)], capture_output=True, text=True,
                           timeout=300, env=dict(os.environ, **{arm: "0"}))
        assert r.returncode == 0 and "DONE %d rows" % len(names) in r.stdout, (arm, r.stdout[-1000:], r.stderr[-3000:])
        got = json.loads(fout.read_text())
        bad = [(n, k) for n in names for k in _DIGESTS[n] if got[n].get(k) != _DIGESTS[n][k]]
        assert not bad, "%s=0 changes the bits of %s" % (arm, bad)
        print("%s=0: %d rows bit-identical to the default arm" % (arm, len(names)))
