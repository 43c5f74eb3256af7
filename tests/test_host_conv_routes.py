"""tests/conv_routes.py against the source it restates, on the CPU: every FMRI_FWD(...) launch site of csrc/conv3d_mfma.hip, expanded to
its kernel instantiations, is either the route of a row of the table or listed as unreachable (a launch site added later fails here until
it has a row); the generated rows sit where they claim to at three CU counts; and the reference the GPU test compares with is exact."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import conv_routes as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "fetal-mri-segmentation_amd", "csrc", "conv3d_mfma.hip")


def source_instantiations():
    """{(launcher, instantiation)} and the number of launch sites: by_width and fwd_choose expanded textually (NT / decltype(nt)::value ->
    1, 2; FH -> true, false)"""
    text = open(SRC).read()
    a, b = text.index("static int conv3d_fwd_mfma_launch_f32("), text.index("static int conv3d_fwd_mfma_launch(")
    end = text.index("#undef FMRI_FWD")
    out, sites = set(), 0
    for launcher, body in (("f32", text[a:b]), ("bf16", text[b:end])):
        for m in re.finditer(r"FMRI_FWD\((k_conv_fwd_\w+<[^;]*>)\);", body):
            sites += 1
            variants = [m.group(1).replace("decltype(nt)::value", "NT")]
            for name, values in (("NT", ("1", "2")), ("FH", ("true", "false"))):
                if any(re.search(r"\b%s\b" % name, v) for v in variants):
                    variants = [re.sub(r"\b%s\b" % name, val, v) for v in variants for val in values]
            out.update((launcher, v) for v in variants)
    assert text.count("FMRI_FWD(") == sites + 1, "a launch site this parser does not read"          # + the macro's definition
    return out, sites


def census(ncu):
    """(launcher, instantiation) -> [(row name, arm)]: every launch of every placed row, in the default process and in the arms whose
    switch changes the launch"""
    seen = {}
    for t, row in CR.rows_cached(ncu):
        if row is None:
            continue
        for arm, kw in [("default", {})] + [(a, k) for a, k in CR.ARMS.items() if a != "FMRI_F32_MFMA"]:
            try:
                ls = CR.launches(t.op, t.f32, t.planar, *row.shape, ncu=ncu, use_ws=kw.get("use_ws", True))
                if t.op == "bias27" and not kw.get("use_ws", True):
                    continue
                for lc in ls:
                    r = CR.route_of(lc, t.f32, ncu, **kw)
                    seen.setdefault(("f32" if t.f32 else "bf16", r.inst), []).append((t.name, arm))
            except CR.Refused:
                continue
    return seen


def test_every_launch_site_has_a_row_or_a_reason():
    src, sites = source_instantiations()
    assert sites == 26 and len(src) == 70, (sites, len(src))          # 27 occurrences of FMRI_FWD( with the macro itself
    seen = census(256)
    unreachable = set(CR.UNREACHABLE)
    assert not unreachable & set(seen), "listed as unreachable, yet a row reaches it: %s" % sorted(unreachable & set(seen))
    assert src - set(seen) - unreachable == set(), "launch sites without a row: %s" % sorted(src - set(seen) - unreachable)
    assert (set(seen) | unreachable) - src == set(), "not in the source: %s" % sorted((set(seen) | unreachable) - src)
    for key in src - unreachable:              # reached by a TARGET row (not only in passing, as the other launch of a two-launch wrapper)
        targeted = [t for t, row in CR.rows_cached(256) if row is not None and (("f32" if t.f32 else "bf16"), t.inst) == key]
        assert targeted or all(arm != "default" for _, arm in seen[key]), key
    for reason in CR.UNREACHABLE.values():
        assert "conv3d_api.hip" in reason or "conv3d_mfma.hip" in reason


def _k(row):
    lc = row.launch
    return row.route.ntile * (lc.Cout // 64) * ((4 if lc.planar else 8) if lc.mode == 1 else 1)


@pytest.mark.parametrize("ncu", [256, 304, 64])
def test_generated_rows_sit_where_they_claim(ncu):
    placed = [(t, r) for t, r in CR.rows_cached(ncu) if r is not None]
    missing = [t.name for t, r in CR.rows_cached(ncu) if r is None]
    assert len(missing) * 10 <= len(CR.ROWS) and (ncu != 256 or not missing), missing
    for t, row in placed:
        r, lc, where = row.route, row.launch, dict(t.where)
        N, D, H, W, C0, C1, Cout = row.shape
        assert r.inst == t.inst and r.grid == min(r.np, ncu), t.name
        assert N * D * H * W <= CR.MAX_VOXELS and set((C0, C1, Cout)) <= set(CR.CHANNELS_F32 if t.f32 else CR.CHANNELS) | {0}, t.name
        assert (r.np == ncu if t.rel == "np_eq" else r.np > ncu if t.rel == "np_gt" else r.np > 2 * ncu if t.rel == "np_gt2" else
                r.np < ncu if t.rel == "np_lt" else (_k(row) == ncu and r.wide) if t.rel == "wide_eq" else
                (lc.Cout % 64 == 0 and _k(row) < ncu and not r.wide)), (t.name, r)
        if t.rel == "np_gt2":
            assert -(-r.np // r.grid) >= 3, t.name                 # some workgroup handles a third item
        if "N" in where:
            assert N == where["N"], t.name
        if "compact" in where:
            assert r.compact == where["compact"], t.name
        if where.get("odd_ntile"):
            assert (r.ntile // N) % 2 == 1, t.name
        if where.get("odd_grid"):
            assert r.grid % 8 != 0 and not r.drain, t.name            # np < ncu: never a drain
        # decode() restated: the pairs tile the output exactly once
        if r.np <= 600 and lc.mode != 1:
            tiles = set(CR.tile_of_pair(r, p, lc.mode, lc.planar, lc.N, lc.D, lc.H, lc.W, lc.Cout) for p in range(r.np))
            assert len(tiles) == r.np and all(0 <= n < lc.N and d0 + r.tile[0] <= lc.D and h0 + r.tile[1] <= lc.H and w0 + r.tile[2] <= lc.W
                                              for n, d0, h0, w0, _, _ in tiles), t.name


def test_the_table_covers_what_the_thresholds_split():
    """at 256 CUs: both sides of np > ncu and of fwd_wide for every instantiation they split, a third item on every drain route, and the
    carries between items across the table"""
    rows = [(t, r) for t, r in CR.rows_cached(256) if r is not None]
    by_inst = {}
    for t, r in rows:
        by_inst.setdefault((t.f32, t.inst), []).append((t, r))
    drains = {k for k, v in by_inst.items() if not k[0] and any(r.route.drain for _, r in v)}
    assert len(drains) == 18                       # EPI 0, 1 x NT x FH; EPI 2, 3 x NT; EPI 4, 5, 6 x NT
    for k in drains:
        rels = {t.rel for t, _ in by_inst[k]}
        assert {"np_gt", "np_gt2"} <= rels, k
        # the other side: the same wrapper at np == ncu (normalisation tails: the entry point refuses there)
        for op in {t.op for t, _ in by_inst[k]} - {"stats", "upcat_stats", "dgrad_norm"}:
            assert any(t.op == op and r.route.np == 256 and not r.route.drain for t, r in rows), (k, op)
    for (f32, inst), v in by_inst.items():
        if f32:
            continue
        if re.match(r"k_conv_fwd_\w+<2,", inst) and (False, inst) not in drains:
            assert any(_k(r) == 256 for _, r in v), inst              # wide by the >=
        if re.match(r"k_conv_fwd_\w+<1,", inst):
            # just below: 32-wide blocks on a Cout that 64 divides.  Not reachable on the non-drain plain / residual 3-D kernels (np = 2k <= ncu
            # means k <= ncu / 2: their rows at np == ncu stand in) nor with the logits (Cout == 32)
            if re.search(r"ws<1, 0, (false|true), false, -1|ws<1, 0, false, true, 2", inst):
                continue
            assert any(t.rel == "wide_lt" for t, _ in v), inst
    dr = [(t, r) for t, r in rows if r.route.drain and not t.f32]
    assert any(r.route.compact and r.shape[0] == 3 for _, r in dr)
    assert any(not r.route.compact and (r.route.ntile // r.shape[0]) % 2 == 1 for _, r in dr)
    assert any(r.launch.C1 and r.launch.C0 != r.launch.C1 for _, r in dr)
    assert any(r.launch.up0 for _, r in dr)
    assert any(r.route.grid % 8 for _, r in rows)
    # fp32: every site on both sides of np > ncu, and bias27 with its residual in both types
    for inst in {t.inst for t, _ in rows if t.f32}:
        sides = {r.route.np > 256 for t, r in rows if t.f32 and t.inst == inst}
        assert sides == {False, True}, inst
    for f32 in (False, True):
        assert {r.route.np > 256 for t, r in rows if t.op == "bias27" and t.f32 == f32} == {False, True}
    # every planar instantiation of the source is a TARGET of a row
    src, _ = source_instantiations()
    for launcher, inst in src - set(CR.UNREACHABLE):
        if re.match(r"k_conv_fwd_mfma<\d, true", inst):
            assert any(t.inst == inst and t.planar for t, _ in rows), inst


def _exact_units(row):
    """the largest |partial sum| of any launch of the row, in units of its smallest product (plus the bias): 27 taps x input channels x
    max|x| x max|w|; the up-backward launch sums the 8 children of a low-resolution voxel on top"""
    t = row.target
    N, D, H, W, C0, C1, Cout = row.shape
    if t.op in ("dgrad", "dgrad_mask", "dgrad_norm"):
        return 27 * C0 * 2 * 2                                    # dy k/2 (|k| <= 2) x w k/8 (|k| <= 2), unit 1/16
    if t.op.startswith("upcat_dgrad"):
        return 8 * 27 * Cout * 2 * 2
    return 27 * (C0 + C1) * 4 * 2 + 8 * 4                         # x k/4 (|k| <= 4) x w k/8 (|k| <= 2), unit 1/32; bias k/4 = 8 units each


def test_every_partial_sum_is_exact_in_fp32():
    for ncu in (256, 304, 64):
        for t, row in CR.rows_cached(ncu):
            if row is not None:
                assert _exact_units(row) < 1 << 24, t.name


def test_torch_fp32_cpu_convolution_is_exact_on_this_data():
    """the three rows with the most input channels: torch's fp32 CPU convolution, forward and backward, equals the fp64 one bit for bit"""
    rows = [r for _, r in CR.rows_cached(256) if r is not None and r.target.op in ("fwd", "fwd_mask", "stats")]
    rows.sort(key=lambda r: (-(r.shape[4] + r.shape[5]), r.shape[0] * r.shape[1] * r.shape[2] * r.shape[3] * r.shape[6]))
    assert rows[0].shape[4] + rows[0].shape[5] >= 128
    for row in rows[:3]:
        N, D, H, W, C0, C1, Cout = row.shape
        g = torch.Generator().manual_seed(N + D + H + W + C0 + C1 + Cout)
        x = (torch.randint(-4, 5, (N, C0 + C1, D, H, W), generator=g).float() / 4).requires_grad_(True)
        w = (torch.randint(-2, 3, (Cout, C0 + C1, 3, 3, 3), generator=g).float() / 8).requires_grad_(True)
        b = torch.randint(-4, 5, (Cout,), generator=g).float() / 4
        dy = torch.randint(-2, 3, (N, Cout, D, H, W), generator=g).float() / 2
        y = F.conv3d(x, w, b, padding=1)
        y.backward(dy)
        x64, w64 = x.detach().double().requires_grad_(True), w.detach().double().requires_grad_(True)
        y64 = F.conv3d(x64, w64, b.double(), padding=1)
        y64.backward(dy.double())
        assert torch.equal(y.detach().double(), y64.detach()), row.target.name
        assert torch.equal(x.grad.double(), x64.grad), row.target.name
