#!/usr/bin/env python3
"""Timing of what norm_net_model adds (one MI355X; device events around many launches, both arms in one process, alternating):

  kernel  fmri_conv3d_first_dgrad against fmri_conv3d_dgrad(impl = GENERIC) - the only way to this tensor before the kernel existed - at
          4 x 64x128x128, Cout = 32, Cin = 1, on dyadic data (both results are exact: the new fp32 one, rounded to bf16, must equal the
          generic one bit for bit).  The floor is one read of dy, 268 MB.
  step    one NormNet training step: isensee2017_model_3d depth 5 / 16 filters with a linear output in front of the configs[1] U-Net
          (depth 4 / 32 filters), batch 2 x 64x128x128, bf16, with the first-layer kernel and with FMRI_FIRST_DGRAD=0 (a child process per
          arm, alternating: the switch is read when the engine is built).

usage: bench_norm_net.py [--iters 50] [--rounds 5] [--steps 10] [--skip-step]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fetal-mri-segmentation_amd"))
sys.path.insert(0, ROOT)


def _time(f, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def kernel(iters, rounds):
    import torch
    from fmri_hip import ops
    from fmri_hip._lib import IMPL_GENERIC
    N, D, H, W, Cout, Cin = 4, 64, 128, 128, 32, 1
    g = torch.Generator(device="cuda").manual_seed(7)
    dy = (torch.randint(-4, 5, (N, D, H, W, Cout), generator=g, device="cuda").float() / 4).to(torch.bfloat16)
    w = (torch.randint(-2, 3, (27, Cout, Cin), generator=g, device="cuda").float() / 8).to(torch.bfloat16)
    wd = w.flip(0).transpose(1, 2).contiguous()
    dx = torch.empty((N, D, H, W, Cin), dtype=torch.float32, device="cuda")
    old = torch.empty((N, D, H, W, Cin), dtype=torch.bfloat16, device="cuda")
    arms = {"first_dgrad": lambda: ops.conv3d_first_dgrad(dy, w, dx), "generic": lambda: ops.conv3d_dgrad(dy, wd, old, impl=IMPL_GENERIC)}
    for f in arms.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    same = bool(torch.equal(dx.to(torch.bfloat16), old))
    t = {k: [] for k in arms}
    for _ in range(rounds):
        for k, f in arms.items():
            t[k].append(_time(f, iters))
    mb = dy.numel() * 2 / 1e6
    out = {"shape": [N, D, H, W, Cout, Cin], "dy_MB": mb, "results_equal_after_bf16_rounding": same}
    for k, v in t.items():
        out[k] = {"us_min": min(v) * 1e3, "us_max": max(v) * 1e3, "TBps_of_dy_at_min": mb / min(v) / 1e3}
    return out


def step(steps):
    import numpy as np
    import torch
    import fetal_net.model as fmodel
    sp, N = (64, 128, 128), 2
    seg = fmodel.unet_model_3d((1,) + sp, depth=4, n_base_filters=32, compute_dtype="bf16")
    model = fmodel.norm_net_model((1,) + sp, n_base_filters=16, depth=5, n_segmentation_levels=3, old_model_path=seg, compute_dtype="bf16")
    eng = model.engine(N)
    x = torch.randn((N,) + sp + (1,), device="cuda").to(eng.dtype)
    y = (torch.rand(N * int(np.prod(sp)), device="cuda") < 0.3).to(torch.uint8)
    for _ in range(3):
        eng.train_step(x, y, 1e-4)
    torch.cuda.synchronize()
    ms = _time(lambda: eng.train_step(x, y, 1e-4), steps)
    loss = eng.metrics_from_sums(eng.sums.cpu().numpy())["loss"]
    return {"route": eng.seg.route["first_dgrad"], "ms_per_step": ms, "loss_finite": bool(np.isfinite(loss))}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(step(a.steps)))
        sys.exit(0)
    print("kernel " + json.dumps(kernel(a.iters, a.rounds)), flush=True)
    if not a.skip_step:
        res = {"first": [], "generic": []}
        for rd in range(2):
            for arm, sw in (("first", "1"), ("generic", "0")):
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--steps", str(a.steps)],
                                     env=dict(os.environ, FMRI_FIRST_DGRAD=sw), capture_output=True, text=True, timeout=280)
                if out.returncode != 0:
                    print(out.stdout[-2000:], out.stderr[-4000:])
                    sys.exit(out.returncode)                  # nothing more is started on the device after a failure
                r = json.loads([l for l in out.stdout.splitlines() if l.startswith("RESULT ")][0][7:])
                assert r["route"] == arm, r
                res[arm].append(r["ms_per_step"])
        print("step " + json.dumps({k: {"ms_min": min(v), "ms_max": max(v)} for k, v in res.items()}), flush=True)
