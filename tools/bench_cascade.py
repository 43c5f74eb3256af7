#!/usr/bin/env python3
"""2-D models with previous-slice truth channels (reference fetal/config_utils.py:128-131: 5 slices + 1 truth slice = 6 input channels) against
the plain 5-slice model, on every layer the option touches.  Prints one JSON line:
  first_layer   fwd / wgrad us per launch at 64 x 256x256 -> 32 channels, C0 = 5 and 6, impl AUTO (first-layer kernels) and GENERIC
  train_step    ms per step of the 2-D U-Net (depth 4 / 32 filters, batch 64, bf16) at 5 and 6 input channels
  prediction    s per patch_wise_prediction of a 160x256x256 volume (patch 64x64x5, overlap 0.5): no truth, truth on the device, truth through
                the host tiling (a duck-typed proxy of the same model)
  generator     ms per batch of 64 patches (64x64x5, reference default augmentation minus piecewise affine): no truth (batched), prev-truth
                batched and patch by patch
usage: python tools/bench_cascade.py [--skip-host]"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "fetal-mri-segmentation_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch

AUG = {"flip": [0.5, 0.5, 0.5], "permute": False, "translate": (15, 15, 7), "scale": (0.1, 0.1, 0), "rotate": (0, 0, 90), "poisson_noise": 1,
       "gaussian_filter": {"prob": 0.0, "max_sigma": 1}, "contrast": {"prob": 0, "min_factor": 0.2, "max_factor": 0.1},
       "elastic_transform": {"alpha": 5, "sigma": 10}, "coarse_dropout": {"rate": 0.2, "size_percent": [0.10, 0.30], "per_channel": True},
       "gaussian_noise": {"prob": 0.5, "sigma": 0.05}, "speckle_noise": {"prob": 0.5, "sigma": 0.05}}


def _time_us(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def first_layer():
    from fmri_hip import ops
    from fmri_hip._lib import IMPL_AUTO, IMPL_GENERIC
    S, H, W, Cout = 64, 256, 256, 32
    out = {}
    for C0 in (5, 6):
        x = (torch.randn((1, S, H, W, C0), device="cuda")).to(torch.bfloat16)
        w = (torch.randn((27, Cout, C0), device="cuda") * 0.2).to(torch.bfloat16)
        b = torch.zeros(Cout, device="cuda")
        y = torch.empty((1, S, H, W, Cout), device="cuda", dtype=torch.bfloat16)
        dy = torch.randn((1, S, H, W, Cout), device="cuda").to(torch.bfloat16)
        dw = torch.zeros((27, Cout, C0), device="cuda")
        db = torch.zeros(Cout, device="cuda")
        for name, impl, reps in (("auto", IMPL_AUTO, 50), ("generic", IMPL_GENERIC, 5)):
            out["c%d_%s_fwd_us" % (C0, name)] = _time_us(lambda: ops.conv3d_fwd(x, None, w, b, y, act=1, impl=impl, planar=True), reps)
            out["c%d_%s_wgrad_us" % (C0, name)] = _time_us(lambda: ops.conv3d_wgrad(x, None, dy, dw, db, impl=impl, planar=True), reps)
    out["c6_over_c5_fwd"] = out["c6_auto_fwd_us"] / out["c5_auto_fwd_us"]
    out["c6_over_c5_wgrad"] = out["c6_auto_wgrad_us"] / out["c5_auto_wgrad_us"]
    return out


def train_step(steps=20):
    import learnable_task as LT
    from fmri_hip.engine import UNetEngine, UNetPlan
    B, X, Y = 64, 256, 256
    out = {}
    for C in (5, 6, 5, 6):                                 # interleaved: the clock settles over the first legs
        eng = UNetEngine(UNetPlan(C, (X, Y), depth=4, n_base_filters=32, ndim=2), B, dtype=torch.bfloat16)
        pool = []
        for k in range(2):
            xb, yb = LT.device_batch_2d(5_000 + k * B, B, (X, Y), C)
            pool.append((xb.to(torch.bfloat16).unsqueeze(0).contiguous(), yb.reshape(-1).contiguous()))
        for i in range(10):
            eng.train_step(*pool[i % 2], 1e-4)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            eng.train_step(*pool[i % 2], 1e-4)
        torch.cuda.synchronize()
        out["c%d_ms" % C] = (time.perf_counter() - t0) / steps * 1e3        # the second leg of each count is kept
        del eng
    out["c6_over_c5"] = out["c6_ms"] / out["c5_ms"]
    return out


def prediction(skip_host):
    import fetal_net.model as fmodel
    from fetal_net.prediction import patch_wise_prediction
    rs = np.random.RandomState(0)
    data = rs.randn(1, 160, 256, 256).astype(np.float32)
    truth = (rs.rand(1, 160, 256, 256) > 0.7).astype(np.uint8)
    patch = (64, 64, 5)
    m5 = fmodel.unet_model_2d(input_shape=(64, 64, 5))
    m6 = fmodel.unet_model_2d(input_shape=(64, 64, 6))

    class Proxy:
        output_shape = m6.output_shape

        @staticmethod
        def predict(x):
            return m6.predict(x)

    def timed(model, reps, **kw):
        patch_wise_prediction(model, data, patch, overlap_factor=0.5, **kw)          # captures the graphs
        t = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            patch_wise_prediction(model, data, patch, overlap_factor=0.5, **kw)
            t.append(time.perf_counter() - t0)
        return min(t)

    tk = dict(truth_data=truth, prev_truth_index=1, prev_truth_size=1)
    out = {"no_truth_s": timed(m5, 3), "truth_device_s": timed(m6, 3, **tk)}
    out["truth_device_over_no_truth"] = out["truth_device_s"] / out["no_truth_s"]
    if not skip_host:
        t0 = time.perf_counter()
        patch_wise_prediction(Proxy(), data, patch, overlap_factor=0.5, **tk)
        out["truth_host_s"] = time.perf_counter() - t0
        out["host_over_device"] = out["truth_host_s"] / out["truth_device_s"]
    return out


def generator(batches=20):
    import learnable_task as LT
    from fetal_net.device_generator import DeviceDataFile, device_data_generator

    class Root:
        pass

    class Vols:
        def __init__(self, n, shape):
            v = [LT.host_patch(i, shape) for i in range(n)]
            self.root = Root()
            self.root.data, self.root.truth = [a[0] for a in v], [a[1] for a in v]
            self.root.subject_ids = [b"s"] * n

    patch = (64, 64, 5)
    ddf = DeviceDataFile(Vols(4, (96, 160, 160)), patch)
    out = {}
    for name, prev, batched in (("no_truth_batched", None, True), ("prev_truth_batched", 1, True), ("prev_truth_patch_by_patch", 1, False)):
        np.random.seed(0)
        random.seed(0)
        g = device_data_generator(ddf, list(range(4)), batch_size=64, patch_shape=patch, augment=AUG, truth_index=2, truth_size=1, is3d=False,
                                  categorical=False, skip_blank=False, prev_truth_index=prev, prev_truth_size=1 if prev is not None else None,
                                  batched=batched)
        for _ in range(3):
            next(g)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(batches):
            next(g)
        torch.cuda.synchronize()
        out[name + "_ms"] = (time.perf_counter() - t0) / batches * 1e3
        g.close()
    out["prev_truth_batched_over_no_truth"] = out["prev_truth_batched_ms"] / out["no_truth_batched_ms"]
    out["patch_by_patch_over_batched"] = out["prev_truth_patch_by_patch_ms"] / out["prev_truth_batched_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-host", action="store_true", help="leave out the host-tiled prediction (the slowest leg)")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    out = {"first_layer": first_layer(), "train_step": train_step(), "prediction": prediction(a.skip_host), "generator": generator()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
