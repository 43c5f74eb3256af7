#!/usr/bin/env python3
"""Cost of FMRI_DETERMINISTIC=1: ms per training step in deterministic against default mode of one build, alternated in one process.

    bench_deterministic.py [--rounds 3] [--steps 10] [--only batch_norm,instance_norm,isensee]

Workloads: the batch-norm and the instance-norm variant of BASELINE configs[1] (depth-4 / 32-filter U-Net, 4 x 64x128x128, bf16,
UNetEngine) and isensee2017_model_3d at the reference defaults (1 x 128^3, depth 5, 16 filters, bf16, layer-graph engine).  Every
measurement builds its engine afresh under the switch (the engines read it once, at construction), warms it for >= 1.5 s on live data
(tools/learnable_task.py) and times `steps` steps between two clock stamps.  One JSON line per measurement, then one summary line per
workload with the medians and their ratio."""
import argparse
import gc
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fetal-mri-segmentation_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch


def unet_variant(norm):
    def make():
        import learnable_task as LT
        from fmri_hip.engine import UNetEngine, UNetPlan
        spatial, B = (64, 128, 128), 4
        eng = UNetEngine(UNetPlan(1, spatial, depth=4, n_base_filters=32, norm=norm), B, dtype=torch.bfloat16)
        pool = []
        for k in range(2):
            xb, yb = LT.device_batch(k * B, B, spatial)
            pool.append((xb.to(torch.bfloat16).reshape(B, *spatial, 1).contiguous(), yb.reshape(-1).contiguous()))
        return eng, (lambda i: eng.train_step(*pool[i % 2], 1e-4))
    return make


def isensee():
    import learnable_task as LT
    from fetal_net.metrics import dice_coefficient_loss
    from fetal_net.model import isensee2017_model_3d
    shape = (1, 128, 128, 128)
    model = isensee2017_model_3d(input_shape=shape, loss_function=dice_coefficient_loss)
    pool = [LT.device_batch(k, 1, shape[1:]) for k in range(2)]
    eng = model.engine(1)
    return eng, (lambda i: model.train_on_batch(*pool[i % 2]))


WORKLOADS = {"batch_norm": unet_variant("batch"), "instance_norm": unet_variant("instance"), "isensee": isensee}


def measure(name, mode, steps):
    from fmri_hip import ops
    os.environ["FMRI_DETERMINISTIC"] = mode
    eng, step = WORKLOADS[name]()
    assert bool(eng.deterministic) == (mode == "1")
    t0, i = time.time(), 0
    while time.time() - t0 < 1.5:
        step(i)
        i += 1
        if i % 5 == 0:
            torch.cuda.synchronize()
    s0, s1 = torch.zeros(16, dtype=torch.int64, device="cuda"), torch.zeros(16, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ops.clock_stamp(s0)
    t0 = time.time()
    for k in range(steps):
        step(i + k)
    ops.clock_stamp(s1)
    torch.cuda.synchronize()
    ms = (time.time() - t0) / steps * 1e3
    ghz, _ = ops.clock_ghz(s0, s1)
    eng.close()
    del eng, step
    gc.collect()
    torch.cuda.empty_cache()
    return dict(workload=name, deterministic=int(mode), ms_per_step=round(ms, 3), steps=steps, clock_ghz=None if ghz is None else round(ghz, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--only", default=",".join(WORKLOADS))
    a = ap.parse_args()
    for name in a.only.split(","):
        ms = {"0": [], "1": []}
        for _ in range(a.rounds):
            for mode in ("0", "1"):
                r = measure(name, mode, a.steps)
                ms[mode].append(r["ms_per_step"])
                print(json.dumps(r), flush=True)
        med = {m: sorted(v)[len(v) // 2] for m, v in ms.items()}
        print(json.dumps(dict(workload=name, summary=True, default_ms=med["0"], deterministic_ms=med["1"],
                              cost=round(med["1"] / med["0"] - 1.0, 4))), flush=True)


if __name__ == "__main__":
    main()
