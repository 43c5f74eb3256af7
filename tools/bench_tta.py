#!/usr/bin/env python3
"""Whole-volume prediction with the eight-flip TTA at the configs[4] workload (160 x 256 x 256 float64 volume, patch 64 x 128 x 128,
overlap 0.5, bf16 network, 36 tiles per variant): the resident route against the kept host route, same process, same model, same
captured graphs, warm, the two arms ALTERNATED round by round; median with min and max of ROUNDS rounds each.
  Stage.infer(augment='flip')      numpy in, numpy out: resident (one upload, 8 variants and their median on the device, one download)
                                   against host (8 x mirrored host volume -> slab-pipelined tile loop -> download, stack, median)
  patch_wise_prediction            numpy in / numpy out (host-fed loop) against CUDA tensor in / CUDA tensor out (resident loop)
  kernels                          fmri_volume_pad_flip and fmri_tile_finalize_flip on the resident volume, per flip mask, next to
                                   fmri_tile_finalize on the same volume: device events around LAUNCHES back-to-back launches, GB/s from
                                   the bytes the pass has to move (84 MB acc + 42 MB cnt + 84 MB out stay below the 256 MiB Infinity Cache,
                                   for every row alike)
The arms' outputs are compared in the same run."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "fetal-mri-segmentation_amd"))
os.environ.setdefault("FMRI_DTYPE", "bf16")
import numpy as np
import torch
import bench
import fetal_net.model as fmodel
from fetal_net import prediction as P
from fetal_net.pipeline import Stage
from fmri_hip import ops

ROUNDS = int(os.environ.get("ROUNDS", "5"))
LAUNCHES = int(os.environ.get("LAUNCHES", "20"))
SHAPE = (160, 256, 256)
PATCH = (64, 128, 128)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def alternate(arms, rounds=ROUNDS):
    """arms: {name: fn}; one warm call each, then `rounds` rounds in which every arm runs once, in turn -> {name: (times, last output)}"""
    res = {name: ([], None) for name in arms}
    for name, fn in arms.items():
        fn()
    for _ in range(rounds):
        for name, fn in arms.items():
            t, out = timed(fn)
            res[name][0].append(t)
            res[name] = (res[name][0], out)
    return res


def show(title, res, base, other):
    for name, (ts, _) in res.items():
        print("%-58s median %8.4f s  (min %8.4f, max %8.4f; %d rounds)" % (title + " " + name, np.median(ts), min(ts), max(ts), len(ts)), flush=True)
    tb, to = res[base][0], res[other][0]
    gap, spread = np.median(tb) - np.median(to), max(max(tb) - min(tb), max(to) - min(to))
    print("%-58s %s is %.2fx of %s; difference of medians %.4f s, largest spread of the rounds %.4f s -> %s" % (
        title, other, np.median(tb) / np.median(to), base, gap, spread,
        "below the host route by more than the spread" if gap > spread else "NOT separated from the host route by more than the spread"), flush=True)


def dev_us(fn, launches=LAUNCHES, reps=5):
    fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / launches)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def kernel_row(name, fn, nbytes):
    med, lo, hi = dev_us(fn)
    print("%-58s %8.1f us (min %8.1f, max %8.1f)  %7.0f GB/s of %.0f MB" % (name, med, lo, hi, nbytes / med / 1e3, nbytes / 1e6), flush=True)


def main():
    assert torch.cuda.is_available(), "tools/bench_tta.py measures on the GPU"
    model = fmodel.unet_model_3d(input_shape=(1,) + PATCH)
    cfg = {"patch_shape": list(PATCH[:2]), "patch_depth": PATCH[2]}
    rs = np.random.RandomState(0)
    vol = 100.0 + 50.0 * rs.randn(*SHAPE)
    print("# kernel_source_hash=%s  %s  volume %s float64, patch %s, overlap 0.5, %s, %d rounds alternated, host: %d CPUs available to this process" % (
        bench.kernel_source_hash(), torch.cuda.get_device_name(0), SHAPE, PATCH, os.environ["FMRI_DTYPE"], ROUNDS, len(os.sched_getaffinity(0))),
        flush=True)

    stage = Stage(model, cfg, augment="flip", overlap=0.5)
    assert stage._resident_refusal(vol) is None
    res = alternate({"host route": lambda: stage._infer_host(vol), "resident route": lambda: stage._infer_resident(vol, False)})
    show("Stage.infer(augment='flip')", res, "host route", "resident route")
    print("%-58s max |resident - host| %.3e" % ("Stage.infer(augment='flip')", np.abs(res["resident route"][1] - res["host route"][1]).max()), flush=True)

    data = vol[np.newaxis]
    d_data = torch.from_numpy(data).cuda()
    res = alternate({"numpy in, numpy out": lambda: P.patch_wise_prediction(model, data, PATCH, overlap_factor=0.5),
                     "tensor in, tensor out": lambda: P.patch_wise_prediction(model, d_data, PATCH, overlap_factor=0.5)})
    show("patch_wise_prediction", res, "numpy in, numpy out", "tensor in, tensor out")
    print("%-58s max |tensor - numpy| %.3e" % ("patch_wise_prediction", np.abs(res["tensor in, tensor out"][1].cpu().numpy() - res["numpy in, numpy out"][1]).max()),
          flush=True)
    del res

    # ---- the two kernels on the resident volume
    n = int(np.prod(SHAPE))
    d_vol = d_data[0].contiguous()
    v32 = torch.empty(SHAPE, dtype=torch.float32, device="cuda")
    for mask in (0, 1, 2, 4, 7):
        kernel_row("fmri_volume_pad_flip f64 -> f32, mask %d" % mask, lambda m=mask: ops.volume_pad_flip(d_vol, v32, (0, 0, 0), m, 0.0), n * 12)
    grown = torch.empty(tuple(s + 6 for s in SHAPE), dtype=torch.float64, device="cuda")
    kernel_row("fmri_volume_pad_flip f64 -> f64, border 3", lambda: ops.volume_pad_flip(d_vol, grown, (3, 3, 3), 0, 0.0), n * 8 + grown.numel() * 8)
    kernel_row("fmri_volume_pad_flip f64 -> f64, crop 3", lambda: ops.volume_pad_flip(grown, d_vol, (-3, -3, -3), 0, 0.0), n * 16)
    acc = torch.rand(SHAPE + (1,), dtype=torch.float64, device="cuda")
    cnt = torch.randint(1, 9, SHAPE, dtype=torch.int32, device="cuda")
    out = torch.empty_like(acc)
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    kernel_row("fmri_tile_finalize", lambda: ops.tile_finalize(acc, cnt, out, bad), n * 20)
    for mask in (0, 1, 2, 4, 7):
        kernel_row("fmri_tile_finalize_flip mask %d" % mask, lambda m=mask: ops.tile_finalize_flip(acc, cnt, out, bad, (0, 0, 0), m), n * 20)
    stack = torch.rand((8,) + SHAPE, dtype=torch.float64, device="cuda")
    kernel_row("fmri_median_stack_f64 of 8", lambda: ops.median_stack_f64(stack), n * 72)


if __name__ == "__main__":
    main()
