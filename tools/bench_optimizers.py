#!/usr/bin/env python3
"""The optimizer step kernels and the gradient sum of squares at the headline model's n_flat, next to fmri_adam_step as the yardstick,
and the headline training step (configs[1]: 4 patches of 64 x 128 x 128, bf16) with clipnorm on against off.

One process, arms alternated: every round runs each arm once (LAUNCHES launches resp. STEPS training steps between two device events),
ROUNDS rounds; reported per arm: the median over the rounds with min - max.  Bandwidth = bytes the update has to read + write (4-byte
elements: parameters, gradient and each slot read, parameters and each slot written) over the kernel's time.
ROUNDS / LAUNCHES / STEPS can be lowered through the environment for a quick look."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "fetal-mri-segmentation_amd"))
import torch
import bench
from fmri_hip import ops
from fmri_hip.engine import UNetEngine, UNetPlan

ROUNDS = int(os.environ.get("ROUNDS", "15"))
LAUNCHES = int(os.environ.get("LAUNCHES", "50"))
STEPS = int(os.environ.get("STEPS", "20"))


def timed(fn, count):
    """milliseconds per call of `count` back-to-back calls of fn between two device events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(count):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / count


def alternate(arms, count, rounds):
    """arms: [(name, fn)] -> {name: [ms per call, one value per round]}, every round running the arms in turn"""
    for _, fn in arms:
        timed(fn, 3)                                        # warm-up: code objects loaded, buffers touched
    out = dict((name, []) for name, _ in arms)
    for _ in range(rounds):
        for name, fn in arms:
            out[name].append(timed(fn, count))
    return out


def spread(vals, scale=1.0):
    return statistics.median(vals) * scale, min(vals) * scale, max(vals) * scale


def main():
    torch.cuda.set_device(0)
    eng = UNetEngine(UNetPlan(1, (64, 128, 128), depth=4, n_base_filters=32), 4, dtype=torch.bfloat16, seed=42)
    n = eng.n_flat
    print("# kernel_source_hash=%s  %s  n_flat=%d (%.1f MB per buffer)  rounds=%d launches=%d steps=%d" % (
        bench.kernel_source_hash(), torch.cuda.get_device_name(0), n, n * 4 / 1e6, ROUNDS, LAUNCHES, STEPS), flush=True)

    # ---- the kernels alone, on buffers of their own (small gradients and lr: the values stay finite over thousands of launches)
    g = torch.randn(n, device="cuda") * 1e-3
    p, m, v, h = (torch.zeros(n, device="cuda") for _ in range(4))
    work, out = ops.grad_sumsq_workspace("cuda")
    arms = [
        ("fmri_adam_step", 7, lambda: ops.adam_step(p, g, m, v, 1e-6, 0.9, 0.999, 1e-7, 1.0)),
        ("fmri_adam_step_ex plain", 7, lambda: ops.adam_step_ex(p, g, m, v, None, 1e-6)),
        ("fmri_adam_step_ex amsgrad", 9, lambda: ops.adam_step_ex(p, g, m, v, h, 1e-6)),
        ("fmri_adam_step_ex clipnorm", 7, lambda: ops.adam_step_ex(p, g, m, v, None, 1e-6, gnorm=out, clipnorm=1.0)),
        ("fmri_sgd_step momentum", 5, lambda: ops.sgd_step(p, g, m, 1e-6, 0.9, False)),
        ("fmri_sgd_step nesterov", 5, lambda: ops.sgd_step(p, g, m, 1e-6, 0.9, True)),
        ("fmri_rmsprop_step", 5, lambda: ops.rmsprop_step(p, g, v, 1e-6, 0.9, 1e-7)),
        ("fmri_grad_sumsq (2 launches)", 1, lambda: ops.grad_sumsq(g, 1.0, work, out)),
    ]
    ops.grad_sumsq(g, 1.0, work, out)
    res = alternate([(name, fn) for name, _, fn in arms], LAUNCHES, ROUNDS)
    for name, streams, _ in arms:
        med, lo, hi = spread(res[name], 1e3)
        print("%-30s %7.1f us (%6.1f - %6.1f)   %d x n x 4 B = %6.1f MB   %5.2f TB/s (%.2f - %.2f)" % (
            name, med, lo, hi, streams, streams * n * 4 / 1e6, streams * n * 4 / (med * 1e-6) / 1e12,
            streams * n * 4 / (hi * 1e-6) / 1e12, streams * n * 4 / (lo * 1e-6) / 1e12), flush=True)

    # ---- the headline training step, clipnorm on against off (both Adam; on = fmri_grad_sumsq's two launches + fmri_adam_step_ex)
    x = torch.randn(4, 64, 128, 128, 1, device="cuda").to(torch.bfloat16)
    y = (torch.rand(4 * 64 * 128 * 128, device="cuda") < 0.3).to(torch.uint8)

    def step_with(spec):
        def fn():
            eng.set_optimizer(spec)
            eng.train_step(x, y, 1e-4)
        return fn
    res = alternate([("clipnorm off", step_with(None)), ("clipnorm on", step_with(dict(clipnorm=1.0)))], STEPS, ROUNDS)
    off, on = spread(res["clipnorm off"]), spread(res["clipnorm on"])
    for name, (med, lo, hi) in (("clipnorm off", off), ("clipnorm on", on)):
        print("headline step, %-13s %7.3f ms (%7.3f - %7.3f)" % (name, med, lo, hi), flush=True)
    print("clipnorm costs %+.3f ms per step (medians; %+.2f %%)" % (on[0] - off[0], 100.0 * (on[0] - off[0]) / off[0]), flush=True)


if __name__ == "__main__":
    main()
