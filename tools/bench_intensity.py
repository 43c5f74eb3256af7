#!/usr/bin/env python3
"""The once-per-volume intensity passes in front of the model at the configs[4] volume size (160 x 256 x 256 float64), device form against
the host form it replaces: the 1-99 percentile window, laplace, grad (gaussian_gradient_magnitude, sigma 1), the min-max and z-score maps,
and Stage.intensities as a whole (window -> grad_norm -> z-score: one upload, one download).
Per pass: shapes warmed first, then REPS rounds that alternate host and device in the same process (median of each); device time between
two events around the kernels alone (volume resident), and end to end as the pipeline calls it (numpy in, numpy out: upload, kernels,
download).  The volume is MRI-like: integer-valued, most voxels hold one background value (the header line says how many).  The radix
select is timed at both digit widths, on that volume and on normal deviates."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "fetal-mri-segmentation_amd"))
import numpy as np
import torch
import bench
from fetal_net import preprocess
from fetal_net.pipeline import Stage, normalize_data, window_intensities_data
from fmri_hip import ops

REPS = int(os.environ.get("REPS", "3"))
SHAPE = (160, 256, 256)


def alternate(host, device, reps=REPS):
    """median seconds of host() and device(), called in turns after one warm-up of each; the last results"""
    want, got = host(), device()
    th, td = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        want = host()
        t1 = time.perf_counter()
        got = device()
        t2 = time.perf_counter()
        th.append(t1 - t0)
        td.append(t2 - t1)
    return float(np.median(th)), float(np.median(td)), want, got


def dev_ms(fn, reps=5):
    fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def line(name, t_host, t_e2e, t_dev, want, got):
    ident = "identical" if np.array_equal(want, got, equal_nan=True) else "max |difference| %.2e" % np.nanmax(np.abs(got - want))
    print("%-44s host %8.3f s | device end to end %8.4f s (%6.1fx) | kernels %8.3f ms | %s" % (
        name, t_host, t_e2e, t_host / t_e2e, t_dev, ident), flush=True)


rs = np.random.RandomState(0)
g = np.stack(np.meshgrid(*[np.arange(n) for n in SHAPE], indexing="ij"), -1).astype(np.float64)
r2 = (((g - np.array([80, 120, 130])) / np.array([45.0, 70.0, 70.0])) ** 2).sum(-1)
del g
vol = np.where(r2 < 1.0, np.round(100.0 + 400.0 * np.exp(-r2) + 25.0 * rs.randn(*SHAPE)), 0.0)          # integer-valued, as scanners store
del r2
print("# kernel_source_hash=%s  %s  volume %s float64 (%.0f %% background), median of %d alternating rounds, host: %d CPUs available" % (
    bench.kernel_source_hash(), torch.cuda.get_device_name(0), SHAPE, 100.0 * (vol == 0).mean(), REPS, len(os.sched_getaffinity(0))), flush=True)
d = torch.from_numpy(vol).cuda()

for bits in (8, 11):
    os.environ["FMRI_SELECT_BITS"] = str(bits)
    for name, t in (("MRI-like", d), ("randn", torch.randn(SHAPE, dtype=torch.float64, device="cuda"))):
        print("radix select, %2d-bit digits, %-8s: percentiles (1, 99) %8.3f ms, of which one 4-rank select %8.3f ms" % (
            bits, name, dev_ms(lambda: ops.percentile_f64(t, [1, 99])), dev_ms(lambda: ops.order_stats_f64(t, [0, 1, 2, 3]))), flush=True)
del os.environ["FMRI_SELECT_BITS"]

th, td, want, got = alternate(lambda: window_intensities_data(vol, device=False), lambda: window_intensities_data(vol, device=True))
line("window_1_99 (two percentiles + map)", th, td, dev_ms(lambda: ops.window_intensities_f64(d)), want, got)
win = want

th, td, want, got = alternate(lambda: preprocess.laplace(win, device=False), lambda: preprocess.laplace(win, device=True))
dw = torch.from_numpy(win).cuda()
line("laplace", th, td, dev_ms(lambda: ops.laplace_f64(dw)), want, got)

th, td, want, got = alternate(lambda: preprocess.grad(win, device=False), lambda: preprocess.grad(win, device=True))
line("grad (gaussian_gradient_magnitude, sigma 1)", th, td, dev_ms(lambda: ops.gaussian_gradient_magnitude_f64(dw, (1, 1, 1))), want, got)
gr = want

th, td, want, got = alternate(lambda: preprocess.norm_minmax(gr, device=False), lambda: preprocess.norm_minmax(gr, device=True))
dg = torch.from_numpy(gr).cuda()
line("norm_minmax (min, max + map)", th, td, dev_ms(lambda: ops.norm_minmax_f64(dg)), want, got)

th, td, want, got = alternate(lambda: normalize_data(gr, 0.1, 0.5, device=False), lambda: normalize_data(gr, 0.1, 0.5, device=True))
line("normalize_data (z-score map)", th, td, dev_ms(lambda: ops.normalize_f64(dg, 0.1, 0.5)), want, got)

cfg = {"patch_shape": [16, 16], "patch_depth": 8, "preproc": "grad_norm"}
norm = {"mean": 0.1, "std": 0.5}
sh, sd = Stage(None, cfg, "window_1_99", norm, device=False), Stage(None, cfg, "window_1_99", norm, device=True)
th, td, want, got = alternate(lambda: sh.intensities(vol, []), lambda: sd.intensities(vol, []))
line("Stage.intensities window, grad_norm, z-score", th, td,
     dev_ms(lambda: ops.normalize_f64(ops.norm_minmax_f64(ops.gaussian_gradient_magnitude_f64(ops.window_intensities_f64(d), (1, 1, 1))), 0.1, 0.5)),
     want, got)
