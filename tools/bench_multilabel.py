#!/usr/bin/env python3
"""Several labels: what the label-map path, the label-wise metrics and the four label kernels cost.  Prints one JSON line:
  prediction   s per 160x256x256 volume, L = 4, depth-4 / 32-filter unet_model_3d (patch 64x128x128, overlap 0.5): patch_wise_label_map
               against get_prediction_labels(patch_wise_prediction(...)), alternated in one process after a warm-up of every shape;
               median and min / max over the rounds, every timed region ends in a synchronise
  train_step   ms per training step of that model (batch 2) with and without the label-wise Dice metrics, alternated the same way
  kernels      GB/s of fmri_labels_expand_u8, fmri_label_sums, fmri_tile_finalize_labels and fmri_label_counts_u8 at the volume's size
               (bytes read + written per launch over the median time of the launches)
usage: python tools/bench_multilabel.py [--rounds 7] [--small]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "fetal-mri-segmentation_amd"))
import torch

L = 4


def _stats(ts):
    ts = sorted(ts)
    return dict(median=ts[len(ts) // 2], min=ts[0], max=ts[-1], n=len(ts))


def _model(patch, labelwise):
    import fetal_net.model as fmodel
    return fmodel.unet_model_3d(input_shape=(1,) + patch, depth=4, n_base_filters=32, n_labels=L,
                                include_label_wise_dice_coefficients=labelwise)


def prediction(vol_shape, patch, rounds):
    from fetal_net.prediction import get_prediction_labels, patch_wise_label_map, patch_wise_prediction
    model = _model(patch, False)
    data = np.random.RandomState(0).randn(1, *vol_shape).astype(np.float32)

    def label_map():
        return patch_wise_label_map(model=model, data=data, patch_shape=patch, overlap_factor=0.5)

    def via_probabilities():
        p = patch_wise_prediction(model=model, data=data, patch_shape=patch, overlap_factor=0.5)
        return get_prediction_labels(np.moveaxis(p, -1, 0)[np.newaxis])[0]

    a, b = label_map(), via_probabilities()                  # warm-up of every shape: graphs captured, buffers made
    equal = bool(np.array_equal(a, b))
    times = {"label_map": [], "via_probabilities": []}
    for _ in range(rounds):
        for name, fn in (("label_map", label_map), ("via_probabilities", via_probabilities)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
    return dict(volume=list(vol_shape), patch=list(patch), labels=L, equal=equal, label_map_s=_stats(times["label_map"]),
                via_probabilities_s=_stats(times["via_probabilities"]))


def train_step(patch, rounds, steps=10):
    models = {"with_label_metrics": _model(patch, True), "without": _model(patch, False)}
    rs = np.random.RandomState(1)
    x = torch.from_numpy(rs.randn(2, 1, *patch).astype(np.float32)).cuda()
    y = torch.from_numpy((rs.rand(2, L, *patch) > 0.8).astype(np.uint8)).cuda()
    for m in models.values():                                # warm-up
        for _ in range(3):
            m.train_on_batch(x, y)
    times = {k: [] for k in models}
    for _ in range(rounds):
        for name, m in models.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pend = [m._step_async(m._stage_inline(x, y), train=True) for _ in range(steps)]
            pend[-1].values()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3 / steps)
    return dict(batch=2, patch=list(patch), with_label_metrics_ms=_stats(times["with_label_metrics"]), without_ms=_stats(times["without"]))


def kernels(vol_shape, rounds):
    from fmri_hip import ops
    n = int(np.prod(vol_shape))
    rs = np.random.RandomState(2)
    values = [1, 2, 3, 4]
    blob = np.zeros(vol_shape, np.uint8)                     # label regions are contiguous, as in a segmentation
    for v in values:
        c = [rs.randint(s // 4, 3 * s // 4) for s in vol_shape]
        blob[c[0] - 20:c[0] + 20, c[1] - 30:c[1] + 30, c[2] - 30:c[2] + 30] = v
    lab = torch.from_numpy(blob).cuda()
    lab2 = torch.roll(lab, (2, -3, 1), (0, 1, 2)).contiguous()
    out_e = torch.empty(vol_shape + (L,), dtype=torch.uint8, device="cuda")
    probs = torch.rand(n * L, device="cuda")
    lsums = torch.empty(3 * L, dtype=torch.float64, device="cuda")
    acc = torch.rand(vol_shape + (L,), dtype=torch.float64, device="cuda")
    cnt = torch.ones(vol_shape, dtype=torch.int32, device="cuda")
    out_l = torch.empty(vol_shape, dtype=torch.uint8, device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    counts_out = torch.empty(3 * L, dtype=torch.int64, device="cuda")
    vals = ops.label_values(values)

    def counts():                                            # the entry point itself: ops.label_counts_u8 ends in a read-back
        ops.check(ops.lib().fmri_label_counts_u8(lab.data_ptr(), lab2.data_ptr(), n, vals, L, counts_out.data_ptr(), ops._s()),
                  "fmri_label_counts_u8")

    cases = {
        "fmri_labels_expand_u8": (lambda: ops.labels_expand_u8(lab, values, out=out_e), n * (1 + L)),
        "fmri_label_sums": (lambda: ops.label_sums(probs, out_e.reshape(-1), L, lsums), n * L * 5),
        "fmri_tile_finalize_labels": (lambda: ops.tile_finalize_labels(acc, cnt, out_l, bad, 0.5, values), n * (8 * L + 4 + 1)),
        "fmri_label_counts_u8": (counts, n * 2),
    }
    out = {}
    for name, (fn, nbytes) in cases.items():
        for _ in range(3):
            fn()
        ts = []
        for _ in range(max(rounds, 7)):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e-3)
        s = _stats(ts)
        out[name] = dict(bytes=nbytes, us=dict(median=s["median"] * 1e6, min=s["min"] * 1e6, max=s["max"] * 1e6),
                         gb_per_s=nbytes / s["median"] / 1e9)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--small", action="store_true", help="a 40x64x64 volume and a 16x32x32 patch: a functional run, not a measurement")
    args = ap.parse_args()
    vol, patch = ((40, 64, 64), (16, 32, 32)) if args.small else ((160, 256, 256), (64, 128, 128))
    res = dict(prediction=prediction(vol, patch, args.rounds), train_step=train_step(patch, args.rounds), kernels=kernels(vol, args.rounds),
               dtype=os.environ.get("FMRI_DTYPE", "bf16"), device=torch.cuda.get_device_name(0))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
