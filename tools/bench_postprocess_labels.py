#!/usr/bin/env python3
"""Timing of the multi-label clean-up (one MI355X; host clock around calls that end in a device synchronise or a download, the arms of
one label count alternating in one process; medians with the spread next to them).

Volume 160x256x256 (BASELINE configs[4]) with L = 1, 4, 32 channels of smooth random probabilities, threshold at the 0.6 quantile:

  new_host    postprocess_label_map(array, device=True): upload, all labels in one pass, one byte per voxel back
  new_device  the same from a float64 CUDA tensor to a uint8 CUDA tensor (no transfer)
  loop_api    the loop over the labels: postprocess_prediction(pred[..., l], device=True) per label, the smoothed channel from
              ops.gaussian_filter_f64 (the merge needs it and postprocess_prediction does not return it), then the definition's
              argmax / masking with numpy on the host
  single      L = 1 only: postprocess_prediction(device=True), the same word kernels at one label with the mask brought to the host
  stages      device-event time of each stage of new_device

usage: bench_postprocess_labels.py [--labels 1,4,32] [--reps 5] [--shape 160,256,256] [--out FILE]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fetal-mri-segmentation_amd"))
sys.path.insert(0, ROOT)


def _field(shape, n_labels, seed=11):
    """channels-last smooth probabilities in [0, 1]; four distinct fields, the further channels are shifted copies of them"""
    import numpy as np
    from scipy import ndimage
    rs = np.random.RandomState(seed)
    base = [ndimage.gaussian_filter(rs.rand(*shape), 4.0) for _ in range(min(n_labels, 4))]
    lo, hi = min(b.min() for b in base), max(b.max() for b in base)
    p = np.empty(tuple(shape) + (n_labels,), np.float64)
    for l in range(n_labels):
        p[..., l] = (np.roll(base[l % 4], 23 * (l // 4), axis=1) - lo) / (hi - lo)
    return p


def _merge(smoothed, masks, values):
    import numpy as np
    index = np.argmax(np.where(masks, smoothed, -np.inf), axis=0) + 1
    index[~masks.any(axis=0)] = 0
    return np.asarray([0] + list(values), np.uint8)[index]


def _clock(f):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def _stats(ms):
    import numpy as np
    return {"ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms)), "n": len(ms)}


def run(shape, n_labels, reps):
    import numpy as np
    import torch
    from fetal_net.postprocess import postprocess_label_map, postprocess_prediction
    from fmri_hip import ops
    pred = _field(shape, n_labels)
    thr = float(np.quantile(pred[::4, ::4, ::4], 0.6))
    values = list(range(1, n_labels + 1))
    dev_in = torch.from_numpy(pred).cuda()

    def loop_api():
        sm = np.stack([ops.gaussian_filter_f64(torch.from_numpy(np.ascontiguousarray(pred[..., l])).cuda(), 1).cpu().numpy()
                       for l in range(n_labels)])
        mk = np.stack([postprocess_prediction(np.ascontiguousarray(pred[..., l]), threshold=thr, device=True) for l in range(n_labels)])
        return _merge(sm, mk, values)

    arms = {"new_host": lambda: postprocess_label_map(pred, threshold=thr, device=True),
            "new_device": lambda: postprocess_label_map(dev_in, threshold=thr),
            "loop_api": loop_api}
    if n_labels == 1:
        arms["single"] = lambda: postprocess_prediction(pred[..., 0], threshold=thr, device=True)
    results = {k: f() for k, f in arms.items()}                         # warm-up of every arm, and the results to compare
    same = bool(np.array_equal(results["new_host"], results["loop_api"])
                and np.array_equal(results["new_device"].cpu().numpy(), results["loop_api"]))
    if n_labels == 1:
        same = same and bool(np.array_equal(results["single"], results["new_host"] != 0))
    times = {k: [] for k in arms}
    for _ in range(reps):
        for k, f in arms.items():
            times[k].append(_clock(f)[0])

    def stages():
        out = {}
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
        ev[0].record()
        sm = ops.gaussian_filter_channels_f64(dev_in, 1)
        ev[1].record()
        w = ops.threshold_bits_f64(sm, thr)
        ev[2].record()
        w = ops.binary_fill_holes_bits(w, n_labels)
        ev[3].record()
        w = ops.largest_components_bits(w, n_labels)
        ev[4].record()
        ops.label_map_from_bits(w, sm, values)
        ev[5].record()
        torch.cuda.synchronize()
        for i, name in enumerate(("smooth", "threshold", "fill_holes", "components", "combine")):
            out[name] = ev[i].elapsed_time(ev[i + 1])
        return out

    st = [stages() for _ in range(max(3, reps))]
    out = {"labels": n_labels, "shape": list(shape), "threshold": thr, "labels_present": int(len(np.unique(results["loop_api"])) - 1),
           "foreground_fraction": float((results["loop_api"] != 0).mean()), "results_equal": same}
    out.update({k: _stats(v) for k, v in times.items()})
    out["stages_ms_median"] = {k: float(np.median([s[k] for s in st])) for k in st[0]}
    out["speedup_new_host_over_loop_api"] = out["loop_api"]["ms_median"] / out["new_host"]["ms_median"]
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--labels", default="1,4,32")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shape", default="160,256,256")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_postprocess_labels.py measures on the GPU: none found")
    lines = ["# tools/bench_postprocess_labels.py --labels %s --reps %d --shape %s (%s)" % (a.labels, a.reps, a.shape,
                                                                                          torch.cuda.get_device_name(0))]
    print(lines[0], flush=True)
    for n_labels in [int(v) for v in a.labels.split(",")]:
        r = run(tuple(int(v) for v in a.shape.split(",")), n_labels, a.reps if n_labels < 16 else max(2, a.reps // 2))
        lines.append(json.dumps(r))
        print(lines[-1], flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
