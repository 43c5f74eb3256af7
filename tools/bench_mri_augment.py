#!/usr/bin/env python3
"""Device time of the fetal acquisition augmenters (slice_motion, gamma, bias_field, slice_intensity) at the headline patch, 4 x 64x128x128.
   python tools/bench_mri_augment.py [--rounds 9] [--batches 4]
1. chain: device ms per batch of the device generator's sampling chain (HIP events around `--batches` batches enqueued behind a blocker) with the
   reference's default augmentation, without and with the four keys at prob 1 (and with slice_motion alone, gamma + bias_field alone); the arms alternate round by round in
   one process on the same global draws, medians with min - max; and the launches per batch of either arm, counted from the calls into the library.
2. gather: fmri_affine_sample_batch with an identity table against the same call without a table on the same patches, image (trilinear) and
   labels (nearest), alternated, us per launch with the bytes the gather has to move; and fmri_mri_intensity_ws_batch beside
   fmri_rescale_intensity_ws_batch on the same batch.
Prints one JSON line."""
import argparse
import json
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "fetal-mri-segmentation_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_sampler import FULL, Vols  # noqa: E402

KEYS = {"slice_motion": {"prob": 1, "slice_prob": 0.5, "rotate": 3.0, "translate": 2.0}, "gamma": {"prob": 1, "range": (0.7, 1.5)},
        "bias_field": {"prob": 1, "order": 3, "coefficient": 0.5}, "slice_intensity": {"prob": 1, "slice_prob": 0.3, "sigma": 0.15}}


def stats(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--blocker", type=int, default=12, help="8192^3 fp32 matrix products in front of every timed window")
    ap.add_argument("--batch", type=int, default=4)
    a = ap.parse_args()
    import torch
    from fetal_net.device_generator import DeviceDataFile, device_data_generator
    from fmri_hip import _lib, ops
    patch = (64, 128, 128)
    ddf = DeviceDataFile(Vols(6, (96, 192, 192)), patch)
    out = {"patch": list(patch), "batch": a.batch, "rounds": a.rounds, "batches_per_round": a.batches}

    blocker = torch.randn(8192, 8192, device="cuda")
    behind = []

    def timed(fn, n):
        """device ms per call: the n calls are enqueued BEHIND ~0.1 s of matrix products, so the host (a plan is milliseconds of numpy, a launch
        tens of microseconds of ctypes) runs ahead and the events bracket device work only; `behind` counts windows where it did not"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(a.blocker):
            torch.mm(blocker, blocker)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        behind.append(e0.query())                 # True: the device was already through the products when the last call was enqueued
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    # ---- 1. the chain
    arms = {"reference_default": FULL, "with_mri_keys": dict(FULL, **KEYS), "slice_motion_only": dict(FULL, slice_motion=KEYS["slice_motion"]),
            "gamma_bias_only": dict(FULL, gamma=KEYS["gamma"], bias_field=KEYS["bias_field"])}
    gens = {}
    for name, aug in arms.items():
        np.random.seed(0)
        random.seed(0)
        gens[name] = device_data_generator(ddf, list(range(6)), batch_size=a.batch, patch_shape=patch, augment=aug, truth_index=0, truth_size=patch[2],
                                           is3d=True, categorical=False, skip_blank=False, shuffle_index_list=False)    # shuffling re-seeds numpy from the OS on every pass
        for _ in range(3):
            next(gens[name])
    torch.cuda.synchronize()
    # launches per batch: every call into the library is one launch, except the two of the shot noise
    L = _lib.lib()
    calls = {}
    def reseed(k):
        # the new keys draw from a state of their own: with numpy's and python's global states set alike, every arm plans the same patches, the
        # same affines and the same steps of the reference's chain
        np.random.seed(k)
        random.seed(k)

    for name, g in gens.items():
        reseed(1000)
        seen = []
        wrapped = {}
        for sym in _lib.SIGNATURES:
            f = getattr(L, sym)
            wrapped[sym] = f
            setattr(L, sym, (lambda f, sym: lambda *args: (seen.append(sym), f(*args))[1])(f, sym))
        next(g)
        for sym, f in wrapped.items():
            setattr(L, sym, f)
        calls[name] = {s: seen.count(s) for s in sorted(set(seen))}
    out["library_calls_per_batch"] = calls
    ms = {name: [] for name in gens}
    for r in range(a.rounds):
        for name, g in gens.items():
            reseed(r)
            ms[name].append(timed(lambda: next(g), a.batches))
    out["chain_ms_per_batch"] = {k: stats(v) for k, v in ms.items()}
    out["chain_added_ms"] = {k: v["median"] - out["chain_ms_per_batch"]["reference_default"]["median"] for k, v in out["chain_ms_per_batch"].items()
                             if k != "reference_default"}

    # ---- 2. the kernels alone
    B = a.batch
    rs = np.random.RandomState(1)
    from fetal_net.augment import distort_image
    affines = [distort_image(np.empty((96, 192, 192)), np.eye(4), scale_factor=[1.05, 0.95, 1], rotate_factor=np.deg2rad([0, 0, rs.uniform(-40, 40)]),
                             translate_factor=rs.uniform(-5, 5, 3))[1] for _ in range(B)]
    idx = [b % 6 for b in range(B)]
    corners = [[int(rs.randint(0, h)) for h in np.array(ddf.data[i].shape) - np.array(patch)] for i in idx]
    ident = torch.from_numpy(np.tile(np.array([1.0, 0, 0, 0, 1.0, 0]), (B, patch[2], 1))).cuda()
    xo = torch.empty((B,) + patch, device="cuda")
    yo = torch.empty((B,) + patch, device="cuda", dtype=torch.uint8)
    vox = B * patch[0] * patch[1] * patch[2]
    gather = {
        "image_plain": lambda: ops.affine_sample_batch([ddf.data[i] for i in idx], affines, corners, patch, xo, 1, [ddf.min[i] for i in idx]),
        "image_identity_table": lambda: ops.affine_sample_batch([ddf.data[i] for i in idx], affines, corners, patch, xo, 1, [ddf.min[i] for i in idx], table=ident),
        "labels_plain": lambda: ops.affine_sample_batch([ddf.truth[i] for i in idx], affines, corners, patch, yo, 0, [0.0] * B),
        "labels_identity_table": lambda: ops.affine_sample_batch([ddf.truth[i] for i in idx], affines, corners, patch, yo, 0, [0.0] * B, table=ident),
    }
    ref = gather["image_plain"]().clone()
    out["identity_table_equal"] = bool(torch.equal(gather["image_identity_table"](), ref))
    st, ws = ops.aug_workspace("cuda", B)
    gains = [torch.ones(patch[2], device="cuda") for _ in range(B)]
    coef = rs.uniform(-0.5, 0.5, 20)
    ops.minmax_ws_batch(xo, st, ws)
    gather["rescale_intensity_ws"] = lambda: ops.rescale_intensity_ws_batch(xo, st, ws, [[2, -1.0, 3.0, 1.0]] * B)
    gather["mri_intensity_all_three"] = lambda: ops.mri_intensity_ws_batch(xo, st, ws, [1.0001] * B, [coef * 1e-3] * B, gains, [0.0] * B)
    gather["mri_intensity_gamma_only"] = lambda: ops.mri_intensity_ws_batch(xo, st, ws, [1.0001] * B, [None] * B, [None] * B, [0.0] * B)
    for f in gather.values():
        for _ in range(5):
            f()
    us = {k: [] for k in gather}
    for _ in range(a.rounds):
        for k, f in gather.items():
            us[k].append(timed(f, 50) * 1e3)
    out["kernel_us_per_launch"] = {k: stats(v) for k, v in us.items()}
    # bytes the algorithm has to move: the gather writes the patch and reads about as much (trilinear taps share lines); in-place passes read + write
    moved = {"image": vox * 8, "labels": vox * 2, "rescale": vox * 8, "mri": vox * 8}
    out["kernel_GBps"] = {k: moved[k.split("_")[0]] / (v["median"] * 1e-6) / 1e9 for k, v in out["kernel_us_per_launch"].items()}
    out["windows_where_the_host_fell_behind"] = "%d of %d" % (sum(behind), len(behind))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
