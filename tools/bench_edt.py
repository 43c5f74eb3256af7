#!/usr/bin/env python3
"""The distance mask of one label volume at the configs[4] volume size (160 x 256 x 256 uint8, a box plus an ellipsoid, voxel spacing
(0.4, 0.4, 3.0)): `ops.distance_mask_u8` on the device (volume resident, median of 20 calls after 3 warm-ups, device synchronised around
each) against the reference's two scipy.ndimage.distance_transform_edt calls on the same host."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "fetal-mri-segmentation_amd"))
import numpy as np
import torch
from scipy import ndimage
import bench
from fmri_hip import ops

SAMPLING = (0.4, 0.4, 3.0)
shape = (160, 256, 256)
x, y, z = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
vol = ((((x - 90) / 40.0) ** 2 + ((y - 140) / 60.0) ** 2 + ((z - 120) / 70.0) ** 2 < 1) |
       ((x >= 20) & (x < 50) & (y >= 30) & (y < 90) & (z >= 40) & (z < 200))).astype(np.uint8)
del x, y, z
print("# kernel_source_hash=%s  volume %s uint8, foreground %.1f %%, sampling %s" % (bench.kernel_source_hash(), shape, 100.0 * vol.mean(), SAMPLING))

t0 = time.perf_counter()
want = ndimage.distance_transform_edt(vol, sampling=SAMPLING) + ndimage.distance_transform_edt(1 - vol, sampling=SAMPLING)
t_host = time.perf_counter() - t0

d = torch.from_numpy(vol).cuda()
for name, fn, fields in (("distance_mask_u8 (both fields, 3 launches)", ops.distance_mask_u8, 2),
                         ("distance_transform_edt_u8 (one field)", ops.distance_transform_edt_u8, 1)):
    for _ in range(3):
        got = fn(d, SAMPLING)
    times = []
    for _ in range(20):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = fn(d, SAMPLING)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    t_dev = float(np.median(times))
    # the floor: every pass reads and writes each field once in fp64 (the z pass reads the mask instead, the last pass writes one field)
    n = vol.size
    floor_bytes = n * (1 + 8 * fields) + n * 16 * fields + n * (8 * fields + 1 + 8)
    print("%s: median %.3f ms (min %.3f, max %.3f); traffic floor %.2f GB = %.2f TB/s effective" % (
        name, 1e3 * t_dev, 1e3 * min(times), 1e3 * max(times), floor_bytes / 1e9, floor_bytes / t_dev / 1e12))
    if fields == 2:
        g = got.cpu().numpy()
        print("    two scipy calls on this host: %.2f s (%.0fx); max relative difference %.2e, zeros agree: %s" % (
            t_host, t_host / t_dev, float(np.max(np.abs(g - want) / np.maximum(want, 1e-300))), bool(np.array_equal(g == 0, want == 0))))
