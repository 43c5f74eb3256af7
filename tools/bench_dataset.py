#!/usr/bin/env python3
"""Building a cohort's data file (fetal_net.data.write_data_to_file), host form against device form in the same process: 8 synthetic
subjects of 160 x 256 x 256 stored as float32 NIfTI (uncompressed, so that reading a file is a small cost common to both forms) in a
temporary folder, normalize='all', for three settings: plain, scale=(0.33, 0.33, 1) and preproc='laplace_norm'.  Each build is timed as
a whole - reading the scans, the per-volume arithmetic, the transfers and writing the HDF5 file - and reported per subject; the device
form runs first once per setting as a warm-up of its kernels' shapes (not timed).  Last line: fmri_hip.ops.moments_f64 alone (volume
resident; the launches and the one read-back) against ndarray.mean() + ndarray.std() on the same volume.
SUBJECTS / SHAPE can be lowered through the environment for a quick look."""
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "fetal-mri-segmentation_amd"))
import numpy as np
import torch
import bench
from fetal_net.data import open_data_file, write_data_to_file
from fetal_net.utils.nifti import save_nifti
from fmri_hip import ops

SUBJECTS = int(os.environ.get("SUBJECTS", "8"))
SHAPE = tuple(int(v) for v in os.environ.get("SHAPE", "160,256,256").split(","))
SETTINGS = [("plain", {}), ("scale (0.33, 0.33, 1)", {"scale": (0.33, 0.33, 1)}), ("preproc laplace_norm", {"preproc": "laplace_norm"})]


def make_scans(root):
    rs = np.random.RandomState(0)
    g = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float32) for n in SHAPE], indexing="ij"), -1)
    files = []
    for i in range(SUBJECTS):
        centre = np.array(SHAPE, np.float32) * (0.45 + 0.02 * i)
        r2 = (((g - centre) / (np.array(SHAPE, np.float32) * 0.28)) ** 2).sum(-1)
        vol = np.where(r2 < 1.0, np.round(100.0 + 400.0 * np.exp(-r2) + 25.0 * rs.standard_normal(SHAPE).astype(np.float32)), 0.0)
        names = (os.path.join(root, "s%d_volume.nii" % i), os.path.join(root, "s%d_truth.nii" % i))
        save_nifti(vol.astype(np.float32), names[0])         # integer-valued, mostly background: what scanners store
        save_nifti((r2 < 0.5).astype(np.uint8), names[1])
        files.append(names)
    return files


def build(files, out, device, **kw):
    t0 = time.perf_counter()
    _, (mean, std) = write_data_to_file(files, out, normalize="all", device=device, **kw)
    return time.perf_counter() - t0, float(mean), float(std)


def main():
    tmp = tempfile.mkdtemp(prefix="bench_dataset_")
    try:
        files = make_scans(tmp)
        print("# kernel_source_hash=%s  %s  %d subjects %s float32 NIfTI, normalize='all', host: %d CPUs available" % (
            bench.kernel_source_hash(), torch.cuda.get_device_name(0), SUBJECTS, SHAPE, len(os.sched_getaffinity(0))), flush=True)
        out_h, out_d = os.path.join(tmp, "host.h5"), os.path.join(tmp, "device.h5")
        for name, kw in SETTINGS:
            build(files[:1], out_d, True, **kw)
            th, mh, sh = build(files, out_h, False, **kw)
            td, md, sd = build(files, out_d, True, **kw)
            with open_data_file(out_h) as fh, open_data_file(out_d) as fd:
                a, b = fh.root.data[SUBJECTS - 1], fd.root.data[SUBJECTS - 1]
                same = np.array_equal(fh.root.truth[SUBJECTS - 1], fd.root.truth[SUBJECTS - 1])
            print("%-24s host %7.3f s / subject | device %7.3f s / subject (%5.1fx) | mean %.17g vs %.17g, std %.17g vs %.17g | last volume: "
                  "max |difference| %.2e, truth %s" % (name, th / SUBJECTS, td / SUBJECTS, th / td, mh, md, sh, sd,
                                                        float(np.abs(a - b).max()), "identical" if same else "DIFFERS"), flush=True)
        from fetal_net.utils.nifti import load_nifti
        vol = np.ascontiguousarray(load_nifti(files[0][0]), dtype=np.float64)
        d = torch.from_numpy(vol).cuda()
        ops.moments_f64(d)
        th, td = [], []
        for _ in range(5):
            t0 = time.perf_counter()
            want = (vol.mean(), vol.std())
            t1 = time.perf_counter()
            got = ops.moments_f64(d)
            t2 = time.perf_counter()
            th.append(t1 - t0)
            td.append(t2 - t1)
        print("moments of one volume: ndarray.mean() + ndarray.std() %.1f ms | moments_f64 (resident, with its read-back) %.3f ms | mean %s, "
              "std %.17g vs %.17g" % (1e3 * np.median(th), 1e3 * np.median(td), "identical" if want[0] == got[0] else "%.17g vs %.17g" % (
                  want[0], got[0]), want[1], got[1]), flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
