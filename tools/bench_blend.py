#!/usr/bin/env python3
"""Cost of Gaussian tile blending at the configs[4] workload (160 x 256 x 256 float64 volume, patch 64 x 128 x 128, bf16 network): the device
tile loop behind `patch_wise_prediction`, end to end (numpy in, numpy out: upload, tile loop, download) and in device time per volume
(CUDA tensor in, tensor out, device events), for three arms:
  parent     the parent commit's package and library (a checkout of it, built, under --parent-tree; default build/parent):
                 git archive HEAD~1 fetal-mri-segmentation_amd include | tar -x -C build/parent && make -C build/parent/fetal-mri-segmentation_amd/csrc
  none       this tree, blend=None: the same kernels and the same graphs as the parent
  gaussian   this tree, blend="gaussian"
Every measurement runs in a child process of its own (one package per process), the arms ALTERNATED round by round; each child warms its
graphs up, then times REPS volumes.  Reported per arm: median, min and max over all rounds x REPS.  `none` has to lie inside the
run-to-run spread of `parent` (between its min and max; the tool exits 1 otherwise); `gaussian` is reported against `none`.  Then `gaussian`
at overlap 0.9, 0.75 and 0.5 with the tile counts: what lowering the overlap buys."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (160, 256, 256)
PATCH = (64, 128, 128)


def child(tree, arm, overlap, reps):
    sys.path.insert(0, os.path.join(tree, "fetal-mri-segmentation_amd"))
    os.environ.setdefault("FMRI_DTYPE", "bf16")
    import numpy as np
    import torch
    import fetal_net.model as fmodel
    from fetal_net import prediction as P
    assert torch.cuda.is_available(), "tools/bench_blend.py measures on the GPU"
    assert os.path.realpath(P.__file__).startswith(os.path.realpath(tree)), (P.__file__, tree)
    kw = {"parent": {}, "none": dict(blend=None), "gaussian": dict(blend="gaussian")}[arm]
    model = fmodel.unet_model_3d(input_shape=(1,) + PATCH)
    data = (100.0 + 50.0 * np.random.RandomState(0).randn(*SHAPE))[np.newaxis]
    d_data = torch.from_numpy(data).cuda()
    n_tiles = len(P._geometry_of_shape(model, SHAPE, PATCH, overlap)[4])
    warm = 1 if n_tiles > 200 else 2
    for _ in range(warm):                                     # graph capture, lazy allocations, pinned buffers
        P.patch_wise_prediction(model, data, PATCH, overlap_factor=overlap, **kw)
        P.patch_wise_prediction(model, d_data, PATCH, overlap_factor=overlap, **kw)
    torch.cuda.synchronize()
    end_to_end, device = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = P.patch_wise_prediction(model, data, PATCH, overlap_factor=overlap, **kw)
        torch.cuda.synchronize()
        end_to_end.append(time.perf_counter() - t0)
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        P.patch_wise_prediction(model, d_data, PATCH, overlap_factor=overlap, **kw)
        b.record()
        b.synchronize()
        device.append(a.elapsed_time(b) * 1e-3)
    print("RESULT " + json.dumps(dict(arm=arm, overlap=overlap, tiles=n_tiles, end_to_end_s=end_to_end, device_s=device,
                                      checksum=float(np.asarray(out, dtype=np.float64).sum()), gpu=torch.cuda.get_device_name(0))), flush=True)


def run_child(tree, arm, overlap, reps, limit):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", arm, "--tree", tree, "--overlap", str(overlap), "--reps", str(reps)]
    env = dict(os.environ)
    env.pop("FMRI_LIB", None)                                 # every tree loads the library it built
    res = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=limit)
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("RESULT ")]
    if res.returncode != 0 or not lines:
        sys.stdout.write(res.stdout[-4000:])
        raise SystemExit("arm %s failed (exit %d): nothing further is started" % (arm, res.returncode))
    return json.loads(lines[-1][len("RESULT "):])


def stats(xs):
    xs = sorted(xs)
    mid = xs[len(xs) // 2] if len(xs) % 2 else 0.5 * (xs[len(xs) // 2 - 1] + xs[len(xs) // 2])
    return mid, xs[0], xs[-1]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-tree", default=os.path.join(ROOT, "build", "parent"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds one child may take")
    ap.add_argument("--child", default=None)
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--overlap", type=float, default=0.5)
    args = ap.parse_args()
    if args.child:
        return child(args.tree, args.child, args.overlap, args.reps)
    sys.path.insert(0, ROOT)
    import bench
    trees = {"parent": args.parent_tree, "none": ROOT, "gaussian": ROOT}
    if not os.path.exists(os.path.join(args.parent_tree, "fetal-mri-segmentation_amd", "lib", "libfmri_hip.so")):
        raise SystemExit("no built parent tree under %s (see the docstring): the requirement compares with it" % args.parent_tree)
    print("# tools/bench_blend.py kernel_source_hash=%s volume %s float64, patch %s, %d rounds alternated x %d volumes per child, %d CPUs" % (
        bench.kernel_source_hash(), SHAPE, PATCH, args.rounds, args.reps, len(os.sched_getaffinity(0))), flush=True)
    res = {arm: dict(end_to_end_s=[], device_s=[]) for arm in trees}
    for r in range(args.rounds):
        for arm, tree in trees.items():
            one = run_child(tree, arm, 0.5, args.reps, args.limit)
            for key in ("end_to_end_s", "device_s"):
                res[arm][key] += one[key]
            res[arm]["tiles"], res[arm]["checksum"], gpu = one["tiles"], one["checksum"], one["gpu"]
            print("round %d %-8s %d tiles  end to end %s  device %s" % (r, arm, one["tiles"], " ".join("%.4f" % t for t in one["end_to_end_s"]),
                                                                        " ".join("%.4f" % t for t in one["device_s"])), flush=True)
    print("# %s, overlap 0.5, seconds per volume: median (min, max) over %d measurements" % (gpu, args.rounds * args.reps))
    for arm in trees:
        print("%-8s end to end %.4f (%.4f, %.4f)   device %.4f (%.4f, %.4f)   checksum %.9e" % (
            (arm,) + stats(res[arm]["end_to_end_s"]) + stats(res[arm]["device_s"]) + (res[arm]["checksum"],)), flush=True)
    ok = True
    for key, what in (("end_to_end_s", "end to end"), ("device_s", "device")):
        med_p, lo_p, hi_p = stats(res["parent"][key])
        med_n, _, _ = stats(res["none"][key])
        med_g, _, _ = stats(res["gaussian"][key])
        inside = lo_p <= med_n <= hi_p
        ok = ok and inside
        print("%-10s none's median %.4f s is %s parent's spread [%.4f, %.4f] (parent's median %.4f); gaussian / none = %.4f (+%.2f ms)" % (
            what, med_n, "inside" if inside else "OUTSIDE", lo_p, hi_p, med_p, med_g / med_n, (med_g - med_n) * 1e3), flush=True)
    assert res["parent"]["checksum"] == res["none"]["checksum"] or abs(res["parent"]["checksum"] - res["none"]["checksum"]) <= 1e-9 * abs(
        res["none"]["checksum"]), "blend=None does not compute what the parent computes"
    print("# gaussian at three overlaps (one child each, %d volumes)" % args.reps)
    for overlap in (0.9, 0.75, 0.5):
        one = run_child(ROOT, "gaussian", overlap, args.reps, args.limit)
        print("gaussian overlap %.2f: %5d tiles  end to end %.4f (%.4f, %.4f)   device %.4f (%.4f, %.4f)" % (
            (overlap, one["tiles"]) + stats(one["end_to_end_s"]) + stats(one["device_s"])), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
