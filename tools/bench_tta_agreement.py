#!/usr/bin/env python3
"""Cost of the agreement kernel at the configs[4] stack (8 variants of a 160 x 256 x 256 float64 volume, 671 MB), in device time per call:
  a  parent    the parent commit's `ops.median_stack_f64` (a checkout of it, built, under --parent-tree; default build/parent):
                   git archive HEAD~1 fetal-mri-segmentation_amd include | tar -x -C build/parent && make -C build/parent/fetal-mri-segmentation_amd/csrc
  b  median    this tree's `ops.median_stack_f64`: has to lie inside a's run-to-run spread
  c  counts    `ops.tta_agreement_f64(stack, maps=())`: median + counts, the bytes of the median
  d  maps      `ops.tta_agreement_f64(stack)`: median, four maps, counts: (K + 5) / (K + 1) = 1.44x the bytes of the median
  e  torch     what a caller writes today on the device: stack.mean(0), stack.var(0, unbiased=False), the entropy, the thresholds, the
               disagreement, the three count sums, plus `median_stack_f64`
Every arm runs in a child process of its own (one package per process), the arms ALTERNATED round by round; a child warms up, then times
REPS calls between device events.  Reported per arm: median, min and max over rounds x REPS, and the bytes per second of c and d.
The bars, all against a's median of the same run: c <= 1.25 a; d <= 1.25 * 1.44 a (the kernel is bound by the memory traffic, 25 % are
the allowance for ballots, two log2 and the registers next to the sort network).  The tool exits 1 when b is outside a's spread or a
bar is missed.  Then end to end: `predict_volume(augment="flip")` with and without return_agreement=True, numpy in, numpy out."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, SHAPE = 8, (160, 256, 256)
PATCH = (64, 128, 128)
ARMS = ("parent", "median", "counts", "maps", "torch")
COPY_RATE = 6.3e12                                            # bytes per second of a float4 copy on the MI355X


def torch_arm(ops, stack, thr=0.5):
    import torch
    mu = stack.mean(0)
    var = stack.var(0, unbiased=False)
    p = mu.clamp(0.0, 1.0)
    ent = -(torch.xlogy(p, p) + torch.xlogy(1.0 - p, 1.0 - p)) / 0.6931471805599453
    med = ops.median_stack_f64(stack)
    V, M = stack > thr, med > thr
    dis = (V != M).sum(0).double() / stack.shape[0]
    counts = torch.cat([M.sum().reshape(1), V.flatten(1).sum(1), (V & M).flatten(1).sum(1)])
    return med, mu, var, ent, dis, counts


def child(tree, arm, reps):
    sys.path.insert(0, os.path.join(tree, "fetal-mri-segmentation_amd"))
    import torch
    from fmri_hip import ops
    assert torch.cuda.is_available(), "tools/bench_tta_agreement.py measures on the GPU"
    assert os.path.realpath(ops.__file__).startswith(os.path.realpath(tree)), (ops.__file__, tree)
    g = torch.Generator(device="cuda").manual_seed(0)
    stack = torch.rand((K,) + SHAPE, generator=g, dtype=torch.float64, device="cuda")
    fn = {"parent": lambda: ops.median_stack_f64(stack), "median": lambda: ops.median_stack_f64(stack),
          "counts": lambda: ops.tta_agreement_f64(stack, maps=()), "maps": lambda: ops.tta_agreement_f64(stack),
          "torch": lambda: torch_arm(ops, stack)}[arm]
    for _ in range(5):
        out = fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e-3)
    med = out["median"] if isinstance(out, dict) else (out[0] if isinstance(out, tuple) else out)
    print("RESULT " + json.dumps(dict(arm=arm, seconds=times, checksum=float(med.sum()), gpu=torch.cuda.get_device_name(0))), flush=True)


def child_end_to_end(tree, arm, reps):
    sys.path.insert(0, os.path.join(tree, "fetal-mri-segmentation_amd"))
    os.environ.setdefault("FMRI_DTYPE", "bf16")
    import numpy as np
    import torch
    import fetal_net.model as fmodel
    from fetal_net import pipeline
    model = fmodel.unet_model_3d(input_shape=(1,) + PATCH)
    cfg = {"patch_shape": list(PATCH[:2]), "patch_depth": PATCH[2]}
    vol = 100.0 + 50.0 * np.random.RandomState(0).randn(*SHAPE)
    kw = dict(return_agreement=True) if arm == "e2e_agreement" else {}
    for _ in range(2):
        out = pipeline.predict_volume(vol, model, cfg, overlap_factor=0.5, augment="flip", **kw)
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = pipeline.predict_volume(vol, model, cfg, overlap_factor=0.5, augment="flip", **kw)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    extra = dict(estimated_dice=float(out["agreement"].estimated_dice[0])) if kw else {}
    print("RESULT " + json.dumps(dict(arm=arm, seconds=times, checksum=float(out["prediction"].sum()), gpu=torch.cuda.get_device_name(0),
                                      **extra)), flush=True)


def run_child(tree, arm, reps, limit):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", arm, "--tree", tree, "--reps", str(reps)]
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--e2e-reps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=180, help="seconds one child may take")
    ap.add_argument("--child", default=None)
    ap.add_argument("--tree", default=ROOT)
    args = ap.parse_args()
    if args.child:
        return (child_end_to_end if args.child.startswith("e2e") else child)(args.tree, args.child, args.reps)
    sys.path.insert(0, ROOT)
    import bench
    if not os.path.exists(os.path.join(args.parent_tree, "fetal-mri-segmentation_amd", "lib", "libfmri_hip.so")):
        raise SystemExit("no built parent tree under %s (see the docstring): the bars compare with it" % args.parent_tree)
    n = SHAPE[0] * SHAPE[1] * SHAPE[2]
    print("# tools/bench_tta_agreement.py kernel_source_hash=%s stack %d x %s float64 (%.0f MB), %d rounds alternated x %d calls per child" % (
        bench.kernel_source_hash(), K, SHAPE, K * n * 8 / 1e6, args.rounds, args.reps), flush=True)
    res = {arm: [] for arm in ARMS}
    sums = {}
    for r in range(args.rounds):
        for arm in ARMS:
            one = run_child(args.parent_tree if arm == "parent" else ROOT, arm, args.reps, args.limit)
            res[arm] += one["seconds"]
            sums[arm], gpu = one["checksum"], one["gpu"]
            print("round %d %-7s %s" % (r, arm, " ".join("%.1f" % (t * 1e6) for t in one["seconds"])), flush=True)
    print("# %s, microseconds per call: median (min, max) over %d measurements" % (gpu, args.rounds * args.reps))
    moved = {"parent": (K + 1) * n * 8, "median": (K + 1) * n * 8, "counts": (K + 1) * n * 8, "maps": (K + 5) * n * 8}
    for arm in ARMS:
        mid, lo, hi = stats(res[arm])
        rate = "   %.2f TB/s of %d MB (%.0f %% of the %.1f TB/s copy rate)" % (
            moved[arm] / mid / 1e12, moved[arm] / 1e6, 100 * moved[arm] / mid / COPY_RATE, COPY_RATE / 1e12) if arm in moved else ""
        print("%-7s %8.1f (%8.1f, %8.1f)   median checksum %.9e%s" % (arm, mid * 1e6, lo * 1e6, hi * 1e6, sums[arm], rate), flush=True)
    assert len({sums[arm] for arm in ARMS}) == 1, "the arms' medians differ"
    a, a_lo, a_hi = stats(res["parent"])
    b, c, d, e = (stats(res[arm])[0] for arm in ARMS[1:])
    ok_b = a_lo <= b <= a_hi
    ok_c, ok_d = c <= 1.25 * a, d <= 1.25 * (K + 5) / (K + 1) * a
    print("b: this tree's median_stack_f64 %.1f us is %s the parent's spread [%.1f, %.1f] us" % (b * 1e6, "inside" if ok_b else "OUTSIDE", a_lo * 1e6, a_hi * 1e6))
    print("c: median + counts   = %.3f x a (bar 1.25): %s" % (c / a, "met" if ok_c else "MISSED"))
    print("d: median + 4 maps + counts = %.3f x a (bar 1.25 x %.3f = %.3f): %s" % (d / a, (K + 5) / (K + 1), 1.25 * (K + 5) / (K + 1), "met" if ok_d else "MISSED"))
    print("e: the torch composition = %.2f x d; it replaces a download of the stack (%d MB) and five or six numpy passes over it" % (e / d, K * n * 8 // 10 ** 6))
    print("# end to end, predict_volume(augment='flip'), numpy in, numpy out, seconds per volume (%d per child, %d rounds alternated)" % (args.e2e_reps, args.rounds), flush=True)
    e2e = {"e2e_plain": [], "e2e_agreement": []}
    info = {}
    for r in range(args.rounds):
        for arm in e2e:
            one = run_child(ROOT, arm, args.e2e_reps, args.limit)
            e2e[arm] += one["seconds"]
            info[arm] = one
    for arm in e2e:
        print("%-14s %.4f (%.4f, %.4f)   prediction checksum %.9e%s" % ((arm,) + stats(e2e[arm]) + (info[arm]["checksum"],
              "   estimated Dice %.4f" % info[arm]["estimated_dice"] if "estimated_dice" in info[arm] else "")), flush=True)
    print("return_agreement=True adds %.1f ms: four more volumes of 84 MB come down" % ((stats(e2e["e2e_agreement"])[0] - stats(e2e["e2e_plain"])[0]) * 1e3))
    return 0 if ok_b and ok_c and ok_d else 1


if __name__ == "__main__":
    sys.exit(main())
