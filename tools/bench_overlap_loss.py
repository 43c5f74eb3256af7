#!/usr/bin/env python3
"""Loss head of a training step at the headline shape (batch 4 x 64x128x128 voxels, L = 1 and L = 4 labels): what an overlap loss (kind 0,
Tversky) enqueues - fmri_sigmoid_dice_fwd, fmri_label_sums, fmri_overlap_coeffs, fmri_overlap_loss_bwd - against the Dice path -
fmri_sigmoid_dice_fwd, fmri_sigmoid_loss_bwd kind 0 - whose kernels this tree shares with its parent.  Each arm is timed with device events
over `--iters` back-to-back launches, the arms alternated for `--rounds` rounds in one process; median (min - max) in microseconds, and
GB/s of the 9 bytes per element the two gradient passes have to move.  usage: python tools/bench_overlap_loss.py [--iters 50] [--rounds 7]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fetal-mri-segmentation_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    import torch
    from fmri_hip import ops
    assert torch.cuda.is_available(), "needs the GPU: there is no CPU path to time"
    nvox = 4 * 64 * 128 * 128
    for L in (1, 4):
        n = nvox * L
        g = torch.Generator(device="cuda").manual_seed(3 + L)
        logits = torch.randn(n, generator=g, device="cuda") * 3
        y = (torch.rand(n, generator=g, device="cuda") < 0.2).to(torch.uint8)
        probs, dl, dl2 = torch.empty_like(logits), torch.empty_like(logits), torch.empty_like(logits)
        sums = torch.zeros(ops.SUMS_TOTAL, dtype=torch.float64, device="cuda")
        coef = sums[ops.SUMS_OVERLAP_VALUE - 2 * L:]

        def fwd():
            sums[:16].zero_()
            ops.sigmoid_dice_fwd(logits, y, probs, sums[:16])

        def dice_bwd():
            ops.sigmoid_loss_bwd(probs, y, sums[:16], dl, 0, 1.0)

        def label_sums():
            ops.label_sums(probs, y, L, sums[16:])

        def coeffs():
            ops.overlap_coeffs(sums[16:], sums[:16], coef, L, 0, 0.5, 0.5, 1.0, 0.5)

        def overlap_bwd():
            ops.overlap_loss_bwd(probs, y, coef, dl2, L)

        arms = [("dice path: fwd + sigmoid_loss_bwd", lambda: (fwd(), dice_bwd())),
                ("overlap path: fwd + label_sums + coeffs + overlap_loss_bwd", lambda: (fwd(), label_sums(), coeffs(), overlap_bwd())),
                ("k_sigmoid_loss_bwd", dice_bwd), ("k_overlap_loss_bwd", overlap_bwd), ("k_label_sums (+ memset)", label_sums),
                ("k_overlap_coeffs", coeffs)]
        for _, fn in arms:                      # warm every arm; the coefficients and sums are in place for the stand-alone gradient arms
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        same = float((dl - dl2).abs().max()) / float(dl.abs().max())
        times = {name: [] for name, _ in arms}
        for _ in range(a.rounds):
            for name, fn in arms:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) / a.iters * 1e3)
        print("L = %d, %d elements (alpha = beta = smooth = 1/2: the gradients of the two paths differ by %.2e of the max)" % (L, n, same))
        for name, _ in arms:
            t = times[name]
            med = statistics.median(t)
            rate = "  %6.2f TB/s" % (9.0 * n / med / 1e6) if name.endswith("loss_bwd") else ""
            print("  %-60s %8.1f us (%.1f - %.1f)%s" % (name, med, min(t), max(t), rate))


if __name__ == "__main__":
    main()
