"""Child process of test_gpu_overlap_losses.py: under FMRI_DETERMINISTIC=1 (set by the parent before this interpreter starts, so that the
engine reads it in a fresh process), two engines from the same seed take the same two focal-Tversky steps; every loss slot, dlogits, the
gradient and the weights must agree bit for bit.  Prints BITS EQUAL and exits 0, else raises."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "fetal-mri-segmentation_amd")):
    sys.path.insert(0, p)

import numpy as np          # noqa: E402
import torch                # noqa: E402


def main():
    from fmri_hip import ops
    from fmri_hip.engine import UNetEngine, UNetPlan
    assert os.environ.get("FMRI_DETERMINISTIC") == "1"
    N, sp, L = 2, (16, 16, 16), 3
    rs = np.random.RandomState(11)
    x = torch.from_numpy(rs.randn(N, *sp, 1).astype(np.float32)).cuda()
    y = torch.from_numpy((rs.rand(N, *sp, L) > 0.7).astype(np.uint8)).cuda().reshape(-1)
    runs = []
    for _ in range(2):
        eng = UNetEngine(UNetPlan(in_channels=1, spatial=sp, depth=2, n_base_filters=8, n_labels=L), N, dtype=torch.float32, seed=4)
        try:
            assert eng.deterministic
            eng.loss_kind, eng.loss_param, eng.loss_overlap = ops.LOSS_KINDS["focal_tversky_loss"], 1.0, (0.3, 0.7, 4.0 / 3, 0.0)
            snaps = []
            for step in (1, 2):
                eng.forward(x)
                eng.loss_forward(y)
                eng.backward(y)
                snaps += [("sums %d" % step, eng.log_sums().clone()), ("dlogits %d" % step, eng.dlogits.clone()), ("G %d" % step, eng.G.clone())]
                eng.adam_step(1e-3)
                snaps.append(("P %d" % step, eng.P.clone()))
            torch.cuda.synchronize()
            runs.append(snaps)
        finally:
            eng.close()
    a, b = runs
    for (name, ta), (_, tb) in zip(a, b):
        assert bool(torch.isfinite(ta.double()).all()), name
        view = torch.int64 if ta.element_size() == 8 else torch.int32
        assert torch.equal(ta.view(view), tb.view(view)), "%s differs between the two runs" % name
    value = float(a[0][1][ops.SUMS_OVERLAP_VALUE])
    assert 0.0 < value < 1.0 and float(a[1][1].abs().max()) > 0 and not torch.equal(a[3][1], a[7][1])
    print("BITS EQUAL loss %.17g" % value)


if __name__ == "__main__":
    main()
