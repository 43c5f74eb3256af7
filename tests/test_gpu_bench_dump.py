"""bench.py --dump-outputs on the GPU: two runs of the real timed path with the same arguments dump the same outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _files(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def _two_runs(tmp_path, args, env=None):
    lines, dumps = [], []
    for k in range(2):
        d = str(tmp_path / ("run%d" % k))
        r = subprocess.run([sys.executable, BENCH, "--gpus", "1"] + args + ["--no-secondary", "--val-dice-steps", "0", "--no-cpu-baseline",
                                                                           "--dump-outputs", d],
                           capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
        assert r.returncode == 0, r.stderr[-3000:]
        lines.append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]))
        dumps.append(_files(d))
    a, b = dumps
    assert set(a) == set(b) == {"sums", "logits", "params"}
    for line in lines:
        assert line["ms_per_step"] > 0
        assert line["dump_outputs"] == {"sums": [8], "logits": [4, 64, 128, 128, 1], "params": [1 << 22]}
    for k in a:
        assert np.all(np.isfinite(a[k])), k
    assert a["sums"][1] > 0 and a["sums"][7] == 4 * 64 * 128 * 128           # foreground voxels, voxel count
    return lines, a, b


def _diff(a, b, k):
    return float(np.abs(a[k].astype(np.float64) - b[k]).max())


@pytest.mark.gpu
def test_two_dump_runs_of_the_timed_path_are_bit_identical(tmp_path):
    """with the bit-reproducible gradient sums (FMRI_DETERMINISTIC=1) the last timed step's outputs of two runs are the same bits"""
    lines, a, b = _two_runs(tmp_path, ["--steps", "6", "--warmup", "2", "--prewarm-seconds", "0.5", "--no-launch-timing"],
                            env=dict(os.environ, FMRI_DETERMINISTIC="1"))
    assert all(line["steps"] == 6 for line in lines)
    for k in a:
        assert np.array_equal(a[k], b[k]), (k, _diff(a, b, k))


@pytest.mark.gpu
def test_default_dump_runs_agree_to_rounding_after_many_steps(tmp_path):
    """the default step sums weight-gradient partials with fp32 atomics; 60 such Adam steps drift apart far beyond rounding (logits by
    several percent), which is why the dumped step starts from the seeded state: its forward pass sees the same weights and batch (the
    same logits), and its own atomics reach the sums and the updated weights only as rounding"""
    lines, a, b = _two_runs(tmp_path, ["--steps", "50", "--warmup", "10"])
    assert all(line["steps"] == 50 for line in lines)
    print("max |run0 - run1|:", {k: _diff(a, b, k) for k in a})
    assert _diff(a, b, "logits") <= 1e-6 * float(np.abs(a["logits"]).max()), _diff(a, b, "logits")
    assert _diff(a, b, "sums") <= 1e-9 * float(np.abs(a["sums"]).max()), _diff(a, b, "sums")
    assert _diff(a, b, "params") <= 1e-7, _diff(a, b, "params")     # a few float32 ulps of the largest weights (~0.3); one Adam step moves one by <= 1e-4
