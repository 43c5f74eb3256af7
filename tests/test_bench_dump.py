"""bench.py --dump-outputs on the CPU: the files dump_outputs writes (names, dtypes, the 64 MB bound, fixed samples of large outputs) with a
stand-in engine, and `--steps` validation.  tests/test_gpu_bench_dump.py runs the real timed path."""
import os
import subprocess
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _files(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_small_outputs_are_written_whole(tmp_path):
    import bench
    eng = types.SimpleNamespace(logits=torch.randn(2 * 4 * 8 * 8, 1), P=torch.randn(1000))
    sums = torch.arange(16, dtype=torch.float64)
    sums[9] = float("inf")                              # a focal-loss slot of a saturated sigmoid: not one of the Dice step's 8 sums
    shapes = bench.dump_outputs(str(tmp_path), eng, sums, 2, (4, 8, 8))
    got = _files(str(tmp_path))
    assert shapes == {"sums": [8], "logits": [2, 4, 8, 8, 1], "params": [1000]}
    assert got["sums"].dtype == np.float64 and np.array_equal(got["sums"], np.arange(8.0))
    assert got["logits"].dtype == np.float32 and np.array_equal(got["logits"].reshape(-1), eng.logits.numpy().reshape(-1))
    assert got["params"].dtype == np.float32 and np.array_equal(got["params"], eng.P.numpy())


def test_large_outputs_are_a_fixed_sample_within_64_mb(tmp_path):
    import bench
    n = (1 << 23) + 5
    eng = types.SimpleNamespace(logits=torch.arange(n, dtype=torch.float32).reshape(n, 1), P=torch.arange(n, dtype=torch.float32))
    bench.dump_outputs(str(tmp_path / "a"), eng, torch.zeros(16, dtype=torch.float64), 1, (n, 1, 1))
    bench.dump_outputs(str(tmp_path / "b"), eng, torch.zeros(16, dtype=torch.float64), 1, (n, 1, 1))
    a, b = _files(str(tmp_path / "a")), _files(str(tmp_path / "b"))
    assert sum(os.path.getsize(os.path.join(str(tmp_path / "a"), f)) for f in os.listdir(str(tmp_path / "a"))) <= 64 << 20
    for k in a:
        assert np.array_equal(a[k], b[k]), k                        # the same sample every time
    for k in ("logits", "params"):
        v = a[k]
        assert v.ndim == 1 and v.size < n and np.all(np.diff(v) > 0)      # distinct elements in their original order (arange values)


def test_steps_must_be_positive():
    r = subprocess.run([sys.executable, BENCH, "--steps", "0", "--selftest-cpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps must be >= 1" in r.stderr

