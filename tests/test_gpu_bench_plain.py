"""GPU: a plain `bench.py --gpus 1 --steps K --warmup W` run (no --full), in a process of its own: ONE JSON line with the
headline's keys for exactly K timed steps and nothing of what --full adds, at most 30 s of wall clock outside the
W + K steps (set-up, settle steps, compilation, the line), and --dump-outputs files within 64 MB."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_run_is_lean_and_dumps_its_last_step(tmp_path):
    steps, warmup, out = 10, 3, tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
           "--dump-outputs", str(out)]
    t0 = time.perf_counter()
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=ROOT)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    j = json.loads(lines[0])
    assert j["metric"] == "train-step images/sec (fwd+bwd) @1M Gaussians 1920x1280"
    assert j["unit"] == "images/sec" and j["higher_is_better"] is True and j["dtype"] == "f32"
    assert j["steps"] == steps and j["warmup"] == warmup
    assert j["ms_per_step"] > 0 and abs(j["value"] * j["ms_per_step"] - 1e3) < 1e-6 * 1e3
    assert j["roofline"] is None
    assert not {"workloads", "cpu_baseline", "repeat", "kernels_avg_ms", "fused_path", "without_settle_steps"} & set(j)
    outside = wall - (steps + warmup) * j["ms_per_step"] * 1e-3
    assert outside < 30.0, f"{outside:.1f} s of the run outside its {warmup} + {steps} steps"
    files = sorted(os.listdir(out))
    assert sum(os.path.getsize(out / f) for f in files) <= 64 * 10**6
    for name in ("rgb", "alpha", "loss", "grad_means", "grad_features_rest", "radii", "rows"):
        assert name + ".npy" in files, name
    for f in files:
        a = np.load(out / f)
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), f
    assert np.load(out / "rgb.npy").shape == (1280, 1920, 3) and np.load(out / "alpha.npy").shape == (1280, 1920)
