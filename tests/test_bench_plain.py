"""bench.py without --full: the headline configuration sets up, warms up, times its steps and prints the line - no
secondary configuration, CPU baseline, parity check, eager per-kernel pass or loader / all-reduce diagnostic."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO


@pytest.mark.gpu
def test_plain_bench_run_measures_only_the_headline():
    """The headline's arguments (1 GPU, 1024 molecules of set A, trainer, 5 A) on a small dataset: the one line carries
    the contract's keys and `step_roofline`, and none of what --full adds."""
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--dataset-mols", "8192"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=REPO)
    assert r.returncode == 0, r.stdout[-1500:] + "\n" + r.stderr[-1500:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["metric"].startswith("molecules/s/GPU SchNet+DDM fwd+bwd") and out["unit"] == "molecules/s"
    assert out["higher_is_better"] is True and out["dtype"] == "f32" and out["n_gpus"] == 1
    assert out["steps"] == 3 and out["warmup"] == 1 and np.isfinite(out["final_loss"])
    assert np.isfinite(out["value"]) and out["value"] > 0
    assert abs(out["value"] - 1024 * 3 / (out["ms_per_step"] * 3e-3)) < 1e-4 * out["value"]   # (the line's 6 digits)
    assert out["step_roofline"]["alg_MB_per_mol"] > 0
    assert out["cpu_baseline"] is None and out["roofline"] is None and not out.get("multi_gpu")
    for k in ("secondary", "value_24bit", "parity_vs_oracle"):
        assert k not in out, k
