"""bench.py --dump-outputs: what the timed path computed in its last step, as DIR/<name>.npy, bounded in size and the
same from run to run on the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

sys.path.insert(0, REPO)


def test_dump_outputs_writes_float_arrays_whole_when_they_fit(tmp_path):
    import bench
    bench.dump_outputs(str(tmp_path), {"loss": np.array([1.5], np.float32), "grads": np.arange(12.0).reshape(4, 3),
                                       "counts": np.arange(5)})
    loss, grads, counts = (np.load(tmp_path / (n + ".npy")) for n in ("loss", "grads", "counts"))
    assert loss.dtype == np.float32 and loss.tolist() == [1.5]
    assert grads.dtype == np.float64 and grads.shape == (4, 3) and np.array_equal(grads, np.arange(12.0).reshape(4, 3))
    assert counts.dtype == np.float32 and counts.tolist() == [0, 1, 2, 3, 4]


def test_dump_outputs_samples_the_same_elements_past_the_limit(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_LIMIT", 2 * 4096 + 4000)   # 4000 bytes left for the arrays
    a = np.random.default_rng(5).standard_normal(3000).astype(np.float32)
    b = np.random.default_rng(6).standard_normal(1000).astype(np.float32)
    for d in ("one", "two"):
        bench.dump_outputs(str(tmp_path / d), {"a": a, "b": b})
    files = [tmp_path / d / n for d in ("one", "two") for n in ("a.npy", "b.npy")]
    assert sum(os.path.getsize(f) for f in files[:2]) <= bench.DUMP_LIMIT
    sa, sb = np.load(files[0]), np.load(files[1])
    assert sa.size == 3000 * 4000 // 16000 and sb.size == 1000 * 4000 // 16000
    assert np.isin(sa, a).all() and np.isin(sb, b).all()
    assert np.array_equal(sa, np.load(files[2])) and np.array_equal(sb, np.load(files[3]))


@pytest.mark.gpu
def test_bench_dumps_the_last_timed_step_and_repeats_it_bit_for_bit(tmp_path):
    """Two runs of the same small bench command: the loss, parameters and gradients of the last timed step are written
    as float32, the loss is the line's final_loss, and both runs write the same arrays bit for bit."""
    runs = []
    for d in ("one", "two"):
        cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
               "--mols", "128", "--dataset-mols", "4096", "--no-cpu-baseline", "--no-secondary", "--no-roofline",
               "--dump-outputs", str(tmp_path / d)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=REPO)
        assert r.returncode == 0, r.stdout[-1500:] + "\n" + r.stderr[-1500:]
        line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        assert line["steps"] == 3
        runs.append(({n: np.load(tmp_path / d / (n + ".npy")) for n in ("loss", "params", "grads")}, line))
    (out, line), (again, _) = runs
    assert all(a.dtype == np.float32 for a in out.values())
    assert out["loss"].shape == (1,) and abs(float(out["loss"][0]) - line["final_loss"]) <= 1e-5 * abs(line["final_loss"])
    assert out["params"].shape == out["grads"].shape and out["params"].size > 100000
    assert np.isfinite(out["params"]).all() and np.isfinite(out["grads"]).all() and np.abs(out["grads"]).max() > 0
    for n in out:
        assert np.array_equal(out[n], again[n]), n
