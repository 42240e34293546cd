"""bench.py --dump-outputs: what the timed path computed in its last step, written as DIR/<name>.npy within 64 MB,
the same from run to run with the same arguments."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

BENCH = os.path.join(REPO, "bench.py")


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_keeps_float32_widens_the_rest_and_samples_within_the_budget(tmp_path):
    import bench
    arrays = {"losses": np.array([0.5, 1.5, -2.0], np.float32), "count": torch.tensor(7),
              "small.weight": torch.arange(12, dtype=torch.float32).view(3, 4),
              "x64": np.linspace(0, 1, 5), "big.weight": torch.randn(4096, 4096)}
    bench.dump_outputs(str(tmp_path / "a"), arrays)
    bench.dump_outputs(str(tmp_path / "b"), arrays)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == sorted(arrays)
    assert a["losses"].dtype == np.float32 and np.array_equal(a["losses"], arrays["losses"])
    assert a["count"].dtype == np.float64 and a["count"] == 7
    assert a["x64"].dtype == np.float64 and np.array_equal(a["x64"], arrays["x64"])
    assert a["small.weight"].shape == (3, 4) and np.array_equal(a["small.weight"], arrays["small.weight"].numpy())
    # 64 MB of float32 does not fit: a fixed sample of the flat array, the same in both dumps, elements unchanged
    big = arrays["big.weight"].numpy().ravel()
    assert a["big.weight"].ndim == 1 and 0 < a["big.weight"].size < big.size
    assert np.array_equal(a["big.weight"], b["big.weight"])
    assert np.isin(a["big.weight"], big).all()
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 64_000_000


def test_dump_needs_a_single_process_run(tmp_path):
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True)
    assert r.returncode == 2 and "--dump-outputs" in r.stderr
    assert not os.listdir(tmp_path)


def _bench_dump(out_dir, steps):
    env = dict(os.environ, PORL_BENCH_SUSTAINED="0")
    cmd = [sys.executable, BENCH, "--gpus", "1", "--steps", str(steps), "--warmup", "2", "--hidden", "256",
           "--batch", "256", "--rows-per-gpu", "20000", "--no-secondary", "--no-cpu-baseline", "--no-roofline",
           "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return _load(out_dir)


@pytest.mark.gpu
def test_bench_dump_is_the_last_timed_update_and_repeats(tmp_path):
    a = _bench_dump(tmp_path / "a", 3)
    b = _bench_dump(tmp_path / "b", 3)
    c = _bench_dump(tmp_path / "c", 4)
    assert "losses" in a and a["losses"].shape == (3,) and np.isfinite(a["losses"]).all()
    assert any(k.startswith("vf.") for k in a) and any(k.startswith("goal_policy.") for k in a)
    assert sorted(a) == sorted(b) == sorted(c)
    for k in a:
        assert a[k].dtype == np.float32 and np.isfinite(a[k]).all(), k
        np.testing.assert_allclose(a[k], b[k], rtol=1e-5, atol=1e-6, err_msg=k)
    # one more timed step is one more update: --steps is the number of updates the dump comes after
    assert not np.array_equal(a["losses"], c["losses"])
    assert any(not np.array_equal(a[k], c[k]) for k in a if k.startswith("vf."))
