"""bench.py: a plain run times the headline and nothing else; --full adds what the headline does not need (sustained
rate, instrumented roofline pass, CPU baseline, secondary workloads), each part still dropped by its --no-* option."""
import json
import os
import subprocess
import sys

import pytest

from conftest import REPO

BENCH = os.path.join(REPO, "bench.py")
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
EXTRAS = ("sustained_1000_updates_per_sec", "sustained_runs", "roofline", "secondary", "cpu_baseline",
          "speedup_vs_cpu_baseline")
ROWS = ("--rows-per-gpu", "20000")                   # the headline's network and batch on a small replay


def _bench(*args):
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "2", *args],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_carries_the_headline_only():
    out = _bench(*ROWS)
    assert all(k in out for k in HEADLINE) and out["steps"] == 3 and out["warmup"] == 2
    assert not set(EXTRAS) & set(out), sorted(out)
    cql = _bench("--workload", "cql")
    assert all(k in cql for k in HEADLINE) and cql["steps"] == 3
    assert not set(EXTRAS) & set(cql), sorted(cql)


@pytest.mark.gpu
def test_full_run_adds_the_extras_and_keeps_the_no_options():
    out = _bench(*ROWS, "--full", "--no-cpu-baseline", "--no-secondary")
    assert all(k in out for k in HEADLINE)
    assert out["sustained_1000_updates_per_sec"] > 0 and len(out["sustained_runs"]) == 5
    assert out["roofline"]["kernel"] and out["roofline"]["launches"] > 0
    assert "cpu_baseline" not in out and "secondary" not in out
    out = _bench(*ROWS, "--full", "--no-cpu-baseline", "--no-secondary", "--no-roofline")
    assert "roofline" not in out and "sustained_1000_updates_per_sec" in out
    cql = _bench("--workload", "cql", "--full", "--no-cpu-baseline")
    assert cql["roofline"]["launches"] > 0 and "cpu_baseline" not in cql
