"""bench.py end to end on a small map: a plain run prints the headline line and nothing it would need an extra leg for;
--full adds the profiled step's figures, the trajectory errors and the sustained leg."""
import json
import math
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "n_gpus", "steps", "warmup", "iterations_executed",
            "final_cost", "initial_cost", "config"}
FULL_ONLY = {"timed_region", "ate_rmse_m", "phase_ms_per_iteration", "roofline", "roofline_potrf", "roofline_iteration", "roofline_build", "sustained"}


def bench_line(*extra):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "small", "--steps", "2", "--warmup", "1", *extra],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_bench_plain_run_prints_the_headline_only():
    d = bench_line()
    assert HEADLINE <= d.keys(), HEADLINE - d.keys()
    assert not FULL_ONLY & d.keys(), FULL_ONLY & d.keys()
    assert d["steps"] == 2 and d["warmup"] == 1 and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["iterations_executed"] > 0
    assert abs(d["value"] - d["iterations_executed"] / (d["steps"] * d["ms_per_step"] * 1e-3)) <= 1e-9 * d["value"]
    assert d["final_cost"] < d["initial_cost"]


@pytest.mark.gpu
def test_bench_full_run_adds_the_other_legs():
    d = bench_line("--full", "--no-cpu-baseline", "--no-e2e", "--sustain-s", "0.5")
    assert (HEADLINE | FULL_ONLY) <= d.keys(), (HEADLINE | FULL_ONLY) - d.keys()
    assert d["phase_ms_per_iteration"]["linearise+schur"] > 0 and d["sustained"]["steps"] >= 1
    assert set(d["ate_rmse_m"]) == {"initial", "final", "initial_sim3", "final_sim3"}
    assert all(math.isfinite(v) and v >= 0 for v in d["ate_rmse_m"].values())
    assert "nnzS_fill" in d["config"]
