"""bench.py itself on the GPU: a plain run (the headline line, nothing after the timed steps) with --dump-outputs, the dumped scores
against the CPU oracle and against a strong-scaling run of the same list, and --full with everything it adds."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _bench(*argv, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "LCHD_BENCH_FORCE_DIST")}
    run = subprocess.run([sys.executable, str(ROOT / "bench.py"), *argv], cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert run.returncode == 0, run.stderr[-3000:]
    return json.loads(run.stdout.strip().splitlines()[-1])


def test_plain_run_dumps_the_last_step(tmp_path, oracle):
    sys.path.insert(0, str(ROOT))
    import bench

    line = _bench("--gpus", "1", "--steps", "3", "--warmup", "1", "--pairs", "200000", "--dump-outputs", str(tmp_path / "weak"))
    assert all(k in line for k in HEADLINE) and line["steps"] == 3 and line["unit"] == "pairs/s" and line["dtype"] == "f64"
    assert line["value"] == pytest.approx(200_000 / (line["ms_per_step"] * 1e-3))
    for extra in ("roofline", "cpu_baseline", "max_abs_err_vs_cpu", "value_incl_h2d_d2h", "extras"):
        assert extra not in line, extra
    scores = np.load(tmp_path / "weak" / "scores.npy")
    assert scores.dtype == np.float64 and scores.shape == (200_000,) and np.all((scores >= 0) & (scores <= 1))
    w = bench.make_workload("c2a", 0, 200_000)
    lo = oracle.LoCoHD([f"c{i}" for i in range(w["C"])], oracle.WeightFunction(*w["wf"]))
    tag = np.zeros(w["n"], dtype=np.int32)
    sample = w["pairs"][::97]
    want = np.asarray(lo.from_arrays(w["xyz_a"], w["cat_a"], tag, w["xyz_b"], w["cat_b"], tag, sample, w["thr"]))
    assert np.max(np.abs(scores[::97] - want)) <= 1e-6
    # the same list sharded (one rank: its share is the whole list, in the partition's order) comes back in anchor-pair order
    _bench("--gpus", "1", "--steps", "2", "--warmup", "0", "--pairs", "200000", "--scaling", "strong", "--dump-outputs", str(tmp_path / "strong"))
    assert np.array_equal(np.load(tmp_path / "strong" / "scores.npy"), scores)


def test_full_run_keeps_everything_beyond_the_headline():
    line = _bench("--gpus", "1", "--steps", "2", "--warmup", "1", "--pairs", "200000", "--full")
    assert all(k in line for k in HEADLINE) and line["steps"] == 2
    assert {"bound", "achieved", "frac"} <= set(line["roofline"]) and line["config"]["mean_env_points_per_pair"] > 0
    assert line["cpu_baseline"]["value"] > 0 and line["max_abs_err_vs_cpu"] <= 1e-6 and "parity_failed" not in line
    assert {"unique_anchor_call", "two_streams"} <= set(line["extras"]) and line["extras"]["host_call_scores_equal_device_resident"] is True
    assert line["value_incl_h2d_d2h"]["value"] > 0
