"""-m gpu: what `python bench.py --gpus 1` prints.  A plain run carries the headline alone (set-up, warm-up, the timed
window and its repetitions, --dump-outputs, the line); --full adds the records that need runs of their own."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

# the records of the N = 1 line that only --full takes
FULL_ONLY = ("roofline", "roofline_dense_only", "hbm_bound", "config5", "cli_end_to_end", "cpu_baseline",
             "speedup_vs_cpu_1core", "cpu_baseline_allcores")


def _line(args, tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + args,
                       capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.split("\n") if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_is_the_headline_alone(tmp_path):
    d = tmp_path / "dump"
    out = _line(["--steps", "20", "--warmup", "5", "--dump-outputs", str(d)], tmp_path)
    assert out["metric"] == "edge-updates/sec (link-sampling SVI step)" and out["unit"] == "edge-updates/s"
    assert out["higher_is_better"] is True and out["dtype"] == "f64" and out["n_gpus"] == 1
    assert out["steps"] == 20 and out["warmup"] == 5 and out["full"] is False
    # value is links per sweep over ms_per_step, and both come from the median of the repeated windows
    links = int(re.search(r"links/sweep=(\d+)", out["config"]["workload"]).group(1))
    assert out["value"] > 0 and abs(out["value"] * out["ms_per_step"] * 1e-3 / links - 1.0) < 1e-9
    assert out["repeat"]["reps"] == 50 and out["repeat"]["end_state_identical"] is True
    assert not [k for k in FULL_ONLY if k in out], sorted(out)
    assert {"gamma", "lambda", "converged"} <= set(out["dump_outputs"]["arrays"])
    g = np.load(str(d / "gamma.npy"))
    assert g.shape == (17903, 20) and np.all(g > 0)


def test_full_run_adds_the_records(tmp_path):
    out = _line(["--steps", "20", "--warmup", "5", "--reps", "5", "--full",
                 "--no-hbm-bound", "--no-config5", "--no-cli", "--no-cpu-baseline"], tmp_path)
    assert out["full"] is True and out["value"] > 0 and out["repeat"]["reps"] == 5
    assert out["roofline"]["launches_timed"] >= 10 and 0 < out["roofline"]["frac"] <= 1.0
    assert out["roofline_dense_only"]["launches_timed"] >= 10
    # the --no-* options still leave their records out
    assert not [k for k in ("hbm_bound", "config5", "cli_end_to_end", "cpu_baseline") if k in out]
