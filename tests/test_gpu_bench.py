"""bench.py end to end (-m gpu), each run a fresh child process with a few steps: a plain run prints the headline figure and
writes its dump, and none of what --full adds; --full adds the oracle spot check and the roofline of the kernel pass."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _bench(*args):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5", *args]
    proc = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stdout[-3000:] + proc.stderr[-3000:]
    line = json.loads(proc.stdout.strip().splitlines()[-1])
    assert all(k in line for k in HEADLINE), line
    assert line["unit"] == "sims/s" and line["dtype"] == "f32" and line["higher_is_better"] is True
    assert line["value"] > 0 and line["ms_per_step"] > 0 and line["steps"] == 20 and line["warmup"] == 5
    return line


def test_plain_run_measures_the_headline_only(tmp_path):
    line = _bench("--dump-outputs", str(tmp_path))
    assert line["roofline"] is None and line["config"]["kernel_pass_after_timed_loop"] is False
    assert not {"configs", "cpu_baseline", "oracle_spot_check"} & set(line), sorted(line)
    assert sorted(os.listdir(tmp_path)) == ["grad_z.npy", "log_prob.npy", "red_chi2.npy"]


def test_full_run_adds_the_oracle_check_and_the_roofline():
    line = _bench("--full", "--no-configs", "--no-cpu-baseline")
    assert line["oracle_spot_check"]["ok"] and line["oracle_spot_check"]["samples"] == 4
    assert line["roofline"]["kernel_launches_timed"] >= 20 and line["config"]["kernel_pass_after_timed_loop"] is True
