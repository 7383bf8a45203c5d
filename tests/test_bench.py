"""bench.py: a plain run prints the headline alone; `--full` adds the legs outside the timed region."""
import importlib
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LEGS = ("value_incl_frame_d2h", "roofline", "cpu_baseline")


def test_full_is_off_by_default(monkeypatch):
    sys.path.insert(0, ROOT)
    bench = importlib.import_module("bench")
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1"])
    assert bench.parse().full is False
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1", "--full"])
    assert bench.parse().full is True


def _run_bench(*extra):
    """bench.py in a child process on a small frame of the canonical scene; returns its JSON result line."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "1",
           "--width", "256", "--height", "256", "--spp", "4"] + list(extra)
    out = subprocess.run(cmd, check=True, timeout=600, capture_output=True, text=True).stdout
    return json.loads(out.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_run_skips_the_extra_legs_and_full_runs_them():
    plain = _run_bench()
    assert plain["value"] > 0 and plain["ms_per_step"] > 0 and plain["unit"] == "Mrays/s"
    for k in LEGS:
        assert plain[k] is None, k

    full = _run_bench("--full", "--cpu-seconds", "0.1")
    for k in LEGS:
        assert full[k] is not None, k
    assert full["config"]["rays_per_frame"] == plain["config"]["rays_per_frame"]
    assert full["roofline"]["raw"]["rays"] == full["config"]["rays_per_frame"]  # counting pass = the timed frame's rays
    assert full["value_incl_frame_d2h"]["value"] > 0 and full["cpu_baseline"]["value"] > 0
