"""bench.py as a command (MI355X): a plain run does only what its headline figure needs; --full adds the secondary measurements."""
import json
import os
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
OUTSIDE_STEPS_LIMIT_S = 30.0  # what a plain run may spend outside its warm-up and timed steps, start of the process to its exit


def _bench(*argv, timeout):
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().split("\n")[-1]), wall


@pytest.mark.gpu
def test_plain_run_prints_the_headline_alone_and_is_lean(tmp_path):
    steps, warmup = 5, 2
    line, wall = _bench("--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", str(tmp_path / "dump"), timeout=300)
    assert all(k in line for k in HEADLINE), sorted(line)
    assert line["unit"] == "steps/s" and line["higher_is_better"] is True and line["dtype"] == "f16" and line["value"] > 0
    assert abs(line["value"] * line["ms_per_step"] - 1e3) < 1.0  # one GPU: value = 1000 / ms_per_step
    assert line["roofline"] is None and line["cpu_baseline"] is None
    assert (tmp_path / "dump" / "grad.npy").exists() and (tmp_path / "dump" / "opt_steps.npy").exists()
    outside = wall - (steps + warmup) * line["ms_per_step"] * 1e-3
    print(f"plain run: {wall:.2f} s in all, {outside:.2f} s outside its {steps + warmup} steps")
    assert outside <= OUTSIDE_STEPS_LIMIT_S, (wall, line["ms_per_step"])


@pytest.mark.gpu
def test_full_run_carries_the_roofline_leg():
    """--full (the CPU baseline left out: minutes of host time, nothing of the device's)"""
    line, _ = _bench("--gpus", "1", "--steps", "5", "--warmup", "2", "--full", "--no-cpu-baseline", timeout=300)
    assert all(k in line for k in HEADLINE), sorted(line)
    roof = line["roofline"]
    assert roof is not None and roof["table"] and set(roof["classes"]) >= {"conv", "linear", "attention", "norm"}
    assert roof["sustained_peak"] > 0 and roof["dominant_tile_clock"] is not None
    assert line["cpu_baseline"] is None
