"""-m gpu: a plain `bench.py --gpus 1 --steps K --warmup W` does what its headline figure needs and nothing else — no kernel-only
loop, no long run, no CPU baseline, no secondary legs — and spends at most 30 s outside its W + K steps (the time of the whole
process, start to exit, less (K + W) x ms_per_step: imports, library load, LUT build and allocations all count).  `--full` brings
every other figure back in the same line, within 10 minutes."""
import json
import os
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
DROP = ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")
STEPS, WARMUP = 20, 5
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
OUTSIDE_STEPS_MAX_S = 30.0
FULL_MAX_S = 600.0


def _bench(extra, timeout):
    env = {k: v for k, v in os.environ.items() if k not in DROP}
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP)] + extra, env=env,
                       capture_output=True, text=True, timeout=timeout)
    wall = time.perf_counter() - t0
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, r.stderr[-3000:]
    return json.loads(lines[0]), wall


def test_plain_run_times_the_steps_and_nothing_else():
    out, wall = _bench([], 300)
    outside = wall - (STEPS + WARMUP) * out["ms_per_step"] * 1e-3
    print(f"plain run: {wall:.2f} s start to exit, {outside:.2f} s outside its {WARMUP} + {STEPS} steps")
    assert out["full"] is False and out["steps"] == STEPS and out["warmup"] == WARMUP and out["n_gpus"] == 1
    assert out["value"] > 0 and out["ms_per_step"] > 0 and out["unit"] == "env-steps/s" and out["dtype"] == "u8"
    assert out["higher_is_better"] is True
    assert abs(out["value"] - 8192 * 32 * STEPS / (out["ms_per_step"] * STEPS * 1e-3)) < 1e-6 * out["value"]
    assert out["roofline"] is None and out["cpu_baseline"] is None and out["ranks"][0]["kernel_ms"] is None
    assert not {"long_run", "python_api", "secondary"} & set(out)
    assert outside <= OUTSIDE_STEPS_MAX_S, f"{outside:.1f} s outside the steps"


def test_full_run_measures_everything_else_too():
    plain, _ = _bench([], 300)
    out, wall = _bench(["--full"], FULL_MAX_S)
    print(f"--full run: {wall:.1f} s start to exit")
    assert wall <= FULL_MAX_S and out["full"] is True
    for k in HEADLINE:   # the same headline, whatever follows the timed region
        assert k in out and (out[k] == plain[k] if k not in ("value", "ms_per_step") else out[k] > 0), k
    assert out["roofline"]["frac"] > 0.05 and out["roofline"]["kernel_ms"] > 0 and out["ranks"][0]["kernel_ms"] > 0
    assert out["roofline"]["plain_fill"]["ms"] > 0
    assert out["long_run"]["steps"] == 2000 and out["long_run"]["value"] > 0 and out["python_api"]["value"] > 0
    assert out["cpu_baseline"]["kind"] == "port" and out["cpu_baseline"]["value"] > 0
    sec = out["secondary"]
    assert "error" not in sec and "failed" not in sec, sec
    assert sec["config3"]["update"]["ms"] > 0 and sec["config2"]["ms"] > 0
