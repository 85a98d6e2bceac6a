"""-m gpu: `bench.py --dump-outputs DIR` — what the last timed step computed, written after the timed region.  Two runs with the
same arguments write the same bytes (the device warm-up runs for a time, not a number of steps, and must not leak into the
inputs of the timed steps), `--steps` is the number of timed steps, and the dumped step is the oracle's rollout number W + K of
the same tables and LUT, column for column."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
DROP = ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")
STEPS, WARMUP = 3, 2


def _bench_dump(out_dir):
    env = {k: v for k, v in os.environ.items() if k not in DROP}
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP), "--no-cpu-baseline",
                        "--no-secondary", "--dump-outputs", str(out_dir)], env=env, capture_output=True, text=True, timeout=600)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0 and lines, r.stderr[-3000:]
    return json.loads(lines[-1])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


def test_bench_dump_outputs_are_reproducible_and_match_the_oracle(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    out = _bench_dump(a)
    _bench_dump(b)
    assert out["steps"] == STEPS and out["warmup"] == WARMUP and out["ms_per_step"] > 0
    got, again = _load(a), _load(b)
    assert sorted(got) == sorted(out["dump_outputs"]["arrays"]) and out["dump_outputs"]["bytes"] <= 64 << 20
    assert all(g.dtype in (np.float32, np.float64) for g in got.values())
    for name in got:
        assert np.array_equal(got[name], again[name]), f"{name}: two runs with the same arguments differ"

    sys.path.insert(0, ROOT)
    import bench
    from oracle import Oracle

    orc = Oracle(*bench.synthetic_lut(bench.LUT_LEN, 0))
    st = orc.init_random(bench.NUM_ENVS, seed=0)
    T, tc = bench.NUM_STEPS, 0
    for i in range(WARMUP + STEPS):
        want = orc.rollout_random(st, T, seed=0, draw_base=i * T)
        tc += want["terminated_count"]
    cols = got["sample_envs"].astype(np.int64)
    for name in ("action", "value", "reward", "log_prob", "done"):
        assert np.array_equal(got[name], want[name].astype(np.float32)), name
    for name in ("obs", "legal_action_mask"):
        assert np.array_equal(got[name], want[name][:, cols].astype(np.float32)), name
    adv, tgt = orc.gae(want["done"], want["value"], want["reward"], np.zeros(bench.NUM_ENVS, np.float32), 1.0, 0.95)
    assert np.array_equal(got["advantages"], adv) and np.array_equal(got["targets"], tgt)
    assert int(got["terminated_count"][0]) == tc
