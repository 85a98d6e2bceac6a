"""Throughput of the supervised pre-trainer's graph-captured step (brl_amd/sl.py SLStep) on synthetic trajectories.

Prints one JSON line: us per step and steps/s for train_batch 128 and 1024, S = 1 and 8 steps per hipGraph, DeepMind and
FAIR, and the wall time of the reference recipe (400 000 steps of batch 128, sl.py:62) projected from the measured rate.
Timing: device events around `reps` graph replays after a warm-up of the same replays.
  python scripts/sl_throughput.py [--steps 400] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--trajectories", type=int, default=20000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="one case, e.g. DeepMind:128:8 (for a profiler run)")
    a = ap.parse_args()
    import sl_teacher as T
    from brl_amd import sl, sl_data
    from brl_amd.models import make_forward_pass
    dev = torch.device("cuda", 0)
    t0 = time.perf_counter()
    ts = sl_data.parse_trajectories(T.random_file(a.trajectories, seed=1))
    data = sl.DeviceSet(ts, dev)
    load_s = time.perf_counter() - t0
    cases = []
    for model in ("DeepMind", "FAIR"):
        for B in (128, 1024):
            for S in (1, 8):
                if a.only and a.only != f"{model}:{B}:{S}":
                    continue
                net = make_forward_pass("relu", model).init(0, device=dev)
                step = sl.SLStep(net, sl.make_optimizer(net, 1e-4), data, B, 0, 0.0, steps_per_graph=S)
                reps = max(1, a.steps // S)
                for _ in range(max(1, reps // 4)):   # warm-up: code objects, GEMM algorithm choice, caches
                    step.run(S)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    step.run(S)
                e1.record()
                torch.cuda.synchronize()
                us = e0.elapsed_time(e1) * 1000.0 / (reps * S)
                cases.append({"model": model, "train_batch": B, "steps_per_graph": S, "us_per_step": round(us, 2),
                              "steps_per_s": round(1e6 / us, 1)})
                del step, net
    ref = next((c for c in cases if (c["model"], c["train_batch"], c["steps_per_graph"]) == ("DeepMind", 128, 8)), None)
    res = {"metric": "sl_step", "trajectories": a.trajectories, "load_and_check_s": round(load_s, 2), "cases": cases,
           "device": torch.cuda.get_device_name(0)}
    if ref is not None:
        res["reference_recipe_400000x128_DeepMind_wall_s"] = round(400000 * ref["us_per_step"] / 1e6, 1)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
