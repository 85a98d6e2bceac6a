"""Round robins of random-init DeepMind 4 x 1024 networks: the batched league (brl_amd/league.py) against the loop of single
evaluations, alternated in one process.  One warm-up of each, then ``--repeats`` of each; host clock around work that ends in a
synchronise; median and spread per case.  ``--cases 16x100`` restricts the cases (for a run under rocprofv3 --kernel-trace --stats).

    python scripts/league_throughput.py [--out profiles/league/throughput.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="16x100,16x1000,64x100")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--methods", default="batched,loop")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import brl_amd
    from bench import synthetic_lut
    from brl_amd.league import all_pairs, make_league_evaluate
    from brl_amd.models import make_forward_pass
    env = brl_amd.BridgeBidding(lut=synthetic_lut(100_000, 10_000))
    fp = make_forward_pass("relu", "DeepMind")
    methods = args.methods.split(",")
    results = []
    for case in args.cases.split(","):
        M, n = (int(x) for x in case.split("x"))
        nets = [fp.init(100 + k, device="cuda") for k in range(M)]
        pairs = all_pairs(M)
        evs = {m: make_league_evaluate(env, "relu", "DeepMind", n, method=m) for m in methods}
        times = {m: [] for m in methods}
        imps = {}
        for rep in range(args.repeats + 1):            # (repeat 0 is the warm-up of each)
            for m in methods:                          # alternated
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                imp = evs[m](nets, pairs, 0)[0]
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                imps[m] = imp
                if rep:
                    times[m].append(dt)
        rec = {"networks": M, "boards": n, "matches": len(pairs)}
        if "batched" in methods:   # (untimed) the rows the batched league routes = forwards; FLOPs of their hidden layers and heads
            record = {}
            make_league_evaluate(env, "relu", "DeepMind", n, record=record)(nets, pairs, 0)
            torch.cuda.synchronize()
            rows = sum(int(gf[-1]) for b in record["batches"] for gf in b["group_first"])
            rec["iterations"] = sum(len(b["group_first"]) for b in record["batches"])
            rec["rows_routed"] = rows
            rec["layer_flops"] = rows * 2 * (480 * 1024 + 3 * 1024 * 1024)
        for m in methods:
            rec[m] = {"median_s": statistics.median(times[m]), "min_s": min(times[m]), "max_s": max(times[m]), "runs_s": times[m]}
        if len(methods) == 2:
            rec["loop_over_batched"] = rec["loop"]["median_s"] / rec["batched"]["median_s"]
            rec["max_abs_imp_difference"] = float((imps["batched"] - imps["loop"]).abs().max())
        print(json.dumps(rec), flush=True)
        results.append(rec)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
