"""Cross-play (brl_amd/crossplay.py) on the GPU: the route against the league's on the same batch, and ``cross_play`` batched against
the loop.  Methods alternate in one process, one warm-up and ``REPEATS`` repeats of each; median with min and max.

* route: ``brl_xplay_route`` with line-ups (i, i, j, j) against ``brl_league_route`` with pairs (i, j) — 64 matches x 100 and x 1000
  boards, 30 % of the boards finished, players uniform; ``CALLS`` calls back to back between two device events, per call.
* cross_play: 8 random-init DeepMind 4 x 1024 networks and a ninth as the opponent, 64 line-ups x 100 boards; host clock around work
  that ends in a synchronise.

    python scripts/crossplay_throughput.py [out.json]        (default: profiles/crossplay/throughput.json)
"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPEATS, CALLS = 3, 2000


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "runs": xs}


def route_case(nmatch, n):
    from brl_amd import _capi
    from brl_amd.crossplay import lineup_order
    from brl_amd.league import team_order
    rng = np.random.default_rng(nmatch * n)
    M = 8
    pairs = np.array([(i, j) for i in range(M) for j in range(M)])[:nmatch]
    lineups = np.stack([pairs[:, 0], pairs[:, 0], pairs[:, 1], pairs[:, 1]], axis=1)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    term = d((rng.random(nmatch * n) < 0.3).astype(np.uint8))
    cur = d(rng.integers(0, 4, nmatch * n).astype(np.int32))
    rows = torch.zeros(nmatch * n, dtype=torch.int64, device="cuda")
    gf = torch.zeros(M + 1, dtype=torch.int32, device="cuda")
    work = torch.zeros(4 * nmatch, dtype=torch.int32, device="cuda")
    L, team = _capi.lib(), 0
    xo, xg, xn = lineup_order(lineups, team)
    lo, lg, ln = team_order(pairs, team)
    args = {"xplay": (L.brl_xplay_route, d(xo), d(xn[xg].astype(np.int32))), "league": (L.brl_league_route, d(lo), d(ln[lg].astype(np.int32)))}

    def run(which, calls):
        fn, order, group_of = args[which]
        s = _capi.stream()
        a = (0, term.data_ptr(), cur.data_ptr(), team, n, order.data_ptr(), group_of.data_ptr(), nmatch, M, work.data_ptr(),
             rows.data_ptr(), gf.data_ptr(), s)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            _capi.check(fn(*a))
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / calls, int(gf[-1])     # us per call (three launches), rows routed

    times, routed = {"xplay": [], "league": []}, {}
    for rep in range(REPEATS + 1):              # (repeat 0 is the warm-up of each)
        for which in ("league", "xplay"):       # alternated
            us, routed[which] = run(which, CALLS)
            if rep:
                times[which].append(us)
    assert routed["xplay"] == routed["league"]
    rec = {"matches": nmatch, "boards": n, "rows_routed": routed["xplay"], "calls_per_repeat": CALLS,
           "xplay_us_per_call": spread(times["xplay"]), "league_us_per_call": spread(times["league"])}
    rec["xplay_over_league"] = rec["xplay_us_per_call"]["median"] / rec["league_us_per_call"]["median"]
    return rec


def cross_play_case(M, n):
    import brl_amd
    from bench import synthetic_lut
    from brl_amd.crossplay import cross_play
    from brl_amd.models import make_forward_pass
    env = brl_amd.BridgeBidding(lut=synthetic_lut(100_000, 10_000))
    fp = make_forward_pass("relu", "DeepMind")
    nets = [fp.init(100 + k, device="cuda") for k in range(M + 1)]
    times, gaps = {"batched": [], "loop": []}, {}
    for rep in range(REPEATS + 1):
        for method in ("batched", "loop"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            cp = cross_play(nets[:M], nets[M], env, "relu", "DeepMind", n, rng_key=0, method=method)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert cp.last_method == method
            gaps[method] = cp.gap
            if rep:
                times[method].append(dt)
    rec = {"networks": M, "boards": n, "lineups": M * M, "batched_s": spread(times["batched"]), "loop_s": spread(times["loop"])}
    rec["loop_over_batched"] = rec["loop_s"]["median"] / rec["batched_s"]["median"]
    rec["max_abs_gap_difference"] = float(np.abs(gaps["batched"] - gaps["loop"]).max())
    return rec


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "crossplay", "throughput.json")
    if not torch.cuda.is_available():
        raise SystemExit("crossplay_throughput.py measures on the GPU: none found")
    result = {"device": torch.cuda.get_device_name(0), "route": [], "cross_play": []}
    for nmatch, n in ((64, 100), (64, 1000)):
        result["route"].append(route_case(nmatch, n))
        print(json.dumps(result["route"][-1]), flush=True)
    result["cross_play"].append(cross_play_case(8, 100))
    print(json.dumps(result["cross_play"][-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
