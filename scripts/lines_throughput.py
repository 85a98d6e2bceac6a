"""Device time of the auction lines (brl_amd/lines.py) on 10 000 boards x 2 tables, for a pair of random-init DeepMind 4 x 1024
networks and for the bidder pair (tests/bidder_net.py):

  * brl_lines_expand per launch for K = 1, 4, 16 on a beam five steps into the search, beside a device-to-device copy of the bytes
    it moves (the beam read and the beam written), and brl_lines_imp beside a copy of what it reads (HIP events around 100
    back-to-back launches after a warm-up, median of three);
  * the whole search (both tables, the results and the board sums) for K = 1, 4, 16 beside the board_match of the same boards (HIP
    events around one call that ends in a synchronise, three warm-up calls, median of five), the steps it ran and the rows
    forwarded per step, and the summary it gives;
  * the 10 000-board make_simple_duplicate_evaluate — what ``python -m brl_amd.eval`` runs without ``lines`` — at the start,
    between and at the end.

    python scripts/lines_throughput.py [out.json] [parent=DIR]      (default: profiles/lines/throughput.json)

``parent=DIR``: a built checkout of the parent commit; its evaluator is timed by a child process (boards_throughput.py
``--evaluate-only`` with DIR as the package root) between this tree's measurements, in the same process order."""
import json
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

import brl_amd  # noqa: E402
from brl_amd import boards, evaluation, lines  # noqa: E402
from brl_amd.evaluation import make_simple_duplicate_evaluate  # noqa: E402
from brl_amd.models import make_forward_pass  # noqa: E402
from tests import bidder_net  # noqa: E402

DEV, N, KS = "cuda:0", 10000, (1, 4, 16)
d = np.load(os.path.join(HERE, "tests", "golden", "wb5_dds_1000.npz"))
env = brl_amd.BridgeBidding(lut=(d["keys"], d["values"]), device=DEV)
fp = make_forward_pass("relu", "DeepMind")


def timed(fn):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return {"median_of_5": statistics.median(ts), "runs": ts}


def launches(fn):
    """us per launch: 100 back-to-back launches between two events, median of three"""
    for _ in range(20):
        fn()
    ts = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(100):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 10.0)
    return statistics.median(ts), ts


def copy_us(nbytes):
    src, dst = torch.zeros(nbytes, dtype=torch.uint8, device=DEV), torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    return launches(lambda: dst.copy_(src))


def kernels(nets, k):
    """brl_lines_expand on the beam five steps in, brl_lines_imp on the final beams"""
    fwd1, fwd2 = evaluation._team_forwards(fp, nets[0], fp, nets[1])
    state = env.init(5, num_envs=N)
    beam = lines.lines_init(state.packed, k, lines.MAX_CALLS)
    for _ in range(5):
        obs, _ = env._observe_raw(beam.tables, None)
        l1, l2 = evaluation._Forward.whole_pair(fwd1, fwd2, obs)
        beam = lines.lines_expand(beam, l1, l2)
    obs, _ = env._observe_raw(beam.tables, None)
    l1, l2 = evaluation._Forward.whole_pair(fwd1, fwd2, obs)
    spare = lines.Beam(N, k, lines.MAX_CALLS, DEV)
    us, runs = launches(lambda: lines.lines_expand(beam, l1, l2, spare))
    live = int(((beam.flags & (lines.EMPTY | lines.FINISHED | lines.VOID)) == 0).sum())
    per_line = 128 + lines.MAX_CALLS + 8 + 1
    moved = 2 * N * k * per_line + live * 38 * 4 + N * k * 16 + N        # the beam read and written, the live rows, requests, done
    cus, cruns = copy_us(moved)
    out = {"expand": {"boards": N, "k": k, "live_lines": live, "us_per_launch": us, "runs_us": runs, "bytes_moved": moved,
                      "copy_us": cus, "copy_runs_us": cruns, "launch_over_copy": us / cus}}
    res = lines.lines_finish(beam.tables, beam.flags)
    us, runs = launches(lambda: lines.lines_imp(beam.score, beam.flags, res, beam.score, beam.flags, res, N, k))
    read = 2 * N * k * (8 + 1 + 16) + N * 64
    cus, cruns = copy_us(read)
    out["imp"] = {"boards": N, "k": k, "us_per_launch": us, "runs_us": runs, "bytes_moved": read, "copy_us": cus, "copy_runs_us": cruns,
                  "launch_over_copy": us / cus}
    return out


def measure(nets):
    bm = boards.make_board_match(env, "relu", "DeepMind", "relu", "DeepMind", N)
    out = {"boards": N, "board_match_ms": timed(lambda: bm(nets[0], nets[1], 5))}
    for k in KS:
        al_fn = lines.make_auction_lines(env, "relu", "DeepMind", "relu", "DeepMind", N, k=k)
        al = al_fn(nets[0], nets[1], 5)
        entry = kernels(nets, k)
        entry["search_ms"] = timed(lambda: al_fn(nets[0], nets[1], 5))
        entry["steps"], entry["rows_per_step"] = list(al.steps), al.rows_per_step
        entry["rows_forwarded"] = sum(al.steps) * al.rows_per_step * 2       # every line through both networks
        entry["search_over_board_match"] = entry["search_ms"]["median_of_5"] / out["board_match_ms"]["median_of_5"]
        entry["summary"] = al.summary()
        out[f"k{k}"] = entry
    return out


args = [a for a in sys.argv[1:] if not a.startswith("parent=")]
parent = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("parent=")), None)
out = {"device": torch.cuda.get_device_name(0)}
net_a, net_b = fp.init(1, device=DEV), fp.init(2, device=DEV)
ev = make_simple_duplicate_evaluate(env, "relu", "DeepMind", "relu", "DeepMind", N)
out["evaluate_10000_ms"] = timed(lambda: ev(net_a, net_b, 5))
if parent:
    r = subprocess.run([sys.executable, os.path.join(HERE, "scripts", "boards_throughput.py"), "--evaluate-only"],
                       env=dict(os.environ, BRL_BOARDS_ROOT=os.path.abspath(parent)), capture_output=True, text=True, timeout=600)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("EVALUATE ")]
    if r.returncode != 0 or not line:
        raise SystemExit("parent run failed:\n" + r.stderr[-2000:])
    out["parent_evaluate_10000_ms"] = json.loads(line[-1][len("EVALUATE "):])
    out["evaluate_10000_again_ms"] = timed(lambda: ev(net_a, net_b, 5))
out["random_init"] = measure((net_a, net_b))
out["bidder_pair"] = measure(bidder_net.pair(DEV))
out["evaluate_10000_last_ms"] = timed(lambda: ev(net_a, net_b, 5))

path = args[0] if args else os.path.join(HERE, "profiles", "lines", "throughput.json")
os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
json.dump(out, open(path, "w"), indent=1)
print(json.dumps(out, indent=1))
