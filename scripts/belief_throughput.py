"""Device time of the hand beliefs (brl_amd/belief.py) on the bidder pair (tests/bidder_net.py):

  * brl_belief_deal, brl_belief_logp and brl_belief_reduce per launch at Q = 64 queries x K = 4096 samples, each beside a
    device-to-device copy of the bytes it moves (HIP events around 100 back-to-back launches after a warm-up, median of three);
  * ``hand_belief`` as a whole at Q = 1 and Q = 64, K = 4096, for a 4-call and a 12-call prefix (HIP events around one call that
    ends in a synchronise, three warm-up calls, median of five), with the rows forwarded counted on the host, and per forwarded row;
  * the 10 000-board make_simple_duplicate_evaluate — what ``python -m brl_amd.eval`` runs without ``belief_board`` — before,
    between and after.

    python scripts/belief_throughput.py [out.json] [parent=DIR]      (default: profiles/belief/throughput.json)

``parent=DIR``: a built checkout of the parent commit; its evaluator is timed by a child process (boards_throughput.py
``--evaluate-only`` with DIR as the package root) between this tree's measurements."""
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
from brl_amd import belief, boards  # noqa: E402
from brl_amd.evaluation import make_simple_duplicate_evaluate  # noqa: E402
from brl_amd.models import make_forward_pass  # noqa: E402
from tests import bidder_net  # noqa: E402

DEV, K = "cuda:0", 4096
d = np.load(os.path.join(HERE, "tests", "golden", "wb5_dds_1000.npz"))
env = brl_amd.BridgeBidding(lut=(d["keys"], d["values"]), device=DEV)
fp = make_forward_pass("relu", "DeepMind")
words = boards.read_deals(os.path.join(HERE, "tests", "golden", "wb5_named_24.json")).hand_words()
PREFIX = {4: ["P", "P", "1C", "P"], 12: ["P", "1D", "2D", "P", "P", "3D", "P", "P", "X", "P", "P", "XX"]}


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


def queries(Q, T):
    """Q queries with the T-call prefix: the hands of the named deals in turn, every own seat"""
    return [belief.BeliefQuery(i & 3, int(words[i % 24, i & 3]), "W" if T == 12 else "S", "None", PREFIX[T]) for i in range(Q)]


def kernels(Q):
    qs = queries(Q, 4)
    qdev = torch.from_numpy(belief.query_array(qs).view(np.uint8).reshape(Q, 16)).to(DEV)
    n = Q * K
    out = {"queries": Q, "samples": K, "rows": n}
    us, runs = launches(lambda: belief.deal(qdev, K, 0, 0))
    written = n * (128 + 32)
    cus, cruns = copy_us(written)
    out["deal"] = {"us_per_launch": us, "runs_us": runs, "bytes_written": written, "GB_per_s": written / us / 1e3, "copy_us": cus,
                   "copy_runs_us": cruns, "launch_over_copy": us / cus}
    _, hands = belief.deal(qdev, K, 0, 0)
    logits = torch.randn((n, 39), device=DEV) * 8
    rows = torch.arange(n, dtype=torch.int64, device=DEV)
    query_of = torch.arange(Q, dtype=torch.int32, device=DEV).repeat_interleave(K)
    legal = torch.full((Q,), (1 << 38) - 7, dtype=torch.int64, device=DEV)
    action = torch.full((Q,), 5, dtype=torch.int32, device=DEV)
    logw, greedy = torch.zeros(n, device=DEV), torch.ones(n, dtype=torch.uint8, device=DEV)
    us, runs = launches(lambda: belief.logp(logits, rows, query_of, legal, action, logw, greedy))
    moved = n * (39 * 4 + 8 + 4 + 2 * 4 + 2)
    cus, cruns = copy_us(moved)
    out["logp"] = {"us_per_launch": us, "runs_us": runs, "bytes_moved": moved, "GB_per_s": moved / us / 1e3, "copy_us": cus,
                   "copy_runs_us": cruns, "launch_over_copy": us / cus}
    logw = torch.randn(n, device=DEV) * 3
    us, runs = launches(lambda: belief.reduce(qdev, K, hands, logw, greedy))
    read = n * (32 + 4 + 1)
    cus, cruns = copy_us(read)
    out["reduce"] = {"us_per_launch": us, "runs_us": runs, "bytes_read": read, "bytes_written": Q * belief.ENTRY_DTYPE.itemsize,
                     "copy_of_read_us": cus, "copy_of_read_runs_us": cruns, "launch_over_copy": us / cus}
    return out


def whole(nets):
    hb = belief.make_hand_belief(env, "relu", "DeepMind", "relu", "DeepMind", samples=K)
    out = {}
    for Q in (1, 64):
        for T in (4, 12):
            qs = queries(Q, T)
            counts = {}
            res = hb(nets[0], nets[1], qs, counts=counts)
            ms = timed(lambda: hb(nets[0], nets[1], qs))
            out[f"Q{Q}_T{T}"] = {"ms": ms, "rows_forwarded": counts["forwarded"], "us_per_forwarded_row": ms["median_of_5"] * 1e3 / counts["forwarded"],
                                 "ess_mean": float(np.nanmean(res.ess)), "consistent_mean": float(res.consistent.mean())}
    return out


args = [a for a in sys.argv[1:] if not a.startswith("parent=")]
parent = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("parent=")), None)
out = {"device": torch.cuda.get_device_name(0), "max_rows": belief.MAX_ROWS}
net_a, net_b = fp.init(1, device=DEV), fp.init(2, device=DEV)
ev = make_simple_duplicate_evaluate(env, "relu", "DeepMind", "relu", "DeepMind", 10000)
out["evaluate_10000_ms"] = timed(lambda: ev(net_a, net_b, 5))
if parent:
    r = subprocess.run([sys.executable, os.path.join(HERE, "scripts", "boards_throughput.py"), "--evaluate-only"],
                       env=dict(os.environ, BRL_BOARDS_ROOT=os.path.abspath(parent)), capture_output=True, text=True, timeout=600)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("EVALUATE ")]
    if r.returncode != 0 or not line:
        raise SystemExit("parent run failed:\n" + r.stderr[-2000:])
    out["parent_evaluate_10000_ms"] = json.loads(line[-1][len("EVALUATE "):])
    out["evaluate_10000_again_ms"] = timed(lambda: ev(net_a, net_b, 5))
out["kernels"] = kernels(64)
out["hand_belief"] = whole(bidder_net.pair(DEV))
out["evaluate_10000_last_ms"] = timed(lambda: ev(net_a, net_b, 5))

path = args[0] if args else os.path.join(HERE, "profiles", "belief", "throughput.json")
os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
json.dump(out, open(path, "w"), indent=1)
print(json.dumps(out, indent=1))
