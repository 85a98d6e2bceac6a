"""Device time of the hand beliefs' resample-move stages (brl_amd/belief.py, include/brl_belief_smc.h) on the bidder pair
(tests/bidder_net.py), and whether they pay:

  * brl_belief_resample, brl_belief_propose and brl_belief_accept per launch at Q = 64 queries x K = 4096 particles, each beside a
    device-to-device copy of the bytes it moves (HIP events around 100 back-to-back launches after a warm-up, median of three);
  * ``hand_belief`` of one query (South's hand of named board 0) for the 4-call and the 12-call prefix of DESIGN §15's table with
    ``resample_every`` 1 / ``moves`` 2 at K = 4096 (three warm-up calls, median of five), and beside each plain importance
    sampling at the K — a power of two up to 2^18 — whose wall time is the nearest;
  * for both: the distinct deals, the effective sample size, the consistent count, and the standard deviation over 8 seeds of
    North's mean HCP (the number a user reads; the smaller, the better the estimator at that cost);
  * the 10 000-board make_simple_duplicate_evaluate before, between and after, and a parent checkout's.

    python scripts/belief_smc_throughput.py [out.json] [parent=DIR]      (default: profiles/belief/smc_throughput.json)"""
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
from brl_amd import _capi, belief, boards  # noqa: E402
from brl_amd.evaluation import make_simple_duplicate_evaluate  # noqa: E402
from brl_amd.models import make_forward_pass  # noqa: E402
from tests import bidder_net  # noqa: E402

DEV, K = "cuda:0", 4096
NET = ("relu", "DeepMind", "relu", "DeepMind")
d = np.load(os.path.join(HERE, "tests", "golden", "wb5_dds_1000.npz"))
env = brl_amd.BridgeBidding(lut=(d["keys"], d["values"]), device=DEV)
fp = make_forward_pass("relu", "DeepMind")
words = boards.read_deals(os.path.join(HERE, "tests", "golden", "wb5_named_24.json")).hand_words()
PREFIX = {4: ["P", "P", "1C", "P"], 12: ["P", "1D", "2D", "P", "P", "3D", "P", "P", "X", "P", "P", "XX"]}
SEEDS = range(8)


def timed(fn):
    """ms of one call that ends in a synchronise: three warm-up calls, median of five"""
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
    """a device-to-device copy that reads and writes nbytes each"""
    src, dst = torch.zeros(nbytes, dtype=torch.uint8, device=DEV), torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    return launches(lambda: dst.copy_(src))


def kernels(Q):
    qs = [belief.BeliefQuery(i & 3, int(words[i % 24, i & 3]), "S", "None", PREFIX[4]) for i in range(Q)]
    qdev = torch.from_numpy(belief.query_array(qs).view(np.uint8).reshape(Q, 16)).to(DEV)
    n = Q * K
    out = {"queries": Q, "particles": K, "rows": n}
    tables, hands = belief.deal(qdev, K, 0, 0)
    qlist = torch.arange(Q, dtype=torch.int32, device=DEV)
    stream_of = torch.arange(Q, dtype=torch.int64, device=DEV)
    logw, logl = torch.randn(n, device=DEV) * 3, torch.randn(n, device=DEV)
    greedy = torch.ones(n, dtype=torch.uint8, device=DEV)
    row = 128 + 32 + 4 + 1                                   # a particle's table, hands, logl and greedy
    for name, lw in (("resample", logw), ("resample_one_dominant", torch.where(torch.arange(n, device=DEV) % K == 7, 0.0, -2000.0))):
        ins = (tables, hands, logl, lw, greedy)
        outs = [torch.empty_like(x) for x in ins] + [torch.empty(n, dtype=torch.int32, device=DEV)]      # (allocated once: the launch is timed)
        ptrs = [x.data_ptr() for x in ins] + [x.data_ptr() for x in outs]
        us, runs = launches(lambda: _capi.check(_capi.lib().brl_belief_resample(0, qlist.data_ptr(), Q, stream_of.data_ptr(), Q, K, 0, 3, *ptrs,
                                                                                _capi.stream(0))))
        moved = n * (4 + row + row + 4 + 4)                  # logw read, the ancestor's row read, the row, logw' and the ancestor written
        cus, cruns = copy_us(moved // 2)
        out[name] = {"us_per_launch": us, "runs_us": runs, "bytes_moved": moved, "GB_per_s": moved / us / 1e3, "copy_us": cus,
                     "copy_runs_us": cruns, "launch_over_copy": us / cus}
    t_new, h_new = torch.empty_like(tables), torch.empty_like(hands)
    us, runs = launches(lambda: belief.propose(qdev, qlist, stream_of, K, 0, 3, 1, hands, t_new, h_new))
    moved = n * (32 + 128 + 32)
    cus, cruns = copy_us(moved // 2)
    out["propose"] = {"us_per_launch": us, "runs_us": runs, "bytes_moved": moved, "GB_per_s": moved / us / 1e3, "copy_us": cus,
                      "copy_runs_us": cruns, "launch_over_copy": us / cus}
    counters = torch.zeros((Q, 2), dtype=torch.int64, device=DEV)
    for name, ll_new in (("accept_all_taken", logl.clone()), ("accept_none_taken", torch.full_like(logl, -float("inf")))):
        live = [tables.clone(), hands.clone(), logl.clone(), greedy.clone()]
        us, runs = launches(lambda: belief.accept(qlist, stream_of, K, 0, 3, 1, t_new, h_new, ll_new, greedy, *live, counters))
        moved = n * (4 + 4 + (2 * row if name == "accept_all_taken" else 0))
        cus, cruns = copy_us(moved // 2)
        out[name] = {"us_per_launch": us, "runs_us": runs, "bytes_moved": moved, "GB_per_s": moved / us / 1e3, "copy_us": cus,
                     "copy_runs_us": cruns, "launch_over_copy": us / cus}
    return out


def describe(make, nets, q, north):
    """the estimator ``make(seed)``: its time (seed 0), and over the 8 seeds distinct / effective / consistent and North's mean HCP"""
    hb0 = make(0)
    ms = timed(lambda: hb0(nets[0], nets[1], [q]))
    stats = {"distinct": [], "ess": [], "consistent": [], "north_hcp": []}
    for s in SEEDS:
        rows = []
        res = make(s)(nets[0], nets[1], [q], rows=rows)
        stats["distinct"].append(int(len(np.unique(rows[0]["hands"], axis=0))))
        stats["ess"].append(float(res.ess[0]))
        stats["consistent"].append(int(res.consistent[0]))
        stats["north_hcp"].append(float(res.hcp_mean[0, north]))
    return {"ms": ms, **{k + "_mean": float(np.mean(v)) for k, v in stats.items()}, "north_hcp_std_over_seeds": float(np.std(stats["north_hcp"], ddof=1)),
            "runs": stats}


def whole(nets):
    out = {}
    for T in (4, 12):
        q = belief.BeliefQuery("S", int(words[0, 2]), "S" if T == 4 else "W", "None", PREFIX[T])
        north = [(q.seat + 1 + h) & 3 for h in range(3)].index(0)
        smc = describe(lambda s: belief.make_hand_belief(env, *NET, samples=K, seed=s, resample_every=1, moves=2), nets, q, north)
        counts = {}
        belief.make_hand_belief(env, *NET, samples=K, resample_every=1, moves=2)(nets[0], nets[1], [q], counts=counts)
        smc["rows_forwarded"] = counts["forwarded"]
        # plain importance sampling at every power of two from K to 2^18: the one whose time is the nearest
        plain_ms = {}
        for e in range(12, 19):
            hb = belief.make_hand_belief(env, *NET, samples=1 << e)
            plain_ms[1 << e] = timed(lambda: hb(nets[0], nets[1], [q]))["median_of_5"]
        k_equal = min(plain_ms, key=lambda k: abs(plain_ms[k] - smc["ms"]["median_of_5"]))
        plain = describe(lambda s: belief.make_hand_belief(env, *NET, samples=k_equal, seed=s), nets, q, north)
        plain4096 = describe(lambda s: belief.make_hand_belief(env, *NET, samples=K, seed=s), nets, q, north)
        out[f"T{T}"] = {"resample_move_K4096": smc, "plain_ms_by_K": plain_ms, "equal_cost_K": k_equal, "plain_equal_cost": plain,
                        "plain_K4096": plain4096}
    return out


args = [a for a in sys.argv[1:] if not a.startswith("parent=")]
parent = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("parent=")), None)
out = {"device": torch.cuda.get_device_name(0)}
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

path = args[0] if args else os.path.join(HERE, "profiles", "belief", "smc_throughput.json")
os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
json.dump(out, open(path, "w"), indent=1)
print(json.dumps(out, indent=1))
