"""Device time of the call review (brl_amd/review.py) of a 1000-board x 2-table match at depth 12, for a match of random-init
DeepMind 4 x 1024 networks and for a match of the bidder pair (tests/bidder_net.py):

  * decisions, branches (slots that are not void) and rows forwarded;
  * brl_review_expand and brl_review_reduce per launch on table A's decisions (one chunk of at most review.MAX_BRANCHES slots),
    each beside a device-to-device copy of the bytes it writes (HIP events around 100 back-to-back launches after a warm-up,
    median of three);
  * the whole review beside the board_match that produced its records (HIP events around one call that ends in a synchronise,
    three warm-up calls, median of five), and both per forwarded row;
  * the 10 000-board make_simple_duplicate_evaluate — what ``python -m brl_amd.eval`` runs without ``review`` — before and after.

    python scripts/review_throughput.py [out.json] [parent=DIR]      (default: profiles/review/throughput.json)

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
from brl_amd import boards, evaluation, review  # noqa: E402
from brl_amd.evaluation import make_simple_duplicate_evaluate  # noqa: E402
from brl_amd.models import make_forward_pass  # noqa: E402
from oracle import Oracle  # noqa: E402
from tests import bidder_net  # noqa: E402

DEV, DEPTH = "cuda:0", 12
d = np.load(os.path.join(HERE, "tests", "golden", "wb5_dds_1000.npz"))
env = brl_amd.BridgeBidding(lut=(d["keys"], d["values"]), device=DEV)
fp = make_forward_pass("relu", "DeepMind")
orc = Oracle(d["keys"], d["values"])
hand = np.stack([orc.key_to_hand(k) for k in d["keys"]])
deals = boards.Deals(np.sort(hand.reshape(-1, 4, 13), axis=2).reshape(-1, 52).astype(np.int32), d["dealer"], d["vul_ns"], d["vul_ew"],
                     d["tricks"].reshape(-1, 20), d["board_id"])


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


ROWS = [0]
_Real = evaluation._Forward


class _Counting(_Real):
    """counts the rows every forward is asked for"""

    def rows(self, obs_bool, idx, m, out, env_):
        ROWS[0] += int(m)
        return super().rows(obs_bool, idx, m, out, env_)

    def __call__(self, obs_bool, obs_f32):
        ROWS[0] += int((obs_bool if obs_bool is not None else obs_f32).shape[0])
        return super().__call__(obs_bool, obs_f32)


def counted(make, run):
    """rows forwarded by one run of a function built while evaluation._Forward counts"""
    evaluation._Forward = _Counting
    try:
        fn = make()
        ROWS[0] = 0
        run(fn)
        torch.cuda.synchronize()
        return ROWS[0]
    finally:
        evaluation._Forward = _Real


def copy_us(nbytes):
    src, dst = torch.zeros(nbytes, dtype=torch.uint8, device=DEV), torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    return launches(lambda: dst.copy_(src))


def measure(nets):
    make_match = lambda: boards.make_board_match(env, "relu", "DeepMind", "relu", "DeepMind")            # noqa: E731
    make_review = lambda: review.make_call_review(env, "relu", "DeepMind", "relu", "DeepMind", depth=DEPTH)   # noqa: E731
    bm, cr = make_match(), make_review()
    _, records = bm(nets[0], nets[1], deals)
    out = {"boards": len(records), "depth": DEPTH, "mean_calls": float(np.mean([records.cpu(t)["n_calls"].mean() for t in "ab"]))}
    rv = cr(nets[0], nets[1], records)
    out["decisions"], out["branches"] = len(rv), int((rv.imp != review.VOID).sum())
    out["slots"] = len(rv) * review.ACTIONS
    out["loss_gt_0_share"] = float((rv.loss > 0).mean())
    out["team_stats"] = {k: {x: v[x] for x in ("decisions", "best_share", "mean_loss", "loss_per_board")} for k, v in rv.team_stats().items()}
    # ---- the two kernels, on table A's first chunk
    rec, dda = records.table_a, records.dda.contiguous()
    first, _ = review.first_decisions(rec, DEPTH)
    nd = min(int(first[-1]), review.MAX_BRANCHES // review.ACTIONS)
    us, runs = launches(lambda: review.expand(rec, dda, DEPTH, first, 0, nd))
    written = nd * review.ACTIONS * 128 + nd * 16
    cus, cruns = copy_us(written)
    out["expand"] = {"decisions": nd, "us_per_launch": us, "runs_us": runs, "bytes_written": written, "GB_per_s": written / us / 1e3,
                     "copy_us": cus, "copy_runs_us": cruns, "launch_over_copy": us / cus}
    decisions, branch = review.expand(rec, dda, DEPTH, first, 0, nd)
    evaluation._eval_loop(env, brl_amd.bridge_bidding.State(env, branch), *evaluation._team_forwards(fp, nets[0], fp, nets[1]),
                          None, None, 0, None, None)
    us, runs = launches(lambda: review.reduce(branch, decisions, records.table_b))
    written, read = nd * review.ACTIONS + nd * 8, nd * review.ACTIONS * 40 + nd * 16
    cus, cruns = copy_us(written)
    rus, rruns = copy_us(read)
    out["reduce"] = {"decisions": nd, "us_per_launch": us, "runs_us": runs, "bytes_written": written, "bytes_read": read,
                     "copy_of_written_us": cus, "copy_of_written_runs_us": cruns, "copy_of_read_us": rus, "copy_of_read_runs_us": rruns}
    # ---- the whole review beside the match
    out["board_match_ms"] = timed(lambda: bm(nets[0], nets[1], deals))
    out["review_ms"] = timed(lambda: cr(nets[0], nets[1], records))
    out["board_match_rows"] = counted(make_match, lambda f: f(nets[0], nets[1], deals))
    out["review_rows"] = counted(make_review, lambda f: f(nets[0], nets[1], records))
    out["board_match_us_per_row"] = out["board_match_ms"]["median_of_5"] * 1e3 / out["board_match_rows"]
    out["review_us_per_row"] = out["review_ms"]["median_of_5"] * 1e3 / out["review_rows"]
    chunks = -(-out["slots"] // (review.MAX_BRANCHES // review.ACTIONS * review.ACTIONS))
    scale = out["decisions"] / nd           # both kernels are linear in the decisions
    out["chunks"] = chunks
    out["kernels_share_of_review"] = (out["expand"]["us_per_launch"] + out["reduce"]["us_per_launch"]) * scale / 1e3 / out["review_ms"]["median_of_5"]
    return out


args = [a for a in sys.argv[1:] if not a.startswith("parent=")]
parent = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("parent=")), None)
out = {"device": torch.cuda.get_device_name(0), "max_branches": review.MAX_BRANCHES}
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
out["random_init"] = measure((net_a, net_b))
out["bidder_pair"] = measure(bidder_net.pair(DEV))
out["evaluate_10000_last_ms"] = timed(lambda: ev(net_a, net_b, 5))

path = args[0] if args else os.path.join(HERE, "profiles", "review", "throughput.json")
os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
json.dump(out, open(path, "w"), indent=1)
print(json.dumps(out, indent=1))
