"""Device time of the double-dummy par (brl_amd/par.py): brl_par per launch at 10 000 and 65 536 boards on real tables (the
fixture's 1000, tiled, under every dealer and vulnerability) and on uniform-random 0..13 tables, beside a device-to-device copy
of the same input + output bytes (54 per board) measured in the same run; brl_par_imp per launch; and the 10 000-board
make_simple_duplicate_evaluate the launch is budgeted against.  HIP events around 100 back-to-back launches after a warm-up,
median of three; the evaluation: HIP events around one call that ends in a synchronise, three warm-up calls, median of five.

    python scripts/par_throughput.py [out.json] [parent=DIR]      (default: profiles/par/throughput.json)

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
from brl_amd import _capi, boards, par  # noqa: E402
from brl_amd.evaluation import make_simple_duplicate_evaluate  # noqa: E402
from brl_amd.models import make_forward_pass  # noqa: E402

DEV = "cuda:0"
d = np.load(os.path.join(HERE, "tests", "golden", "wb5_dds_1000.npz"))
env = brl_amd.BridgeBidding(lut=(d["keys"], d["values"]), device=DEV)
fp = make_forward_pass("relu", "DeepMind")
net_a, net_b = fp.init(1, device=DEV), fp.init(2, device=DEV)


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


def measure(n, kind):
    rng = np.random.default_rng(n)
    if kind == "real":
        i = np.arange(n)
        dda, dealer, vul = d["tricks"].reshape(-1, 20)[i % 1000], (i // 1000) % 4, (i // 4000) % 4
    else:
        dda, dealer, vul = rng.integers(0, 14, size=(n, 20)), rng.integers(0, 4, size=n), rng.integers(0, 4, size=n)
    dda = torch.from_numpy(np.ascontiguousarray(dda, dtype=np.uint8)).to(DEV)
    dealer, vul = (torch.from_numpy(x.astype(np.uint8)).to(DEV) for x in (dealer, vul))
    out = torch.zeros((n, 32), dtype=torch.uint8, device=DEV)
    L, s = _capi.lib(), _capi.stream(0)
    us, runs = launches(lambda: _capi.check(L.brl_par(0, _capi.ptr(dda), _capi.ptr(dealer), _capi.ptr(vul), n, _capi.ptr(out), s)))
    # the same bytes, copied: 22 in (the table, the dealer, the vulnerability) and 32 out per board as one 54-byte-per-board copy
    src, dst = torch.zeros(n * 54, dtype=torch.uint8, device=DEV), torch.zeros(n * 54, dtype=torch.uint8, device=DEV)
    us_copy, runs_copy = launches(lambda: dst.copy_(src))
    rec = par.par_array(out)
    return {"boards": n, "tables": kind, "us_per_launch": us, "runs_us": runs, "bytes": n * 54, "GB_per_s": n * 54 / us / 1e3,
            "copy_us": us_copy, "copy_runs_us": runs_copy, "launch_over_copy": us / us_copy,
            "dealer_dependent": int(((rec["flags"] & par.DEALER_DEPENDENT) != 0).sum()),
            "passed_out": int(((rec["flags"] & par.PASSED_OUT) != 0).sum())}


args = [a for a in sys.argv[1:] if not a.startswith("parent=")]
parent = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("parent=")), None)
out = {"device": torch.cuda.get_device_name(0)}
for n in (10000, 65536):
    for kind in ("real", "random"):
        out[f"par_{n}_{kind}"] = measure(n, kind)

# brl_par_imp on a match's records
for n in (10000, 65536):
    _, records = boards.make_board_match(env, "relu", "DeepMind", "relu", "DeepMind", n)(net_a, net_b, 5)
    at = lambda name: records.table_a[:, boards.RECORD_DTYPE.fields[name][1]]   # noqa: E731
    pr = par.par_of(records.dda, at("dealer"), at("vul_ns"), at("vul_ew"))
    imp = torch.zeros(n, dtype=torch.int32, device=DEV)
    ta = records.table_a
    us, runs = launches(lambda: _capi.check(_capi.lib().brl_par_imp(0, _capi.ptr(ta), _capi.ptr(pr), n, 1, _capi.ptr(imp), _capi.stream(0))))
    out[f"par_imp_{n}"] = {"boards": n, "us_per_launch": us, "runs_us": runs}
    if n == 10000:
        out["par_of_records_10000_ms"] = timed(lambda: par.par_of(records.dda, at("dealer"), at("vul_ns"), at("vul_ew")))
        stats = par.par_stats(records)
        out["par_stats_10000"] = {k: stats["teams"][k]["imp"] for k in stats["teams"]}

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
    out["launch_share_of_parent_evaluate"] = out["par_10000_real"]["us_per_launch"] / 1e3 / out["parent_evaluate_10000_ms"]["median_of_5"]

path = args[0] if args else os.path.join(HERE, "profiles", "par", "throughput.json")
os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
json.dump(out, open(path, "w"), indent=1)
print(json.dumps(out, indent=1))
