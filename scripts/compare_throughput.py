"""Device time of the system diff (brl_amd/compare.py): brl_compare_tables, brl_compare_rows and brl_compare_reduce on a 10 000-board x
2-table match, each beside a device-to-device copy of the bytes it has to move (HIP events around 100 back-to-back launches
after a warm-up, median of three), policy_diff as a whole at depth 4 and 10 beside the board_match that produced the records
(median of five calls), and the 10 000-board make_simple_duplicate_evaluate on this tree and on a parent checkout, in one session.

    python scripts/compare_throughput.py [out.json] [parent=DIR]      (default: profiles/compare/throughput.json)

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
from brl_amd import boards, compare  # noqa: E402
from brl_amd.evaluation import make_simple_duplicate_evaluate  # noqa: E402
from brl_amd.models import make_forward_pass  # noqa: E402

N = 10000
d = np.load(os.path.join(HERE, "tests", "golden", "wb5_dds_1000.npz"))
env = brl_amd.BridgeBidding(lut=(d["keys"], d["values"]), device="cuda:0")
fp = make_forward_pass("relu", "DeepMind")
net_a, net_b = fp.init(1, device="cuda:0"), fp.init(2, device="cuda:0")


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


def beside_copy(fn, nbytes):
    """a launch beside a device-to-device copy of ``nbytes`` (read once, written once: half of them each way)"""
    src = torch.empty(max(1, nbytes // 2), dtype=torch.uint8, device="cuda:0")
    dst = torch.empty_like(src)
    us, runs = launches(fn)
    us_c, runs_c = launches(lambda: dst.copy_(src))
    return {"us_per_launch": us, "runs_us": runs, "bytes": nbytes, "GB_per_s": nbytes / us / 1e3, "copy_us": us_c, "copy_runs_us": runs_c,
            "launch_over_copy": us / us_c}


def kernels(records, depth):
    """the three launches on table A's records, with random logits (the kernels' time does not depend on their values)"""
    rec = records.table_a
    n = rec.shape[0]
    rows = torch.arange(n, dtype=torch.int64, device="cuda:0")
    gen = torch.Generator(device="cuda:0").manual_seed(1)
    lx = torch.randn((n, 39), generator=gen, device="cuda:0") * 3
    ly = lx + torch.randn((n, 39), generator=gen, device="cuda:0")
    legal = torch.full((n,), (1 << 38) - 1, dtype=torch.int64, device="cuda:0")
    dec = torch.zeros((n * depth, 64), dtype=torch.uint8, device="cuda:0")
    out = {"boards": n, "depth": depth}
    # tables: 48 of a record's bytes and the row index in, a table and its hand row out
    out["tables"] = beside_copy(lambda: compare.compare_tables(rec, rows), n * (48 + 8 + 128 + 32))
    # rows: 64 of a record's bytes, the row index, two logit rows and the legal word in, one decision record out
    out["rows"] = beside_copy(lambda: compare.compare_rows(rec, rows, 0, depth, lx, ly, legal, dec), n * (64 + 8 + 2 * 38 * 4 + 8 + 64))
    for t in range(depth):
        compare.compare_rows(rec, rows, t, depth, lx, ly, legal, dec)
    keys = dec.view(torch.int64)[:, 0]
    top = torch.tensor(-2 ** 63, dtype=torch.int64, device="cuda:0")
    ordered, perm = torch.sort(torch.bitwise_xor(keys, top), stable=True)
    unique, counts = torch.unique_consecutive(ordered, return_counts=True)
    start = torch.zeros(unique.shape[0] + 1, dtype=torch.int64, device="cuda:0")
    start[1:] = counts.cumsum(0)
    first = int((unique[0] == top).item())
    start = start[first:].contiguous()
    sdec = dec[perm].contiguous()
    k = start.shape[0] - 1
    # reduce: the sorted decisions in, the entries written twice (the memset and the counters)
    out["reduce"] = dict(beside_copy(lambda: compare.compare_reduce(sdec, start), sdec.shape[0] * 64 + 2 * k * compare.ENTRY_DTYPE.itemsize + (k + 1) * 8),
                         K=k, longest_run=int(counts[first:].max()))
    out["sort_us"] = launches(lambda: torch.sort(torch.bitwise_xor(keys, top), stable=True))[0]
    return out


args = [a for a in sys.argv[1:] if not a.startswith("parent=")]
parent = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("parent=")), None)
out = {"device": torch.cuda.get_device_name(0), "block": compare.BLOCK, "boards": N}
bm = boards.make_board_match(env, "relu", "DeepMind", "relu", "DeepMind", N)
_, records = bm(net_a, net_b, 5)
for depth in (4, 10):
    out[f"kernels_depth_{depth}"] = kernels(records, depth)
ev = make_simple_duplicate_evaluate(env, "relu", "DeepMind", "relu", "DeepMind", N)
out["evaluate_10000_ms"] = timed(lambda: ev(net_a, net_b, 5))
if parent:
    r = subprocess.run([sys.executable, os.path.join(HERE, "scripts", "boards_throughput.py"), "--evaluate-only"],
                       env=dict(os.environ, BRL_BOARDS_ROOT=os.path.abspath(parent)), capture_output=True, text=True, timeout=600)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("EVALUATE ")]
    if r.returncode != 0 or not line:
        raise SystemExit("parent run failed:\n" + r.stderr[-2000:])
    out["parent_evaluate_10000_ms"] = json.loads(line[-1][len("EVALUATE "):])
out["board_match_10000_ms"] = timed(lambda: bm(net_a, net_b, 5))
for depth in (4, 10):
    policy_diff = compare.make_policy_diff(env, "relu", "DeepMind", "relu", "DeepMind", depth=depth)
    pd = policy_diff(net_a, net_b, records)
    out[f"policy_diff_10000_depth_{depth}_ms"] = dict(timed(lambda: policy_diff(net_a, net_b, records)), decisions=len(pd), prefixes=len(pd.entries))
out["evaluate_10000_again_ms"] = timed(lambda: ev(net_a, net_b, 5))

path = args[0] if args else os.path.join(HERE, "profiles", "compare", "throughput.json")
os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
json.dump(out, open(path, "w"), indent=1)
print(json.dumps(out, indent=1))
