"""Device time of the bidding-system book (brl_amd/book.py): brl_book_samples and brl_book_reduce at 10 000 and 65 536 boards x 2
tables, depth 4 and 10 (HIP events around 100 back-to-back launches after a warm-up, median of three), system_book as a whole
(median of five calls), the worst case beside them (every table with the same auction), the 10 000-board
make_simple_duplicate_evaluate it is budgeted against, and once the host route it replaces (the records copied to the host plus
tests/book_ref.py), in one session.

    python scripts/book_throughput.py [out.json] [parent=DIR]      (default: profiles/book/throughput.json)

``parent=DIR``: a built checkout of the parent commit; its evaluator is timed by a child process (boards_throughput.py
``--evaluate-only`` with DIR as the package root) between this tree's measurements."""
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "tests"))

import brl_amd  # noqa: E402
from brl_amd import book, boards  # noqa: E402
from brl_amd.evaluation import make_simple_duplicate_evaluate  # noqa: E402
from brl_amd.models import make_forward_pass  # noqa: E402

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


def measure(records, depth):
    """the two launches and the whole call on one match's records"""
    n = len(records)
    ta, tb, imp = records.table_a, records.table_b, records.imp
    per = n * depth
    keys = torch.zeros(2 * per + 1, dtype=torch.int64, device="cuda:0")
    feats = torch.zeros(2 * per + 1, dtype=torch.int32, device="cuda:0")
    us_s, runs_s = launches(lambda: book.book_samples(ta, depth, imp, 1, keys[:per], feats[:per]))
    book.book_samples(tb, depth, imp, -1, keys[per:2 * per], feats[per:2 * per])
    top = torch.tensor(-2 ** 63, dtype=torch.int64, device="cuda:0")
    ordered, perm = torch.sort(torch.bitwise_xor(keys, top))
    unique, inverse = torch.unique_consecutive(ordered, return_inverse=True)
    k = int(unique.shape[0]) - 1
    fs, idx, ek = feats[perm], (inverse - 1).to(torch.int32), torch.bitwise_xor(unique[1:], top).contiguous()
    samples = int((idx >= 0).sum())
    us_r, runs_r = launches(lambda: book.book_reduce(fs, idx, ek))
    us_sort, _ = launches(lambda: torch.sort(torch.bitwise_xor(keys, top)))
    # the bytes each launch has to move: 64 of a record's 368 in and 12 per position out; 8 per sorted sample in and the
    # entries written twice (the memset and the counters)
    b_s, b_r = n * (64 + 12 * depth), (2 * per + 1) * 8 + 2 * k * book.ENTRY_DTYPE.itemsize
    return {"boards": n, "depth": depth, "samples": samples, "K": k,
            "samples_us_per_launch_one_table": us_s, "samples_runs_us": runs_s, "samples_bytes": b_s, "samples_GB_per_s": b_s / us_s / 1e3,
            "reduce_us_per_launch": us_r, "reduce_runs_us": runs_r, "reduce_bytes": b_r, "reduce_GB_per_s": b_r / us_r / 1e3,
            "sort_us": us_sort, "system_book_ms": timed(lambda: book.system_book(records, depth))}


args = [a for a in sys.argv[1:] if not a.startswith("parent=")]
parent = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("parent=")), None)
out = {"device": torch.cuda.get_device_name(0), "chunk": 1024}
matches = {}
for n in (10000, 65536):
    _, matches[n] = boards.make_board_match(env, "relu", "DeepMind", "relu", "DeepMind", n)(net_a, net_b, 5)
    for depth in (4, 10):
        out[f"match_{n}_depth_{depth}"] = measure(matches[n], depth)
        same = boards.BoardRecords(matches[n].table_a[:1].expand(n, 368).contiguous(), matches[n].table_b[:1].expand(n, 368).contiguous(),
                                   matches[n].imp)
        out[f"same_auction_{n}_depth_{depth}"] = measure(same, depth)

ev = make_simple_duplicate_evaluate(env, "relu", "DeepMind", "relu", "DeepMind", 10000)
out["evaluate_10000_ms"] = timed(lambda: ev(net_a, net_b, 5))
if parent:
    r = subprocess.run([sys.executable, os.path.join(HERE, "scripts", "boards_throughput.py"), "--evaluate-only"],
                       env=dict(os.environ, BRL_BOARDS_ROOT=os.path.abspath(parent)), capture_output=True, text=True, timeout=600)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("EVALUATE ")]
    if r.returncode != 0 or not line:
        raise SystemExit("parent run failed:\n" + r.stderr[-2000:])
    out["parent_evaluate_10000_ms"] = json.loads(line[-1][len("EVALUATE "):])
out["system_book_10000_depth_4_again_ms"] = timed(lambda: book.system_book(matches[10000], 4))

# the host route, once: both tables to the host, then the Python restatement
import book_ref  # noqa: E402

fresh = boards.BoardRecords(matches[10000].table_a, matches[10000].table_b, matches[10000].imp)
torch.cuda.synchronize()
t0 = time.perf_counter()
ra, rb = fresh.cpu("a"), fresh.cpu("b")
t1 = time.perf_counter()
ref, _ = book_ref.book_of(ra, rb, 4, fresh.imp.cpu().numpy())
t2 = time.perf_counter()
out["host_route_10000_depth_4_ms"] = {"copy": (t1 - t0) * 1e3, "python": (t2 - t1) * 1e3, "entries": len(ref)}

path = args[0] if args else os.path.join(HERE, "profiles", "book", "throughput.json")
os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
json.dump(out, open(path, "w"), indent=1)
print(json.dumps(out, indent=1))
