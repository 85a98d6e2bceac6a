"""Device time of brl_board_records at 10 000 and 65 536 tables and of brl_board_keep_a at 10 000 (HIP events around 100
back-to-back launches after a warm-up, median of three), and the 10 000-board make_simple_duplicate_evaluate beside board_match
(HIP events around one call that ends in a synchronise, three warm-up calls, median of five), in one session.

    python scripts/boards_throughput.py [out.json] [parent=DIR]      (default: profiles/boards/throughput.json)

``parent=DIR``: a built checkout of the parent commit; its evaluator is timed the same way by a child process of this script
(``--evaluate-only``, run with DIR as the package root) between this tree's measurements."""
import json
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.environ.get("BRL_BOARDS_ROOT", HERE)     # the package root whose code is timed
sys.path.insert(0, ROOT)

import brl_amd  # noqa: E402
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


ev = make_simple_duplicate_evaluate(env, "relu", "DeepMind", "relu", "DeepMind", N)
if "--evaluate-only" in sys.argv:
    print("EVALUATE " + json.dumps(timed(lambda: ev(net_a, net_b, 5))))
    sys.exit(0)

from brl_amd import _capi, boards  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("parent=")]
parent = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("parent=")), None)
out = {"device": torch.cuda.get_device_name(0)}
for n in (10000, 65536):
    st = env.init(1, num_envs=n)
    for _ in range(14):   # live and finished tables mixed
        m = st.legal_action_mask
        st = env.step(st, (torch.rand(m.shape, device=m.device) * m).argmax(dim=1).to(torch.int32))
    packed = st.packed
    rec = torch.empty((n, 368), dtype=torch.uint8, device="cuda:0")
    us, runs = launches(lambda: _capi.check(_capi.lib().brl_board_records(0, _capi.ptr(packed), n, _capi.ptr(rec), _capi.stream(0))))
    out[f"records_{n}"] = {"us_per_launch_median_of_3": us, "runs_us": runs, "bytes_written": n * 368, "GB_per_s": n * 368 / us / 1e3,
                          "mean_calls": float(rec.cpu().numpy().view(boards.RECORD_DTYPE)["n_calls"].mean())}
    if n == N:
        prev, fin = packed.clone(), torch.zeros_like(packed)
        act = torch.zeros(n, dtype=torch.int32, device="cuda:0")
        done, taken = torch.zeros(n, dtype=torch.uint8, device="cuda:0"), torch.zeros(n, dtype=torch.uint8, device="cuda:0")
        us, runs = launches(lambda: _capi.check(_capi.lib().brl_board_keep_a(0, _capi.ptr(packed), _capi.ptr(prev), _capi.ptr(act),
                                                                              _capi.ptr(done), _capi.ptr(taken), _capi.ptr(fin), n, _capi.stream(0))))
        out[f"keep_a_{n}"] = {"us_per_launch_median_of_3": us, "runs_us": runs}

bm = boards.make_board_match(env, "relu", "DeepMind", "relu", "DeepMind", N)
out["evaluate_10000_ms"] = timed(lambda: ev(net_a, net_b, 5))
if parent:
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--evaluate-only"], env=dict(os.environ, BRL_BOARDS_ROOT=os.path.abspath(parent)),
                       capture_output=True, text=True, timeout=600)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("EVALUATE ")]
    if r.returncode != 0 or not line:
        raise SystemExit("parent run failed:\n" + r.stderr[-2000:])
    out["parent_evaluate_10000_ms"] = json.loads(line[-1][len("EVALUATE "):])
out["board_match_10000_ms"] = timed(lambda: bm(net_a, net_b, 5))


def with_copy():
    _, r = bm(net_a, net_b, 5)
    r.cpu("a")
    r.cpu("b")


out["board_match_10000_with_copy_ms"] = timed(with_copy)
out["evaluate_10000_again_ms"] = timed(lambda: ev(net_a, net_b, 5))
path = args[0] if args else os.path.join(HERE, "profiles", "boards", "throughput.json")
os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
json.dump(out, open(path, "w"), indent=1)
print(json.dumps(out, indent=1))
