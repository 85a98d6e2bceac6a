"""Device time of the position queries (brl_amd/positions.py): brl_position_rows and brl_position_answers per launch at n = 1, 64,
10 000 and 262 144 positions with auctions of 4 and of 12 calls, each beside a device-to-device copy of the bytes it has to move
(HIP events around 100 back-to-back launches after a warm-up, median of three); the same rows produced the way the tree could
produce them before — empty tables that exist already, t launches of brl_step, one brl_observe —; and ``ask`` as a whole (host time
of a call that ends with its copy to the host, median of 21 at n = 1 and of 5 at n = 10 000).

    python scripts/positions_throughput.py [out.json]      (default: profiles/positions/throughput.json)"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

import brl_amd  # noqa: E402
from brl_amd import _capi, positions  # noqa: E402
from brl_amd.models import make_forward_pass  # noqa: E402

DEV = "cuda:0"
AUCTIONS = {4: [3, 0, 4, 0], 12: [3, 0, 4, 0, 5, 0, 6, 0, 7, 0, 8, 0]}     # 1C P 1D P (1H P 1S P 1NT P 2C P): legal, still open
SIZES = (1, 64, 10000, 262144)
d = np.load(os.path.join(HERE, "tests", "golden", "wb5_dds_1000.npz"))
env = brl_amd.BridgeBidding(lut=(d["keys"], d["values"]), device=DEV)
net = make_forward_pass("relu", "DeepMind").init(1, device=DEV)
L = _capi.lib()


def launches(fn, reps=100):
    """us per launch: ``reps`` back-to-back launches between two events, median of three"""
    for _ in range(20):
        fn()
    ts = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1000.0 / reps)
    return statistics.median(ts), ts


def beside_copy(fn, nbytes):
    """a launch beside a device-to-device copy of ``nbytes`` (read once, written once: half of them each way)"""
    src = torch.empty(max(1, nbytes // 2), dtype=torch.uint8, device=DEV)
    dst = torch.empty_like(src)
    us, runs = launches(fn)
    us_c, runs_c = launches(lambda: dst.copy_(src))
    return {"us_per_launch": us, "runs_us": runs, "bytes": nbytes, "GB_per_s": nbytes / us / 1e3, "copy_us": us_c, "copy_runs_us": runs_c,
            "launch_over_copy": us / us_c}


def make_positions(n, calls, seed=0):
    rng = np.random.default_rng(seed)
    arr = np.zeros(n, positions.POSITION_DTYPE)
    deck = np.argsort(rng.random((n, 52)), axis=1)[:, :13].astype(np.uint64)
    arr["hand"] = (np.uint64(1) << deck).sum(1)
    arr["dealer"], arr["vul_ns"], arr["vul_ew"] = rng.integers(0, 4, n), rng.integers(0, 2, n), rng.integers(0, 2, n)
    arr["n_calls"], arr["calls"] = len(calls), positions.FILL
    arr["calls"][:, :len(calls)] = calls
    return arr


def case(n, t):
    arr = make_positions(n, AUCTIONS[t])
    pos = torch.from_numpy(arr.view(np.uint8).reshape(n, 64)).to(DEV)
    obs = torch.empty((n, 480), dtype=torch.bool, device=DEV)
    mask = torch.empty((n, 38), dtype=torch.uint8, device=DEV)
    legal = torch.empty(n, dtype=torch.int64, device=DEV)
    status = torch.empty(n, dtype=torch.int32, device=DEV)
    tables = torch.empty((n, 16), dtype=torch.int64, device=DEV)
    s = _capi.stream(0)
    rows = lambda tb: _capi.check(L.brl_position_rows(0, pos.data_ptr(), n, obs.data_ptr(), mask.data_ptr(), legal.data_ptr(),     # noqa: E731
                                                      status.data_ptr(), tb, s))
    out = {"n": n, "calls": t}
    out["rows"] = beside_copy(lambda: rows(None), n * (64 + 480 + 38 + 8 + 4))
    out["rows_with_tables"] = beside_copy(lambda: rows(tables.data_ptr()), n * (64 + 480 + 38 + 8 + 4 + 128))
    torch.cuda.synchronize()
    assert int((status != 0).sum()) == 0
    want_obs, want_mask = obs.clone(), mask.clone()

    # the yardstick: the empty tables exist already (their construction is not timed); t brl_step launches and one brl_observe
    empty_pos = pos.clone()
    empty_pos[:, 11], empty_pos[:, 16:] = 0, positions.FILL
    dealer_turn = torch.from_numpy(((arr["dealer"].astype(np.int64) + t) & 3).astype(np.uint8)).to(DEV)     # the caller's hand sits at the caller's seat
    empty = torch.empty((n, 16), dtype=torch.int64, device=DEV)
    shifted = empty_pos.clone()
    shifted[:, 8] = dealer_turn                                                                             # (dealer := caller: the hand lands at its seat)
    _capi.check(L.brl_position_rows(0, shifted.data_ptr(), n, obs.data_ptr(), mask.data_ptr(), legal.data_ptr(), status.data_ptr(),
                                    empty.data_ptr(), s))
    sc = empty[:, 11]
    empty[:, 11] = (sc & ~3) | torch.from_numpy(arr["dealer"].astype(np.int64)).to(DEV)                     # and the real dealer back into the scalars
    work = torch.empty_like(empty)
    acts = [torch.full((n,), a, dtype=torch.int32, device=DEV) for a in AUCTIONS[t]]

    def loop():
        for k, a in enumerate(acts):
            _capi.check(L.brl_step(env._h, (empty if k == 0 else work).data_ptr(), work.data_ptr(), n, a.data_ptr(), 0, None, None, None, None,
                                   None, s))
        _capi.check(L.brl_observe(env._h, work.data_ptr(), n, None, obs.data_ptr(), mask.data_ptr(), s))

    us, runs = launches(loop, reps=20)
    torch.cuda.synchronize()
    assert torch.equal(obs, want_obs) and torch.equal(mask, want_mask)                                     # the same rows
    out["step_loop"] = {"us": us, "runs_us": runs, "launches": t + 1, "over_one_launch": us / out["rows"]["us_per_launch"]}

    gen = torch.Generator(device=DEV).manual_seed(1)
    logits = torch.randn((n, 39), generator=gen, device=DEV) * 3
    answers = torch.empty((n, 96), dtype=torch.uint8, device=DEV)
    probs = torch.empty((n, 38), dtype=torch.float64, device=DEV)
    rows(None)
    ans = lambda pr: _capi.check(L.brl_position_answers(0, logits.data_ptr(), 39, logits.data_ptr() + 152, 39, legal.data_ptr(),     # noqa: E731
                                                        status.data_ptr(), n, 3, answers.data_ptr(), pr, s))
    out["answers"] = beside_copy(lambda: ans(None), n * (39 * 4 + 8 + 4 + 96))
    out["answers_with_probs"] = beside_copy(lambda: ans(probs.data_ptr()), n * (39 * 4 + 8 + 4 + 96 + 38 * 8))
    return out


def host_ms(fn, reps):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "calls": reps}


out = {"device": torch.cuda.get_device_name(0), "cases": [case(n, t) for t in (4, 12) for n in SIZES]}
bidder = positions.Bidder(net, "relu", "DeepMind")
ask = positions.make_bidder("relu", "DeepMind")
one, many = make_positions(1, AUCTIONS[4]), make_positions(10000, AUCTIONS[12])
out["ask"] = {"bidder_n_1": host_ms(lambda: bidder.ask(one), 21), "make_bidder_n_1": host_ms(lambda: ask(net, one), 21),
              "bidder_n_10000": host_ms(lambda: bidder.ask(many), 5), "make_bidder_n_10000": host_ms(lambda: ask(net, many), 5)}

path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "profiles", "positions", "throughput.json")
os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
json.dump(out, open(path, "w"), indent=1)
print(json.dumps(out, indent=1))
