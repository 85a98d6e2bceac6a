"""-m gpu: the board records (brl_amd/boards.py, include/brl_boards.h) — the kernel against recorded actions and the oracle on
every table, against its Python restatement bit for bit, board_match against the evaluator and against oracle replays, the 1000
real deals, the command line, and a graph replay."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import board_records_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMED = os.path.join(ROOT, "tests", "golden", "wb5_named_24.json")


def _env(dds):
    import brl_amd
    return brl_amd.BridgeBidding(lut=(dds["keys"], dds["values"]), device=DEV)


def _plans(n, seed):
    """n call lists: the 319-call auction, pass-outs, finished random auctions, tables stopped after k calls, and (table n - 1,
    n > 3) a table ended by an illegal call; returns (calls, illegal call or None per table)"""
    rng = np.random.default_rng(seed)
    plans, bad = [], []
    for i in range(n):
        stop = None if i % 3 else int(rng.integers(0, 25))
        calls = R.longest_auction() if i == 0 else [0, 0, 0, 0] if i in (1, 2) else \
            R.random_auction(rng, stop=stop, p_pass=float(rng.uniform(0.05, 0.6)))
        plans.append(calls)
        bad.append(None)
    if n > 3:
        for i in (n - 1, n - 2):
            while True:
                calls = R.random_auction(rng, stop=int(rng.integers(1, 12)))
                t = R.encode(0, calls)
                if not t.term:
                    break
            plans[i] = calls
            choices = [a for a in (1, 2) if not t.legal(a)]
            bad[i] = choices[i % len(choices)]
    return plans, bad


@pytest.mark.parametrize("n", [1, 5, 64, 4099])
def test_records_equal_the_recorded_actions_and_the_oracle_on_every_table(dds, oracle, n):
    from brl_amd import boards
    env = _env(dds)
    rng = np.random.default_rng(100 + n)
    rows = rng.integers(0, 1000, size=n)
    hand = np.stack([oracle.key_to_hand(dds["keys"][r]) for r in rows])
    dealer = (np.arange(n) & 3).astype(np.int32)                       # all four dealers
    vns, vew = ((np.arange(n) >> 2) & 1).astype(np.uint8), ((np.arange(n) >> 3) & 1).astype(np.uint8)   # all vulnerabilities
    perms = np.array([[0, 1, 2, 3], [1, 0, 3, 2], [2, 3, 0, 1], [3, 2, 1, 0]], np.int32)
    shuf = perms[(np.arange(n) >> 4) & 3]
    tricks = dds["tricks"][rows].reshape(n, 20)
    plans, bad = _plans(n, 200 + n)
    st = env.init_from_deals(hand, dealer, vns, vew, shuf, tricks)
    orc = oracle.init_explicit(hand, dealer, vns, vew, shuf, tricks)
    lens = np.array([len(p) + (b is not None) for p, b in zip(plans, bad)])
    full = [p + ([b] if b is not None else []) for p, b in zip(plans, bad)]
    score = np.zeros(n, np.int64)
    # a table that has no call left is parked: stepping it further would change it, so only the others are stepped (by index)
    for k in range(int(lens.max())):
        live = np.nonzero(lens > k)[0]
        act = np.array([full[i][k] for i in live], np.int32)
        sub = env.step(type(st)(env, st.packed[torch.from_numpy(live).to(DEV)].contiguous()), torch.from_numpy(act).to(DEV))
        st.packed[torch.from_numpy(live).to(DEV)] = sub.packed
        o = orc[live]
        was = o["terminated"].copy()
        oracle.step(o, act)
        ended = (o["terminated"] != 0) & (was == 0)
        ns_player = o["shuffled_players"][:, 0]
        score[live[ended]] = o["rewards"][np.arange(len(live)), ns_player][ended].astype(np.int64)
        orc[live] = o
    torch.cuda.synchronize()
    rec = boards.board_records(st.packed).cpu().numpy().view(boards.RECORD_DTYPE).reshape(-1)
    assert rec.shape == (n,)
    for i in range(n):                                                  # EVERY table
        r, want = rec[i], plans[i]
        assert r["flags"] & boards.OK, i
        assert r["n_calls"] == len(want) and r["calls"][:len(want)].tolist() == want, (i, want, r["calls"][:r["n_calls"]])
        assert (r["calls"][len(want):] == boards.FILL).all(), i
        o = orc[i]
        assert bool(r["flags"] & boards.TERMINATED) == bool(o["terminated"]) and bool(r["flags"] & boards.ILLEGAL) == bool(o["illegal"])
        assert (r["dealer"], r["vul_ns"], r["vul_ew"]) == (dealer[i], vns[i], vew[i])
        assert [(int(r["seating"]) >> (2 * s)) & 3 for s in range(4)] == shuf[i].tolist()
        if bad[i] is not None:
            assert r["flags"] & boards.ILLEGAL and (r["level"], r["strain"], r["doubled"], r["declarer"], r["score_ns"]) == (0, 0, 0, 0, 0)
        elif o["terminated"] and o["last_bid"] >= 0:
            den = int(o["last_bid"]) % 5
            side = [int(p) for p in shuf[i]].index(int(o["last_bidder"])) & 1
            decl = int((o["first_denomination_ew"] if side else o["first_denomination_ns"])[den])
            assert (r["level"], r["strain"]) == (int(o["last_bid"]) // 5 + 1, den), i
            assert r["doubled"] == (2 if o["call_xx"] else int(o["call_x"])) and r["declarer"] == decl, i
            assert r["tricks"] == tricks[i, decl * 5 + den] and r["score_ns"] == score[i], (i, r["score_ns"], score[i])
            assert not r["flags"] & boards.PASSED_OUT
        else:
            assert (r["level"], r["strain"], r["doubled"], r["declarer"], r["tricks"], r["score_ns"]) == (0, 0, 0, 0, 0, 0)
            assert bool(r["flags"] & boards.PASSED_OUT) == bool(o["terminated"])
        assert r["hands"].tolist() == [sum(1 << int(b) for b in boards._pgx_to_bit(hand[i, s * 13:(s + 1) * 13])) for s in range(4)]
    # the Python restatement decodes the same buffer to the same bytes
    want = R.decode(st.packed.cpu().numpy())
    assert rec.tobytes() == want.tobytes()
    if n == 4099:
        assert rec["n_calls"].max() == 319 and (rec["flags"] & boards.PASSED_OUT).any() and (~(rec["flags"] & boards.TERMINATED).astype(bool)).any()
        # the host API hands a record on only with its self-check bit
        raw = boards.board_records(st.packed)
        raw[7, 5] &= ~boards.OK
        with pytest.raises(ValueError, match="record 7 fails the self-check"):
            boards.BoardRecords(raw).cpu()


def test_a_table_ended_by_an_illegal_bid_gets_no_record(dds, oracle):
    """include/brl_boards.h: an illegal bid overwrites _last_bid — ILLEGAL | TERMINATED, n_calls 0, an all-fill row, no OK bit —
    and the host API refuses the set; its neighbours' records are untouched"""
    from brl_amd import boards
    env = _env(dds)
    hand = np.stack([oracle.key_to_hand(dds["keys"][r]) for r in range(3)])
    st = env.init_from_deals(hand, [0, 1, 2], 0, 0, [0, 1, 2, 3], dds["tricks"][:3].reshape(3, 20))
    plans = [[3 + 10, 0, 3 + 4], [3 + 10, 0, 3 + 12], [0, 3 + 7, 1, 3 + 7]]     # too low / a live auction / the same bid again
    for k in range(4):
        live = [i for i in range(3) if len(plans[i]) > k]
        idx = torch.tensor(live, device=DEV)
        sub = env.step(type(st)(env, st.packed[idx].contiguous()), torch.tensor([plans[i][k] for i in live], dtype=torch.int32, device=DEV))
        st.packed[idx] = sub.packed
    raw = boards.board_records(st.packed)
    rec = raw.cpu().numpy().view(boards.RECORD_DTYPE).reshape(-1)
    for i in (0, 2):
        assert rec[i]["flags"] == boards.TERMINATED | boards.ILLEGAL and rec[i]["n_calls"] == 0
        assert (rec[i]["calls"] == boards.FILL).all() and rec[i]["level"] == 0 and rec[i]["score_ns"] == 0
    assert rec[1]["flags"] == boards.OK and rec[1]["calls"][:3].tolist() == plans[1]
    assert rec.tobytes() == R.decode(st.packed.cpu().numpy()).tobytes()
    with pytest.raises(ValueError, match="record 0 fails the self-check"):
        boards.BoardRecords(raw).cpu()


def _nets(seeds=(1, 2)):
    from brl_amd.models import make_forward_pass
    fp = make_forward_pass("relu", "DeepMind")
    return [fp.init(s, device=DEV) for s in seeds]


def _replay(oracle, rec, dda):
    """each record's calls through the oracle from the record's own deal: (terminated, last_bid, x, xx, score_ns)"""
    from brl_amd import boards
    n = rec.shape[0]
    hand = np.zeros((n, 52), np.int32)
    for s in range(4):
        b = (rec["hands"][:, s][:, None] >> np.arange(52, dtype=np.uint64)[None, :]) & np.uint64(1)
        hand[:, s * 13:(s + 1) * 13] = np.sort(boards._bit_to_pgx(np.nonzero(b)[1].reshape(n, 13)), axis=1)
    shuf = np.stack([(rec["seating"] >> (2 * s)) & 3 for s in range(4)], axis=1).astype(np.int32)
    o = oracle.init_explicit(hand, rec["dealer"].astype(np.int32), rec["vul_ns"], rec["vul_ew"], shuf, dda)
    score = np.zeros(n, np.int64)
    for k in range(int(rec["n_calls"].max())):
        live = np.nonzero(rec["n_calls"] > k)[0]
        sub = o[live]
        oracle.step(sub, rec["calls"][live, k].astype(np.int32))
        assert not sub["illegal"].any()
        ended = sub["terminated"] != 0
        score[live[ended]] = sub["rewards"][np.arange(len(live)), sub["shuffled_players"][:, 0]][ended].astype(np.int64)
        o[live] = sub
    return o, score


@pytest.mark.parametrize("n", [640, 10000])
def test_board_match_equals_the_evaluator_and_replays_through_the_oracle(dds, oracle, n):
    from brl_amd import boards
    from brl_amd.evaluation import make_simple_duplicate_evaluate
    env = _env(dds)
    net1, net2 = _nets()
    want, ta, tb = make_simple_duplicate_evaluate(env, "relu", "DeepMind", "relu", "DeepMind", n)(net1, net2, 5)
    log, records = boards.make_board_match(env, "relu", "DeepMind", "relu", "DeepMind", n)(net1, net2, 5)
    for a, b in zip(log, want):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    ra, rb = records.cpu("a"), records.cpu("b")
    # the evaluator's per-board return is player 0's: the IMP of table A's North-South pair when player 0 sits there
    sign = np.where((ra["seating"] & 3) < 2, 1, -1)
    assert np.array_equal(records.imp.cpu().numpy() * sign, records.cum_return.cpu().numpy().astype(np.int64))
    assert (rb["seating"] == (((ra["seating"] >> 2) & 0x33) | ((ra["seating"] & 0x33) << 2))).all()     # seats [1,0,3,2]
    for name in ("hands", "dealer", "vul_ns", "vul_ew"):
        assert np.array_equal(ra[name], rb[name])
    dda = records.dda.cpu().numpy()
    for rec, info in ((ra, ta), (rb, tb)):
        assert ((rec["flags"] & boards.TERMINATED) != 0).all() and ((rec["flags"] & boards.ILLEGAL) == 0).all()
        o, score = _replay(oracle, rec, dda)
        assert (o["terminated"] != 0).all()
        has = o["last_bid"] >= 0
        assert np.array_equal(has, (rec["flags"] & boards.PASSED_OUT) == 0)
        assert np.array_equal(rec["level"][has], o["last_bid"][has] // 5 + 1) and np.array_equal(rec["strain"][has], o["last_bid"][has] % 5)
        assert np.array_equal(rec["doubled"][has], np.where(o["call_xx"][has] != 0, 2, o["call_x"][has]))
        assert np.array_equal(rec["score_ns"], score)
        # and the evaluator's own Table_info says the same of every board
        assert np.array_equal(info.last_bid.cpu().numpy(), o["last_bid"])
        p_ns = (rec["seating"] & 3).astype(np.int64)
        assert np.array_equal(info.rewards.cpu().numpy()[np.arange(n), p_ns].astype(np.int64), rec["score_ns"])


def _legal(calls):
    """the rule check: increasing bids, X only of an opponent's undoubled bid, XX only of one's own side's doubled bid, the end
    after three passes behind a bid or four passes"""
    last, seat_of, x, xx, passes = -1, None, False, False, 0
    for k, c in enumerate(calls):
        assert passes < (3 if last >= 0 else 4), "a call after the end"
        if c == "P":
            passes += 1
            continue
        passes = 0
        if c == "X":
            assert last >= 0 and (k - seat_of) % 2 == 1 and not x and not xx
            x = True
        elif c == "XX":
            assert last >= 0 and (k - seat_of) % 2 == 0 and x and not xx
            xx = True
        else:
            b = (int(c[0]) - 1) * 5 + ("C", "D", "H", "S", "NT").index(c[1:])
            assert b > last
            last, seat_of, x, xx = b, k, False, False
    assert passes == (3 if last >= 0 else 4), "the auction does not end"


def test_board_match_plays_the_1000_real_deals(dds, oracle):
    from brl_amd import boards
    env = _env(dds)
    net1, net2 = _nets((3, 4))
    hand = np.stack([oracle.key_to_hand(k) for k in dds["keys"]])
    deals = boards.Deals(np.sort(hand.reshape(-1, 4, 13), axis=2).reshape(-1, 52).astype(np.int32), dds["dealer"], dds["vul_ns"], dds["vul_ew"],
                         dds["tricks"].reshape(-1, 20), dds["board_id"])
    log, records = boards.make_board_match(env, "relu", "DeepMind", "relu", "DeepMind")(net1, net2, deals)
    assert len(records) == 1000 and np.isfinite(float(log[0]))
    named = json.load(open(NAMED))["logs"]
    for t in ("a", "b"):
        rec = records.cpu(t)
        assert np.array_equal(rec["hands"], deals.hand_words())
        assert np.array_equal(rec["dealer"], dds["dealer"]) and np.array_equal(rec["vul_ns"], dds["vul_ns"]) and np.array_equal(rec["vul_ew"], dds["vul_ew"])
        has = (rec["flags"] & boards.PASSED_OUT) == 0
        idx = np.nonzero(has)[0]
        assert np.array_equal(rec["tricks"][idx], dds["tricks"][idx, rec["declarer"][idx], rec["strain"][idx]])
        for i in range(24):   # by string handling alone: suit by suit S,H,D,C, ranks high to low
            want = "N:" + " ".join(".".join("".join(sorted((c[1] for c in named[i]["deal"][seat] if c[0] == s), key="23456789TJQKA".index,
                                                              reverse=True)) for s in "SHDC") for seat in "NESW")
            assert records.hands(i, t) == want
        for i in range(1000):
            _legal(records.auction(i, t))
    assert np.array_equal(records.dda.cpu().numpy(), dds["tricks"].reshape(-1, 20))
    assert np.array_equal(boards.read_deals(NAMED).lut_keys(), deals.lut_keys()[:24])


def test_the_command_line_writes_boards_it_reads_back(tmp_path, dds):
    from brl_amd import boards, checkpoint
    from brl_amd.models import make_forward_pass
    fp = make_forward_pass("relu", "DeepMind")
    for k in range(2):
        checkpoint.save_params(fp.init(50 + k), str(tmp_path / f"params-{k:08}.pt"))
    envv = dict(os.environ, PYTHONPATH=ROOT)
    base = [sys.executable, "-m", "brl_amd.eval", f"team1_model_path={tmp_path / 'params-00000000.pt'}",
            f"team2_model_path={tmp_path / 'params-00000001.pt'}", f"deals_path={NAMED}"]
    lines = []
    for extra in ([], [f"save_boards={tmp_path / 'out.json'}"], [f"save_boards={tmp_path / 'out.pbn'}"]):
        r = subprocess.run(base + extra, cwd=tmp_path, env=envv, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines.append([ln for ln in r.stdout.splitlines() if ln.startswith("IMP: ")][-1])
    assert lines[0] == lines[1] == lines[2]
    want = boards.read_deals(NAMED)
    for name in ("out.json", "out.pbn"):
        back = boards.read_deals(str(tmp_path / name))
        assert all(np.array_equal(a, b) for a, b in zip(back, want))
    # without a deal file: the evaluator's own path against the save_boards path, on the boards the evaluator deals
    lut = tmp_path / "lut.npy"
    np.save(lut, np.stack([dds["keys"], dds["values"]]))
    dealt = []
    for extra in ([], [f"save_boards={tmp_path / 'dealt.json'}"]):
        r = subprocess.run(base[:-1] + ["num_eval_envs=64", f"dds_path={lut}"] + extra, cwd=tmp_path, env=envv, capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        dealt.append([ln for ln in r.stdout.splitlines() if ln.startswith("IMP: ")][-1])
    assert dealt[0] == dealt[1]
    assert boards.read_deals(str(tmp_path / "dealt.json")).n == 64
    logs = json.load(open(tmp_path / "out.json"))["logs"]
    assert len(logs) == 24 and all(set(b) >= {"table_a", "table_b", "imp"} for b in logs)
    for b in logs:
        _legal(b["table_a"]["auction"])
        _legal(b["table_b"]["auction"])


def test_the_records_launch_is_captured_and_replayed(dds):
    from brl_amd import _capture, boards
    env = _env(dds)
    st = env.init(9, num_envs=3000)
    rng = np.random.default_rng(9)
    for _ in range(12):
        mask = st.legal_action_mask.cpu().numpy().astype(np.uint8)
        r = rng.random(mask.shape) * mask
        st = env.step(st, torch.from_numpy(r.argmax(axis=1).astype(np.int32)).to(DEV))
    packed = st.packed.clone()
    eager = boards.board_records(packed).clone()
    out = torch.zeros_like(eager)
    from brl_amd import _capi

    def launch():
        _capi.check(_capi.lib().brl_board_records(0, _capi.ptr(packed), packed.shape[0], _capi.ptr(out), _capi.stream(0)))

    _capture.warm_up(launch, 2)
    g = _capture.capture(launch)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    other = env.init(10, num_envs=3000).packed     # new tables in the captured buffer: the replay reads them
    packed.copy_(other)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, boards.board_records(other))
