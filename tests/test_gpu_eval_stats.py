"""-m gpu: every counter behind ``make_evaluate``'s statistics, on input that reaches it.

The evaluators' other tests play two randomly initialised networks against each other; a counter that is zero on both sides
compares equal whatever offset, team or table it was filed under.  Measured once on the MI355X: the n = 2048 run of
test_duplicate_evaluate_with_statistics_matches_oracle leaves 80 of the 231 ``brl_eval_reduce`` counters non-zero (its n = 640
run 73: no pass-out, 7 of the 70 contract bins per table, 31 of the 70 bid bins; not asserted: it describes random weights);
the scripted duplicate run in here all 231.

* ``brl_eval_reduce`` alone on synthetic, deliberately skewed tables (tests/eval_counts_ref.py): exact against the numpy
  restatement of the counter layout, at the edges of its 256-thread blocks, with one and two tables, with and without
  ``bid_count`` / ``state``, and with counts whose sum needs more than 32 bits.
* The scripted contract matrix (tests/contract_matrix.py: 35 284 boards, all 35 contracts and bids of both teams at both
  tables) through ``_eval_loop`` with statistics — duplicate and single table, the lock-step loop and the team-alternating one —
  against an oracle replay of the calls each loop recorded: the step log per board, the counters, and ``log_info``.
* count versus set of ``bid_count``, told apart by a prefilled buffer (no team makes the same bid twice on a board of the matrix)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import contract_matrix as cm
from tests import eval_counts_ref as er
from tests.gpu_util import _assert_log_info, make_env, to_np

pytestmark = pytest.mark.gpu

SEED = 11
TABLE_FIELDS = ("terminated", "rewards", "last_bid", "last_bidder", "call_x", "call_xx")


# ---- brl_eval_reduce alone ---------------------------------------------------------------------------------------------------------
def _device_table(T, dev):
    import brl_amd
    return brl_amd.Table_info(torch.from_numpy(T["terminated"]).to(dev).to(torch.bool), torch.from_numpy(T["rewards"]).to(dev),
                              torch.from_numpy(T["last_bid"]).to(dev), torch.from_numpy(T["last_bidder"]).to(dev),
                              torch.from_numpy(T["call_x"]).to(dev).to(torch.bool), torch.from_numpy(T["call_xx"]).to(dev).to(torch.bool))


def _stepped_states(env, oracle, n, seed):
    """real packed states, board i stepped i % 8 calls (ascending bids: always legal) -> (packed, the oracle's step_count)"""
    from brl_amd.bridge_bidding import State
    st = env.init(seed, num_envs=n)
    ref = oracle.init_random(n, seed=seed)
    packed = st.packed
    for k in range(7):
        live = np.nonzero(np.arange(n) % 8 > k)[0]
        if len(live) == 0:
            break
        act = (3 + 5 * k + live % 5).astype(np.int32)
        idx = torch.from_numpy(live).to(env.device)
        packed[idx] = env.step(State(env, packed[idx].contiguous()), torch.from_numpy(act).to(env.device)).packed
        sub = ref[live]
        oracle.step(sub, act)
        ref[live] = sub
    assert n < 8 or len(set(ref["step_count"].tolist())) == 8
    return packed, ref["step_count"].astype(np.int64)


@pytest.fixture(scope="module")
def reduce_env(dds):
    return make_env(dds, 4)


def _reduce_case(env, oracle, n, two, with_bids=True, with_state=True):
    from brl_amd import _capi
    from brl_amd._capi import check, ptr, stream
    dev = env.device
    A, B = er.synthetic_table(n, SEED, 0), (er.synthetic_table(n, SEED, 1) if two else None)
    bc = er.synthetic_bid_count(n, SEED) if with_bids else None
    packed, steps = _stepped_states(env, oracle, n, 5 + n) if with_state else (None, None)
    want = er.eval_counts_ref(A, B, bc, steps)
    tables = [_device_table(T, dev) for T in (A, B) if T is not None]
    pa, pb = tables[0]._ptrs(), (tables[1]._ptrs() if two else None)
    dbc = torch.from_numpy(bc).to(dev) if with_bids else None
    out = torch.full((_capi.EVAL_COUNTS,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev)   # (the entry point clears it itself)
    check(_capi.lib().brl_eval_reduce(env._h, n, C.byref(pa), C.byref(pb) if two else None, ptr(dbc), ptr(packed), ptr(out), stream()))
    return to_np(out), want, bc


@pytest.mark.parametrize("two", [False, True], ids=["one-table", "two-tables"])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 5000])
def test_eval_reduce_counters_exact(reduce_env, oracle, n, two):
    got, want, bc = _reduce_case(reduce_env, oracle, n, two)
    if n == 5000:   # of the input, not of the code under test: no two counters that a mix-up would exchange are equal
        assert er.equal_exchange_pairs(want, two) == [], "change SEED / the weights of tests/eval_counts_ref.py"
        assert (want[:er.EV_TABLE * (2 if two else 1)] != 0).all() and (want[er.EV_BIDS:] != 0).all()
    if n >= 255:
        assert want[er.EV_BIDS + 35 + 17] > 2 ** 32 and (bc == 0).all(axis=(1, 2)).sum() > n // 3
    assert want.shape == (er.EV_TOTAL,) and np.array_equal(got, want), np.nonzero(got != want)[0]


@pytest.mark.parametrize("missing", ["state", "bid_count"])
def test_eval_reduce_without_state_or_bid_count(reduce_env, oracle, missing):
    got, want, _ = _reduce_case(reduce_env, oracle, 257, True, with_bids=missing != "bid_count", with_state=missing != "state")
    assert (want[er.EV_STEPS] == 0) == (missing == "state") and (want[er.EV_BIDS:er.EV_STEPS] == 0).all() == (missing == "bid_count")
    assert np.array_equal(got, want), np.nonzero(got != want)[0]


# ---- the scripted matrix through the evaluators' loop ----------------------------------------------------------------------------
class _Script:
    """the calls every board is to make and how far it has come: ``after_step`` advances a board when it made a call"""

    def __init__(self, calls, length, dev):
        n, self.L = calls.shape
        self.calls = torch.from_numpy(np.concatenate([calls, np.zeros((n, 1), np.int32)], axis=1)).to(dev).to(torch.int64)
        self.length = torch.from_numpy(length).to(dev).to(torch.int64)
        self.pos = torch.zeros(n, dtype=torch.int64, device=dev)

    def after_step(self, packed, action):
        made = (action >= 0) & (self.pos < self.length)     # (-1: the board waited; a finished board is stepped on)
        self.pos += made.to(torch.int64)


class _ScriptedForward:
    """a "network" whose arg-max over any legal set that holds the scripted call is that call: fresh normal noise every time,
    the scripted call 0.5 above the row's maximum, so that the mass on illegal calls is neither 0 nor 1"""
    constant = True       # (_ActiveRows.forward calls it directly)

    def __init__(self, script, seed, dev):
        self.script, self.returned = script, []
        self.gen = torch.Generator(device=dev).manual_seed(seed)

    def __call__(self, obs_bool, obs_f32):
        s = self.script
        lg = torch.randn((s.pos.shape[0], 38), generator=self.gen, device=s.pos.device, dtype=torch.float32)
        act = s.calls.gather(1, s.pos.clamp(max=s.L)[:, None])
        lg.scatter_(1, act, lg.max(dim=1, keepdim=True).values + 0.5)
        self.returned.append(lg.clone())
        return lg


def _play(dds, m, rows, dup, alternate, bid_set, prefill=0):
    """the boards ``rows`` of the matrix through _eval_loop with statistics, then eval_counts and eval_log_info"""
    import brl_amd
    from brl_amd.bridge_bidding import State
    from brl_amd.evaluation import EvalStats, _eval_loop, _Shard, eval_counts, eval_log_info
    env = make_env(dds, 4)
    dev = env.device
    st = env.init_from_deals(m.hand[rows], m.dealer[rows], m.vul_ns[rows], m.vul_ew[rows], m.shuffled[rows], m.tricks[rows])
    n = st.num_envs
    script = _Script(*((m.pair_calls[rows], m.pair_length[rows]) if dup else (m.calls[rows], m.length[rows])), dev)
    f1, f2 = _ScriptedForward(script, 1001, dev), _ScriptedForward(script, 2002, dev)
    tables = (brl_amd.Table_info.from_state(st), brl_amd.Table_info.from_state(st)) if dup else None
    cum = torch.zeros(n, dtype=torch.float32, device=dev)
    rsum = None if dup else torch.zeros((n, 4), dtype=torch.float32, device=dev)
    stats = EvalStats(n, dev)
    stats.bid_count.fill_(prefill)
    rec = []
    with torch.no_grad():
        state, count = _eval_loop(env, st, f1, f2, tables, stats, bid_set, cum, rsum, calls=rec, full=not alternate,
                                  after_step=script.after_step)
        if not dup:
            f = State(env, state.packed)
            tables = (brl_amd.Table_info(f.terminated, rsum, f._last_bid, f._last_bidder, f._call_x, f._call_xx),)
        counts = eval_counts(env, n, tables, stats.bid_count, state.packed)
        log_info = eval_log_info(counts.to(torch.float64), stats, cum, dup, _Shard(n, None))
    torch.cuda.synchronize()
    assert len(rec) == count and bool(state.terminated.all())
    return {"rec": [to_np(a) for a in rec], "logits": tuple([to_np(x) for x in f.returned] for f in (f1, f2)),
            "pos": to_np(script.pos), "counts": to_np(counts), "log_info": log_info, "cum": to_np(cum),
            "tables": [{k: to_np(getattr(T, k)) for k in TABLE_FIELDS} for T in tables],
            "stats": {k: to_np(getattr(stats, k)) for k in ("illegal_prob_sum", "step_count", "pass_count", "bid_count")}}


def _replay(oracle, m, rows, dup, alternate, bid_set, rec, logits):
    """The recorded calls (-1: the board waited) through the oracle, with the reference's step log (oracle/eval_stats.StepLog), the
    float64 sum of softmax(logits) . ~mask over exactly the steps each board logged, and the bound on its float32 accumulation:
    1e-6 + 1e-5 * mass per step (test_illegal_mass_against_float64) + 2**-24 * the running sum per addition."""
    from oracle import Oracle
    from oracle.eval_stats import StepLog
    ref = cm.oracle_init(oracle, m, rows)
    oA, oB = Oracle.table_info_from(ref), Oracle.table_info_from(ref)
    n = len(ref)
    r = np.arange(n)
    calls, length = (m.pair_calls[rows], m.pair_length[rows]) if dup else (m.calls[rows], m.length[rows])
    calls = np.concatenate([calls, np.zeros((n, 1), np.int32)], axis=1)
    log, pos = StepLog(n), np.zeros(n, np.int64)
    mass, bound = np.zeros((n, 2)), np.zeros((n, 2))
    cum, rsum = np.zeros(n, np.float32), np.zeros((n, 4), np.float32)
    for i, act in enumerate(rec):
        idle = act < 0
        live = (ref["terminated"] == 0) & ~idle
        team = ref["current_player"] >> 1
        if alternate:   # iteration i is team i & 1's: its boards act, the others wait
            assert (team[live] == (i & 1)).all() and (team[idle] != (i & 1)).all() and not (idle & (ref["terminated"] != 0)).any()
            lg = logits[i & 1][i // 2]
        else:
            assert not idle.any()
            lg = np.where((team == 0)[:, None], logits[0][i], logits[1][i])
        mask = ref["legal_action_mask"].astype(bool)
        a = np.where(idle, 0, act).astype(np.int32)
        assert np.array_equal(a[live], calls[r, np.minimum(pos, calls.shape[1] - 1)][live]) and mask[r, a][live].all(), i
        log.update(np.where(live, 0, 1), ref["current_player"], ref["legal_action_mask"], lg, a, bid_set=bid_set)
        x = lg.astype(np.float64)
        e = np.exp(x - x.max(1, keepdims=True))
        step_mass = ((e / e.sum(1, keepdims=True)) * ~mask).sum(1)
        mass[r[live], team[live]] += step_mass[live]
        bound[r[live], team[live]] += 1e-6 + 1e-5 * step_mass[live] + 2.0 ** -24 * mass[r[live], team[live]]
        pos[live] += 1
        keep = (ref[idle].copy(), oA[idle].copy(), oB[idle].copy())
        if dup:
            oracle.duplicate_step(ref, a, oA, oB)
        else:
            oracle.step(ref, a)
        ref[idle], oA[idle], oB[idle] = keep
        cum[~idle] += ref["rewards"][~idle, 0]
        rsum[~idle] += ref["rewards"][~idle]
    assert ref["terminated"].all() and np.array_equal(pos, length)       # every board finished, every scripted call was made
    if dup:
        assert oA["terminated"].all() and oB["terminated"].all()
        tables = [oA, oB]
    else:
        tables = [{"terminated": ref["terminated"], "rewards": rsum, "last_bid": ref["last_bid"], "last_bidder": ref["last_bidder"],
                   "call_x": ref["call_x"], "call_xx": ref["call_xx"]}]
    bids = log.bid.astype(np.int64)
    assert np.array_equal(bids, log.bid)
    want = er.eval_counts_ref(tables[0], tables[1] if dup else None, bids, ref["step_count"].astype(np.int64))
    return {"ref": ref, "tables": tables, "log": log, "mass": mass, "bound": bound, "cum": cum, "rsum": rsum, "counts": want}


_RUNS = {}


def _run(dds, oracle, dup, alternate):
    key = (dup, alternate)
    if key not in _RUNS:
        m = cm.matrix(dds, oracle)
        rows, bid_set = slice(None), 0 if dup else 1     # the single-table evaluator marks a bid as made, the duplicate one counts it
        got = _play(dds, m, rows, dup, alternate, bid_set)
        _RUNS[key] = (got, _replay(oracle, m, rows, dup, alternate, bool(bid_set), got["rec"], got["logits"]))
    return _RUNS[key]


@pytest.mark.parametrize("loop", ["lock-step", "alternating"])
@pytest.mark.parametrize("kind", ["duplicate", "single-table"])
def test_scripted_matrix_statistics(dds, oracle, kind, loop):
    from oracle.eval_stats import duplicate_log_info, single_log_info
    dup, alternate = kind == "duplicate", loop == "alternating"
    m = cm.matrix(dds, oracle)
    got, want = _run(dds, oracle, dup, alternate)
    log, ref, stats = want["log"], want["ref"], got["stats"]
    # preconditions, on the reference side: this input reaches what the test is about
    assert (log.step_count >= 1).all() and log.step_count.max() <= 10
    for T in want["tables"]:
        assert (T["rewards"][:, 0][T["last_bid"] >= 0] != 0).all()          # no played contract is a tie between "make" and "down"
    if dup:
        assert (want["counts"] != 0).all()
    assert alternate == any((a < 0).any() for a in got["rec"])
    # the loop itself
    assert np.array_equal(got["pos"], m.pair_length if dup else m.length)
    for T, oT in zip(got["tables"], want["tables"]):
        for f in TABLE_FIELDS:
            assert np.array_equal(T[f].astype(np.float64), np.asarray(oT[f]).astype(np.float64)), f
    assert np.array_equal(got["cum"], want["cum"])
    # the step log, per board and team
    assert np.array_equal(stats["step_count"], log.step_count)
    assert np.array_equal(stats["pass_count"], log.pass_count)
    assert np.array_equal(stats["bid_count"], log.bid)
    err = np.abs(stats["illegal_prob_sum"].astype(np.float64) - want["mass"])
    print(f"{kind} {loop}: illegal_prob_sum off by at most {err.max():.3e}, at most {np.max(err / want['bound']):.3f} of its bound; "
          f"mass per board and team {want['mass'].min():.3f} .. {want['mass'].max():.3f}")
    assert (err <= want["bound"]).all(), (err.max(), np.max(err / want["bound"]))
    assert want["mass"].min() > 1e-3 and (want["mass"] / log.step_count).max() < 0.99
    # the counters and log_info
    assert np.array_equal(got["counts"], want["counts"]), np.nonzero(got["counts"] != want["counts"])[0]
    if dup:
        _assert_log_info(got["log_info"], duplicate_log_info(want["cum"], log, ref["step_count"], *want["tables"]))
    else:
        _assert_log_info(got["log_info"], single_log_info(want["cum"], log, ref))


def test_scripted_duplicate_loops_agree(dds, oracle):
    """both loops play the same auctions: equal log_info, entry for entry, except the two means of the illegal mass, which
    depend on the noise each loop drew"""
    a, b = _run(dds, oracle, True, False)[0], _run(dds, oracle, True, True)[0]
    assert np.array_equal(a["counts"], b["counts"]) and len(a["log_info"]) == len(b["log_info"]) == 23
    for i, (x, y) in enumerate(zip(a["log_info"], b["log_info"])):
        if i not in (3, 4):
            assert torch.equal(torch.as_tensor(x), torch.as_tensor(y)), i


@pytest.mark.parametrize("bid_set", [0, 1])
def test_bid_count_counts_or_sets(dds, oracle, bid_set):
    """No team makes the same bid at both tables of a board of the matrix, so a count and a mark give the same bytes on a zeroed
    buffer.  On one filled with 1: counting (the duplicate evaluator, one-hot + bid) gives 1 + the log, marking (the single-table
    evaluator, .at[bid].set(1)) leaves every entry 1."""
    m = cm.matrix(dds, oracle)
    rows = slice(0, 512)
    got = _play(dds, m, rows, True, False, bid_set, prefill=1)
    want = _replay(oracle, m, rows, True, False, False, got["rec"], got["logits"])
    assert want["log"].bid.sum() >= 2 * 512 and want["log"].bid.max() == 1
    assert np.array_equal(got["stats"]["bid_count"], np.ones_like(want["log"].bid) if bid_set else 1 + want["log"].bid)
    assert np.array_equal(got["stats"]["step_count"], want["log"].step_count)
