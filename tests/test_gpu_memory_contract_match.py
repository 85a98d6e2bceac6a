"""-m gpu: the memory contract (tests/guarded.py; DESIGN.md "Memory contract") of the entry points that play and record a match:
the environment-side calls (brl_init_from_deals, brl_get_fields, brl_imp_reward, brl_duplicate_step), the evaluators' loop
(brl_eval_step, brl_eval_step_team, brl_eval_reduce), the routes and the grouped forward of the league and of cross-play
(brl_league_route, brl_xplay_route, brl_league_forward) and the board records (brl_board_records, brl_board_imp, brl_board_keep_a).

As tests/test_gpu_memory_contract.py: every case runs on plain dense tensors and on arrays placed in ONE Arena at exactly the
alignment the header states (where a header was silent it now states what the kernel moves), and asserts: the same bits both
ways; no guard byte and no element of a read-only input changed; every output element written (the `partial` ones by hand);
an optional output passed as NULL leaves nothing written; and the guarded result against the reference the project already holds
that entry point to — the oracle, tests/eval_counts_ref.py, the numpy routes, tests/board_records_ref.py, tests/nets.forward64.
The last test hands every entry point a pointer off its stated alignment: BRL_E_ARG on the host, nothing launched.
Nothing here can fault by design: no pointer that reaches a kernel is below its required alignment or outside the arena."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import board_records_ref as R
from tests import eval_counts_ref as er
from tests.crossplay_ref import xroute_numpy
from tests.gpu_util import assert_state_equal, make_env
from tests.guarded import Guarded, Plain, _bits, both  # noqa: F401
from tests.nets import forward64, observations, raw_net
from tests.test_league_host import route_numpy

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, U8, I32, I64 = torch.float32, torch.uint8, torch.int32, torch.int64
BRL_E_ARG = -1
TABLE_MEMBERS = (("terminated", U8, 1), ("rewards", F32, 16), ("last_bid", I32, 4), ("last_bidder", I32, 4), ("call_x", U8, 1),
                 ("call_xx", U8, 1))        # brl_table_info: (member, element type, the alignment include/brl_hip.h states)
FIELD_MEMBERS = (("current_player", I32, ()), ("terminated", U8, ()), ("rewards", F32, (4,)), ("step_count", I32, ()), ("turn", I32, ()),
                 ("dealer", I32, ()), ("vul_ns", U8, ()), ("vul_ew", U8, ()), ("shuffled_players", I32, (4,)), ("last_bid", I32, ()),
                 ("last_bidder", I32, ()), ("call_x", U8, ()), ("call_xx", U8, ()), ("pass_num", I32, ()),
                 ("first_denomination_ns", I32, (5,)), ("first_denomination_ew", I32, (5,)), ("hand", I32, (52,)), ("tricks", U8, (20,)),
                 ("lut_idx", I32, ()), ("board_ctr", I32, ()), ("illegal", U8, ()))     # brl_fields, in the struct's order


def _s():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _lib():
    from brl_amd import _capi
    return _capi.lib(), _capi.check


@pytest.fixture(scope="module")
def env(dds):
    return make_env(dds, 4)


def _col(a):
    """a column of an oracle record array as a dense array of its own"""
    return np.ascontiguousarray(a).copy()     # (a copy: one row of a record array keeps the record's stride)


def _align_of(dt, name):
    return 16 if name == "rewards" else torch.empty((), dtype=dt).element_size()


def _place_fields(mem, tag, n, only=None):
    """every member of a brl_fields (or the one named `only`) an output placement of its own -> (struct, {name: view})"""
    from brl_amd import _capi
    f, views = _capi.Fields(), {}
    for name, dt, tail in FIELD_MEMBERS:
        if only is None or name == only:
            views[name] = mem.out(f"{tag}.{name}", (n,) + tail, dt, _align_of(dt, name))
            setattr(f, name, views[name].data_ptr())
    return f, views


def _place_table(mem, tag, values, inout=True):
    """a brl_table_info whose six members are placements of their own, holding `values` -> (struct, {name: view})"""
    from brl_amd import _capi
    p, views = _capi.TableInfoPtrs(), {}
    for name, dt, align in TABLE_MEMBERS:
        views[name] = mem.inp(f"{tag}.{name}", _col(values[name]), dt, align, inout=inout)
        setattr(p, name, views[name].data_ptr())
    return p, views


# ---- brl_get_fields, brl_init_from_deals ---------------------------------------------------------------------------------------
def _mixed_calls(n):
    """four calls per table: a live doubled and redoubled auction, a contract, a pass-out; the last of three or more tables ends
    by an illegal call (a bid below the one on the table) and takes its later calls as a finished table does"""
    calls = np.zeros((4, n), np.int32)
    for i in range(n):
        k = i % 25
        calls[:, i] = ((0, 3 + k, 1, 2), (3 + k, 0, 0, 0), (0, 0, 0, 0))[i % 3]
    if n >= 3:
        calls[:, n - 1] = (3 + 10, 3 + 5, 0, 0)
    return calls


@pytest.mark.parametrize("n", [1, 3, 33, 65])
def test_fields_and_explicit_deals_guarded(env, oracle, n):
    """brl_get_fields on live tables, finished tables and one ended by an illegal call: state at exactly 8 bytes, every member
    of brl_fields a placement of its own (int32 at 4, uint8 at 1, rewards — one 16-byte store per table — at 16), once with
    every member and once with every member NULL but `turn`: then nothing else is written anywhere.  Every field against the
    oracle.  brl_init_from_deals from the oracle's deal fields of those tables (int32 at 4, uint8 at 1, state at 8): the rebuilt
    state's fields equal oracle.init_explicit's."""
    L, check = _lib()
    seed = 700 + n
    st = env.init(seed, num_envs=n)
    ref = oracle.init_random(n, seed=seed)
    for a in _mixed_calls(n):
        st = env.step(st, torch.from_numpy(a))
        oracle.step(ref, a)
    assert n < 3 or (ref["illegal"][n - 1] and ref["terminated"][1] and not ref["terminated"][0] and ref["rewards"][1].any())
    packed = st.packed.cpu()
    deal = {k: _col(ref[k]).astype(np.uint8 if k in ("vul_ns", "vul_ew", "tricks") else np.int32)
            for k in ("hand", "dealer", "vul_ns", "vul_ew", "shuffled_players", "tricks")}
    ref2 = oracle.init_explicit(deal["hand"], deal["dealer"], deal["vul_ns"], deal["vul_ew"], deal["shuffled_players"], deal["tricks"])

    def run(mem):
        s = mem.inp("state", packed, I64, 8)
        f_all, v_all = _place_fields(mem, "all", n)
        check(L.brl_get_fields(env._h, _p(s), n, C.byref(f_all), _s()))
        f_one, v_one = _place_fields(mem, "one", n, only="turn")
        check(L.brl_get_fields(env._h, _p(s), n, C.byref(f_one), _s()))
        d = {k: mem.inp(k, deal[k], U8 if deal[k].dtype == np.uint8 else I32, 1 if deal[k].dtype == np.uint8 else 4) for k in deal}
        s2 = mem.out("state_rebuilt", (n, 16), I64, 8)
        check(L.brl_init_from_deals(env._h, _p(s2), n, _p(d["hand"]), _p(d["dealer"]), _p(d["vul_ns"]), _p(d["vul_ew"]),
                                    _p(d["shuffled_players"]), _p(d["tricks"]), _s()))
        f_re, v_re = _place_fields(mem, "rebuilt", n)
        check(L.brl_get_fields(env._h, _p(s2), n, C.byref(f_re), _s()))
        return {"turn_only": v_one["turn"], "state_rebuilt": s2, **{f"all.{k}": v for k, v in v_all.items()},
                **{f"rebuilt.{k}": v for k, v in v_re.items()}}
    _, g, _ = both(run)
    assert torch.equal(g["turn_only"], g["all.turn"])
    for tag, want in (("all", ref), ("rebuilt", ref2)):
        for name, _, _ in FIELD_MEMBERS:
            got = g[f"{tag}.{name}"].cpu().numpy()
            assert np.array_equal(got.astype(np.float64), want[name].astype(np.float64)), (tag, name)
    assert (ref2["lut_idx"] == -1).all() and np.array_equal(ref2["hand"], ref["hand"])


# ---- brl_imp_reward ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 33, 65])
def test_imp_reward_guarded(env, oracle, n):
    """a and b (of a row only its first float is read) at exactly 4 bytes, out (one 16-byte store per board) at 16; table scores
    with +-7600 and 0 among them; against oracle.imp_reward, bit for bit."""
    L, check = _lib()
    rng = np.random.default_rng(40 + n)
    sign = np.array([1, 1, -1, -1])
    a = (rng.integers(-760, 761, (n, 1)) * 10 * sign).astype(np.float32)
    b = (rng.integers(-760, 761, (n, 1)) * 10 * sign).astype(np.float32)
    for i, (x, y) in enumerate(((7600, 7600), (-7600, -7600), (0, 0), (0, 7600), (7600, -7600))[:n]):
        a[i], b[i] = x * sign, y * sign

    def run(mem):
        aa, bb, out = mem.inp("a", a, F32, 4), mem.inp("b", b, F32, 4), mem.out("out", (n, 4), F32, 16)
        check(L.brl_imp_reward(env._h, _p(aa), _p(bb), _p(out), n, _s()))
        return {"out": out}
    _, g, _ = both(run)
    want = np.stack([oracle.imp_reward(a[i], b[i]) for i in range(n)])
    assert np.array_equal(g["out"].cpu().numpy(), want) and abs(want[0, 0]) == 24.0


# ---- the scripted duplicate match: brl_duplicate_step, brl_eval_step, brl_eval_step_team, brl_board_keep_a -------------------------
def _script(n):
    """The calls of every board, table A's and then table B's (a call is made when the board's turn comes: the tables are
    re-dealt seat-swapped in between): 0 passes both tables out (the hand-overs after 4 and 8 calls); 1 needs six calls for
    table A's doubled contract; 2 plays a contract at A and passes B out (a non-zero IMP); 3 plays a contract at A and is still
    bidding table B's doubled one after 8."""
    s = np.zeros((n, 16), np.int32)
    for i in range(n):
        k = i % 30
        s[i, :9] = ((0,) * 9, (0, 3 + k, 1, 0, 0, 0, 0, 0, 0), (3 + k, 0, 0, 0, 0, 0, 0, 0, 0), (3 + k, 0, 0, 0, 4 + k, 1, 0, 0, 0))[i % 4]
    return s


_PLANS = {}


def _plan(oracle, n, seed, dup, alternate, K):
    """K iterations of an evaluator's loop on the boards of init_random(n, seed), replayed through the oracle ONCE per shape:
    lock-step (every board calls: brl_duplicate_step / brl_eval_step) or alternating (iteration i is team i & 1's, the other
    unfinished boards wait: brl_eval_step_team).  The logits are normal noise with the scripted call 0.5 above the row's maximum
    (tests/test_gpu_eval_stats.py's scripted forward), different for the two teams.  Holds what each iteration's launch is
    given and what the oracle, its StepLog (oracle/eval_stats.py) and float64 say it leaves."""
    from oracle import Oracle
    from oracle.eval_stats import StepLog
    key = (n, seed, dup, alternate, K)
    if key in _PLANS:
        return _PLANS[key]
    ref = oracle.init_random(n, seed=seed)
    oA, oB = Oracle.table_info_from(ref), Oracle.table_info_from(ref)
    tables0 = (oA.copy(), oB.copy())
    script, r = _script(n), np.arange(n)
    rng = np.random.default_rng(seed)
    pos = np.zeros(n, np.int64)
    logs = {0: StepLog(n), 1: StepLog(n)}
    mass, bound = np.zeros((n, 2)), np.zeros((n, 2))
    cum, rsum = np.zeros(n, np.float32), np.zeros((n, 4), np.float32)
    l1, l2 = np.zeros((K, n, 38), np.float32), np.zeros((K, n, 38), np.float32)
    actions, waits, given = np.zeros((K, n), np.int32), np.zeros((K, n), bool), np.zeros((K, n), np.int32)
    final_a, a_taken = ref.copy(), np.zeros(n, bool)
    for i in range(K):
        team = ref["current_player"] >> 1
        term = ref["terminated"] != 0
        idle = (~term & (team != (i & 1))) if alternate else np.zeros(n, bool)
        live = ~term & ~idle
        call = script[r, pos]
        for lg in (l1[i], l2[i]):
            lg[:] = rng.standard_normal((n, 38)).astype(np.float32)
            lg[r, call] = lg.max(1) + np.float32(0.5)
        mask = ref["legal_action_mask"].astype(bool)
        assert mask[r, call][live].all()                     # the script is a legal auction
        if alternate:
            used = l1[i] if (i & 1) == 0 else l2[i]
        else:
            used = np.where((team == 0)[:, None], l1[i], l2[i])
        act = np.where(mask, used, -np.inf).argmax(1).astype(np.int32)        # masked_pi.mode()
        assert np.array_equal(act[live], call[live])
        for bid_set in (0, 1):
            logs[bid_set].update(np.where(live, 0, 1), ref["current_player"], ref["legal_action_mask"], used, act, bid_set=bid_set)
        x = used.astype(np.float64)
        e = np.exp(x - x.max(1, keepdims=True))
        step_mass = ((e / e.sum(1, keepdims=True)) * ~mask).sum(1)
        mass[r[live], team[live]] += step_mass[live]
        # (test_scripted_matrix_statistics' bound: 1e-6 + 1e-5 * mass per step, 2**-24 of the running sum per addition)
        bound[r[live], team[live]] += 1e-6 + 1e-5 * step_mass[live] + 2.0 ** -24 * mass[r[live], team[live]]
        pos[live] += 1
        a = np.where(idle, 0, act).astype(np.int32)
        given[i], actions[i], waits[i] = a, np.where(idle, -1, act), idle
        keep = (ref[idle].copy(), oA[idle].copy(), oB[idle].copy())
        before, a_was = ref.copy(), oA["terminated"] != 0
        if dup:
            oracle.duplicate_step(ref, a, oA, oB)
        else:
            oracle.step(ref, a)
        ref[idle], oA[idle], oB[idle] = keep
        cum[~idle] += ref["rewards"][~idle, 0]
        rsum[~idle] += ref["rewards"][~idle]
        ended = (oA["terminated"] != 0) & ~a_was
        if dup and ended.any():        # table A's final state: the table before the launch, stepped by its call without the re-deal
            sub = before[ended]
            oracle.step(sub, a[ended])
            final_a[ended], a_taken[ended] = sub, True
    p = {"ref": ref, "tables0": tables0, "tables": (oA, oB), "logs": logs, "mass": mass, "bound": bound, "cum": cum, "rsum": rsum,
         "l1": l1, "l2": l2, "given": given, "actions": actions, "waits": waits, "final_a": final_a, "a_taken": a_taken}
    _PLANS[key] = p
    return p


def _step_outputs(mem, n, tag=""):
    """brl_step's optional outputs at what the header states: obs at 8, rewards at 16, mask / terminated at 1, current_player at 4"""
    return {"obs": mem.out(f"obs{tag}", (n, 480), U8, 8), "mask": mem.out(f"mask{tag}", (n, 38), U8, 1),
            "rewards": mem.out(f"rewards{tag}", (n, 4), F32, 16), "terminated": mem.out(f"terminated{tag}", (n,), U8, 1),
            "current_player": mem.out(f"current_player{tag}", (n,), I32, 4)}


def _assert_tables(g, plan, n):
    for t, want in zip("ab", plan["tables"]):
        for name, _, _ in TABLE_MEMBERS:
            got = g[f"table_{t}.{name}"].cpu().numpy()
            assert np.array_equal(got.astype(np.float64), want[name].astype(np.float64)), (t, name)


@pytest.mark.parametrize("n", [1, 3, 33])
def test_duplicate_step_guarded(env, oracle, n):
    """Eight launches of brl_duplicate_step on the scripted boards: table A ends on every board, table B on the boards that pass
    it out.  States ping-pong between two arrays at exactly 8 bytes, both brl_table_info blocks are updated in place with every
    member a placement of its own (rewards at 16), every launch's optional outputs are placements of their own; a second run of
    the same launches with every optional output NULL ends in the same state and tables.  Every launch's outputs, the final
    state and the tables against the oracle's duplicate step."""
    L, check = _lib()
    seed, K = 300 + n, 8
    plan = _plan(oracle, n, seed, True, False, K)
    state0 = env.init(seed, num_envs=n).packed.cpu()
    assert plan["tables"][0]["terminated"].all() and (n < 3 or (plan["tables"][1]["terminated"][0] and plan["cum"][2] != 0))
    assert n < 3 or not plan["tables"][1]["terminated"][1]

    def run(mem):
        out = {}
        act = mem.inp("action", plan["given"], I32, 4)
        for tag, with_outputs in (("", True), ("_bare", False)):
            bufs = [mem.inp("state" + tag, state0, I64, 8, inout=True), mem.out("state_other" + tag, (n, 16), I64, 8)]
            (pa, va), (pb, vb) = (_place_table(mem, f"table_{t}{tag}", plan["tables0"][j]) for j, t in enumerate("ab"))
            for i in range(K):
                o = _step_outputs(mem, n, f"[{i}]") if with_outputs else dict.fromkeys(("obs", "mask", "rewards", "terminated", "current_player"))
                check(L.brl_duplicate_step(env._h, _p(bufs[i & 1]), _p(bufs[(i & 1) ^ 1]), n, _p(act[i]), C.byref(pa), C.byref(pb),
                                           _p(o["obs"]), _p(o["mask"]), _p(o["rewards"]), _p(o["terminated"]), _p(o["current_player"]), _s()))
                if with_outputs:
                    out.update({f"{k}[{i}]": v for k, v in o.items()})
            out["state" + tag] = bufs[K & 1]
            out.update({f"table_{t}{tag}.{k}": v for t, vs in (("a", va), ("b", vb)) for k, v in vs.items()})
        return out
    _, g, _ = both(run, capacity=1 << 23)
    assert torch.equal(g["state"], g["state_bare"])
    for t in "ab":
        for name, _, _ in TABLE_MEMBERS:
            assert torch.equal(g[f"table_{t}.{name}"], g[f"table_{t}_bare.{name}"]), name
    _assert_tables(g, plan, n)
    # every launch's outputs: the oracle, replayed launch by launch
    from oracle import Oracle
    ref = oracle.init_random(n, seed=seed)
    oA, oB = Oracle.table_info_from(ref), Oracle.table_info_from(ref)
    for i in range(K):
        oracle.duplicate_step(ref, plan["given"][i], oA, oB)
        for name, field in (("obs", "observation"), ("mask", "legal_action_mask"), ("rewards", "rewards"), ("terminated", "terminated"),
                            ("current_player", "current_player")):
            assert np.array_equal(g[f"{name}[{i}]"].cpu().numpy().astype(np.float64), ref[field].astype(np.float64)), (name, i)
    from brl_amd.bridge_bidding import State
    assert_state_equal(State(env, g["state"].contiguous().clone()), ref, where="after the eight launches")


EVAL_VARIANTS = [     # (stats: every member / the struct NULL / bid_count NULL, bid_set, accumulators, step outputs, obs_f32)
    ("all", 0, True, True, True), (None, 1, False, True, False), ("no_bid_count", 1, True, False, True), ("all", 1, True, True, False)]


@pytest.mark.parametrize("duplicate", [True, False], ids=["duplicate", "single-table"])
@pytest.mark.parametrize("team_form", [False, True], ids=["brl_eval_step", "brl_eval_step_team"])
@pytest.mark.parametrize("n", [1, 3, 33])
def test_eval_step_guarded(env, oracle, n, team_form, duplicate):
    """The evaluators' step, updating its state in place (as the evaluators call it): logits of team 1 at row stride 38 and of
    team 2 at 40 with NaN in columns 38 and 39 (brl_eval_step_team: the acting team's array, acting_team alternating); every
    brl_table_info and brl_eval_stats member a placement of its own; stats NULL, its bid_count NULL, all given; bid_set 0 and 1
    on counters that start at 2; cum_return / rewards_sum (one 16-byte piece per board: at 16) / action_out given and NULL; the
    step outputs given and NULL; obs_f32 at exactly 16 and NULL; with the tables and without (env.step).  Tables, statistics,
    accumulators and the last launch's outputs against the oracle, its StepLog and float64; boards that wait keep the bits of
    their state, statistics and accumulators and report the call -1."""
    from brl_amd import _capi
    from brl_amd.bridge_bidding import State
    L, check = _lib()
    seed, K = 500 + n, 11 if team_form else 8
    plan = _plan(oracle, n, seed, duplicate, team_form, K)
    state0 = env.init(seed, num_envs=n).packed.cpu()
    if n >= 3:
        assert plan["ref"]["terminated"][0] and (not team_form or plan["waits"].any())
    for stats_kind, bid_set, with_acc, with_outputs, with_f32 in EVAL_VARIANTS:
        trace = {}

        def run(mem):
            st = mem.inp("state", state0, I64, 8, inout=True)
            l1 = mem.inp("logits1", plan["l1"], F32, 4)
            l2 = mem.inp("logits2", plan["l2"], F32, 4, ld=40, plain_ld=40)
            out, tabs = {"state": st}, (None, None)
            if duplicate:
                (pa, va), (pb, vb) = (_place_table(mem, f"table_{t}", plan["tables0"][j]) for j, t in enumerate("ab"))
                tabs = (C.byref(pa), C.byref(pb))
                out.update({f"table_{t}.{k}": v for t, vs in (("a", va), ("b", vb)) for k, v in vs.items()})
            ps = None
            if stats_kind is not None:
                ps = _capi.EvalStatsPtrs()
                for name, dt, tail, fill in (("illegal_prob_sum", F32, (2,), 0), ("step_count", I32, (2,), 0), ("pass_count", I32, (2,), 0),
                                             ("bid_count", I32, (2, 35), 2)):
                    if name == "bid_count" and stats_kind == "no_bid_count":
                        continue
                    out[name] = mem.inp(name, torch.full((n,) + tail, fill), dt, 4, inout=True)
                    setattr(ps, name, out[name].data_ptr())
            if with_acc:
                out["cum_return"] = mem.inp("cum_return", torch.zeros(n), F32, 4, inout=True)
                out["rewards_sum"] = mem.inp("rewards_sum", torch.zeros(n, 4), F32, 16, inout=True)
                out["action_out"] = mem.out("action_out", (n,), I32, 4)
                if mem.arena is not None:       # (x + 0.0f stores x's own bits: an update of table n would not show on the pattern)
                    mem.arena.signalling_margins(out["cum_return"])
                    mem.arena.signalling_margins(out["rewards_sum"])
            if with_outputs:
                out.update(_step_outputs(mem, n))
            if with_f32 and team_form:
                out["obs_f32"] = mem.out("obs_f32", (n, 480), F32, 16)
            tail = [_p(out.get(k)) for k in ("cum_return", "rewards_sum", "action_out", "obs", "mask", "rewards", "terminated", "current_player")]
            snaps = trace.setdefault(type(mem).__name__, [])
            watched = [k for k in ("state", "illegal_prob_sum", "step_count", "pass_count", "bid_count", "cum_return", "rewards_sum") if k in out]
            snaps.append({k: _bits(out[k]).reshape(n, -1) for k in watched})
            for i in range(K):
                if team_form:
                    lg = (l1, l2)[i & 1]
                    check(L.brl_eval_step_team(env._h, _p(st), _p(st), n, _p(lg[i]), lg.stride(1), i & 1, *tabs,
                                               C.byref(ps) if ps is not None else None, bid_set, *tail, _p(out.get("obs_f32")), _s()))
                else:
                    check(L.brl_eval_step(env._h, _p(st), _p(st), n, _p(l1[i]), l1.stride(1), _p(l2[i]), l2.stride(1), *tabs,
                                          C.byref(ps) if ps is not None else None, bid_set, *tail, _s()))
                snaps.append({k: _bits(out[k]).reshape(n, -1) for k in watched})
                if "action_out" in out:
                    snaps[-1]["action_out"] = out["action_out"].cpu().clone()
            return out
        _, g, _ = both(run, capacity=1 << 22)
        ref, log = plan["ref"], plan["logs"][bid_set]
        assert_state_equal(State(env, g["state"].contiguous().clone()), ref, where=f"variant {stats_kind} {bid_set}")
        if duplicate:
            _assert_tables(g, plan, n)
        if stats_kind is not None:
            assert np.array_equal(g["step_count"].cpu().numpy(), log.step_count) and np.array_equal(g["pass_count"].cpu().numpy(), log.pass_count)
            err = np.abs(g["illegal_prob_sum"].cpu().double().numpy() - plan["mass"])
            assert (err <= plan["bound"] + 1e-30).all(), float(err.max())
        if stats_kind == "all":
            want = np.where(log.bid > 0, 1, 2) if bid_set else 2 + log.bid
            assert np.array_equal(g["bid_count"].cpu().numpy(), want)
        if with_acc:
            assert np.array_equal(g["cum_return"].cpu().numpy(), plan["cum"]) and np.array_equal(g["rewards_sum"].cpu().numpy(), plan["rsum"])
            assert np.array_equal(g["action_out"].cpu().numpy(), plan["actions"][K - 1])
        if with_outputs:
            for name, field in (("obs", "observation"), ("mask", "legal_action_mask"), ("terminated", "terminated"), ("current_player", "current_player")):
                assert np.array_equal(g[name].cpu().numpy().astype(np.int64), ref[field].astype(np.int64)), name
            if not team_form:     # (a waiting board's last step output is the launch's, not the board's last call's)
                assert np.array_equal(g["rewards"].cpu().numpy(), ref["rewards"])
        if "obs_f32" in g:
            assert torch.equal(g["obs_f32"].cpu(), torch.from_numpy(ref["observation"]).float())
        # boards that wait: the bits of their state, statistics and accumulators stay, the call is -1
        snaps = trace["Guarded"]
        for i in range(K):
            idle = torch.from_numpy(plan["waits"][i])
            for k, v in snaps[i + 1].items():
                if k == "action_out":
                    assert np.array_equal(v.numpy(), plan["actions"][i]), i
                else:
                    assert torch.equal(v[idle], snaps[i][k][idle]), (k, i)


@pytest.mark.parametrize("n", [1, 3, 65])
def test_board_keep_a_guarded(env, oracle, n):
    """brl_board_keep_a behind each of five alternating launches of the scripted match: state / prev / final_a at exactly 16 bytes,
    taken and a_done (table A's `terminated`) at 1, action — brl_eval_step_team's action_out, -1 where a board waited — at 4.
    The rows of final_a whose table A has not ended stay unwritten; the others hold table A's final state by the oracle (the
    table before the launch stepped by its call, without the re-deal) although the match goes on: no board is taken twice."""
    from brl_amd.bridge_bidding import State
    L, check = _lib()
    seed, K = 800 + n, 5
    plan = _plan(oracle, n, seed, True, True, K)
    state0 = env.init(seed, num_envs=n).packed.cpu()
    taken_rows = np.nonzero(plan["a_taken"])[0]
    assert len(taken_rows) > 0 and (n < 3 or len(taken_rows) < n) and (plan["actions"] == -1).any()
    idx = torch.from_numpy(taken_rows)

    def run(mem):
        st = mem.inp("state", state0, I64, 16, inout=True)
        prev = mem.inp("prev", state0, I64, 16, inout=True)
        final_a = mem.out("final_a", (n, 16), I64, 16)
        taken = mem.inp("taken", torch.zeros(n), U8, 1, inout=True)
        l1, l2 = mem.inp("logits1", plan["l1"], F32, 4), mem.inp("logits2", plan["l2"], F32, 4, ld=40, plain_ld=40)
        (pa, va), (pb, vb) = (_place_table(mem, f"table_{t}", plan["tables0"][j]) for j, t in enumerate("ab"))
        action = mem.out("action", (n,), I32, 4)
        for i in range(K):
            lg = (l1, l2)[i & 1]
            check(L.brl_eval_step_team(env._h, _p(st), _p(st), n, _p(lg[i]), lg.stride(1), i & 1, C.byref(pa), C.byref(pb), None, 0, None, None,
                                       _p(action), None, None, None, None, None, None, _s()))
            check(L.brl_board_keep_a(0, _p(st), _p(prev), _p(action), _p(va["terminated"]), _p(taken), _p(final_a), n, _s()))
        return {"state": st, "prev": prev, "taken": taken, "action": action, "final_a_taken": final_a[idx.to(final_a.device)]}
    _, g, gm = both(run, partial=("final_a",))
    assert torch.equal(g["state"], g["prev"]) and np.array_equal(g["taken"].cpu().numpy().astype(bool), plan["a_taken"])
    u = gm.arena.unwritten(gm.outs["final_a"])
    assert not u[plan["a_taken"]].any() and u[~plan["a_taken"]].all()
    fields = {"terminated", "rewards", "last_bid", "last_bidder", "call_x", "call_xx", "turn", "step_count", "pass_num", "hand", "dealer",
              "shuffled_players", "first_denomination_ns", "first_denomination_ew", "illegal"}
    assert_state_equal(State(env, g["final_a_taken"].contiguous().clone()), plan["final_a"][taken_rows], fields=fields, where="final_a")
    assert plan["final_a"]["terminated"][taken_rows].all()


# ---- brl_eval_reduce -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 257])
def test_eval_reduce_guarded(env, oracle, n):
    """tests/eval_counts_ref.py's skewed tables (257 boards: two blocks add into `out`): the tables read only, rewards at 16;
    bid_count — read as 8-byte pairs — at exactly 8, state at 8, out int64 [231] at 8 and exactly that long; table_b, bid_count
    and state each given and NULL.  Exact against the numpy restatement of the counters."""
    from tests.test_gpu_eval_stats import SEED, _stepped_states
    L, check = _lib()
    A, B = er.synthetic_table(n, SEED, 0), er.synthetic_table(n, SEED, 1)
    bc = er.synthetic_bid_count(n, SEED)
    packed, steps = _stepped_states(env, oracle, n, 5 + n)
    packed = packed.cpu()
    for two, with_bids, with_state in ((True, True, True), (False, True, True), (True, False, True), (True, True, False), (False, False, False)):
        def run(mem):
            pa, va = _place_table(mem, "table_a", A, inout=False)          # (va, vb: the structs hold addresses only)
            pb, vb = _place_table(mem, "table_b", B, inout=False) if two else (None, None)
            b = mem.inp("bid_count", bc, I32, 8) if with_bids else None
            s = mem.inp("state", packed, I64, 8) if with_state else None
            out = mem.out("out", (er.EV_TOTAL,), I64, 8)
            check(L.brl_eval_reduce(env._h, n, C.byref(pa), C.byref(pb) if two else None, _p(b), _p(s), _p(out), _s()))
            torch.cuda.synchronize()
            return {"out": out}
        _, g, _ = both(run)
        want = er.eval_counts_ref(A, B if two else None, bc if with_bids else None, steps if with_state else None)
        assert np.array_equal(g["out"].cpu().numpy(), want), (two, with_bids, with_state)


# ---- brl_league_route, brl_xplay_route -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["league", "xplay"])
@pytest.mark.parametrize("nmatch,n", [(1, 1), (3, 5), (4, 65)])
def test_routes_guarded(kind, nmatch, n):
    """Both routes, ngroups 1 and 3 (the networks 0 and 2: group 1 owns no board), team 0 and 1: terminated at exactly 1 byte,
    the int32 arrays at 4, rows at 8; work exactly as long as the header says (2 per slot: every entry is written), group_first
    exactly ngroups + 1; the entries of rows from R on keep their placed bytes.  Against the numpy restatements of
    tests/test_league_host.py and tests/crossplay_ref.py."""
    from brl_amd.crossplay import lineup_order
    from brl_amd.league import team_order
    L, check = _lib()
    nslots = nmatch * (2 if kind == "xplay" else 1)
    for ngroups in (1, 3):
        for team in (0, 1):
            rng = np.random.default_rng(1000 * nmatch + 10 * ngroups + team)
            term = (rng.random(nmatch * n) < 0.4).astype(np.uint8)
            cur = rng.integers(0, 4, nmatch * n).astype(np.int32)
            term[0], cur[0] = 0, 2 * team + 1                    # at least one board acts
            if kind == "league":
                pairs = np.zeros((nmatch, 2), np.int64) if ngroups == 1 else 2 * rng.integers(0, 2, (nmatch, 2))
                order, _, _ = team_order(pairs, team)
                groups = pairs[order, team].astype(np.int32)
                want_rows, want_gf = route_numpy(term, cur, pairs, team, n, num_groups=ngroups)
            else:
                lineups = np.zeros((nmatch, 4), np.int64) if ngroups == 1 else 2 * rng.integers(0, 2, (nmatch, 4))
                order, group_of, nets = lineup_order(lineups, team)
                groups = nets[group_of].astype(np.int32)
                want_rows, want_gf = xroute_numpy(term, cur, team, n, order, groups, ngroups)
            R_ = int(want_gf[-1])
            assert R_ > 0 and (ngroups == 1 or want_gf[1] == want_gf[2])

            def run(mem):
                t, c = mem.inp("terminated", term, U8, 1), mem.inp("current_player", cur, I32, 4)
                o, gof = mem.inp("order", order, I32, 4), mem.inp("group_of", groups, I32, 4)
                work, rows = mem.out("work", (2 * nslots,), I32, 4), mem.out("rows", (nmatch * n,), I64, 8)
                gf = mem.out("group_first", (ngroups + 1,), I32, 4)
                fn = L.brl_league_route if kind == "league" else L.brl_xplay_route
                check(fn(0, _p(t), _p(c), team, n, _p(o), _p(gof), nmatch, ngroups, _p(work), _p(rows), _p(gf), _s()))
                return {"rows": rows[:R_], "group_first": gf, "work": work}
            _, g, gm = both(run, partial=("rows",))
            assert np.array_equal(g["group_first"].cpu().numpy(), want_gf) and np.array_equal(g["rows"].cpu().numpy(), want_rows)
            u = gm.arena.unwritten(gm.outs["rows"])
            assert not u[:R_].any() and u[R_:].all(), (ngroups, team)
            assert int(g["work"][:nslots].sum()) == R_


# ---- brl_league_forward --------------------------------------------------------------------------------------------------------
def _raw(gen, hidden, nlayers, act):
    dims = [480] + [hidden] * nlayers
    body = [(torch.randn((dims[i + 1], dims[i]), generator=gen) / dims[i] ** 0.5, torch.randn(dims[i + 1], generator=gen) * 0.1)
            for i in range(nlayers)]
    actor = (torch.randn((38, hidden), generator=gen) / hidden ** 0.5, torch.randn(38, generator=gen) * 0.1)
    critic = (torch.randn((1, hidden), generator=gen) / hidden ** 0.5, torch.randn(1, generator=gen) * 0.1)
    return raw_net(body, actor, critic, torch.relu if act == 0 else torch.tanh)


def _forward_rows_dense(net, nlayers, hidden, act, obs, rows, nboards):
    """brl_mlp_forward_rows of one network on dense tensors -> [nboards, 39] (the rows not chosen stay 0)"""
    from brl_amd import _capi
    L, check = _lib()
    r, keep = _capi.MlpRef(), []
    r.nlayers, r.act, r.in_features, r.hidden = nlayers, act, 480, hidden

    def dev(t):
        keep.append(t.to(DEV).contiguous())
        return keep[-1].data_ptr()
    for i, l in enumerate(net.body):
        r.w[i], r.b[i] = dev(l.weight), dev(l.bias)
    r.actor_w, r.actor_b, r.critic_w, r.critic_b = dev(net.actor.weight), dev(net.actor.bias), dev(net.critic.weight), dev(net.critic.bias)
    m = len(rows)
    scratch = torch.empty(m * (480 + 2 * hidden), dtype=F32, device=DEV)
    out = torch.zeros((nboards, 39), dtype=F32, device=DEV)
    check(L.brl_mlp_forward_rows(0, C.byref(r), dev(obs), dev(rows), m, _p(scratch), scratch.numel(), _p(out), 39, _s()))
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("hidden,nlayers,ldo,act", [(64, 1, 40, 0), (64, 3, 44, 1), (260, 1, 44, 1), (260, 3, 40, 0)])
def test_league_forward_guarded(hidden, nlayers, ldo, act):
    """Two networks, the second with a single row: every weight, hidden bias and head weight of every brl_league_net at exactly
    16 bytes, head biases at 4, the records themselves at 8, obs (4-byte pieces) at 4, rows at 8, scratch at 16 and exactly
    rmax * (480 + 2 hidden) floats, for rmax = R and R + 64; out [9, 39] with row pitch 40 / 44: the rows that are not routed
    and the columns >= 39 stay unwritten.  Bit for bit brl_mlp_forward_rows of each network on its rows, and within
    test_mlp_forward_rows_matches_float64's bound of the float64 forward."""
    L, check = _lib()
    nboards, sizes = 9, (4, 1)
    gen = torch.Generator().manual_seed(hidden + nlayers)
    nets = [_raw(gen, hidden, nlayers, act) for _ in sizes]
    obs = observations(nboards, 3).to(U8)
    rows = torch.tensor([7, 2, 8, 0, 4], dtype=I64)
    group_first = torch.tensor([0, 4, 5], dtype=I32)
    R_ = int(group_first[-1])
    want = torch.zeros((nboards, 39))
    for k, net in enumerate(nets):
        rk = rows[int(group_first[k]):int(group_first[k + 1])]
        want[rk] = _forward_rows_dense(net, nlayers, hidden, act, obs, rk, nboards)[rk]
    for rmax in (R_, R_ + 64):
        def run(mem):
            table, keep = torch.zeros((len(nets), 20), dtype=I64), []      # (keep: the records hold addresses only)

            def param(name, values, align):
                keep.append(mem.inp(name, values, F32, align))
                return keep[-1].data_ptr()
            for k, net in enumerate(nets):
                for i, l in enumerate(net.body):
                    table[k, i], table[k, 8 + i] = param(f"net{k}.w{i}", l.weight, 16), param(f"net{k}.b{i}", l.bias, 16)
                table[k, 16], table[k, 17] = param(f"net{k}.actor_w", net.actor.weight, 16), param(f"net{k}.actor_b", net.actor.bias, 4)
                table[k, 18], table[k, 19] = param(f"net{k}.critic_w", net.critic.weight, 16), param(f"net{k}.critic_b", net.critic.bias, 4)
            recs = mem.inp("nets", table, I64, 8)
            ob, rw, gf = mem.inp("obs", obs, U8, 4), mem.inp("rows", rows, I64, 8), mem.inp("group_first", group_first, I32, 4)
            scratch = mem.out("scratch", (rmax * (480 + 2 * hidden),), F32, 16)
            out = mem.out("out", (nboards, 39), F32, 4, ld=ldo, plain_ld=ldo)
            check(L.brl_league_forward(0, _p(recs), len(nets), nlayers, hidden, act, _p(ob), _p(rw), _p(gf), rmax, _p(scratch), scratch.numel(),
                                       _p(out), out.stride(0), _s()))
            torch.cuda.synchronize()
            return {"out": out[rows.to(out.device)]}
        _, g, gm = both(run, capacity=1 << 23, partial=("out", "scratch"))
        u = gm.arena.unwritten(gm.outs["out"])
        chosen = np.zeros(nboards, bool)
        chosen[rows.numpy()] = True
        assert not u[chosen].any() and u[~chosen].all(), rmax
        assert torch.equal(_bits(g["out"]), _bits(want[rows])), rmax
        for k, net in enumerate(nets):
            rk = rows[int(group_first[k]):int(group_first[k + 1])]
            w64 = forward64(net, obs[rk].float())
            got = g["out"].cpu().double()[int(group_first[k]):int(group_first[k + 1])]
            assert float((got - w64).abs().max()) < 2e-4 * max(1.0, float(w64[:, :38].abs().max()))


# ---- brl_board_records, brl_board_imp ------------------------------------------------------------------------------------------
def _board_tables(n, seed):
    """n packed tables by tests/board_records_ref.py's encoder: the 319-call auction, a pass-out, live auctions, finished
    contracts and (the last of three or more) a table ended by an illegal double; every dealer, vulnerability and a seating and
    four disjoint hands of their own"""
    rng = np.random.default_rng(seed)
    perms = np.array([[0, 1, 2, 3], [1, 0, 3, 2], [2, 3, 0, 1], [3, 2, 1, 0]])
    out = np.zeros((n, 16), np.uint64)
    for i in range(n):
        if i == 0:
            calls = R.longest_auction()
        elif i % 5 == 1:
            calls = [0, 0, 0, 0]
        else:
            calls = R.random_auction(rng, stop=None if i % 3 else int(rng.integers(0, 25)), p_pass=float(rng.uniform(0.05, 0.6)))
        if n >= 3 and i == n - 1:
            while True:
                calls = R.random_auction(rng, stop=int(rng.integers(1, 12)))
                t = R.encode(0, calls)
                if not t.term:
                    break
            calls = calls + [[a for a in (1, 2) if not t.legal(a)][0]]
        owner = rng.permutation(np.repeat(np.arange(4), 13))
        hands = [sum(1 << int(b) for b in np.nonzero(owner == s)[0]) for s in range(4)]
        out[i] = R.encode(i & 3, calls, vul_ns=(i >> 2) & 1, vul_ew=(i >> 3) & 1, seating=[int(p) for p in perms[(i >> 4) & 3]],
                          tricks=rng.integers(0, 14, (4, 5)), hands=hands).pack()
    return out


@pytest.mark.parametrize("n", [1, 3, 65, 130])
def test_board_records_and_imp_guarded(oracle, n):
    """brl_board_records: state at exactly 8 bytes, records at exactly 16 and exactly n * 368 bytes (65 and 130 tables: a
    second and a third workgroup, the last one ragged); the bytes of tests/board_records_ref.py's decoder.  brl_board_imp on
    those records and on the records of the same tables in reverse order: records at 16, out_imp at 4; against oracle.imp_reward."""
    from brl_amd import boards
    L, check = _lib()
    tables = _board_tables(n, 60 + n)
    want = R.decode(tables)
    assert want["n_calls"].max() == 319 and (n < 3 or (want["flags"][n - 1] & boards.ILLEGAL and want["flags"][1] & boards.PASSED_OUT))
    assert n < 65 or ((want["score_ns"] != 0).sum() > 8 and (~(want["flags"] & boards.TERMINATED).astype(bool)).sum() > 8)
    rec_a = np.frombuffer(want.tobytes(), np.uint8).reshape(n, 368).copy()
    rec_b = rec_a[::-1].copy()

    def run(mem):
        st = mem.inp("state", torch.from_numpy(tables.view(np.int64)), I64, 8)
        rec = mem.out("records", (n, 46), I64, 16)      # (as 8-byte words: a record's fill bytes are 0xFF, an unwritten byte's too)
        check(L.brl_board_records(0, _p(st), n, _p(rec), _s()))
        ra, rb = mem.inp("records_a", rec_a, U8, 16), mem.inp("records_b", rec_b, U8, 16)
        imp = mem.out("out_imp", (n,), I32, 4)
        check(L.brl_board_imp(0, _p(ra), _p(rb), n, _p(imp), _s()))
        return {"records": rec, "out_imp": imp}
    _, g, _ = both(run)
    assert g["records"].cpu().numpy().tobytes() == want.tobytes()
    sa, sb = want["score_ns"].astype(np.float32), want["score_ns"][::-1].astype(np.float32)
    sign = np.array([1, 1, -1, -1], np.float32)
    imp = np.array([oracle.imp_reward(sa[i] * sign, -sb[i] * sign)[0] for i in range(n)])
    assert np.array_equal(g["out_imp"].cpu().numpy(), imp.astype(np.int32)) and (n < 65 or (imp != 0).any())


# ---- a pointer off the stated alignment: BRL_E_ARG before anything is launched ---------------------------------------------------
def test_misaligned_pointers_are_refused_on_the_host(env, oracle):
    """Every alignment the kernels above rely on beyond an array's element type is stated in the header and checked by the
    entry point: a pointer 4 bytes off it (8 for the 16-byte table rows of brl_board_keep_a, 2 for the 4-byte observation rows
    of brl_league_forward) is answered with BRL_E_ARG on the host — nothing is launched, so no array changes —, and the same
    call with the pointer in place succeeds afterwards."""
    from brl_amd import _capi
    L, check = _lib()
    n = 3
    st = env.init(5, num_envs=n)
    state = st.packed.clone()
    scratch_state = torch.empty_like(state)

    def z(shape, dt, fill=0):      # one float / int32 more than the shape: the shifted pointer's array stays inside the tensor
        return torch.full((int(np.prod(shape)) + 4,), fill, dtype=dt, device=DEV)

    def table():
        t = {"terminated": z((n,), U8), "rewards": z((n, 4), F32), "last_bid": z((n,), I32, -1), "last_bidder": z((n,), I32, -1),
             "call_x": z((n,), U8), "call_xx": z((n,), U8)}
        return t

    def ptrs(t, **shift):
        p = _capi.TableInfoPtrs()
        for name in t:
            setattr(p, name, t[name].data_ptr() + shift.get(name, 0))
        return p

    ta, tb = table(), table()
    action, rewards, rsum, cum = z((n,), I32), z((n, 4), F32), z((n, 4), F32), z((n,), F32)
    logits = torch.zeros((n, 40), dtype=F32, device=DEV)
    bid_count, counts = z((n, 70), I32), z((231,), I64)
    imp_a, imp_out = z((n, 4), F32), z((n, 4), F32)
    prev, final_a, taken = state.clone(), torch.zeros((n + 1, 16), dtype=I64, device=DEV), z((n,), U8)
    obs = torch.zeros((n + 1, 480), dtype=U8, device=DEV)
    fields_rewards = z((n, 4), F32)
    everything = [state, scratch_state, action, rewards, rsum, cum, bid_count, counts, imp_a, imp_out, prev, final_a, taken, fields_rewards,
                  *ta.values(), *tb.values()]
    h, s = env._h, _s()

    def dup_step(rew=0, tab=0):
        pa, pb = ptrs(ta, rewards=tab), ptrs(tb)
        return L.brl_duplicate_step(h, _p(state), _p(scratch_state), n, _p(action), C.byref(pa), C.byref(pb), None, None,
                                    rewards.data_ptr() + rew, None, None, s)

    def eval_step(rew=0, tab=0, acc=0, team=False):
        pa, pb = ptrs(ta), ptrs(tb, rewards=tab)
        tail = (C.byref(pa), C.byref(pb), None, 0, _p(cum), rsum.data_ptr() + acc, None, None, None, rewards.data_ptr() + rew, None, None)
        if team:
            return L.brl_eval_step_team(h, _p(state), _p(scratch_state), n, _p(logits), 40, 0, *tail, None, s)
        return L.brl_eval_step(h, _p(state), _p(scratch_state), n, _p(logits), 40, _p(logits), 40, *tail, s)

    def reduce(bc=0, tab=0):
        pa = ptrs(ta, rewards=tab)
        return L.brl_eval_reduce(h, n, C.byref(pa), None, bid_count.data_ptr() + bc, _p(state), _p(counts), s)

    def fields(off=0):
        f = _capi.Fields()
        f.rewards = fields_rewards.data_ptr() + off
        return L.brl_get_fields(h, _p(state), n, C.byref(f), s)

    def keep_a(which=None, off=0):
        a = {"state": state.data_ptr(), "prev": prev.data_ptr(), "final_a": final_a.data_ptr()}
        if which:
            a[which] += off
        return L.brl_board_keep_a(0, a["state"], a["prev"], _p(action), _p(ta["terminated"]), _p(taken), a["final_a"], n, s)

    def league_forward(off=0):
        # (refused before the records of `nets` are looked at: any device array stands in for them)
        gf = torch.zeros(2, dtype=I32, device=DEV)
        sc = torch.empty(1 * (480 + 2 * 64), dtype=F32, device=DEV)
        return L.brl_league_forward(0, _p(counts), 1, 1, 64, 0, obs.data_ptr() + off, _p(counts), _p(gf), 1, _p(sc), sc.numel(), _p(imp_out), 40, s)

    cases = {
        "brl_imp_reward: out": lambda: L.brl_imp_reward(h, _p(imp_a), _p(imp_a), imp_out.data_ptr() + 4, n, s),
        "brl_get_fields: rewards": lambda: fields(4),
        "brl_duplicate_step: rewards": lambda: dup_step(rew=4),
        "brl_duplicate_step: table_a.rewards": lambda: dup_step(tab=4),
        "brl_eval_step: rewards": lambda: eval_step(rew=4),
        "brl_eval_step: table_b.rewards": lambda: eval_step(tab=4),
        "brl_eval_step: rewards_sum": lambda: eval_step(acc=4),
        "brl_eval_step_team: rewards": lambda: eval_step(rew=4, team=True),
        "brl_eval_step_team: table_b.rewards": lambda: eval_step(tab=4, team=True),
        "brl_eval_step_team: rewards_sum": lambda: eval_step(acc=4, team=True),
        "brl_eval_reduce: bid_count": lambda: reduce(bc=4),
        "brl_eval_reduce: table_a.rewards": lambda: reduce(tab=4),
        "brl_board_keep_a: state": lambda: keep_a("state", 8),
        "brl_board_keep_a: prev": lambda: keep_a("prev", 8),
        "brl_board_keep_a: final_a": lambda: keep_a("final_a", 8),
        "brl_league_forward: obs": lambda: league_forward(2),
    }
    torch.cuda.synchronize()
    before = [t.clone() for t in everything]
    for name, call in cases.items():
        assert call() == BRL_E_ARG, name
        assert b"aligned" in L.brl_last_error(), name
    torch.cuda.synchronize()
    for t, b in zip(everything, before):
        assert torch.equal(t, b)
    # the same calls with every pointer in place
    check(L.brl_imp_reward(h, _p(imp_a), _p(imp_a), _p(imp_out), n, s))
    check(fields())
    check(dup_step())
    check(eval_step())
    check(eval_step(team=True))
    check(reduce())
    check(keep_a())
    torch.cuda.synchronize()
    assert torch.equal(fields_rewards[:4 * n], torch.zeros(4 * n, device=DEV)) and int(counts[:231].sum()) >= 0
    assert torch.equal(prev, state) and not bool(taken.any())
