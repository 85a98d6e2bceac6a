"""-m gpu: the full duplicate-score table through every scoring path of the device.

Random play ends practically every auction at the 7 level, down (100 000 boards of uniformly random legal calls: 1, 1, 1, 2, 18, 129
and 99 848 contracts at levels 1 .. 7; an 8192 x 32 rollout reaches 230 of the 1978 distinct (strain, level, doubling, |score|)
outcomes), so "bit-exact against the oracle under random play" says little about ``contract_score``.  Here every one of the 2940
outcome cells is declared from every seat through three auction shapes (tests/contract_matrix.py: 35 284 scripted tables) and
played through ``brl_step``, the policy sub-step, the evaluators' step, ``brl_duplicate_step``, the board records with their
IMPs, and — one pass from the end — the three fused random rollouts.  The expectation is ``law_score`` (the Laws as tables), computed
from the case description alone; everything is integers and every comparison is exact."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import contract_matrix as cm
from tests.gpu_util import assert_state_equal, make_env, to_np

pytestmark = pytest.mark.gpu
SCALE = np.float32(cm.REWARD_SCALE)


@pytest.fixture(scope="module")
def m(dds, oracle):
    return cm.matrix(dds, oracle)


def _init(env, m, rows=None):
    sl = slice(None) if rows is None else rows
    return env.init_from_deals(m.hand[sl], m.dealer[sl], m.vul_ns[sl], m.vul_ew[sl], m.shuffled[sl], m.tricks[sl])


def _one_hot(act, width=38):
    """logits whose arg-max over any legal set that holds ``act`` is ``act``"""
    lg = torch.zeros((act.shape[0], width), dtype=torch.float32, device=act.device)
    return lg.scatter_(1, act.to(torch.int64)[:, None], 1.0)


def _assert_rows(got, want, what):
    bad = np.nonzero((np.asarray(got) != np.asarray(want)).reshape(len(want), -1).any(1))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} tables differ, first {bad[:4]}: got {np.asarray(got)[bad[:4]]}, want {np.asarray(want)[bad[:4]]}"


@pytest.fixture(scope="module")
def stepped(dds, oracle, m):
    """the matrix through brl_step in lockstep, no auto-reset: max_len + 1 steps, a finished table is stepped on with passes"""
    env = make_env(dds, 4)
    first = _init(env, m)
    calls = torch.from_numpy(m.calls).to(env.device)
    st, rewards, term = first, [], []
    for k in range(m.max_len + 1):
        st = env.step(st, calls[:, k].contiguous() if k < m.max_len else torch.zeros(m.n, dtype=torch.int32, device=env.device))
        rewards.append(st.rewards)
        term.append(st.terminated)
    torch.cuda.synchronize()
    return {"env": env, "first": first, "final": st, "rewards": [to_np(r) for r in rewards], "terminated": [to_np(t) for t in term]}


def test_step_scores_every_contract(dds, oracle, m, stepped):
    """brl_step: the rewards by player id on the step that ends each table, zeros before it and on later steps of the finished
    table; terminated; brl_get_fields of the final state against the oracle's; the trick table reads back as given"""
    from brl_amd.bridge_bidding import State
    run = cm.oracle_lockstep(dds, oracle)
    env = stepped["env"]
    assert np.array_equal(to_np(stepped["first"]._dds_tricks), m.tricks)
    assert_state_equal(State(env, stepped["first"].packed), run["first"], where="the scripted boards as dealt")
    for k in range(m.max_len + 1):
        _assert_rows(stepped["rewards"][k], cm.expected_step_rewards(m, k), f"rewards of step {k}")
        assert np.array_equal(stepped["terminated"][k] != 0, m.length - 1 <= k), k
    final = State(env, stepped["final"].packed)      # (no cached step outputs: every field through brl_get_fields)
    assert np.array_equal(to_np(final._dds_tricks), m.tricks)
    assert_state_equal(final, run["state"], where="final state of the matrix")


@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_policy_step_scores_every_contract(dds, oracle, m, stepped, k):
    """brl_policy_step_ex in arg-max mode on one-hot logits that force the scripted call, K tables per wave: the reward column
    (the acting player's reward / reward_scale, fp32) and rewards_acc step by step, and a final packed state identical to brl_step's"""
    from brl_amd import _capi
    from brl_amd.utils import MODE, policy_step
    env = make_env(dds, k)
    dev, n = env.device, m.n
    st = _init(env, m)
    packed = st.packed
    calls = torch.from_numpy(m.calls).to(dev)
    actor = st.current_player.clone()
    cur = torch.empty_like(actor)
    action = torch.empty(n, dtype=torch.int32, device=dev)
    got = []
    for s in range(m.max_len + 1):
        act = calls[:, s] if s < m.max_len else torch.zeros(n, dtype=torch.int32, device=dev)
        racc = torch.full((n, 4), 99.0, device=dev)
        tacc = torch.full((n,), 1, dtype=torch.uint8, device=dev)
        reward = torch.full((n,), -9.0, device=dev)
        done = torch.full((n,), 7, dtype=torch.uint8, device=dev)
        ext = _capi.MacroExt(first=1, last=1, done_out=done.data_ptr(), reward_out=reward.data_ptr(), actor=actor.data_ptr(),
                             reward_scale=float(cm.REWARD_SCALE))
        policy_step(env, packed, packed, _one_hot(act), MODE, 0, False, action=action, rewards_acc=racc, terminated_acc=tacc,
                    current_player=cur, ext=ext)
        got.append((action.clone(), racc, reward, done, actor.clone()))
        actor.copy_(cur)
    torch.cuda.synchronize()
    for s, (action, racc, reward, done, actor) in enumerate(got):
        live = m.length > s
        want_actor = m.shuffled[np.arange(n), (m.dealer + s) % 4]
        assert np.array_equal(to_np(actor)[live], want_actor[live]), s
        want_act = m.calls[:, s] if s < m.max_len else np.zeros(n, np.int32)
        assert np.array_equal(to_np(action)[live], want_act[live]), s
        want = cm.expected_step_rewards(m, s)
        _assert_rows(to_np(racc), want, f"K={k} rewards_acc of step {s}")
        # the acting player's reward of the step, divided in fp32 as the launch divides it
        _assert_rows(to_np(reward), want[np.arange(n), to_np(actor)] / SCALE, f"K={k} reward column of step {s}")
        # (done_out is the macro-step's flag: rewards_acc's sibling, set on the step that ends the table; a finished table's
        # no-op steps keep reporting terminated, as env.step does)
        assert np.array_equal(to_np(done) != 0, m.length - 1 <= s), s
    assert torch.equal(packed, stepped["final"].packed), "final packed state differs from brl_step's"


@pytest.fixture(scope="module")
def paired(dds, oracle, m):
    """both tables of every board through brl_duplicate_step in lockstep: table A plays case i, table B the direct auction of case
    i + 1471 on the same board with the seats swapped"""
    import brl_amd
    env = make_env(dds, 4)
    st = _init(env, m)
    A, B = brl_amd.Table_info.from_state(st), brl_amd.Table_info.from_state(st)
    step_fn = brl_amd.duplicate_step(env.step)
    calls = torch.from_numpy(m.pair_calls).to(env.device)
    returns = torch.zeros((m.n, 4), device=env.device)
    for k in range(m.pair_max + 1):
        act = calls[:, k].contiguous() if k < m.pair_max else torch.zeros(m.n, dtype=torch.int32, device=env.device)
        st, A, B = step_fn(st, act, A, B)
        returns += st.rewards
    torch.cuda.synchronize()
    return {"env": env, "state": st, "A": A, "B": B, "returns": to_np(returns)}


def test_duplicate_step_scores_both_tables_and_the_imps(dds, oracle, m, paired):
    from brl_amd.bridge_bidding import State
    run = cm.oracle_pairs(dds, oracle)
    for name, T, oT, want in (("A", paired["A"], run["A"], m.rewards), ("B", paired["B"], run["B"], m.b_rewards)):
        _assert_rows(to_np(T.rewards), want, f"table {name} rewards")
        for f in ("terminated", "rewards", "last_bid", "last_bidder", "call_x", "call_xx"):
            assert np.array_equal(to_np(getattr(T, f)).astype(np.float64), oT[f].astype(np.float64)), (name, f)
    _assert_rows(paired["returns"], m.imp_rewards, "IMPs by player id, summed over the steps")
    assert_state_equal(State(paired["env"], paired["state"].packed), run["state"], where="state after both tables")


def _check_records(rec, m, length, calls, passout, level, strain, doubling, declarer, taken, score_ns, what):
    from brl_amd import boards
    assert ((rec["flags"] & boards.OK) != 0).all() and ((rec["flags"] & boards.TERMINATED) != 0).all(), what
    assert ((rec["flags"] & boards.ILLEGAL) == 0).all() and np.array_equal((rec["flags"] & boards.PASSED_OUT) != 0, passout != 0), what
    assert np.array_equal(rec["n_calls"], length), what
    for i in range(0, m.n, 97):
        assert rec["calls"][i, :length[i]].tolist() == list(calls[i]), (what, i)
    play = passout == 0
    for name, want in (("level", level), ("strain", strain), ("doubled", doubling), ("declarer", declarer), ("tricks", taken),
                       ("score_ns", score_ns)):
        _assert_rows(rec[name][play].astype(np.int64), want[play].astype(np.int64), f"{what}: {name}")
        assert (rec[name][~play] == 0).all(), (what, name)
    assert np.array_equal(rec["dealer"], m.dealer) and np.array_equal(rec["vul_ns"], m.vul_ns) and np.array_equal(rec["vul_ew"], m.vul_ew)


def test_board_records_and_imps_of_every_contract(dds, oracle, m, stepped, paired):
    """brl_board_records of the final states of table A (case i) and table B, and brl_board_imp of the pairs"""
    from brl_amd import boards
    rec_a, rec_b = boards.board_records(stepped["final"].packed), boards.board_records(paired["state"].packed)
    imp = boards.board_imp(rec_a, rec_b)
    torch.cuda.synchronize()
    ra = rec_a.cpu().numpy().view(boards.RECORD_DTYPE).reshape(-1)
    rb = rec_b.cpu().numpy().view(boards.RECORD_DTYPE).reshape(-1)
    _check_records(ra, m, m.length, [m.calls[i, :m.length[i]] for i in range(m.n)], m.passout, m.level, m.strain, m.doubling,
                   m.declarer, m.taken, m.score_ns, "table A")
    _check_records(rb, m, m.b_length, [m.pair_calls[i, m.length[i]:m.pair_length[i]] for i in range(m.n)], m.b_passout, m.b_level,
                   m.b_strain, m.b_doubling, m.b_declarer, m.b_taken, m.b_score_ns, "table B")
    assert [(int(ra["seating"][5]) >> (2 * s)) & 3 for s in range(4)] == m.shuffled[5].tolist()
    assert [(int(rb["seating"][5]) >> (2 * s)) & 3 for s in range(4)] == m.b_shuffled[5].tolist()
    _assert_rows(imp.cpu().numpy(), m.imp_ns, "brl_board_imp")
    assert len(set(m.imp_ns)) == 49


def test_eval_step_team_scores_every_contract(dds, oracle, m):
    """brl_eval_step_team (the evaluators' step: one team's network per launch, the teams alternating) with both Table_info given,
    on logits that force the scripted calls of table A and then of table B: the Table_info rewards of both tables, the summed
    rewards and player 0's return"""
    import brl_amd
    from brl_amd import _capi
    from brl_amd.bridge_bidding import _stream
    env = make_env(dds, 4)
    L, dev, n = _capi.lib(), env.device, m.n
    st = _init(env, m)
    packed = st.packed
    A, B = brl_amd.Table_info.from_state(st), brl_amd.Table_info.from_state(st)
    pa, pb = A._ptrs(), B._ptrs()
    calls = torch.from_numpy(np.concatenate([m.pair_calls, np.zeros((n, 1), np.int32)], axis=1)).to(dev).to(torch.int64)
    length = torch.from_numpy(m.pair_length).to(dev).to(torch.int64)
    pos = torch.zeros(n, dtype=torch.int64, device=dev)
    cum = torch.zeros(n, device=dev)
    rsum = torch.zeros((n, 4), device=dev)
    action = torch.empty(n, dtype=torch.int32, device=dev)
    obs = torch.empty((n, 480), dtype=torch.bool, device=dev)
    term = torch.zeros(n, dtype=torch.bool, device=dev)
    wrong = torch.zeros((), dtype=torch.int64, device=dev)
    launches = 0
    while launches < m.pair_max + 8 and not (launches % 4 == 0 and bool(term.all())):
        act = calls.gather(1, pos.clamp(max=m.pair_max)[:, None])[:, 0]
        lg = _one_hot(act, 39)
        _capi.check(L.brl_eval_step_team(env._h, packed.data_ptr(), packed.data_ptr(), n, lg.data_ptr(), 39, launches & 1, C.byref(pa),
                                         C.byref(pb), None, 0, cum.data_ptr(), rsum.data_ptr(), action.data_ptr(), obs.data_ptr(), None,
                                         None, term.data_ptr(), None, None, _stream()))
        made = (action >= 0) & (pos < length)       # (a board whose team is not acting waits: -1; a finished one is stepped on)
        wrong += (made & (action.to(torch.int64) != act)).sum()
        pos += made.to(torch.int64)
        launches += 1
    torch.cuda.synchronize()
    assert bool(term.all()) and bool((pos == length).all()) and int(wrong) == 0, launches
    _assert_rows(to_np(A.rewards), m.rewards, "table A rewards")
    _assert_rows(to_np(B.rewards), m.b_rewards, "table B rewards")
    run = cm.oracle_pairs(dds, oracle)
    for T, oT in ((A, run["A"]), (B, run["B"])):
        for f in ("terminated", "last_bid", "last_bidder", "call_x", "call_xx"):
            assert np.array_equal(to_np(getattr(T, f)).astype(np.int64), oT[f].astype(np.int64)), f
    _assert_rows(to_np(rsum), m.imp_rewards, "rewards_sum")
    _assert_rows(to_np(cum), m.imp_rewards[:, 0], "cum_return")


@pytest.mark.parametrize("kernel", ["flag-synchronised", "barrier", "with-gae"])
def test_fused_random_rollouts_score_every_cell(dds, oracle, m, kernel):
    """brl_rollout_random (ws=None: the flag-synchronised k_rollout_fs; "ws": its barrier sibling k_rollout_ws) and
    brl_rollout_random_gae at T = 2 on 65 536 slots.  Their scorer takes the tricks of the board a table CAME IN WITH from the
    packed image, which random play checks at level 7 only.  So every one of the 2940 cells is handed in one pass from its end —
    explicit-deal tables (lut_idx -1), which all three kernels accept — in a slot whose first action draw is that pass; the other
    slots hold init_random tables.  Every Transition column, last_obs and the final state against oracle.rollout_random, and the
    step-0 reward of every placed table against law_score."""
    import brl_amd
    from brl_amd.bridge_bidding import State
    p = cm.rollout_placement(dds, oracle)
    slots = p["slots"]
    assert (slots >= 0).all() and len(set(slots)) == cm.N_CELLS, cm.PLACEMENT_HINT     # every cell has its slot, before the launch
    env = make_env(dds, 4, "ws" if kernel == "barrier" else None)
    dev = env.device
    cells = np.arange(cm.N_CELLS)
    pre = _init(env, m, cells)
    for k in range(m.max_len):      # only the tables that still have a call before their last one are stepped
        live = np.nonzero(m.length[cells] - 1 > k)[0]
        if len(live) == 0:
            break
        idx = torch.from_numpy(live).to(dev)
        sub = env.step(State(env, pre.packed[idx].contiguous()), torch.from_numpy(np.ascontiguousarray(m.calls[live, k])).to(dev))
        pre.packed[idx] = sub.packed
    assert_state_equal(State(env, pre.packed), p["prefix"], where="the tables one pass from their end")
    st = env.init(cm.ROLLOUT_SEED, num_envs=cm.ROLLOUT_SLOTS)
    st.packed[torch.from_numpy(slots).to(dev)] = pre.packed
    T, n = cm.ROLLOUT_T, cm.ROLLOUT_SLOTS
    cfg = {"num_steps": T, "reward_scale": cm.REWARD_SCALE, "gamma": 0.99, "gae_lambda": 0.9}
    rs = (None, None, State(env, st.packed), None, 0, cm.ROLLOUT_DRAW_BASE)
    if kernel == "with-gae":
        rs, traj, adv, tgt = brl_amd.make_random_roll_out_with_gae(cfg, env)(rs)
    else:
        rs, traj = brl_amd.make_random_roll_out(cfg, env)(rs)
    torch.cuda.synchronize()
    want = p["want"]
    for name in ("obs", "legal_action_mask", "action", "done", "value", "reward", "log_prob"):
        g, o = to_np(getattr(traj, name)), want[name]
        assert g.shape == o.shape
        if not np.array_equal(g, o):
            bad = np.nonzero((g != o).reshape(T, n, -1).any(2))
            placed = np.isin(bad[1], slots)
            raise AssertionError(f"{kernel}: {name} differs at {len(bad[0])} (step, slot) pairs, {int(placed.sum())} of them placed tables; "
                                 f"first (step {bad[0][0]}, slot {bad[1][0]}): got {g[bad[0][0], bad[1][0]]}, want {o[bad[0][0], bad[1][0]]}")
    assert_state_equal(rs[2], p["final"], where=f"{kernel}: final state")
    assert np.array_equal(to_np(rs[3]), p["final"]["observation"])
    assert int(rs[4].item()) == want["terminated_count"] and rs[5] == cm.ROLLOUT_DRAW_BASE + T
    if kernel == "with-gae":
        wa, wt = oracle.gae(want["done"], want["value"], want["reward"], np.zeros(n, np.float32), 0.99, 0.9)
        assert np.array_equal(to_np(adv), wa) and np.array_equal(to_np(tgt), wt)
    # every cell ends in step 0, with the score the Laws give it, seen from the side of the player who made the last pass
    assert (to_np(traj.done)[0, slots] == 1).all() and (to_np(traj.action)[0, slots] == 0).all()
    score = (p["actor_sign"] * m.score[:cm.N_CELLS]).astype(np.float32)
    _assert_rows(to_np(traj.reward)[0, slots], score / SCALE, f"{kernel}: step-0 reward of the placed tables")
