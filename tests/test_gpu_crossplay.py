"""-m gpu: cross-play (brl_amd/crossplay.py, csrc/brl_crossplay.hip, include/brl_crossplay.h) — the route against its numpy
restatement (tests/crossplay_ref.py), the league's case bit for bit, whole line-ups replayed through the CPU oracle with every
call checked against the network of the PLAYER who made it, the loop method, the board records and ``cross_play`` with its
command line."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.crossplay_ref import decisions_of, replay_lineup, seating_byte, xroute_numpy
from tests.gpu_util import to_np

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE_FIELDS = ("terminated", "rewards", "last_bid", "last_bidder", "call_x", "call_xx")


@pytest.fixture(scope="module")
def env(dds):
    import brl_amd
    return brl_amd.BridgeBidding(lut=(dds["keys"], dds["values"]))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _xroute(term, cur, team, n, order, group_of, nmatch, ngroups):
    from brl_amd import _capi
    rows = torch.full((nmatch * n,), -7, dtype=torch.int64, device="cuda")
    gf = torch.full((ngroups + 1,), -7, dtype=torch.int32, device="cuda")
    work = torch.empty(4 * nmatch, dtype=torch.int32, device="cuda")
    t, c, o, g = _dev(term), _dev(cur), _dev(np.asarray(order, np.int32)), _dev(np.asarray(group_of, np.int32))
    _capi.check(_capi.lib().brl_xplay_route(0, t.data_ptr(), c.data_ptr(), team, n, o.data_ptr(), g.data_ptr(), nmatch, ngroups,
                                            work.data_ptr(), rows.data_ptr(), gf.data_ptr(), _capi.stream()))
    torch.cuda.synchronize()
    return to_np(rows), to_np(gf)


def _league_route(term, cur, order, group_of, team, n, nmatch, ngroups):
    from brl_amd import _capi
    rows = torch.full((nmatch * n,), -7, dtype=torch.int64, device="cuda")
    gf = torch.full((ngroups + 1,), -7, dtype=torch.int32, device="cuda")
    work = torch.empty(2 * nmatch, dtype=torch.int32, device="cuda")
    t, c, o, g = _dev(term), _dev(cur), _dev(np.asarray(order, np.int32)), _dev(np.asarray(group_of, np.int32))
    _capi.check(_capi.lib().brl_league_route(0, t.data_ptr(), c.data_ptr(), team, n, o.data_ptr(), g.data_ptr(), nmatch, ngroups,
                                             work.data_ptr(), rows.data_ptr(), gf.data_ptr(), _capi.stream()))
    torch.cuda.synchronize()
    return to_np(rows), to_np(gf)


def _slot_boards(term, cur, team, n, slot):
    """the boards that act in slot 2 * match + half"""
    b = np.arange((slot >> 1) * n, ((slot >> 1) + 1) * n)
    return b[(term[b] == 0) & ((cur[b] >> 1) == team) & ((cur[b] & 1) == (slot & 1))]


@pytest.mark.parametrize("nmatch,n", [(1, 1), (1, 63), (3, 64), (3, 65), (10, 200), (600, 3)])
@pytest.mark.parametrize("team", [0, 1])
def test_route_equals_the_numpy_restatement(nmatch, n, team):
    """rows[:R] and group_first exactly, rows[R:] untouched; group id = network id with two groups that no slot names.  Cases: random
    boards; nothing acts (every board finished: R = 0); and, where the batch has three matches, a crafted one — line-up 0 seats one
    network on both halves (a match whose two players share a group), the second position of the order is emptied between two
    non-empty ones, and every board of the last position's network is finished (a named group without an acting board).
    600 matches are 1200 slots: two positions per thread of the scan."""
    from brl_amd.crossplay import lineup_order
    rng = np.random.default_rng(1000 * nmatch + 10 * n + team)
    M = 7 if nmatch == 600 else 5
    lineups = rng.integers(0, M, (nmatch, 4))
    lineups[0] = (2, 2, 2, 2)
    if nmatch >= 3:
        lineups[1], lineups[2] = (0, 1, 0, 1), (4, 0, 4, 0)
    order, group_of, nets = lineup_order(lineups, team)
    groups = nets[group_of]                                              # group id = network id: still non-decreasing
    G = M + 2
    if nmatch == 600:                                                    # groups change inside a thread's two positions and at their end
        assert {0, 1} == set(((np.nonzero(np.diff(groups))[0] + 1) % 2).tolist())
    for case in ("random", "nothing acts", "crafted"):
        term = (rng.random(nmatch * n) < 0.4).astype(np.uint8)
        cur = rng.integers(0, 4, nmatch * n).astype(np.int32)
        if case == "nothing acts":
            term[:] = 1
        if case == "crafted":
            if nmatch < 3:
                continue
            for k in (0, 2):                                             # positions 0 and 2 of the order: at least one acting board each
                b = (order[k] >> 1) * n + (3 + k) % n
                term[b], cur[b] = 0, 2 * team + (order[k] & 1)
            term[_slot_boards(term, cur, team, n, order[1])] = 1         # ... and none in position 1, between them
            dead = groups[-1]
            assert dead != groups[0] and dead != groups[2]
            for k in np.nonzero(groups == dead)[0]:
                term[_slot_boards(term, cur, team, n, order[k])] = 1
            sizes = [len(_slot_boards(term, cur, team, n, s)) for s in order]
            assert sizes[0] > 0 and sizes[1] == 0 and sizes[2] > 0 and sizes[-1] == 0
            k0, k1 = int(np.nonzero(order == 0)[0][0]), int(np.nonzero(order == 1)[0][0])
            assert k1 == k0 + 1 and groups[k0] == groups[k1] == 2                         # line-up 0: both halves in one group
        want_rows, want_gf = xroute_numpy(term, cur, team, n, order, groups, G)
        rows, gf = _xroute(term, cur, team, n, order, groups, nmatch, G)
        R = int(want_gf[-1])
        assert R == int(((term == 0) & ((cur >> 1) == team)).sum()) and (R == 0 if case == "nothing acts" else R > 0 or n == 1)
        assert np.array_equal(gf, want_gf), case
        assert np.array_equal(rows[:R], want_rows) and (rows[R:] == -7).all(), case
        if case == "crafted":
            assert gf[dead + 1] == gf[dead] and gf[M + 1] == gf[M] == gf[M + 2] == R


@pytest.mark.parametrize("team", [0, 1])
def test_route_of_shared_partners_gives_the_leagues_row_sets(team):
    """line-ups (i, i, j, j): the slots (2m, 2m + 1) are adjacent and in one group, so group_first is brl_league_route's for the
    pairs (i, j) and every group holds the same boards (inside a match the league orders them by board, the cross-play route
    by half first)"""
    from brl_amd.crossplay import lineup_order
    from brl_amd.league import team_order
    rng = np.random.default_rng(7 + team)
    P, n, M = 7, 130, 4
    pairs = rng.integers(0, M, (P, 2))
    lineups = np.stack([pairs[:, 0], pairs[:, 0], pairs[:, 1], pairs[:, 1]], axis=1)
    term = (rng.random(P * n) < 0.3).astype(np.uint8)
    cur = rng.integers(0, 4, P * n).astype(np.int32)
    order, group_of, nets = lineup_order(lineups, team)
    lorder, lgroup_of, lnets = team_order(pairs, team)
    assert np.array_equal(order, np.stack([2 * lorder, 2 * lorder + 1], axis=1).reshape(-1)) and np.array_equal(nets, lnets)
    rows, gf = _xroute(term, cur, team, n, order, nets[group_of], P, M)
    lrows, lgf = _league_route(term, cur, lorder, lnets[lgroup_of], team, n, P, M)
    assert np.array_equal(gf, lgf) and gf[-1] > 0
    different_order = False
    for g in range(M):
        a, b = rows[gf[g]:gf[g + 1]], lrows[gf[g]:gf[g + 1]]
        assert np.array_equal(np.sort(a), np.sort(b))
        different_order |= not np.array_equal(a, b)
    assert different_order


def _nets(fp, seeds):
    from tests.nets import perturbed
    return [perturbed(fp.init(s, device="cuda"), 1000 + s) for s in seeds]


def test_shared_partners_play_the_leagues_matches_bit_for_bit(env):
    from brl_amd.crossplay import make_lineup_evaluate
    from brl_amd.league import all_pairs, make_league_evaluate
    from brl_amd.models import make_forward_pass
    fp = make_forward_pass("relu", "DeepMind")
    nets = _nets(fp, [3, 4, 5])
    n = 65
    pairs = all_pairs(3)
    lineups = [(i, i, j, j) for i, j in pairs]
    league = make_league_evaluate(env, "relu", "DeepMind", n, method="batched")
    want = [t.clone() for t in league(nets, pairs, 21)]
    assert league.last_method == "batched" and bool(want[3].any())
    for max_boards, nbatches in ((65536, 1), (n, 3)):
        record = {}
        ev = make_lineup_evaluate(env, "relu", "DeepMind", n, max_boards=max_boards, record=record)
        got = ev(nets, lineups, 21)
        torch.cuda.synchronize()
        assert ev.last_method == "batched" and len(record["batches"]) == nbatches and len(got) == 4
        for a, b in zip(got, want):
            assert a.shape == b.shape and torch.equal(a, b)


def _rows_forward(fp, net, obs):
    """brl_mlp_forward_rows of `net` on [m, 480] bool observations -> [m, 38] logits"""
    from brl_amd.evaluation import _Forward
    fwd = _Forward(fp, net)
    assert fwd.ref is not None
    m = obs.shape[0]
    out = torch.zeros((m, 40), dtype=torch.float32, device="cuda")
    fwd.rows(_dev(obs), torch.arange(m, dtype=torch.int64, device="cuda"), m, out, None)
    torch.cuda.synchronize()
    return to_np(out)[:, :38]


def _unpack(batch, P, n):
    actions = np.stack([to_np(a) for a in batch["action"]]).reshape(len(batch["action"]), P, n)
    logits = np.stack([to_np(x)[:, :38] for x in batch["logits"]]).reshape(len(batch["logits"]), P, n, 38)
    return actions, logits


def _tables_equal(batch, sl, oA, oB):
    for T, oT in ((batch["table_a"], oA), (batch["table_b"], oB)):
        for f in TABLE_FIELDS:
            assert np.array_equal(to_np(getattr(T, f))[sl].astype(np.float64), oT[f].astype(np.float64)), f


@pytest.fixture(scope="module")
def three_nets():
    """x = the bidder (tests/bidder_net.py), y and o = random-init networks with perturbed biases"""
    from brl_amd.models import make_forward_pass
    from tests.bidder_net import bidder
    fp = make_forward_pass("relu", "DeepMind")
    return fp, [bidder(1, device="cuda")] + _nets(fp, [4, 5])


def test_calls_come_from_the_players_network(env, oracle, three_nets):
    """Line-up (x, y, o, o) beside (x, x, o, o) on the same 100 boards, one batch.  First the test proves that it can see a route
    by team: on at least one board the two line-ups' auctions part, and where they part first the caller is player 1 (the only
    seat whose network differs).  Then line-up (x, y, o, o) replays through the CPU oracle, and every call of player k is the
    masked arg-max of brl_mlp_forward_rows of network lineup[k] on the oracle's observation — whose logits are, bit for bit,
    the ones the batched forward wrote for that board."""
    from brl_amd.crossplay import make_lineup_evaluate
    fp, nets = three_nets
    n, seed = 100, 99
    lineups = np.array([(0, 1, 2, 2), (0, 0, 2, 2)])
    record = {"logits": True}
    ev = make_lineup_evaluate(env, "relu", "DeepMind", n, record=record)
    imp, se, win, cum = ev(nets, lineups, seed)
    torch.cuda.synchronize()
    assert ev.last_method == "batched" and len(record["batches"]) == 1 and cum.shape == (2, n)
    batch = record["batches"][0]
    actions, logits = _unpack(batch, 2, n)
    want, oA, oB, steps = replay_lineup(oracle, n, seed, actions[:, 0], logits[:, 0])
    # -- the mistake is visible
    differ = actions[:, 0] != actions[:, 1]
    boards = np.nonzero(differ.any(axis=0))[0]
    assert len(boards) > 0, "the bidder and a random-init network never call differently: the inputs are wrong"
    first = differ[:, boards].argmax(axis=0)
    assert all(steps[i]["live"][b] and steps[i]["player"][b] == 1 for i, b in zip(first, boards))
    print(f"auctions of (x, y, o, o) and (x, x, o, o) part on {len(boards)} of {n} boards, always at a call of player 1")
    # -- every call is its player's network's
    for k in range(4):
        it, bd, obs, legal, call = decisions_of(steps, actions[:, 0], k)
        assert len(it) > n // 2
        own = _rows_forward(fp, nets[lineups[0][k]], obs)
        assert np.array_equal(np.where(legal, own, -np.inf).argmax(1), call), f"player {k}"
        assert np.array_equal(logits[it, 0, bd], own), f"player {k}: the routed rows' logits"
    _tables_equal(batch, slice(0, n), oA, oB)
    assert np.array_equal(to_np(cum[0]), want)
    assert abs(float(imp[0]) - want.mean()) < 1e-5 and abs(float(se[0]) - want.std(ddof=1) / np.sqrt(n)) < 1e-5
    assert abs(float(win[0]) - (want > 0).mean()) < 1e-6
    # ... and the league's line-up beside it replays too
    want1, oA1, oB1, _ = replay_lineup(oracle, n, seed, actions[:, 1], logits[:, 1])
    _tables_equal(batch, slice(n, 2 * n), oA1, oB1)
    assert np.array_equal(to_np(cum[1]), want1)


def test_loop_method_replays_through_the_oracle(env, oracle, three_nets):
    """The loop's own recorded logits replay (each call their masked arg-max).  They come from full-batch forwards, so they are
    not brl_mlp_forward_rows' bits: same law.  Each path is held to 2e-4 * max(1, max|logits|) of the float64
    forward by its own tests, so the logits a board was given lie within twice that of brl_mlp_forward_rows of the network of
    the player who called — and far from another network's."""
    from brl_amd.crossplay import make_lineup_evaluate
    fp, nets = three_nets
    n, seed = 100, 99
    lineup = (0, 1, 2, 2)
    record = {"logits": True}
    ev = make_lineup_evaluate(env, "relu", "DeepMind", n, method="loop", record=record)
    imp, se, win, cum = ev(nets, [lineup], seed)
    torch.cuda.synchronize()
    assert ev.last_method == "loop" and len(record["batches"]) == 1 and record["batches"][0]["matches"] == (0, 1)
    batch = record["batches"][0]
    actions, logits = _unpack(batch, 1, n)
    want, oA, oB, steps = replay_lineup(oracle, n, seed, actions[:, 0], logits[:, 0])
    _tables_equal(batch, slice(0, n), oA, oB)
    assert np.array_equal(to_np(cum[0]), want) and abs(float(imp[0]) - want.mean()) < 1e-5
    for k in range(4):
        it, bd, obs, legal, call = decisions_of(steps, actions[:, 0], k)
        own = _rows_forward(fp, nets[lineup[k]], obs).astype(np.float64)
        other = _rows_forward(fp, nets[lineup[k ^ 1] if k < 2 else 0], obs).astype(np.float64)
        got = logits[it, 0, bd].astype(np.float64)
        tol = 4e-4 * max(1.0, float(np.abs(own).max()))
        err = float(np.abs(got - own).max())
        print(f"player {k}: max |loop logits - forward_rows| = {err:.3g} (bound {tol:.3g}), to the other network {float(np.abs(got - other).max()):.3g}")
        assert err < tol
        assert float(np.abs(got - other).max()) > 100 * tol


def test_loop_method_plays_fair_networks(env, oracle):
    from brl_amd.crossplay import make_lineup_evaluate
    from brl_amd.models import make_forward_pass
    fair = make_forward_pass("relu", "FAIR")
    nets = [fair.init(s, device="cuda") for s in (1, 2, 3)]
    n, seed = 64, 12
    record = {"logits": True}
    ev = make_lineup_evaluate(env, "relu", "FAIR", n, method="loop", record=record)
    imp, se, win, cum = ev(nets, [(0, 1, 2, 2)], seed)
    torch.cuda.synchronize()
    assert ev.last_method == "loop" and cum.shape == (1, n)
    batch = record["batches"][0]
    actions, logits = _unpack(batch, 1, n)
    want, oA, oB, _ = replay_lineup(oracle, n, seed, actions[:, 0], logits[:, 0])
    _tables_equal(batch, slice(0, n), oA, oB)
    assert np.array_equal(to_np(cum[0]), want)
    # asked for "batched", a FAIR line-up runs as the loop all the same
    ev = make_lineup_evaluate(env, "relu", "FAIR", n)
    out = ev(nets, np.zeros((0, 4), np.int64), seed)
    assert ev.last_method == "loop" and out[3].shape == (0, n)


@pytest.mark.parametrize("method", ["batched", "loop"])
def test_board_records_of_every_lineup(env, oracle, method):
    """boards=True: per line-up and board the records' calls are the recorded actions in order (table A's, then table B's, then
    the finished board's no-op steps), the seating bytes are the tables', the IMP of the records is cum_return (player 0's: the
    sign by where player 0 sits at table A, as test_gpu_boards.py) and every record carries BRL_BOARD_OK."""
    from brl_amd import boards
    from brl_amd.crossplay import make_lineup_evaluate
    from brl_amd.models import make_forward_pass
    fp = make_forward_pass("relu", "DeepMind")
    nets = _nets(fp, [3, 4, 5])
    n, seed = 65, 5
    lineups = [(0, 1, 2, 2), (1, 0, 2, 1)]
    record = {}
    ev = make_lineup_evaluate(env, "relu", "DeepMind", n, method=method, record=record, boards=True)
    imp, se, win, cum, records = ev(nets, lineups, seed)
    torch.cuda.synchronize()
    assert ev.last_method == method and len(records) == 2
    seat_a = seating_byte(oracle.init_random(n, seed=seed)["shuffled_players"])
    for p, recs in enumerate(records):
        b = record["batches"][0 if method == "batched" else p]
        P = 2 if method == "batched" else 1
        actions = np.stack([to_np(a) for a in b["action"]]).reshape(len(b["action"]), P, n)[:, p if method == "batched" else 0]
        ra, rb = recs.cpu("a"), recs.cpu("b")
        assert len(recs) == n and ((ra["flags"] & boards.OK) != 0).all() and ((rb["flags"] & boards.OK) != 0).all()
        assert np.array_equal(ra["seating"], seat_a)
        assert np.array_equal(rb["seating"], ((seat_a >> 2) & 0x33) | ((seat_a & 0x33) << 2))      # seats [1, 0, 3, 2]
        for i in range(n):
            seq = actions[:, i][actions[:, i] >= 0]
            na, nb = int(ra["n_calls"][i]), int(rb["n_calls"][i])
            assert na >= 4 and nb >= 4 and len(seq) >= na + nb
            assert np.array_equal(ra["calls"][i, :na], seq[:na]) and np.array_equal(rb["calls"][i, :nb], seq[na:na + nb])
        rec_imp = to_np(boards.board_imp(recs.table_a.contiguous(), recs.table_b.contiguous()))
        assert np.array_equal(rec_imp, to_np(recs.imp))
        sign = np.where((ra["seating"] & 3) < 2, 1, -1)
        assert np.array_equal(rec_imp * sign, to_np(cum[p]).astype(np.int64))
        assert np.array_equal(to_np(recs.cum_return), to_np(cum[p])) and recs.dda.shape == (n, 20)
    assert bool(cum.any())


def test_cross_play_and_its_command_line(env, tmp_path, dds):
    from brl_amd import checkpoint
    from brl_amd.crossplay import CrossPlay, cross_play
    from brl_amd.league import make_league_evaluate
    from brl_amd.models import make_forward_pass
    fp = make_forward_pass("relu", "DeepMind")
    nets = _nets(fp, [3, 4, 5])
    n = 64
    cp = cross_play(nets[:2], nets[2], env, "relu", "DeepMind", n, rng_key=8)
    assert isinstance(cp, CrossPlay) and cp.last_method == "batched" and cp.n == n
    for a in (cp.imp, cp.se, cp.sym, cp.gap, cp.gap_se):
        assert a.shape == (2, 2) and a.dtype == np.float64 and np.isfinite(a).all()
    assert (np.diag(cp.gap) == 0.0).all() and (np.diag(cp.gap_se) == 0.0).all() and cp.gap[0, 1] == cp.gap[1, 0]
    league = make_league_evaluate(env, "relu", "DeepMind", n)(nets, [(0, 2), (1, 2)], 8)
    torch.cuda.synchronize()
    for x in range(2):
        assert cp.imp[x, x] == float(league[0][x])          # (IMPs are integers: the float32 mean is exact whatever the order)
        assert abs(cp.se[x, x] - float(league[1][x])) <= 1e-6 * float(league[1][x])
        assert np.array_equal(cp.cum_return[x, x], to_np(league[3][x]).astype(np.float64))
    assert np.abs(cp.cum_return).max() > 0
    # the command line, as a child process
    run = tmp_path / "models" / "run"
    run.mkdir(parents=True)
    for k in range(3):
        checkpoint.save_params(fp.init(30 + k), str(run / f"params-{100 * k:08}.pt"))
    checkpoint.save_params(fp.init(40), str(run / "params-00000150.pt"))     # (filtered out: not a multiple of skip_interval)
    opp = tmp_path / "opp.pt"
    checkpoint.save_params(fp.init(41), str(opp))
    lut = tmp_path / "lut.npy"
    np.save(lut, np.stack([dds["keys"], dds["values"]]))
    envv = dict(os.environ, PYTHONPATH=ROOT)
    args = [sys.executable, "-m", "brl_amd.crossplay", f"models_directory={tmp_path / 'models'}", "exp_name=run", f"opp_model_path={opp}",
            "num_eval_envs=64", f"dds_path={lut}", f"save_path={tmp_path / 'cp.json'}"]
    r = subprocess.run(args, cwd=tmp_path, env=envv, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    m = np.load(tmp_path / "cross_play_run.npy")
    assert m.shape == (4, 3, 3) and (np.diag(m[2]) == 0.0).all() and "±" in r.stdout and (tmp_path / "cp.json").exists()
    r = subprocess.run(args + ["shard=1"], cwd=tmp_path, env=envv, capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "unknown option shard" in r.stderr
