"""CPU checks of the league evaluation's host side (brl_amd/league.py, include/brl_league.h): the binding's argument types, the
checkpoint filter, the three matrices, the batch plan, the per-team match orders, the CLI's parser, the trainer's default, the
matches' statistics (``_match_batch.per_match_stats``: sharded over fake ranks against numpy float64, plain against torch), and a
numpy restatement of the route (``route_numpy``: what tests/test_gpu_league.py compares the kernels with) on hand-made cases."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def route_numpy(terminated, current_player, pairs, team, n, num_groups=None):
    """(rows, group_first) of brl_league_route with one group per NETWORK (group id = network id, ``num_groups`` of them): the
    boards b with terminated[b] == 0 and current_player[b] >> 1 == team, grouped by pairs[b // n][team]; within a group by the
    position of the board's match in the stable order of the matches sorted by that network, then by board index."""
    from brl_amd.league import team_order
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    M = int(pairs.max()) + 1 if num_groups is None else num_groups
    terminated, current_player = np.asarray(terminated), np.asarray(current_player)
    order, _, _ = team_order(pairs, team)
    rows, sizes = [], np.zeros(M, np.int64)
    for m in order:
        b = np.arange(m * n, (m + 1) * n)
        act = b[(terminated[b] == 0) & ((current_player[b] >> 1) == team)]
        rows.extend(act.tolist())
        sizes[pairs[m, team]] += len(act)
    return np.array(rows, np.int64), np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def test_league_header_matches_the_binding():
    from brl_amd import _capi
    from brl_amd import build
    build.build()
    text = open(os.path.join(ROOT, "include", "brl_league.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert _capi.lib().brl_version() == 6      # (the prototypes against the argtypes: tests/test_capi_cpu.py, every header)
    # the record of the header: 8 + 8 + 4 pointers, as the binding's structure
    body = re.search(r"typedef struct brl_league_net \{(.*?)\} brl_league_net;", text, flags=re.S).group(1)
    assert len(re.findall(r"\*", body)) == 6 and ctypes.sizeof(_capi.LeagueNet) == 20 * 8


def test_checkpoint_filter_and_order(tmp_path):
    from brl_amd.league import select_checkpoints
    names = ["params-00000300.pt", "params-00000100.pt", "params-00000200.pkl", "params-00000150.pt", "params-00010100.pt",
             "params-00010000.pt", "opt_state-00000100.pt", "params-00000400.pt.tmp", "config.json", "params-00000000.pt"]
    for nm in names:
        (tmp_path / nm).write_bytes(b"")
    got = select_checkpoints(os.listdir(tmp_path), 100, 10000)
    assert got == ["params-00000000.pt", "params-00000100.pt", "params-00000200.pkl", "params-00000300.pt", "params-00010000.pt"]
    assert select_checkpoints(os.listdir(tmp_path), 50, 200) == ["params-00000000.pt", "params-00000100.pt", "params-00000150.pt",
                                                                  "params-00000200.pkl"]


def test_the_three_matrices():
    from brl_amd.league import all_pairs, league_matrices
    M = 5
    pairs = all_pairs(M)
    assert len(pairs) == 10 and all(i < j for i, j in pairs)
    imp = np.array([0.5, -2.25, 0.0, 3.0, -0.125, 1.0, -1.0, 7.5, 0.75, -4.0])
    win_lose, clip, dis = league_matrices(imp, pairs, M)
    for m in (win_lose, clip, dis):
        assert m.shape == (M, M) and np.array_equal(m, -m.T) and not np.diag(m).any()
    for v, (i, j) in zip(imp, pairs):
        assert win_lose[i][j] == -v and win_lose[j][i] == v
        assert clip[j][i] == min(1.0, max(-1.0, v))
        assert dis[j][i] == (1 if v > 0 else -1 if v < 0 else 0)
    assert np.abs(clip).max() == 1.0 and set(np.unique(dis)) == {-1.0, 0.0, 1.0}


@pytest.mark.parametrize("P,n,max_boards", [(10, 100, 65536), (4950, 100, 65536), (45, 100, 1500), (3, 1000, 1000), (7, 37, 80)])
def test_batch_plan_covers_every_pair_once(P, n, max_boards):
    from brl_amd.league import batch_plan
    plan = batch_plan(P, n, max_boards)
    assert [m for a, b in plan for m in range(a, b)] == list(range(P))
    assert all(0 < (b - a) * n <= max_boards for a, b in plan)
    assert len(plan) == -(-P // (max_boards // n))
    with pytest.raises(ValueError):
        batch_plan(P, n, n - 1)


def test_team_orders_are_sorted_permutations():
    from brl_amd.league import all_pairs, team_order
    rng = np.random.default_rng(0)
    for pairs in (all_pairs(7), rng.integers(0, 9, (40, 2)), np.array([[3, 3]]), np.array([[0, k] for k in range(1, 6)])):
        for team in (0, 1):
            order, group_of, nets = team_order(pairs, team)
            assert sorted(order.tolist()) == list(range(len(pairs)))
            played = np.asarray(pairs)[order, team]
            assert (np.diff(played) >= 0).all() and np.array_equal(nets[group_of], played)
            assert (np.diff(nets) > 0).all() and group_of[0] == 0 and group_of[-1] == len(nets) - 1
            same = np.diff(played) == 0                      # stable: equal networks keep the matches' own order
            assert (np.diff(order)[same] > 0).all()
            assert order.dtype == np.int32 and group_of.dtype == np.int32


def test_parse_rejects_an_unknown_key():
    from brl_amd.eval import EVAL_DEFAULTS
    from brl_amd.league import LEAGUE_DEFAULTS, parse
    cfg = parse(["exp_name=run7", "num_eval_envs=64", "max_boards=640"])
    assert cfg == dict(LEAGUE_DEFAULTS, exp_name="run7", num_eval_envs=64, max_boards=640)
    assert {k: LEAGUE_DEFAULTS[k] for k in ("models_directory", "exp_name", "num_eval_envs", "skip_interval", "max_step",
                                            "save_fig_directory_path", "activation", "model_type")} == dict(
        models_directory="models", exp_name="pretrained-rl-with-sp", num_eval_envs=100, skip_interval=100, max_step=10000,
        save_fig_directory_path="", activation="relu", model_type="DeepMind")
    with pytest.raises(SystemExit):
        parse(["num_envs=3"])
    with pytest.raises(SystemExit):
        parse(["models_directory=x"], EVAL_DEFAULTS)
    assert parse(["team1_model_path=a.pt", "team2_model_type=FAIR"], EVAL_DEFAULTS) == dict(
        EVAL_DEFAULTS, team1_model_path="a.pt", team2_model_type="FAIR")


def test_train_default_keeps_the_loop():
    from brl_amd.train import DEFAULTS, parse_cli
    assert DEFAULTS["league_eval"] == "loop"
    assert parse_cli(["league_eval=batched"])["league_eval"] == "batched"


class _FakeRank:
    """the two members of evaluation._Shard that per_match_stats uses.  ``stacks`` None: ``allsum`` hands this rank's stack back
    (to collect it); a list of every rank's stack: ``allsum`` is their plain Python sum"""
    active = True

    def __init__(self, stacks=None):
        self.stacks, self.own = stacks, None

    def allsum(self, t):
        self.own = t
        return t if self.stacks is None else sum(self.stacks)


@pytest.mark.parametrize("sizes", [(21, 20), (14, 14, 13), (40, 1), (1, 2, 38)])
def test_match_statistics_sharded_and_plain(sizes):
    """Integer-valued rows of odd length n = 41 over 2 and 3 ranks of unequal sizes.  Sharded: every rank gets the numpy float64
    statistics of the whole rows rounded to float32.  Mean and win rate exactly: sums of integers and one division, as numpy's.
    se within one float32 ulp (relative 2^-23): the variance is (sum of squares - n mean^2) / (n - 1) in float64, whose terms are
    below 41 * 24^2 < 2^15 and carry a few 2^-53 relative, 1e-11 absolute at the most, against a numerator of at least
    1 - 1 / 41 for an integer row that is not constant (row 3) — so the float64 values agree to 1e-11 relative and can only fall
    on two neighbouring float32.  A constant row has an exact mean, its numerator is 0 (the clamp keeps what rounding could make
    of it from becoming a NaN): se is 0.  Plain: torch's own mean / std / count, exactly as the evaluators return them."""
    import torch

    from brl_amd._match_batch import per_match_stats
    n = sum(sizes)
    rng = np.random.default_rng(n + len(sizes))
    x = rng.integers(-24, 25, (6, n)).astype(np.float32)
    x[1], x[2] = 7.0, -3.0                                   # constant rows: variance 0
    x[3] = 0.0
    x[3, 5] = 1.0                                            # the smallest non-zero variance of an integer row
    x64 = x.astype(np.float64)
    want = (x64.mean(1).astype(np.float32), (x64.std(1, ddof=1) / np.sqrt(n)).astype(np.float32), (x > 0).mean(1).astype(np.float32))
    bounds = np.concatenate([[0], np.cumsum(sizes)])
    parts = [torch.from_numpy(x[:, a:b].copy()) for a, b in zip(bounds[:-1], bounds[1:])]
    stacks = []
    for part in parts:
        rank = _FakeRank()
        per_match_stats(part, n, rank)
        stacks.append(rank.own)
    for k, part in enumerate(parts):
        rank = _FakeRank(stacks)
        imp, se, win = (t.numpy() for t in per_match_stats(part, n, rank))
        assert torch.equal(rank.own, stacks[k]) and imp.dtype == se.dtype == win.dtype == np.float32
        assert np.array_equal(imp, want[0]) and np.array_equal(win, want[2])
        assert np.isfinite(se).all() and (se[1:3] == 0).all() and (se[[0, 3, 4, 5]] > 0).all()
        assert (np.abs(se - want[1]) <= 2.0 ** -23 * want[1]).all()
    cum = torch.from_numpy(x)
    for shard in (None, type("Idle", (), {"active": False})()):
        imp, se, win = per_match_stats(cum, n, shard)
        assert torch.equal(imp, cum.mean(dim=1)) and torch.equal(se, cum.std(dim=1, unbiased=True) / float(n) ** 0.5)
        assert torch.equal(win, (cum > 0).sum(dim=1) / float(n))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                      # (torch warns about the std of nothing)
        empty = per_match_stats(cum[:0], n)                  # a league without pairs: three empty vectors
    assert all(t.shape == (0,) and t.dtype == torch.float32 for t in empty)


def _case(P, n, pairs, acting):
    """terminated / current_player with exactly the boards `acting` (a set of board indices) acting for team 0"""
    term = np.ones(P * n, np.uint8)
    cur = np.full(P * n, 2, np.int32)
    for b in acting:
        term[b], cur[b] = 0, b & 1            # players 0 and 1: team 0
    return term, cur


def test_route_restatement_on_hand_made_cases():
    n = 70
    pairs = np.array([[2, 0], [0, 3], [2, 4], [0, 2]])          # team 0: network 0 plays matches 1 and 3, network 2 matches 0 and 2
    # a group of exactly 64 rows (network 0: 60 boards of match 1 + 4 of match 3) and of 65 (network 2: 65 boards of match 2)
    acting = list(range(n, n + 60)) + [3 * n + 1, 3 * n + 5, 3 * n + 6, 3 * n + 69] + list(range(2 * n + 5, 2 * n + 70))
    term, cur = _case(4, n, pairs, acting)
    rows, gf = route_numpy(term, cur, pairs, 0, n, num_groups=5)
    assert gf.tolist() == [0, 64, 64, 129, 129, 129]              # networks 1, 3 and 4 never act for team 0: empty groups
    assert rows[:64].tolist() == list(range(n, n + 60)) + [3 * n + 1, 3 * n + 5, 3 * n + 6, 3 * n + 69]
    assert rows[64:].tolist() == list(range(2 * n + 5, 2 * n + 70))
    # the other team: nobody's turn
    rows1, gf1 = route_numpy(term, cur, pairs, 1, n, num_groups=5)
    assert len(rows1) == 0 and gf1.tolist() == [0] * 6
    # a live board whose player is on team 1 acts for team 1 only
    cur[0] = 3
    term[0] = 0
    rows1, gf1 = route_numpy(term, cur, pairs, 1, n, num_groups=5)
    assert rows1.tolist() == [0] and gf1.tolist() == [0, 1, 1, 1, 1, 1]    # match 0's team 1 is network 0
    # all boards finished: R = 0
    rows0, gf0 = route_numpy(np.ones(4 * n, np.uint8), np.zeros(4 * n, np.int32), pairs, 0, n, num_groups=5)
    assert len(rows0) == 0 and gf0.tolist() == [0] * 6
    # every board acts: a group is its matches, whole, in the order of the sort
    rows2, gf2 = route_numpy(np.zeros(4 * n, np.uint8), np.zeros(4 * n, np.int32), pairs, 0, n, num_groups=5)
    assert gf2.tolist() == [0, 2 * n, 2 * n, 4 * n, 4 * n, 4 * n]
    assert rows2.tolist() == [b for m in (1, 3, 0, 2) for b in range(m * n, (m + 1) * n)]


def _oracle_match(oracle, n, seed, w1, w2):
    """one duplicate match on the CPU oracle in lock step: every live board calls arg-max over its legal calls of
    observation @ w (w1 for players {0,1}, w2 for players {2,3}) — a deterministic stand-in policy per network"""
    from oracle import Oracle
    ref = oracle.init_random(n, seed=seed)
    A, B = Oracle.table_info_from(ref), Oracle.table_info_from(ref)
    cum = np.zeros(n, np.float32)
    for _ in range(700):
        if ref["terminated"].all():
            break
        obs = ref["observation"].astype(np.float32)
        logits = np.where((ref["current_player"] < 2)[:, None], obs @ w1, obs @ w2)
        act = np.where(ref["legal_action_mask"].astype(bool), logits, -np.inf).argmax(1).astype(np.int32)
        oracle.duplicate_step(ref, act, A, B)
        cum += ref["rewards"][:, 0]
    assert ref["terminated"].all() and A["terminated"].all() and B["terminated"].all()
    return cum, A, B


def test_mirror_property_on_the_cpu_oracle(oracle):
    """Match (j, i) is match (i, j) with the tables exchanged — table A of one is table B of the other: the same deal, the same
    networks in the same seats — so its IMPs are the negatives, board by board.  Confirmed here on the CPU oracle with a
    stand-in policy per network; tests/test_gpu_league.py asserts the same of the batched league."""
    rng = np.random.default_rng(5)
    w = [rng.normal(size=(480, 38)).astype(np.float32) for _ in range(3)]
    n = 200
    for i, j in ((0, 1), (1, 2)):
        cij, Aij, Bij = _oracle_match(oracle, n, 17, w[i], w[j])
        cji, Aji, Bji = _oracle_match(oracle, n, 17, w[j], w[i])
        assert np.abs(cij).max() > 0
        assert np.array_equal(cji, -cij)
        for f in ("last_bid", "call_x", "call_xx"):                 # the contracts: table A of one = table B of the other
            assert np.array_equal(Aij[f], Bji[f]) and np.array_equal(Bij[f], Aji[f]), f
    c00, _, _ = _oracle_match(oracle, n, 17, w[0], w[0])
    assert not c00.any()
