"""CPU checks of cross-play's host side (brl_amd/crossplay.py, include/brl_crossplay.h): the header against the ctypes binding, the
per-team slot orders, the route's numpy restatement on hand-made cases (tests/crossplay_ref.py: what tests/test_gpu_crossplay.py
compares the kernels with), the CrossPlay arithmetic against a by-hand float64 restatement, and the CLI's parser."""
import json
import os

import numpy as np
import pytest

from tests.crossplay_ref import xroute_numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_header_is_the_binding():
    from brl_amd import _capi
    sigs = _capi.SIGNATURES      # (every header against its entry: tests/test_capi_cpu.py)
    assert sigs["brl_crossplay.h"]["brl_xplay_route"] == sigs["brl_league.h"]["brl_league_route"]      # the same call, another grouping


LINEUP_CASES = {
    "four different networks": [(0, 1, 2, 3), (3, 2, 1, 0), (1, 3, 0, 2)],
    "shared partners": [(0, 0, 1, 1), (1, 1, 2, 2), (0, 0, 2, 2), (2, 2, 0, 0)],
    "a network used by both teams": [(0, 1, 1, 0), (2, 0, 0, 0), (1, 1, 1, 1), (0, 2, 2, 1)],
    "one line-up": [(5, 3, 3, 5)],
    "cross-play": [(x, y, 4, 4) for x in range(4) for y in range(4)],
}


@pytest.mark.parametrize("case", sorted(LINEUP_CASES))
@pytest.mark.parametrize("team", [0, 1])
def test_lineup_order_is_a_sorted_permutation_of_the_slots(case, team):
    from brl_amd.crossplay import lineup_order
    lineups = np.array(LINEUP_CASES[case])
    order, group_of, nets = lineup_order(lineups, team)
    P = len(lineups)
    assert order.dtype == np.int32 and group_of.dtype == np.int32
    assert sorted(order.tolist()) == list(range(2 * P))                                  # a permutation of the slots
    played = lineups[order >> 1, 2 * team + (order & 1)]                                 # the network of slot (match, half)
    assert (np.diff(group_of) >= 0).all() and group_of[0] == 0 and group_of[-1] == len(nets) - 1
    assert (np.diff(nets) > 0).all() and np.array_equal(nets[group_of], played)
    assert set(nets.tolist()) == set(lineups[:, 2 * team:2 * team + 2].reshape(-1).tolist())
    same = np.diff(played) == 0                                                          # stable: equal networks keep the slots' own order
    assert (np.diff(order)[same] > 0).all()


def test_shared_partners_give_the_leagues_order_with_every_match_split_in_two():
    from brl_amd.crossplay import lineup_order
    from brl_amd.league import team_order
    rng = np.random.default_rng(3)
    pairs = rng.integers(0, 5, (12, 2))
    lineups = np.stack([pairs[:, 0], pairs[:, 0], pairs[:, 1], pairs[:, 1]], axis=1)
    for team in (0, 1):
        order, group_of, nets = lineup_order(lineups, team)
        lo, lg, ln = team_order(pairs, team)
        assert np.array_equal(nets, ln)
        assert np.array_equal(order, np.stack([2 * lo, 2 * lo + 1], axis=1).reshape(-1))   # slots (2m, 2m + 1) adjacent
        assert np.array_equal(group_of, np.repeat(lg, 2))                                # ... and in one group


@pytest.mark.parametrize("P,n", [(1100, 3), (600, 3)])
@pytest.mark.parametrize("team", [0, 1])
def test_the_two_route_restatements_agree_on_shared_partners_beyond_1024_slots(P, n, team):
    """the shapes at which tests/test_gpu_league.py and tests/test_gpu_crossplay.py give a thread of the scan two positions: on
    line-ups (i, i, j, j) both restatements give one group_first and the same boards in every group; and the league's 1100 pairs
    (the GPU test's own) change group inside a thread's run of two positions and at its end"""
    from brl_amd.crossplay import lineup_order
    from brl_amd.league import team_order
    from tests.test_league_host import route_numpy
    rng = np.random.default_rng(100 * P + n + team)
    M = 7
    pairs = rng.integers(0, M, (P, 2))
    lineups = np.stack([pairs[:, 0], pairs[:, 0], pairs[:, 1], pairs[:, 1]], axis=1)
    term = (rng.random(P * n) < 0.4).astype(np.uint8)
    cur = rng.integers(0, 4, P * n).astype(np.int32)
    order, group_of, nets = lineup_order(lineups, team)
    lrows, lgf = route_numpy(term, cur, pairs, team, n, num_groups=M + 2)
    rows, gf = xroute_numpy(term, cur, team, n, order, nets[group_of], M + 2)
    assert np.array_equal(gf, lgf) and gf[-1] == gf[M] > 0 and sorted(rows.tolist()) == sorted(lrows.tolist())
    for g in range(M):
        assert np.array_equal(np.sort(rows[gf[g]:gf[g + 1]]), np.sort(lrows[gf[g]:gf[g + 1]]))
    if P == 1100:
        changes = np.nonzero(np.diff(team_order(pairs, team)[1]))[0] + 1  # the league's positions where a new group starts
        assert len(changes) == M - 1 and {0, 1} == set((changes % 2).tolist())


def test_route_restatement_on_hand_made_cases():
    from brl_amd.crossplay import lineup_order
    n = 5
    lineups = np.array([(2, 0, 9, 9), (0, 0, 9, 9), (1, 2, 9, 9)])
    order, group_of, nets = lineup_order(lineups, 0)
    assert order.tolist() == [1, 2, 3, 4, 0, 5] and nets.tolist() == [0, 1, 2] and group_of.tolist() == [0, 0, 0, 1, 2, 2]
    term = np.zeros(3 * n, np.uint8)
    #                  match 0          match 1          match 2
    cur = np.array([0, 1, 1, 2, 0,   1, 0, 3, 1, 0,   1, 1, 1, 0, 1], np.int32)
    term[4] = 1                                   # a finished board does not act, whoever is to call
    term[13] = 1                                  # match 2's only board of half 0: slot 4 (network 1) is empty between two others
    rows, gf = xroute_numpy(term, cur, 0, n, order, group_of, 3)
    #   slot 1 (match 0, half 1): 1, 2 | slot 2 (match 1, half 0): 6, 9 | slot 3 (match 1, half 1): 5, 8 | slot 4: - | slot 0: 0 | slot 5: 10 11 12 14
    assert rows.tolist() == [1, 2, 6, 9, 5, 8, 0, 10, 11, 12, 14] and gf.tolist() == [0, 6, 6, 11]
    rows1, gf1 = xroute_numpy(term, cur, 1, n, *lineup_order(lineups, 1)[:2], 1)
    assert rows1.tolist() == [3, 7] and gf1.tolist() == [0, 2]
    rows0, gf0 = xroute_numpy(np.ones(3 * n, np.uint8), cur, 0, n, order, group_of, 3)
    assert len(rows0) == 0 and gf0.tolist() == [0, 0, 0, 0]


def _by_hand(c, M, n):
    """the issue's formulas, element by element in Python floats (float64)"""
    imp = [[sum(float(v) for v in c[x * M + y]) / n for y in range(M)] for x in range(M)]
    gap, gap_se = [[0.0] * M for _ in range(M)], [[0.0] * M for _ in range(M)]
    for x in range(M):
        for y in range(M):
            g = [(float(c[x * M + y][b]) + float(c[y * M + x][b])) / 2 - (float(c[x * M + x][b]) + float(c[y * M + y][b])) / 2
                 for b in range(n)]
            mean = sum(g) / n
            gap[x][y] = mean
            gap_se[x][y] = (sum((v - mean) ** 2 for v in g) / (n - 1)) ** 0.5 / n ** 0.5
    return imp, gap, gap_se


def test_crossplay_arithmetic_against_a_by_hand_restatement(tmp_path):
    from brl_amd.crossplay import CrossPlay, cross_lineups
    M, n = 3, 5
    assert cross_lineups(M).tolist() == [[x, y, 3, 3] for x in range(3) for y in range(3)]
    rng = np.random.default_rng(11)
    c = rng.integers(-24, 25, (M * M, n)).astype(np.float32)             # IMPs are integers
    cp = CrossPlay(c)
    imp, gap, gap_se = _by_hand(c.tolist(), M, n)
    assert cp.imp.dtype == np.float64 and cp.gap.dtype == np.float64 and cp.imp.shape == cp.se.shape == cp.gap.shape == cp.gap_se.shape == (M, M)
    assert np.allclose(cp.imp, imp, rtol=0, atol=1e-12)
    assert np.allclose(cp.se, [[np.std(c[x * M + y].astype(np.float64), ddof=1) / np.sqrt(n) for y in range(M)] for x in range(M)], rtol=0, atol=1e-12)
    assert np.allclose(cp.gap, gap, rtol=0, atol=1e-12) and np.allclose(cp.gap_se, gap_se, rtol=0, atol=1e-12)
    assert (np.diag(cp.gap) == 0.0).all() and (np.diag(cp.gap_se) == 0.0).all()      # exactly
    assert np.array_equal(cp.sym, cp.sym.T) and np.array_equal(cp.sym, (cp.imp + cp.imp.T) / 2)
    assert np.array_equal(cp.gap, cp.gap.T)
    # given statistics (the evaluator's own float32 ones) are kept as they are
    given = CrossPlay(c, imp=np.arange(9, dtype=np.float32), se=np.ones(9, np.float32))
    assert np.array_equal(given.imp, np.arange(9.0).reshape(3, 3)) and np.array_equal(given.gap, cp.gap)
    # worst: the pairs x < y by gap, most negative first
    w = cp.worst(3)
    assert [(x, y) for x, y, _, _ in w] == sorted([(0, 1), (0, 2), (1, 2)], key=lambda p: cp.gap[p])
    assert [g for _, _, g, _ in w] == sorted(g for _, _, g, _ in w) and len(cp.worst(1)) == 1 and cp.worst(1)[0] == w[0]
    assert all(g == cp.gap[x, y] and e == cp.gap_se[x, y] for x, y, g, e in w)
    # a pair that plays better with itself than mixed has a negative gap of exactly that size
    c2 = np.zeros((4, 4), np.float32)
    c2[0], c2[3] = [2, 4, 0, 2], [1, 1, 1, 1]                            # (0, 0) and (1, 1); mixed: 0 on every board
    cp2 = CrossPlay(c2, names=["a", "b"])
    assert cp2.gap[0, 1] == cp2.gap[1, 0] == -(2.0 + 1.0) / 2 and cp2.worst(5) == [(0, 1, -1.5, cp2.gap_se[0, 1])]
    text = cp2.to_text()
    assert "±" in text and "gap" in text and " a " in text + " "
    path = tmp_path / "cp.json"
    cp2.to_json(path)
    doc = json.loads(path.read_text())
    assert doc["gap"] == cp2.gap.tolist() and doc["imp"] == cp2.imp.tolist() and doc["worst"][0]["gap"] == -1.5 and doc["boards"] == 4
    assert cp2.stacked().shape == (4, 2, 2)
    with pytest.raises(ValueError):
        CrossPlay(np.zeros((5, 4)))


def test_parse_rejects_an_unknown_key_and_keeps_the_leagues_defaults():
    from brl_amd.crossplay import CROSSPLAY_DEFAULTS, parse
    from brl_amd.league import LEAGUE_DEFAULTS
    cfg = parse(["exp_name=run7", "num_eval_envs=64", "opp_model_path=o.pt", "save_path=x.json"])
    assert cfg == dict(CROSSPLAY_DEFAULTS, exp_name="run7", num_eval_envs=64, opp_model_path="o.pt", save_path="x.json")
    shared = set(CROSSPLAY_DEFAULTS) & set(LEAGUE_DEFAULTS)
    assert shared >= {"models_directory", "exp_name", "num_eval_envs", "skip_interval", "max_step", "dds_path", "max_boards"}
    assert all(CROSSPLAY_DEFAULTS[k] == LEAGUE_DEFAULTS[k] for k in shared)
    assert set(CROSSPLAY_DEFAULTS) - set(LEAGUE_DEFAULTS) == {"opp_model_path", "save_path"}
    with pytest.raises(SystemExit):
        parse(["shard=1"])
    with pytest.raises(SystemExit):
        parse(["save_fig_directory_path=figs"])
