"""The full duplicate-score table on the CPU: ``law_score`` (tests/contract_matrix.py, written from the Laws) against the oracle's
and pyref's scorers on all 2940 cells, and the whole matrix of scripted auctions — every cell, from every declarer seat, through
three auction shapes — stepped through the C oracle.  CPU only; the GPU paths play the same matrix in tests/test_gpu_contracts.py."""
import numpy as np

from oracle import pyref
from tests import contract_matrix as cm
from tests import test_oracle_kat as kat


def test_law_score_equals_oracle_and_pyref_on_every_cell(oracle):
    seen = set()
    for c in range(cm.N_CELLS):
        strain, level, dbl, vul, taken = cm.cell_of(c)
        seen.add((strain, level, dbl, vul, taken))
        want = cm.law_score(strain, level, vul, dbl, taken)
        assert oracle.score(strain, level, vul, dbl >= 1, dbl == 2, taken) == want, (strain, level, dbl, vul, taken)
        assert pyref.score(strain, level, bool(vul), dbl, taken) == want, (strain, level, dbl, vul, taken)
    assert len(seen) == 5 * 7 * 3 * 2 * 14 == cm.N_CELLS


def test_law_score_reproduces_the_known_contracts():
    assert len(kat.KNOWN_CONTRACTS) == 40
    for (strain, level, vul, x, xx, taken), want in kat.KNOWN_CONTRACTS:
        assert cm.law_score(strain, level, vul, 2 if xx else int(x), taken) == want, (strain, level, vul, x, xx, taken)


def test_law_score_is_strictly_monotone_in_tricks():
    """what makes the trick table's filler entries tell: another seat's or strain's nibble cannot give the expected score"""
    for c in range(0, cm.N_CELLS, 14):
        strain, level, dbl, vul, _ = cm.cell_of(c)
        s = [cm.law_score(strain, level, vul, dbl, t) for t in range(14)]
        assert all(a < b for a, b in zip(s, s[1:]))


def test_imp_scale():
    assert [cm.imp(d) for d in (0, 10, 20, -20, 40, 50, 3990, 4000, -4000, 15200)] == [0, 0, 1, -1, 1, 2, 23, 24, -24, 24]
    assert all(cm.imp(th) == k + 1 and cm.imp(th - 10) == k for k, th in enumerate(kat.IMP_THRESHOLDS))


def test_the_matrix_covers_every_cell_declarer_seating_and_dealer(dds, oracle):
    m = cm.matrix(dds, oracle)
    assert m.n == cm.N_TABLES == 3 * 4 * 2940 + 4
    case = m.passout == 0
    for shape in range(3):
        for seat in range(4):
            sel = case & (m.shape == shape) & (m.declarer == seat)
            assert np.array_equal(np.sort(m.cell[sel]), np.arange(2940)), (shape, seat)
    assert set(m.declarer[case]) == {0, 1, 2, 3} and set(m.dealer[case]) == {0, 1, 2, 3} and set(m.seating) == set(range(8))
    assert sorted(m.dealer[~case]) == [0, 1, 2, 3]
    assert set(m.vul_ns) == {0, 1} and set(m.vul_ew) == {0, 1} and len(set(m.row)) == len(dds["keys"])
    assert len({tuple(s) for s in m.shuffled}) == 8
    for s in m.shuffled[:56]:
        assert sorted(s) == [0, 1, 2, 3] and {s[0], s[2]} in ({0, 1}, {2, 3})
    # per cell: every dealer and every seating across its 12 tables
    for c in (0, 1, 1469, 2939):
        sel = case & (m.cell == c)
        assert sel.sum() == 12 and set(m.dealer[sel]) == {0, 1, 2, 3} and len(set(m.seating[sel])) == 8
    # the three shapes of one (cell, declarer) differ: at level 1 by their opening passes, above by their calls
    a, b, c = (m.calls[s * 4 * 2940:(s + 1) * 4 * 2940] for s in range(3))
    assert (np.any(a != b, axis=1) & np.any(a != c, axis=1) & np.any(b != c, axis=1)).all()
    assert m.max_len <= 13 and m.pair_max <= 13 + 9
    # the trick table: the cell's count where the declarer's strain is, another count everywhere else
    idx = m.declarer[case] * 5 + m.strain[case]
    t = m.tricks[case]
    assert np.array_equal(t[np.arange(len(t)), idx], m.taken[case])
    assert ((t != m.taken[case][:, None]).sum(1) == 19).all() and t.max() == 13
    # outcomes reached: all 1978 distinct (strain, level, doubling, |score|) of the table
    assert len({(int(s), int(l), int(d), abs(int(x))) for s, l, d, x in zip(m.strain[case], m.level[case], m.doubling[case],
                                                                           m.score[case])}) == 1978


def test_the_matrix_through_the_oracle_in_lockstep(dds, oracle):
    m = cm.matrix(dds, oracle)
    run = cm.oracle_lockstep(dds, oracle)
    assert run["legal"].all(), np.nonzero(~run["legal"])[0][:5]
    steps = run["terminated"].shape[0]
    assert steps == m.max_len + 1
    for k in range(steps):
        # every table ends on its last scripted call and not before; its rewards appear on that step alone
        assert np.array_equal(run["terminated"][k] != 0, m.length - 1 <= k), k
        want = cm.expected_step_rewards(m, k)
        bad = np.nonzero((run["rewards"][k] != want).any(1))[0]
        assert len(bad) == 0, (k, bad[:5], run["rewards"][k][bad[:5]], want[bad[:5]])
    st = run["state"]
    assert (st["illegal"] == 0).all()
    assert np.array_equal(st["last_bid"], m.last_bid) and np.array_equal(st["last_bidder"], m.last_bidder)
    case = m.passout == 0
    assert np.array_equal(st["call_x"][case], (m.doubling[case] >= 1).astype(np.int32))
    assert np.array_equal(st["call_xx"][case], (m.doubling[case] == 2).astype(np.int32))
    assert (st["call_x"][~case] == 0).all() and (st["pass_num"][~case] == 4).all() and (st["pass_num"][case] == 3).all()
    fd = np.where((m.declarer % 2 == 0)[:, None], st["first_denomination_ns"], st["first_denomination_ew"])
    assert np.array_equal(fd[case, m.strain[case]], m.declarer[case])
    assert np.array_equal(st["tricks"], m.tricks) and np.array_equal(st["shuffled_players"], m.shuffled)
    # by player id: + for the two players of the declaring side, - for the others
    r = m.rewards
    assert (r[:, 0] == r[:, 1]).all() and (r[:, 2] == r[:, 3]).all() and (r[:, 0] == -r[:, 2]).all()
    assert np.array_equal(np.abs(r[:, 0]).astype(np.int64), np.abs(m.score))


def test_the_paired_tables_through_the_oracle(dds, oracle):
    """table A (case i) and table B (the direct auction of case i + 1471 on board i) through duplicate_step: both Table_info
    snapshots and the IMPs equal what law_score says of the two contracts"""
    m = cm.matrix(dds, oracle)
    assert np.gcd(cm.PAIR_STRIDE, m.n) == 1
    run = cm.oracle_pairs(dds, oracle)
    A, B, st = run["A"], run["B"], run["state"]
    assert (A["terminated"] == 1).all() and (B["terminated"] == 1).all() and (st["terminated"] == 1).all() and (st["illegal"] == 0).all()
    assert np.array_equal(A["rewards"], m.rewards) and np.array_equal(A["last_bid"], m.last_bid)
    assert np.array_equal(B["rewards"], m.b_rewards) and np.array_equal(B["last_bid"], m.b_last_bid)
    assert np.array_equal(B["call_x"], (m.b_doubling >= 1).astype(np.int32)) and np.array_equal(B["call_xx"], (m.b_doubling == 2).astype(np.int32))
    assert np.array_equal(st["shuffled_players"], m.b_shuffled)
    assert np.array_equal(run["returns"], m.imp_rewards)
    ns_player = m.shuffled[:, 0]
    assert np.array_equal(m.imp_rewards[np.arange(m.n), ns_player].astype(np.int32), m.imp_ns)
    assert len(set(m.imp_ns)) == 49      # every IMP value from -24 to 24 is paid somewhere


def test_rollout_placement_reaches_every_cell(dds, oracle):
    """the fused-rollout test's precondition, on the host: each of the 2940 cells sits, one pass from its end, in a slot whose
    first draw is that pass; the oracle's rollout ends it in step 0 with the score law_score gives"""
    m = cm.matrix(dds, oracle)
    p = cm.rollout_placement(dds, oracle)
    slots = p["slots"]
    assert (slots >= 0).all() and len(set(slots)) == cm.N_CELLS, cm.PLACEMENT_HINT
    assert p["n_legal"].min() == 1 and p["n_legal"].max() == 36
    for c in range(0, cm.N_CELLS, 7):
        assert oracle.random_action(p["prefix"][c:c + 1], int(p["draws"][slots[c]])) == (0, int(p["n_legal"][c]))
    want = p["want"]
    assert (want["action"][0, slots] == 0).all() and (want["done"][0, slots] == 1).all()
    score = (p["actor_sign"] * m.score[:cm.N_CELLS]).astype(np.float32)
    assert np.array_equal(want["reward"][0, slots], score / np.float32(cm.REWARD_SCALE))
    assert (p["final"]["board_ctr"][slots] >= 1).all()
