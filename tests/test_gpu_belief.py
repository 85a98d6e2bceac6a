"""-m gpu: the hand beliefs (brl_amd/belief.py, include/brl_belief.h) — brl_belief_deal, brl_belief_logp and brl_belief_reduce
against their Python restatement (tests/belief_ref.py), and whole beliefs of the bidder pair (tests/bidder_net.py) on hands of the
named deals: every row's weight against the float64 chain on the CPU oracle's observations, the greedy flags, the entries against
the restatement's reduction of the device's own rows, the prior, the direction an auction moves the belief in, the batching, one
network on both sides, queries from a recorded match, the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import belief_ref as BR
from tests import bidder_net as bn
from tests import book_ref as B
from tests.nets import forward64
from tests.test_gpu_forward_biases import _tol32
from tests.test_gpu_review import _oracle_tables

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMED = os.path.join(ROOT, "tests", "golden", "wb5_named_24.json")
SEATINGS = [(0, 2, 1, 3), (2, 0, 3, 1), (1, 3, 0, 2), (3, 1, 2, 0)]
SEED = 0x1234567 + (0x9ABC << 32)      # both key words count


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _entries(raw):
    from brl_amd import belief
    return raw.cpu().numpy().view(belief.ENTRY_DTYPE).reshape(-1)


# ---- deal --------------------------------------------------------------------------------------------------------------------------
def _deal_queries(Q, shift):
    from brl_amd import belief
    rng = np.random.default_rng(40 + Q)
    own = [B.shaped_hand([0, 4, 4, 5], top=False), B.shaped_hand([0, 0, 13, 0])] + [B.random_hands(rng)[0] for _ in range(Q)]
    return [belief.BeliefQuery((i + shift) & 3, own[(i + shift) % len(own)], (i + 1 + shift) & 3, ((i + shift) & 1, ((i + shift) >> 1) & 1),
                               [], SEATINGS[(i + shift) & 3]) for i in range(Q)]


@pytest.mark.parametrize("Q,K,q0", [(1, 1, 0), (1, 64, 1), (5, 257, 7), (3, 4096, 0)])
def test_deal_equals_the_restatement_bit_for_bit(Q, K, q0):
    """every own seat, dealer, vulnerability and seating, an own hand with a void and one with a 13-card suit (Q = 5); K below, at
    and above a wave's 64 samples and no multiple of it; a stream index offset"""
    from brl_amd import belief
    qs = _deal_queries(Q, K)
    if Q == 5:
        assert len({q.seat for q in qs}) == 4 and len({q.dealer for q in qs}) == 4 and len({q.seating for q in qs}) == 4
        assert len({(q.vul_ns, q.vul_ew) for q in qs}) == 4
        lengths = [BR.features(np.uint64(q.hand))[2].tolist() for q in qs]
        assert any(13 in x for x in lengths) and any(0 in x and 13 not in x for x in lengths)
    qdev = _dev(belief.query_array(qs).view(np.uint8).reshape(Q, 16))
    tables, hands = belief.deal(qdev, K, SEED, q0)
    tables, hands = tables.cpu().numpy().view(np.uint64), hands.cpu().numpy().view(np.uint64)
    assert tables.shape == (Q * K, 16) and hands.shape == (Q * K, 4)
    for i, q in enumerate(qs):
        want = BR.sample_hands(q.seat, q.hand, SEED, q0 + i, np.arange(K))
        assert np.array_equal(hands[i * K:(i + 1) * K], want), i
        assert np.array_equal(tables[i * K:(i + 1) * K], BR.sample_tables(q.dealer, q.vul_ns, q.vul_ew, q.seating, want)), i
    again = belief.deal(qdev, K, SEED, q0)
    assert np.array_equal(again[0].cpu().numpy().view(np.uint64), tables)
    if Q > 1:       # a query's samples do not depend on the queries drawn with it
        alone = belief.deal(qdev[1:2].clone(), K, SEED, q0 + 1)[1].cpu().numpy().view(np.uint64)
        assert np.array_equal(alone, hands[K:2 * K])


# ---- logp --------------------------------------------------------------------------------------------------------------------------
U = 2.0 ** -24
LOGP_BOUND = 164 * U
"""|device log-probability - float64 log-softmax of the same fp32 logits|, counted from the kernel's own float32 operations
(policy_common.hpp: categorical<8>, then brl_belief.hip), u = 2^-24 the unit roundoff, logits within +-30, x_i = l_i - m in [-60, 0]:
  * d = l_call - m: one rounding, <= 60 u;
  * e_i = expf(x_i): x_i is rounded (relative u, so e_i is off by the factor exp(x_i u'), relative |x_i| u) and expf is good to
    2 ulp = 4 u relative.  In total = sum e_i the first part weighs |x_i| e^{x_i} <= 1/e per term, at most 37 terms beside the
    maximum's exact 1, against total >= 1: <= (37 / e) u < 13.7 u; the second 4 u; the sum itself is 4 additions inside a lane and
    3 levels across the 8 lanes: 7 u.  relative error of total < 24.7 u;
  * logf(total): that relative error becomes an absolute one, 24.7 u, plus logf's own 2 ulp = 4 u relative of at most ln 38 = 3.64:
    14.6 u;
  * d - logf(total): one rounding of a value within 60 + 3.64: 63.7 u.
  60 + 24.7 + 14.6 + 63.7 = 163 u < 164 u = 9.8e-6."""


def _logp_case(ld, seed):
    rng = np.random.default_rng(seed)
    n, Q = 300, 7
    words = [1, 1 | (1 << 37), (1 << 38) - 1, 1 | 2 | (((1 << 38) - 1) >> 9 << 9), 1 | 4 | (((1 << 38) - 1) >> 20 << 20), 1 | (7 << 35), (1 << 38) - 1]
    actions = [0, 37, 12, 1, 2, 36, 0]
    assert [bin(w).count("1") for w in words[:3]] == [1, 2, 38] and all((w >> a) & 1 for w, a in zip(words, actions))
    query_of = rng.integers(0, Q, size=n).astype(np.int32)
    query_of[:Q] = np.arange(Q)
    rows = rng.permutation(n)[:203].astype(np.int64)              # a strict subset, in no order
    assert len(set(rows.tolist())) == 203 and (np.diff(rows) < 0).any() and set(range(Q)) <= set(query_of[rows].tolist())
    m = len(rows)
    logits = rng.uniform(-30, 30, size=(m, ld)).astype(np.float32)
    for i in range(m):
        q = query_of[rows[i]]
        legal = [a for a in range(38) if (words[q] >> a) & 1]
        a = actions[q]
        kind = i % 5
        if kind == 0:                                             # the call at the largest legal logit, at the range's end
            logits[i, a] = 30.0
        elif kind == 1 and len(legal) > 1:                        # at the smallest, the largest at the other end
            logits[i, a] = -30.0
            logits[i, [x for x in legal if x != a][0]] = 30.0
        elif kind == 2:                                           # everything else far below
            logits[i, [x for x in legal if x != a]] = rng.uniform(-30, -29, size=len(legal) - 1).astype(np.float32)
            logits[i, a] = 30.0
    return n, Q, words, actions, query_of, rows, logits


@pytest.mark.parametrize("ld", [38, 39])
def test_logp_against_float64_of_the_same_logits(ld):
    from brl_amd import belief
    n, Q, words, actions, query_of, rows, logits = _logp_case(ld, 70 + ld)
    rng = np.random.default_rng(1)
    greedy0 = (rng.random(n) < 0.8).astype(np.uint8)
    logw0 = np.zeros(n, np.float32)
    listed = np.zeros(n, bool)
    listed[rows] = True
    logw0[~listed] = 123.0
    logw, greedy = _dev(logw0), _dev(greedy0)
    belief.logp(_dev(logits), _dev(rows), _dev(query_of), _dev(np.array(words, np.int64)), _dev(np.array(actions, np.int32)), logw, greedy)
    logw, greedy = logw.cpu().numpy(), greedy.cpu().numpy()
    assert np.array_equal(logw[~listed], logw0[~listed]) and np.array_equal(greedy[~listed], greedy0[~listed])      # nobody else's rows
    worst, ties, at_top, at_bottom = 0.0, 0, 0, 0
    for i, r in enumerate(rows):
        q = query_of[r]
        lp, g = BR.logp64(logits[i, :38].astype(np.float64), words[q], actions[q])
        worst = max(worst, abs(float(logw[r]) - float(lp)))
        legal = np.sort(logits[i, :38][[(words[q] >> a) & 1 == 1 for a in range(38)]].astype(np.float64))
        ties += int(len(legal) > 1 and legal[-1] - legal[-2] < LOGP_BOUND)
        assert greedy[r] == (greedy0[r] & int(g)), (i, r)
        at_top += int(logits[i, actions[q]] == legal[-1])
        at_bottom += int(len(legal) > 1 and logits[i, actions[q]] == legal[0])
    print(f"logp ld={ld}: largest |device - float64| = {worst:.3e} = {worst / U:.1f} u (bound {LOGP_BOUND:.3e} = 164 u); "
          f"calls at the largest legal logit {at_top}, at the smallest {at_bottom}")
    assert ties == 0 and at_top >= 40 and at_bottom >= 20 and float(np.abs(logits).max()) == 30.0
    assert worst <= LOGP_BOUND
    assert logw[rows].min() < -55.0 and logw[rows].max() == 0.0      # the whole range: a call 60 below the best, a forced call


def test_logp_accumulates_over_calls():
    """two calls on the same rows: logw is the float32 sum of the two terms, greedy the conjunction"""
    from brl_amd import belief
    n, Q, words, actions, query_of, rows, logits = _logp_case(38, 5)
    args = (_dev(query_of), _dev(np.array(words, np.int64)), _dev(np.array(actions, np.int32)))
    one_w, one_g = torch.zeros(n, device=DEV), torch.ones(n, dtype=torch.uint8, device=DEV)
    belief.logp(_dev(logits), _dev(rows), *args, one_w, one_g)
    other = np.ascontiguousarray(logits[::-1])
    two_w, two_g = torch.zeros(n, device=DEV), torch.ones(n, dtype=torch.uint8, device=DEV)
    belief.logp(_dev(other), _dev(rows), *args, two_w, two_g)
    both_w, both_g = one_w.clone(), one_g.clone()
    belief.logp(_dev(other), _dev(rows), *args, both_w, both_g)
    assert torch.equal(both_w, one_w + two_w) and torch.equal(both_g, one_g & two_g) and 0 < int(both_g.sum()) < int(one_g.sum())


def test_logp_on_non_finite_logits():
    """include/brl_belief.h, non-finite values: the float64 log-softmax's NaN / -inf, greedy false wherever the value is NaN"""
    from brl_amd import belief
    nan, inf = np.nan, np.inf
    word, a = 1 | 2 | (0xFF << 10), 11            # legal: 0, 1, 10..17; the call: 11
    base = np.linspace(-3, 3, 38).astype(np.float32)
    cases = []
    for legal_at, called, illegal_at in ((nan, None, None), (None, None, nan), (inf, None, None), (-inf, None, None), (None, -inf, None),
                                         (None, nan, None), (None, inf, None), (None, None, inf), (None, None, -inf), ("all", None, None)):
        row = base.copy()
        row[17] = 9.0 if called is None else row[17]          # (the call is not the arg-max unless made so below)
        if legal_at == "all":
            row[[0, 1] + list(range(10, 18))] = -inf
        elif legal_at is not None:
            row[14] = legal_at
        if called is not None:
            row[a] = called
        if illegal_at is not None:
            row[5] = illegal_at
        cases.append(row)
    greedy_row = base.copy()
    greedy_row[a] = 8.0
    cases.append(greedy_row)
    logits = np.stack(cases)
    m = len(cases)
    logw, greedy = torch.zeros(m, device=DEV), torch.ones(m, dtype=torch.uint8, device=DEV)
    belief.logp(_dev(logits), _dev(np.arange(m, dtype=np.int64)), torch.zeros(m, dtype=torch.int32, device=DEV),
                _dev(np.array([word], np.int64)), _dev(np.array([a], np.int32)), logw, greedy)
    logw, greedy = logw.cpu().numpy(), greedy.cpu().numpy()
    for i in range(m):
        lp, g = BR.logp64(logits[i].astype(np.float64), word, a)
        assert np.isnan(lp) == np.isnan(logw[i]) and (np.isinf(lp) == np.isinf(logw[i])), (i, lp, logw[i])
        if np.isfinite(lp):
            assert abs(float(logw[i]) - float(lp)) <= LOGP_BOUND, i
        assert greedy[i] == int(g), i
    assert np.isnan(logw[[0, 2, 5, 6, 9]]).all() and np.isfinite(logw[[1, 3, 7, 8, 10]]).all() and logw[4] == -inf
    assert greedy.tolist() == [0] * 10 + [1]


# ---- reduce ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 257, 1100])
def test_reduce_equals_the_restatement_on_the_devices_own_rows(K):
    """K = 1, below one tile of 512 samples, and two tiles and a part; per K: a plain query, one whose rows are all inconsistent,
    one with a NaN row, one whose weights differ by e^-40; the device's own hands; the same bytes on a second run"""
    from brl_amd import belief
    qs = _deal_queries(4, K)
    Q = len(qs)
    qdev = _dev(belief.query_array(qs).view(np.uint8).reshape(Q, 16))
    _, hands = belief.deal(qdev, K, SEED, 0)
    rng = np.random.default_rng(K)
    logw = (rng.normal(size=(Q, K)) * 3 - 5).astype(np.float32)
    greedy = (rng.random((Q, K)) < 0.3).astype(np.uint8)
    greedy[1] = 0
    logw[2, K // 2] = np.nan
    logw[3] -= (40 * (np.arange(K) % 2)).astype(np.float32)
    raw = belief.reduce(qdev, K, hands, _dev(logw.reshape(-1)), _dev(greedy.reshape(-1)))
    got = _entries(raw)
    h = hands.cpu().numpy().view(np.uint64).reshape(Q, K, 4)
    worst = 0.0
    for i, q in enumerate(qs):
        worst = max(worst, BR.compare_entry(got[i], BR.reduce64(q.seat, h[i], logw[i], greedy[i]), K))
    print(f"reduce K={K}: largest relative difference of a float64 sum {worst:.2e} (allowed {K * 2.0 ** -52:.2e})")
    assert got["consistent"][1] == 0 and not got["g_card"][1].any() and np.isnan(got["wsum"][2])
    assert got["consistent"][2] == int(greedy[2].sum()) and (K == 1 or got["consistent"][2] > 0)      # the integers of a NaN query stand
    assert np.isfinite(got["wsum"][[0, 1, 3]]).all() and (got["n"] == K).all()
    assert torch.equal(belief.reduce(qdev, K, hands, _dev(logw.reshape(-1)), _dev(greedy.reshape(-1))), raw)


# ---- end to end --------------------------------------------------------------------------------------------------------------------
K_E2E = 4096


def _queries():
    """five queries on hands of the named deals, the prefixes taken from the auctions the bidder pair itself plays on them (so that
    the greedy policy can have made them): (0) board 0's South before any call; (1) the same hand after P P 1C P: partner opened at
    the one level and the next hand passed; (2) board 18's West after 1NT 2D P: an opponent opened and partner overcalled; (3) board
    17's West after P 1D 2D P: a four-call competitive prefix; (4) board 5's South after 1H P P P: a finished auction"""
    from brl_amd import belief, boards
    words = boards.read_deals(NAMED).hand_words()
    south = int(words[0, 2])
    return [belief.BeliefQuery("S", south, "S", "EW", []),
            belief.BeliefQuery("S", south, "S", "EW", ["P", "P", "1C", "P"]),
            belief.BeliefQuery("W", int(words[18, 3]), "N", "NS", ["1NT", "2D", "P"], SEATINGS[1]),
            belief.BeliefQuery("W", int(words[17, 3]), "W", "None", ["P", "1D", "2D", "P"], SEATINGS[2]),
            belief.BeliefQuery("S", int(words[5, 2]), "W", "Both", ["1H", "P", "P", "P"], SEATINGS[3])]


def _chain(oracle, nets, q, hands):
    """belief_ref.chain64 of one query's device hands: the CPU oracle's observations, float64 forwards on the GPU"""
    from brl_amd import boards
    K = hands.shape[0]
    rec = np.zeros(K, boards.RECORD_DTYPE)
    rec["hands"], rec["dealer"], rec["vul_ns"], rec["vul_ew"], rec["seating"] = hands, q.dealer, q.vul_ns, q.vul_ew, q.seating
    tables = _oracle_tables(oracle, rec, np.zeros((K, 20), np.uint8))
    tols = []

    def forward(team, obs):
        ref = forward64(nets[team], torch.from_numpy(np.ascontiguousarray(obs)).to(DEV))[:, :38]
        tols.append(_tol32(ref))
        return ref.cpu().numpy()

    return BR.chain64(tables, lambda tb, a: oracle.step(tb, a), q.seat, q.team_at, q.dealer, q.calls, forward, lambda lg: tols[-1])


@pytest.fixture(scope="module")
def e2e(dds, oracle):
    """the five beliefs (K = 4096: the forwards of 4096 rows and more take the plane route) with the device's rows, and the
    float64 chain of every row, computed once"""
    import brl_amd
    from brl_amd import belief
    nets = bn.pair(DEV)
    env = brl_amd.BridgeBidding(lut=(dds["keys"], dds["values"]), device=DEV)
    qs = _queries()
    rows, counts = [], {}
    hb = belief.make_hand_belief(env, "relu", "DeepMind", "relu", "DeepMind", samples=K_E2E, seed=SEED)(nets[0], nets[1], qs, rows=rows, counts=counts)
    torch.cuda.synchronize()
    chains = [_chain(oracle, nets, q, r["hands"]) for q, r in zip(qs, rows)]
    return dict(env=env, nets=nets, queries=qs, belief=hb, rows=rows, chains=chains, counts=counts)


def _check_rows(q, r, chain, K):
    """a query's device rows against its float64 chain -> (largest |logw - float64| over its bound, consistent rows)"""
    logw64, weighed, tol_sum, below, gap = chain
    assert weighed == sum(1 for s, _, _ in q.plan() if s != q.seat)
    if weighed == 0:
        assert not r["logw"].any() and r["greedy"].all()
        return 0.0, K
    bound = 2.0 * tol_sum                                        # (number of weighed calls) x 2 tol, each forward's own tol
    err = np.abs(r["logw"].astype(np.float64) - logw64)
    assert (err <= bound).all(), (float(err.max()), bound)
    cons = r["greedy"] != 0
    w = ~np.isnan(below).all(axis=0)
    assert (below[cons][:, w] <= 2.0).all()                      # every call of a consistent row is a float64 maximum within 2 tol
    bad = ~cons
    assert ((below[bad][:, w] > 0.0) | (gap[bad][:, w] < 2.0)).any(axis=1).all()     # an inconsistent row has a call that is not
    return float(err.max() / bound), int(cons.sum())


def test_every_rows_weight_is_the_float64_chains(e2e):
    from brl_amd import belief
    hb, qs = e2e["belief"], e2e["queries"]
    forwarded = 0
    for i, (q, r, chain) in enumerate(zip(qs, e2e["rows"], e2e["chains"])):
        assert np.array_equal(r["hands"], BR.sample_hands(q.seat, q.hand, SEED, i, np.arange(K_E2E)))
        ratio, cons = _check_rows(q, r, chain, K_E2E)
        forwarded += chain[1] * K_E2E
        worst = BR.compare_entry(hb.entries[i], BR.reduce64(q.seat, r["hands"], r["logw"], r["greedy"]), K_E2E)
        assert hb.consistent[i] == cons and hb.n[i] == K_E2E
        print(f"query {i} ({' '.join(q.label()['calls']) or 'no call'}): weighed calls {chain[1]}, largest |logw - float64| = {ratio:.3f} of "
              f"its bound, consistent {cons}, effective sample size {hb.ess[i]:.1f}, entry within {worst:.1e} relative")
    assert e2e["counts"]["forwarded"] == forwarded == (0 + 3 + 3 + 3 + 3) * K_E2E
    assert isinstance(hb, belief.HandBelief) and hb.seats.tolist() == [[(q.seat + 1 + h) & 3 for h in range(3)] for q in qs]
    assert hb.consistent[1:].sum() >= 100 and (hb.consistent[1:] < K_E2E).all() and (hb.ess[1:] > 1).all()     # not vacuous


def test_without_a_call_the_belief_is_the_unweighted_share(e2e):
    hb = e2e["belief"]
    e = hb.entries[0]
    assert e["consistent"] == e["n"] == K_E2E and e["wsum"] == K_E2E and e["wsq"] == K_E2E and e["max_logw"] == 0
    assert np.array_equal(e["card"], e["g_card"].astype(np.float64)) and np.array_equal(hb.card_prob[0], e["g_card"] / K_E2E)
    hidden = np.array([not (e2e["queries"][0].hand >> b) & 1 for b in range(52)])
    assert (np.abs(hb.card_prob[0][:, hidden] - 1 / 3) <= 5 * np.sqrt(2 / (9 * K_E2E))).all() and not hb.card_prob[0][:, ~hidden].any()


def test_an_opening_bid_moves_the_belief_the_right_way(e2e):
    """Queries 0 and 1 are the same seat and hand: before any call, and after P P 1C P: North opened, East passed.  North's mean HCP —
    soft and greedy — exceeds its mean before the auction by more than 5 standard errors of the difference, East's does not exceed
    its own.  (A sampler that ignores the auction returns the prior twice and fails the first half.)  Standard error of a mean:
    sqrt(variance / effective sample size), from the belief's own HCP histogram, ess, consistent and n."""
    hb = e2e["belief"]
    assert e2e["queries"][0].hand == e2e["queries"][1].hand and hb.seats[1].tolist() == [3, 0, 1]
    pts = np.arange(38)

    def mean_se(hist, size):
        mean = (hist * pts).sum()
        return mean, np.sqrt(((hist * pts * pts).sum() - mean * mean) / size)

    for h, name in ((1, "North, who opened"), (2, "East, who passed")):
        prior, prior_se = mean_se(hb.hcp_hist[0, h], hb.n[0])
        soft, soft_se = mean_se(hb.hcp_hist[1, h], hb.ess[1])
        greedy, greedy_se = mean_se(hb.greedy_hcp_hist[1, h], hb.consistent[1])
        print(f"{name}: HCP before {prior:.2f} +- {prior_se:.2f}, soft {soft:.2f} +- {soft_se:.2f}, greedy {greedy:.2f} +- {greedy_se:.2f}")
        if h == 1:
            assert soft - prior > 5 * np.hypot(soft_se, prior_se) and greedy - prior > 5 * np.hypot(greedy_se, prior_se)
        else:
            assert soft <= prior and greedy <= prior
    # and the suit North opened is longer in its hand than before
    suit = "CDHS".index(e2e["queries"][1].label()["calls"][2][1])
    assert hb.length_mean[1, 1, suit] > hb.length_mean[0, 1, suit] + 0.5 and hb.greedy_length_mean[1, 1, suit] > hb.length_mean[0, 1, suit] + 0.5


def test_the_result_depends_neither_on_the_batches_nor_on_the_grouping(e2e):
    from brl_amd import belief
    env, nets, qs, hb = e2e["env"], e2e["nets"], e2e["queries"], e2e["belief"]
    one_by_one = belief.make_hand_belief(env, "relu", "DeepMind", "relu", "DeepMind", samples=K_E2E, seed=SEED, max_rows=K_E2E)
    assert one_by_one(nets[0], nets[1], qs).same_as(hb)                          # max_rows = K against 2^18: the same bytes
    default = belief.make_hand_belief(env, "relu", "DeepMind", "relu", "DeepMind", samples=K_E2E, seed=SEED)
    first, second = default(nets[0], nets[1], qs[:2]), default(nets[0], nets[1], qs[2:], query_offset=2)
    assert np.concatenate([first.entries, second.entries]).tobytes() == hb.entries.tobytes()
    with pytest.raises(ValueError, match=r"query 1: call 2 \(1C\)"):
        default(nets[0], nets[1], [qs[0], belief.BeliefQuery("S", qs[0].hand, "N", "None", ["1H", "P", "1C"])])
    with pytest.raises(ValueError, match="max_rows"):
        belief.make_hand_belief(env, "relu", "DeepMind", "relu", "DeepMind", samples=64, max_rows=63)


def test_the_small_batch_route(oracle, e2e):
    """query 2 again with 64 samples: forwards of 64 rows, far below the plane route's 4096"""
    from brl_amd import belief
    env, nets, q = e2e["env"], e2e["nets"], e2e["queries"][2]
    rows = []
    hb = belief.make_hand_belief(env, "relu", "DeepMind", "relu", "DeepMind", samples=64, seed=SEED)(nets[0], nets[1], [q], query_offset=2, rows=rows)
    assert np.array_equal(rows[0]["hands"], e2e["rows"][2]["hands"][:64])        # the same stream: the first 64 of the 4096
    ratio, cons = _check_rows(q, rows[0], _chain(oracle, nets, q, rows[0]["hands"]), 64)
    BR.compare_entry(hb.entries[0], BR.reduce64(q.seat, rows[0]["hands"], rows[0]["logw"], rows[0]["greedy"]), 64)
    print(f"64 samples: largest |logw - float64| = {ratio:.3f} of its bound, consistent {cons}")
    assert hb.n[0] == 64 and hb.consistent[0] == cons


def test_one_network_on_both_sides(oracle, e2e, monkeypatch):
    from brl_amd import belief, evaluation
    made = []
    real = evaluation._Forward

    class Counting(real):
        def __init__(self, *a):
            made.append(1)
            super().__init__(*a)

    monkeypatch.setattr(evaluation, "_Forward", Counting)
    env, net, qs = e2e["env"], e2e["nets"][0], e2e["queries"][2:4]
    rows = []
    hb = belief.make_hand_belief(env, "relu", "DeepMind", "relu", "DeepMind", samples=256, seed=SEED)(net, net, qs, rows=rows)
    assert len(made) == 1
    for i, (q, r) in enumerate(zip(qs, rows)):
        _check_rows(q, r, _chain(oracle, (net, net), q, r["hands"]), 256)
        BR.compare_entry(hb.entries[i], BR.reduce64(q.seat, r["hands"], r["logw"], r["greedy"]), 256)
    made.clear()
    belief.make_hand_belief(env, "relu", "DeepMind", "relu", "DeepMind", samples=64)(e2e["nets"][0], e2e["nets"][1], qs[:1])
    assert len(made) == 2


def test_queries_from_a_recorded_match(e2e):
    from brl_amd import belief, boards
    env, nets = e2e["env"], e2e["nets"]
    deals = boards.read_deals(NAMED)
    env24 = type(env)(lut=(deals.lut_keys(), deals.lut_values()), device=DEV)
    _, records = boards.make_board_match(env24, "relu", "DeepMind", "relu", "DeepMind")(nets[0], nets[1], deals)
    rec = records.cpu("b")
    board = int(np.argmax(rec["n_calls"] >= 3))
    r = rec[board]
    (q,) = belief.queries_from_records(records, "b", board, 2)
    seat = (int(r["dealer"]) + 2) & 3
    by_hand = belief.BeliefQuery("NESW"[seat], belief.hand_text(int(deals.hand_words()[board, seat])), "NESW"[int(r["dealer"])],
                                 boards.VULS[int(deals.vul_ns[board]) + 2 * int(deals.vul_ew[board])], records.auction(board, "b")[:2],
                                 [(int(r["seating"]) >> (2 * s)) & 3 for s in range(4)])
    assert q == by_hand and q.plan() == by_hand.plan() and q.seating != records.cpu("a")[board]["seating"]
    hb = belief.make_hand_belief(env24, "relu", "DeepMind", "relu", "DeepMind", samples=128)(nets[0], nets[1], [q, by_hand])
    assert hb.entries[0].tobytes() != hb.entries[1].tobytes() and hb.n.tolist() == [128, 128]      # (two streams: two sets of deals)
    again = belief.make_hand_belief(env24, "relu", "DeepMind", "relu", "DeepMind", samples=128)(nets[0], nets[1], [by_hand], query_offset=1)
    assert again.entries[0].tobytes() == hb.entries[1].tobytes()


def test_the_command_line_prints_a_belief(tmp_path):
    from brl_amd import belief, boards, checkpoint
    from brl_amd.models import make_forward_pass
    fp = make_forward_pass("relu", "DeepMind")
    for k in range(2):
        checkpoint.save_params(fp.init(60 + k), str(tmp_path / f"params-{k:08}.pt"))
    envv = dict(os.environ, PYTHONPATH=ROOT)
    board_id = int(boards.read_deals(NAMED).board_id[3])
    base = [sys.executable, "-m", "brl_amd.eval", f"team1_model_path={tmp_path / 'params-00000000.pt'}",
            f"team2_model_path={tmp_path / 'params-00000001.pt'}", f"deals_path={NAMED}"]
    out = []
    for extra in ([], [f"belief_board={board_id}", "belief_table=b", "belief_call=2", "belief_samples=256", f"save_belief={tmp_path / 'belief.json'}"]):
        r = subprocess.run(base + extra, cwd=tmp_path, env=envv, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        out.append(r.stdout.splitlines())
    plain, with_belief = out
    start = [i for i, ln in enumerate(with_belief) if ln.startswith("belief 0: ")]
    assert len(start) == 1 and start[0] == [i for i, ln in enumerate(with_belief) if ln.startswith("IMP: ")][-1] + 1
    assert with_belief[:start[0]] == plain and not any(ln.startswith("belief") for ln in plain)
    back = belief.HandBelief.from_json(tmp_path / "belief.json")
    assert with_belief[start[0]:] == back.to_text(0).split("\n") + [f"belief: {tmp_path / 'belief.json'}"]
    assert len(back) == 1 and back.n[0] == 256 and len(back.queries[0]["calls"]) == 2
