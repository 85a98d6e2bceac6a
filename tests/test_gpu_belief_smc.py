"""-m gpu: the resample-move stages of the hand beliefs (include/brl_belief_smc.h) — brl_belief_resample, brl_belief_propose and
brl_belief_accept against their numpy restatement (tests/belief_smc_ref.py), and whole beliefs of the bidder pair with
``resample_every`` set: the plain path's bytes where nothing is scheduled, every final particle's bookkeeping against the float64
chain, the prior left invariant by the moves, agreement with plain importance sampling at 2^18 samples, batching, the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import belief_ref as BR
from tests import belief_smc_ref as SR
from tests import bidder_net as bn
from tests import book_ref as B
from tests.test_gpu_belief import NAMED, ROOT, SEATINGS, SEED, _chain, _check_rows, _dev, _queries

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(1, 1), (1, 64), (3, 257), (2, 4096)]
DECK = (1 << 52) - 1
SENTINEL = 0x5A


def _listed(Q):
    """the launch's list: in no order, and with Q > 1 one query left out"""
    return {1: [0], 2: [1], 3: [2, 0]}[Q]


def _stream_of(Q):
    return np.arange(Q, dtype=np.int64) * 3 + 5          # (stream indices that are not the positions)


# ---- resample ----------------------------------------------------------------------------------------------------------------------
def _eps(K):
    """The relative tolerance of a cumulative sum and of a threshold between the device and the float64 restatement.  Both form
    the same K - 1 additions in the same order, so they differ only through their inputs and the roundings those move:
      * W_k = exp(.): the device's exp and numpy's are each within 2 ulp of the true value: 4 x 2^-52 relative between them;
      * C_k: at most K - 1 additions of non-negative terms, each rounding 2^-53 relative of a partial sum that is at most the
        result, on either side: (K - 1) x 2^-52 between them;
      * x_j = ((j + u) S) / K: S is a C, and two more roundings on either side: 2 x 2^-52.
    C against x therefore moves by at most (4 + (K - 1) + 4 + (K - 1) + 2) x 2^-52 < (K + 6) x 2^-51 relative."""
    return (K + 6) * 2.0 ** -51


WEIGHTS = ("random", "equal", "dominant", "apart", "nan", "none")


def _logw(kind, Q, K, rng):
    lw = (rng.normal(size=(Q, K)) * 3 - 5).astype(np.float32)
    if kind == "equal":
        lw[:] = np.float32(-7.25)
    elif kind == "dominant":
        lw[:] = -2000.0                                    # exp(-1997) is 0 in float64
        lw[np.arange(Q), np.arange(Q) * 7 % K] = -3.0
    elif kind == "apart":
        lw -= (40 * (np.arange(K) % 2)).astype(np.float32)[None, :]
    elif kind == "nan":
        lw[:, K // 2] = np.nan
    elif kind == "none":
        lw[:] = -np.inf
    return lw


@pytest.mark.parametrize("Q,K", SHAPES)
def test_resample_draws_ancestors_of_the_float64_accept_set(Q, K):
    """K = 1, one segment, segments and a part (257), one whole tile of 4096; six weight sets each: random, equal (the identity,
    exactly), one dominant particle, weights e^-40 apart, a NaN row and no weight at all (both left as they are)"""
    from brl_amd import belief
    rng = np.random.default_rng(100 + K)
    n, stage = Q * K, 9
    listed, stream_of = _listed(Q), _stream_of(Q)
    tables = rng.integers(-2 ** 62, 2 ** 62, size=(n, 16), dtype=np.int64)
    hands = rng.integers(0, 2 ** 62, size=(n, 4), dtype=np.int64)
    logl = rng.normal(size=n).astype(np.float32)
    greedy = (rng.random(n) < 0.5).astype(np.uint8)
    eps = _eps(K)
    worst = 0.0
    for kind in WEIGHTS:
        logw = _logw(kind, Q, K, rng)
        args = (_dev(np.array(listed, np.int32)), _dev(stream_of), K, SEED, stage, _dev(tables), _dev(hands), _dev(logl), _dev(logw.reshape(-1)),
                _dev(greedy))
        # (belief.resample allocates its outputs: an unlisted query's rows are checked in the next test, on buffers filled beforehand)
        got = [x.cpu().numpy() for x in belief.resample(*args)]
        again = [x.cpu().numpy() for x in belief.resample(*args)]
        t2, h2, ll2, lw2, g2, anc = got
        for i in listed:
            rows = slice(i * K, (i + 1) * K)
            a = anc[rows].astype(np.int64)
            assert a.min() >= 0 and a.max() < K and (np.diff(a) >= 0).all(), (kind, i)
            want, C, x = SR.resample(logw[i], SR.offset_u(SEED, int(stream_of[i]), stage))
            if kind in ("nan", "none"):
                assert want is None and np.array_equal(a, np.arange(K))
                assert lw2[rows].tobytes() == logw[i].tobytes()                       # logw kept, NaN included
            else:
                assert not lw2[rows].any() and not np.signbit(lw2[rows]).any()         # +0.0
                below = np.where(a > 0, C[np.maximum(a - 1, 0)], 0.0)
                assert (below * (1 - eps) <= x).all() and (x <= C[a] * (1 + eps)).all(), (kind, i)
                share = K * np.exp(logw[i].astype(np.float64) - logw[i].max()) / C[-1]
                count = np.bincount(a, minlength=K)
                delta = 2 * eps * K
                assert (np.floor(share - delta) <= count).all() and (count <= np.ceil(share + delta)).all(), (kind, i)
                worst = max(worst, float(np.abs(a - want).max()))
                if kind == "equal":
                    assert np.array_equal(a, np.arange(K))
                if kind == "dominant":
                    assert (a == i * 7 % K).all()
            src = i * K + a
            assert np.array_equal(t2[rows], tables[src]) and np.array_equal(h2[rows], hands[src])
            assert np.array_equal(ll2[rows], logl[src]) and np.array_equal(g2[rows], greedy[src])
        for x, y in zip(got, again):                                                 # the same bytes on a second run
            for i in listed:
                assert x[i * K:(i + 1) * K].tobytes() == y[i * K:(i + 1) * K].tobytes()
    print(f"resample Q={Q} K={K}: eps = {eps:.2e}; the largest distance of an ancestor from the restatement's own: {worst:.0f}")


def test_resample_leaves_an_unlisted_query_alone():
    """outputs filled beforehand, through the C call itself: only the listed queries' rows change; a list entry out of range is skipped"""
    from brl_amd import _capi
    Q, K = 3, 257
    rng = np.random.default_rng(7)
    n = Q * K
    ins = [_dev(rng.integers(0, 2 ** 62, size=(n, 16), dtype=np.int64)), _dev(rng.integers(0, 2 ** 62, size=(n, 4), dtype=np.int64)),
           _dev(rng.normal(size=n).astype(np.float32)), _dev(rng.normal(size=n).astype(np.float32)), _dev((rng.random(n) < 0.5).astype(np.uint8))]
    outs = [torch.full_like(x.view(torch.uint8), SENTINEL) for x in ins] + [torch.full((n * 4,), SENTINEL, dtype=torch.uint8, device=DEV)]
    qlist, stream_of = _dev(np.array([2, 7, -1, 0], np.int32)), _dev(_stream_of(Q))
    _capi.check(_capi.lib().brl_belief_resample(0, _capi.ptr(qlist), 4, _capi.ptr(stream_of), Q, K, SEED, 3, *[_capi.ptr(x) for x in ins],
                                                *[_capi.ptr(x) for x in outs], _capi.stream(0)))
    for x in outs:
        b = x.cpu().numpy().reshape(Q, -1)
        assert (b[1] == SENTINEL).all() and not (b[0] == SENTINEL).all() and not (b[2] == SENTINEL).all()
    with pytest.raises(_capi.BrlError, match="out of place"):
        _capi.check(_capi.lib().brl_belief_resample(0, _capi.ptr(qlist), 4, _capi.ptr(stream_of), Q, K, SEED, 3, *[_capi.ptr(x) for x in ins],
                                                    *[_capi.ptr(x) for x in ins], _capi.ptr(outs[-1]), _capi.stream(0)))


def test_resample_beyond_one_tile():
    """K = 9000: three tiles of 4096, the outputs handed from tile to tile; ancestors against the restatement as above"""
    from brl_amd import belief
    K, stage = 9000, 2
    rng = np.random.default_rng(11)
    logw = (rng.normal(size=K) * 4).astype(np.float32)
    logw[3000:7000] -= 30.0                                  # a stretch that hardly counts: a tile that receives few outputs
    tables = rng.integers(0, 2 ** 62, size=(K, 16), dtype=np.int64)
    hands = rng.integers(0, 2 ** 62, size=(K, 4), dtype=np.int64)
    got = belief.resample(_dev(np.array([0], np.int32)), _dev(np.array([4], np.int64)), K, SEED, stage, _dev(tables), _dev(hands),
                          _dev(logw), _dev(logw), _dev(np.ones(K, np.uint8)))
    a = got[5].cpu().numpy().astype(np.int64)
    want, C, x = SR.resample(logw, SR.offset_u(SEED, 4, stage))
    eps = _eps(K)
    below = np.where(a > 0, C[np.maximum(a - 1, 0)], 0.0)
    assert (np.diff(a) >= 0).all() and (below * (1 - eps) <= x).all() and (x <= C[a] * (1 + eps)).all()
    print(f"resample K={K}: ancestors that are not the restatement's own: {int((a != want).sum())}")
    assert len(set((a // 4096).tolist())) == 3
    assert np.array_equal(got[0].cpu().numpy(), tables[a]) and np.array_equal(got[1].cpu().numpy(), hands[a])
    assert np.array_equal(got[2].cpu().numpy(), logw[a]) and not got[3].cpu().numpy().any()


# ---- propose -----------------------------------------------------------------------------------------------------------------------
def _smc_queries(Q, K):
    """over the four shapes: every own seat, an own hand with a void and one with a 13-card suit"""
    from brl_amd import belief
    rng = np.random.default_rng(40 + K)
    own = {1: [B.random_hands(rng)[0]], 64: [B.shaped_hand([0, 0, 13, 0])], 257: [B.shaped_hand([0, 4, 4, 5], top=False), B.random_hands(rng)[0],
           B.shaped_hand([0, 0, 13, 0])], 4096: [B.random_hands(rng)[0], B.shaped_hand([0, 4, 4, 5], top=False)]}[K]
    first = {1: 1, 64: 2, 257: 0, 4096: 3}[K]
    return [belief.BeliefQuery((first + i) & 3, own[i], (i + K) & 3, ((i + K) & 1, (i >> 1) & 1), [], SEATINGS[(i + K) & 3]) for i in range(Q)]


def test_the_propose_shapes_cover_every_seat_a_void_and_a_long_suit():
    qs = [q for Q, K in SHAPES for q in _smc_queries(Q, K)]
    lengths = [BR.features(np.uint64(q.hand))[2].tolist() for q in qs]
    assert {q.seat for q in qs} == {0, 1, 2, 3} and any(13 in x for x in lengths) and any(0 in x and 13 not in x for x in lengths)


@pytest.mark.parametrize("Q,K", SHAPES)
def test_propose_equals_the_restatement_bit_for_bit(Q, K):
    from brl_amd import belief
    qs = _smc_queries(Q, K)
    listed, stream_of = _listed(Q), _stream_of(Q)
    L, stage, move = len(listed), 300, 255                   # (the largest stage of a 319-call auction's kind, the last move)
    qdev = _dev(belief.query_array(qs).view(np.uint8).reshape(Q, 16))
    hands = torch.cat([belief.deal(qdev[i:i + 1], K, SEED, int(stream_of[i]))[1] for i in range(Q)])
    t_new = torch.full(((L + 1) * K, 16), SENTINEL, dtype=torch.int64, device=DEV)
    h_new = torch.full(((L + 1) * K, 4), SENTINEL, dtype=torch.int64, device=DEV)
    args = (qdev, _dev(np.array(listed, np.int32)), _dev(stream_of), K, SEED, stage, move, hands)
    cur = hands.cpu().numpy().view(np.uint64).copy()
    belief.propose(*args, t_new, h_new)
    t, h = t_new.cpu().numpy().view(np.uint64), h_new.cpu().numpy().view(np.uint64)
    for p, i in enumerate(listed):
        q = qs[i]
        want, pick, _ = SR.propose(q.seat, cur[i * K:(i + 1) * K], SEED, int(stream_of[i]), stage, move)
        assert np.array_equal(h[p * K:(p + 1) * K], want), (p, i)
        assert np.array_equal(t[p * K:(p + 1) * K], BR.sample_tables(q.dealer, q.vul_ns, q.vul_ew, q.seating, want)), (p, i)
        assert (want[:, q.seat] == np.uint64(q.hand)).all() and (np.bitwise_or.reduce(want, axis=1) == np.uint64(DECK)).all()
        assert (want != cur[i * K:(i + 1) * K]).sum(axis=1).tolist() == [2] * K
    assert (t[L * K:] == np.uint64(SENTINEL)).all() and (h[L * K:] == np.uint64(SENTINEL)).all()      # nothing behind the list's rows
    t_again, h_again = torch.empty_like(t_new), torch.empty_like(h_new)
    belief.propose(*args, t_again, h_again)
    assert torch.equal(t_again[:L * K], t_new[:L * K]) and torch.equal(h_again[:L * K], h_new[:L * K])
    assert torch.equal(hands.cpu(), torch.from_numpy(cur.view(np.int64)))                                  # the particles are only read


# ---- accept ------------------------------------------------------------------------------------------------------------------------
BAND = 8 * 2.0 ** -52 * 32
"""log v, v = (w3 + 0.5) 2^-32 in [2^-33, 1): |log v| < 23 < 32, and the device's log and numpy's are each within 2 ulp of the true
value: 4 ulp of a number below 32 between them, doubled.  logl_new - logl of two float32 values is exact in float64."""


@pytest.mark.parametrize("Q,K", SHAPES)
def test_accept_against_float64(Q, K):
    from brl_amd import belief
    rng = np.random.default_rng(300 + K)
    n, listed, stream_of = Q * K, _listed(Q), _stream_of(Q)
    L, stage = len(listed), 6
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    tables = rng.integers(0, 2 ** 62, size=(n, 16), dtype=np.int64)
    hands = rng.integers(0, 2 ** 62, size=(n, 4), dtype=np.int64)
    greedy = (rng.random(n) < 0.5).astype(np.uint8)
    logl = rng.uniform(-20, 0, size=n).astype(np.float32)
    t_new = rng.integers(0, 2 ** 62, size=(L * K, 16), dtype=np.int64)
    h_new = rng.integers(0, 2 ** 62, size=(L * K, 4), dtype=np.int64)
    g_new = (rng.random(L * K) < 0.5).astype(np.uint8)
    ll_new = np.zeros(L * K, np.float32)
    kinds = np.zeros(L * K, np.int64)
    for p, i in enumerate(listed):
        for k in range(K):
            kind = (k + p) % 8 if K > 1 else 0
            r, c = i * K + k, p * K + k
            kinds[c] = kind
            if kind == 0:
                ll_new[c] = logl[r] + np.float32(rng.uniform(0.01, 5))          # +: always taken
            elif kind in (1, 2):
                ll_new[c] = logl[r] - np.float32(rng.uniform(0.01, 5))          # -: taken by the draw
            elif kind == 3:
                ll_new[c] = logl[r]                                             # equal: always taken (log v < 0)
            elif kind == 4:
                ll_new[c] = nan
            elif kind == 5:
                logl[r], ll_new[c] = nan, np.float32(-1.0)
            elif kind == 6:
                logl[r], ll_new[c] = -inf, np.float32(-3.0)                     # -inf to finite: taken
            else:
                ll_new[c] = -inf                                                # and back: never
    counters = torch.zeros((Q, 2), dtype=torch.int64, device=DEV)
    state = [_dev(tables), _dev(hands), _dev(logl), _dev(greedy)]
    taken_total = np.zeros(Q, np.int64)
    for move in (0, 1):                                      # the second move on what the first left: the counters add up
        cur = [x.cpu().numpy().copy() for x in state]
        want = np.zeros(L * K, bool)
        for p, i in enumerate(listed):
            w3 = SR.move_words(SEED, int(stream_of[i]), stage, move, np.arange(K))[3]
            d = ll_new[p * K:(p + 1) * K].astype(np.float64) - cur[2][i * K:(i + 1) * K].astype(np.float64)
            with np.errstate(invalid="ignore"):
                finite = np.isfinite(d)
                assert (np.abs(np.log(SR.unit(w3))[finite] - d[finite]) > BAND).all()          # no case within the band of log v
            want[p * K:(p + 1) * K] = SR.accept(w3, cur[2][i * K:(i + 1) * K], ll_new[p * K:(p + 1) * K])
            taken_total[i] += want[p * K:(p + 1) * K].sum()
        belief.accept(_dev(np.array(listed, np.int32)), _dev(stream_of), K, SEED, stage, move, _dev(t_new), _dev(h_new), _dev(ll_new), _dev(g_new),
                      *state, counters)
        got = [x.cpu().numpy() for x in state]
        for p, i in enumerate(listed):
            rows, comp, w = slice(i * K, (i + 1) * K), slice(p * K, (p + 1) * K), want[p * K:(p + 1) * K]
            for g, c, new in zip(got, cur, (t_new, h_new, ll_new, g_new)):
                expect = np.where(w.reshape((K,) + (1,) * (c.ndim - 1)), new[comp], c[rows])
                assert expect.tobytes() == g[rows].tobytes(), (move, p, i)
            if move == 0 and K > 8:
                k8 = kinds[comp]
                assert w[(k8 == 0) | (k8 == 3) | (k8 == 6)].all() and not w[(k8 == 4) | (k8 == 5) | (k8 == 7)].any()
                assert 0 < w[(k8 == 1) | (k8 == 2)].sum() < ((k8 == 1) | (k8 == 2)).sum() or K < 100
        for i in set(range(Q)) - set(listed):
            for g, c in zip(got, cur):
                assert g[i * K:(i + 1) * K].tobytes() == c[i * K:(i + 1) * K].tobytes()
    c = counters.cpu().numpy()
    for i in range(Q):
        assert c[i].tolist() == ([2 * K, int(taken_total[i])] if i in listed else [0, 0]), i


# ---- end to end --------------------------------------------------------------------------------------------------------------------
K_E2E = 4096
NET = ("relu", "DeepMind", "relu", "DeepMind")


@pytest.fixture(scope="module")
def world(dds):
    import brl_amd
    from brl_amd import belief
    nets = bn.pair(DEV)
    env = brl_amd.BridgeBidding(lut=(dds["keys"], dds["values"]), device=DEV)
    qs = _queries()
    plain = belief.make_hand_belief(env, *NET, samples=K_E2E, seed=SEED)(nets[0], nets[1], qs)
    rows, counts = [], {}
    smc = belief.make_hand_belief(env, *NET, samples=K_E2E, seed=SEED, resample_every=1, moves=2)(nets[0], nets[1], qs, rows=rows, counts=counts)
    return dict(env=env, nets=nets, queries=qs, plain=plain, smc=smc, rows=rows, counts=counts)


def test_without_the_new_arguments_the_belief_is_todays(world):
    from brl_amd import belief
    env, nets, qs = world["env"], world["nets"], world["queries"]
    zero = belief.make_hand_belief(env, *NET, samples=K_E2E, seed=SEED, resample_every=0, moves=5)(nets[0], nets[1], qs)
    assert zero.same_as(world["plain"]) and zero.resamples is None and world["plain"].distinct is None
    with pytest.raises(ValueError, match="resample_every"):
        belief.make_hand_belief(env, *NET, resample_every=-1)
    with pytest.raises(ValueError, match="moves"):
        belief.make_hand_belief(env, *NET, resample_every=1, moves=257)


def test_where_nothing_is_scheduled_the_bytes_are_the_plain_ones(world):
    """a query without a call, one whose only call is its own, and resample_every beyond the hidden calls of the others"""
    from brl_amd import belief
    env, nets, qs = world["env"], world["nets"], world["queries"]
    own_call = belief.BeliefQuery("S", qs[0].hand, "S", "EW", ["P"])
    some = [qs[0], own_call]
    plain = belief.make_hand_belief(env, *NET, samples=K_E2E, seed=SEED)(nets[0], nets[1], some)
    smc = belief.make_hand_belief(env, *NET, samples=K_E2E, seed=SEED, resample_every=1)(nets[0], nets[1], some)
    assert smc.same_as(plain) and smc.resamples.tolist() == [0, 0] and smc.proposals.tolist() == [0, 0] and smc.distinct.tolist() == [K_E2E] * 2
    rows = []
    late = belief.make_hand_belief(env, *NET, samples=K_E2E, seed=SEED, resample_every=4)(nets[0], nets[1], qs, rows=rows)
    assert late.same_as(world["plain"]) and not late.resamples.any()
    assert all(np.array_equal(r["logl"], r["logw"]) for r in rows)           # logl is the same total where nothing resampled
    assert world["smc"].resamples.tolist() == [0, 3, 3, 3, 3]


def test_every_final_particle_keeps_its_books(world, oracle):
    """hands, logl and greedy of the final particles went through resamplings' gathers and moves' select-and-copy: every particle
    still holds the own hand and a partition of the deck, its logl is the float64 chain of ITS FINAL hands on the CPU oracle's
    observations (within the bound test_gpu_belief.py uses for logw: 2 tol per weighed call), its greedy flag the float64 arg-max's,
    and the entries are the restatement's reduction of the device's final rows"""
    hb, qs = world["smc"], world["queries"]
    forwarded = 0
    for i, (q, r) in enumerate(zip(qs, world["rows"])):
        assert (r["hands"][:, q.seat] == np.uint64(q.hand)).all() and (np.bitwise_or.reduce(r["hands"], axis=1) == np.uint64(DECK)).all()
        assert all(bin(int(x)).count("1") == 13 for x in r["hands"][::37].reshape(-1))
        chain = _chain(oracle, world["nets"], q, r["hands"])
        ratio, cons = _check_rows(q, {"logw": r["logl"], "greedy": r["greedy"]}, chain, K_E2E)
        worst = BR.compare_entry(hb.entries[i], BR.reduce64(q.seat, r["hands"], r["logw"], r["greedy"]), K_E2E)
        assert hb.consistent[i] == cons and hb.distinct[i] == len(np.unique(r["hands"], axis=0))
        assert hb.proposals[i] == 2 * K_E2E * hb.resamples[i] and 0 <= hb.accepted[i] <= hb.proposals[i]
        if hb.resamples[i]:
            assert not r["logw"].any() and hb.ess[i] == K_E2E                  # the last weighed call was followed by a resampling
            assert 0 < hb.accepted[i] < hb.proposals[i] and 1 < hb.distinct[i] <= K_E2E
        w = chain[1]
        forwarded += (w + 2 * w * (w + 1) // 2) * K_E2E                          # the live pass, and per move the replays of 1..w calls
        print(f"query {i}: resamplings {hb.resamples[i]}, moves taken {hb.accepted[i]} of {hb.proposals[i]}, distinct {hb.distinct[i]} "
              f"(plain: effective {world['plain'].ess[i]:.0f}), consistent {cons}, largest |logl - float64| = {ratio:.3f} of its bound, "
              f"entry within {worst:.1e}")
    assert world["counts"]["forwarded"] == forwarded


def _zero_net():
    from brl_amd.models import ActorCritic
    net = ActorCritic(38, "relu", "DeepMind")
    with torch.no_grad():
        for p in net.parameters():
            p.zero_()
    return net.to(DEV)


def test_the_moves_leave_the_prior_invariant(world):
    """A network whose logits are constant: every call has the same probability on every deal, so the posterior is the prior,
    every proposal is taken, and after three resamplings with two moves each the particles must still be uniform deals: the largest
    deviation of a card's share from 1/3 inside 4 sigma, sigma = sqrt(2 / 9K) as in test_belief_host.py.  (A move that drops or
    duplicates a card, or that prefers a seat, fails this; so does the code without the feature.)"""
    from brl_amd import belief
    q = world["queries"][1]
    net = _zero_net()
    rows = []
    hb = belief.make_hand_belief(world["env"], *NET, samples=K_E2E, seed=SEED, resample_every=1, moves=2)(net, net, [q], rows=rows)
    assert hb.resamples[0] == 3 and hb.proposals[0] == 3 * 2 * K_E2E and hb.accepted[0] == hb.proposals[0]
    start = BR.sample_hands(q.seat, q.hand, SEED, 0, np.arange(K_E2E))
    assert (rows[0]["hands"] != start).any(axis=1).mean() > 0.9                   # the particles did move
    assert (np.bitwise_or.reduce(rows[0]["hands"], axis=1) == np.uint64(DECK)).all()
    hidden = np.array([not (q.hand >> b) & 1 for b in range(52)])
    sigma = np.sqrt(2.0 / (9.0 * K_E2E))
    dev = np.abs(hb.card_prob[0][:, hidden] - 1.0 / 3.0).max() / sigma
    print(f"constant logits: largest deviation of a card's share from 1/3 after 6 moves: {dev:.2f} sigma")
    assert dev <= 4.0 and not hb.card_prob[0][:, ~hidden].any() and hb.distinct[0] > 0.99 * K_E2E


def test_agreement_with_plain_importance_sampling_at_2_to_the_18(world):
    """P P 1C P: the three hidden seats' mean HCP from 4096 particles (resample_every 1, moves 2) over 8 seeds against plain
    importance sampling with 2^18 deals, whose own effective sample size must exceed 10^4.  Margin: 4 standard errors — the
    across-seed one of the eight runs' mean combined with the reference's sqrt(variance / effective sample size).  And §15's
    direction: North, who opened, is stronger than before the auction, East, who passed, is not."""
    from brl_amd import belief
    env, nets, q = world["env"], world["nets"], world["queries"][1]
    ref = belief.make_hand_belief(env, *NET, samples=1 << 18, seed=SEED)(nets[0], nets[1], [q])
    assert ref.ess[0] > 1e4, f"the reference is unusable: effective sample size {ref.ess[0]:.0f}"
    pts = np.arange(38)
    ref_mean = ref.hcp_mean[0]
    ref_se = np.sqrt(((ref.hcp_hist[0] * pts * pts).sum(-1) - ref_mean ** 2) / ref.ess[0])
    runs = [belief.make_hand_belief(env, *NET, samples=K_E2E, seed=s, resample_every=1, moves=2)(nets[0], nets[1], [q]) for s in range(8)]
    means = np.array([hb.hcp_mean[0] for hb in runs])                      # [8, 3]
    mean, se = means.mean(0), means.std(0, ddof=1) / np.sqrt(8)
    margin = 4 * np.hypot(se, ref_se)
    for h, name in enumerate(("West", "North", "East")):
        print(f"{name}: HCP {mean[h]:.3f} +- {se[h]:.3f} over 8 seeds, reference {ref_mean[h]:.3f} +- {ref_se[h]:.3f} "
              f"(effective {ref.ess[0]:.0f}): difference {mean[h] - ref_mean[h]:+.3f}, margin {margin[h]:.3f}")
    assert ref.seats[0].tolist() == [3, 0, 1] and (np.abs(mean - ref_mean) <= margin).all()
    prior = world["plain"]
    p_mean = prior.hcp_mean[0]
    p_se = np.sqrt(((prior.hcp_hist[0] * pts * pts).sum(-1) - p_mean ** 2) / prior.n[0])
    greedy = np.array([hb.greedy_hcp_mean[0] for hb in runs])
    g_mean, g_se = greedy.mean(0), greedy.std(0, ddof=1) / np.sqrt(8)
    assert mean[1] - p_mean[1] > 5 * np.hypot(se[1], p_se[1]) and g_mean[1] - p_mean[1] > 5 * np.hypot(g_se[1], p_se[1])
    assert mean[2] <= p_mean[2] and g_mean[2] <= p_mean[2]


def test_the_result_depends_neither_on_the_batches_nor_on_the_grouping(world):
    from brl_amd import belief
    env, nets, qs, hb = world["env"], world["nets"], world["queries"], world["smc"]

    def same(a, b):
        return a.same_as(b) and all(np.array_equal(getattr(a, name), getattr(b, name)) for name in belief.SMC_FIELDS)

    kw = dict(samples=K_E2E, seed=SEED, resample_every=1, moves=2)
    default = belief.make_hand_belief(env, *NET, **kw)
    assert same(default(nets[0], nets[1], qs), hb)                                         # a second call
    assert same(belief.make_hand_belief(env, *NET, max_rows=K_E2E, **kw)(nets[0], nets[1], qs), hb)      # max_rows = K against 2^18
    first, second = default(nets[0], nets[1], qs[:2]), default(nets[0], nets[1], qs[2:], query_offset=2)
    assert np.concatenate([first.entries, second.entries]).tobytes() == hb.entries.tobytes()
    assert np.concatenate([first.accepted, second.accepted]).tolist() == hb.accepted.tolist()
    assert np.concatenate([first.distinct, second.distinct]).tolist() == hb.distinct.tolist()
    assert not hb.same_as(world["plain"])


def test_the_command_line_resamples(tmp_path):
    from brl_amd import belief, boards, checkpoint
    from brl_amd.models import make_forward_pass
    fp = make_forward_pass("relu", "DeepMind")
    for k in range(2):
        checkpoint.save_params(fp.init(60 + k), str(tmp_path / f"params-{k:08}.pt"))
    envv = dict(os.environ, PYTHONPATH=ROOT)
    board_id = int(boards.read_deals(NAMED).board_id[3])
    base = [sys.executable, "-m", "brl_amd.eval", f"team1_model_path={tmp_path / 'params-00000000.pt'}",
            f"team2_model_path={tmp_path / 'params-00000001.pt'}", f"deals_path={NAMED}", f"belief_board={board_id}", "belief_table=b",
            "belief_call=3", "belief_samples=256"]
    out = []
    for extra in ([], ["belief_resample=1", "belief_moves=2", f"save_belief={tmp_path / 'belief.json'}"]):
        r = subprocess.run(base + extra, cwd=tmp_path, env=envv, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        out.append(r.stdout.splitlines())
    plain, smc = out
    start = [i for i, ln in enumerate(smc) if ln.startswith("belief 0: ")]
    assert len(start) == 1 and start[0] == [i for i, ln in enumerate(smc) if ln.startswith("IMP: ")][-1] + 1
    assert smc[:start[0] + 1] == plain[:start[0] + 1]                             # the old lines, and the belief's first one
    assert "consistent with the greedy policy" in plain[start[0] + 1] and "greedy among soft particles" in smc[start[0] + 1]
    back = belief.HandBelief.from_json(tmp_path / "belief.json")
    assert smc[start[0]:] == back.to_text(0).split("\n") + [f"belief: {tmp_path / 'belief.json'}"]
    assert back.n[0] == 256 and back.resamples[0] >= 2 and back.proposals[0] == 2 * 256 * back.resamples[0]
