"""The 231 counters of ``brl_eval_reduce`` restated in numpy, and skewed synthetic tables to feed both (a helper: no tests in here).

``eval_counts_ref`` is written from the layout comment above ``k_eval_reduce`` (brl_amd/csrc/brl_eval.hip) and from
``oracle/eval_stats.terminated_log`` (the reference's make_terminated_log / make_contract_log), not from the kernel body:

    table tb (0 = A, 1 = B) at 80 * tb:  +0 pass-outs, +1 / +2 doubled / redoubled contracts of team 1, +3 / +4 of team 2,
        +5 / +6 "make" of team 1 / team 2, +7 / +8 "down", +9 the sum of rewards[:, 0], +10 .. +44 team 1's contracts by bid,
        +45 .. +79 team 2's
    160 + 35 * team + bid: the sum of bid_count over the boards;  230: the sum of the final states' step counts

Everything is integers: the sums are taken over Python ints, so nothing can wrap or round."""
from __future__ import annotations

import numpy as np

from oracle.eval_stats import terminated_log

EV_TABLE, EV_BIDS, EV_STEPS, EV_TOTAL = 80, 160, 230, 231
SCALARS = ("pass_out", "actor_doubled", "actor_redoubled", "opp_doubled", "opp_redoubled", "actor_make", "opp_make", "actor_down",
           "opp_down")          # offsets +0 .. +8, in the order of the layout comment


def _isum(a) -> int:
    return sum(int(v) for v in np.asarray(a).reshape(-1).tolist())


def eval_counts_ref(A, B=None, bid_count=None, step_count=None):
    """A, B: finished tables (anything indexable by "last_bid", "last_bidder", "call_x", "call_xx" and "rewards" [n, 4]); bid_count
    [n, 2, 35] and step_count [n] integers, or None -> int64 [231]"""
    out = [0] * EV_TOTAL
    for tb, T in enumerate((A, B)):
        if T is None:
            continue
        base = tb * EV_TABLE
        r0 = np.asarray(T["rewards"])[:, 0]
        assert (r0 == np.trunc(r0)).all()                       # scores and IMPs are integers
        t = terminated_log(np.asarray(T["last_bid"]), np.asarray(T["last_bidder"]), np.asarray(T["call_x"]), np.asarray(T["call_xx"]), r0)
        for k, name in enumerate(SCALARS):
            out[base + k] = _isum(t[name])
        out[base + 9] = _isum(r0.astype(np.int64))
        for team, name in enumerate(("actor_contract", "opp_contract")):
            for b in range(35):
                out[base + 10 + 35 * team + b] = _isum(t[name][:, b].astype(np.int64))
    if bid_count is not None:
        bc = np.asarray(bid_count)
        assert bc.dtype.kind in "iu" and bc.shape[1:] == (2, 35)
        for team in range(2):
            for b in range(35):
                out[EV_BIDS + 35 * team + b] = _isum(bc[:, team, b])
    if step_count is not None:
        assert np.asarray(step_count).dtype.kind in "iu"
        out[EV_STEPS] = _isum(step_count)
    assert all(-2 ** 63 <= v < 2 ** 63 for v in out)
    return np.array(out, np.int64)


def exchange_pairs(two_tables=True):
    """the pairs of counters that a mix-up of team, table, x / xx, make / down or of neighbouring bids would exchange"""
    pairs = []
    for tb in range(2 if two_tables else 1):
        base = tb * EV_TABLE
        pairs += [(base + 1, base + 3), (base + 2, base + 4), (base + 5, base + 6), (base + 7, base + 8)]      # team 1 <-> team 2
        pairs += [(base + 10 + b, base + 45 + b) for b in range(35)]
        pairs += [(base + 1, base + 2), (base + 3, base + 4)]                                                    # x <-> xx
        pairs += [(base + 5, base + 7), (base + 6, base + 8)]                                                    # make <-> down
    pairs += [(EV_BIDS + b, EV_BIDS + 35 + b) for b in range(35)]
    if two_tables:
        pairs += [(i, EV_TABLE + i) for i in range(EV_TABLE)]                                                    # table A <-> table B
    hists = [tb * EV_TABLE + 10 + 35 * team for tb in range(2 if two_tables else 1) for team in range(2)] + [EV_BIDS, EV_BIDS + 35]
    for h in hists:                                                                                              # bid b <-> b + 1, b + 5
        pairs += [(h + b, h + b + 1) for b in range(34)] + [(h + b, h + b + 5) for b in range(30)]
    return pairs


def equal_exchange_pairs(counts, two_tables=True):
    return [(i, j) for i, j in exchange_pairs(two_tables) if counts[i] == counts[j]]


def synthetic_table(n, seed, table):
    """One finished table of n boards, deliberately skewed: every (table, team, bid) has its own weight, the teams differ in how
    often they declare, are doubled, redoubled and go down; about 3 % pass-outs coded (-1, -1); rewards[:, 0] integers in
    +-7600 with +0.0 and -0.0 on played contracts; the other reward columns hold numbers nothing should read."""
    rng = np.random.default_rng([seed, table, 77])
    team = (rng.random(n) < (0.37, 0.58)[table]).astype(np.int64)
    w = rng.gamma(0.6, size=(2, 35)) + 0.02 + 0.5 * ((np.arange(35) * (3 + 4 * table) + 11 * np.arange(2)[:, None]) % 7 == 0)
    w /= w.sum(1, keepdims=True)
    last_bid = np.where(team == 0, rng.choice(35, n, p=w[0]), rng.choice(35, n, p=w[1])).astype(np.int32)
    last_bidder = (2 * team + (rng.random(n) < (0.3, 0.8)[table])).astype(np.int32)
    pass_out = rng.random(n) < 0.03
    if n >= 64:
        pass_out[5 + table] = True
    last_bid[pass_out], last_bidder[pass_out] = -1, -1
    px = np.where(team == 0, (0.31, 0.12)[table], (0.52, 0.27)[table])
    pxx =np.where(team == 0, (0.09, 0.21)[table], (0.33, 0.16)[table])
    call_x = (rng.random(n) < px).astype(np.uint8)
    call_xx = (rng.random(n) < pxx).astype(np.uint8)
    down = rng.random(n) < np.where(team == 0, (0.28, 0.41)[table], (0.66, 0.55)[table])
    r0 = rng.integers(1, 7601, n).astype(np.float32) * np.where(down, -1, 1).astype(np.float32)
    z = rng.random(n)
    r0[z < 0.03] = np.float32(0.0)
    r0[(z >= 0.03) & (z < 0.06)] = np.float32(-0.0)
    rewards = rng.integers(-7600, 7601, (n, 4)).astype(np.float32)
    rewards[:, 0] = r0
    return {"terminated": np.ones(n, np.uint8), "rewards": rewards, "last_bid": last_bid, "last_bidder": last_bidder, "call_x": call_x,
            "call_xx": call_xx}


def synthetic_bid_count(n, seed, big=True, at_most_one=False):
    """int32 [n, 2, 35]: about 60 % all-zero rows, small counts at a rate of its own per (team, bid), and — ``big`` — 2**31 - 1 in column
    (1, 17) of every 97th board from board 3 on and of board 0 (their sum needs more than 32 bits from two boards on)"""
    rng = np.random.default_rng([seed, 78])
    rate = 0.03 * 1.09 ** np.stack([rng.permutation(35), rng.permutation(35)])     # 0.03 .. 0.56, no two alike within a team
    bc = rng.poisson(rate, (n, 2, 35)).astype(np.int32)
    if at_most_one:
        bc = np.minimum(bc, 1)
    bc[rng.random(n) < 0.6] = 0
    if big:
        bc[0, 1, 17] = 2 ** 31 - 1
        bc[3::97, 1, 17] = 2 ** 31 - 1
    return bc
