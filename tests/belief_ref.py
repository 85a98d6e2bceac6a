"""Python restatement of the hand beliefs (include/brl_belief.h) for the tests, in plain numpy: the Philox stream and the shuffle
of a sample, its empty table (tests/board_records_ref.py's encoder), the weight as a float64 chain (``nets.forward64`` through a
callable, ``categorical_ref.log_softmax64`` / ``mode64``) and the reduction in float64 with the features of tests/book_ref.py.
It shares no code with brl_amd/belief.py.  No tests in here."""
import numpy as np

from tests import board_records_ref as R
from tests import book_ref as B
from tests import categorical_ref as cref

M32 = np.uint64(0xFFFFFFFF)
STREAM = 0x42524C42          # BRL_BELIEF_STREAM
HIDDEN = 39
RANK_POINTS = [B.POINTS.get(r, 0) for r in "23456789TJQKA"]      # by rank 0..12


# ---- the sampler -----------------------------------------------------------------------------------------------------------------
def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on arrays of counters (uint64 arrays holding 32-bit words) -> four uint64 arrays of 32-bit words"""
    c0, c1, c2, c3 = (np.asarray(c, np.uint64) & M32 for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = np.uint64(k0 & 0xFFFFFFFF), np.uint64(k1 & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ k0) & M32, p1 & M32, ((p0 >> np.uint64(32)) ^ c3 ^ k1) & M32, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def draws(seed, q, ks):
    """uint64 [len(ks), 38]: draw j of sample k of stream index q — word j & 3 of block j >> 2, counter (k, block, STREAM, q)"""
    ks = np.asarray(ks, np.uint64)
    out = np.zeros((len(ks), HIDDEN - 1), np.uint64)
    for blk in range((HIDDEN + 2) // 4):
        words = philox4x32_10(ks, blk, STREAM, q, seed & 0xFFFFFFFF, seed >> 32)
        for i in range(4):
            if blk * 4 + i < HIDDEN - 1:
                out[:, blk * 4 + i] = words[i]
    return out


def sample_hands(seat, hand, seed, q, ks):
    """uint64 [len(ks), 4]: the four hand words (by seat) of the samples ``ks`` of stream index q for ``seat`` holding ``hand``"""
    ks = np.asarray(ks, np.int64)
    rest = [b for b in range(52) if not (int(hand) >> b) & 1]
    assert len(rest) == HIDDEN
    c = np.tile(np.array(rest, np.int64), (len(ks), 1))
    d = draws(seed, q, ks)
    rows = np.arange(len(ks))
    for j in range(HIDDEN - 1):
        r = j + ((d[:, j] * np.uint64(HIDDEN - j)) >> np.uint64(32)).astype(np.int64)
        a, b = c[rows, j].copy(), c[rows, r].copy()
        c[rows, j], c[rows, r] = b, a
    out = np.zeros((len(ks), 4), np.uint64)
    out[:, seat & 3] = np.uint64(int(hand))
    one = np.uint64(1)
    for h in range(3):
        out[:, (seat + 1 + h) & 3] = np.bitwise_or.reduce(one << c[:, 13 * h:13 * h + 13].astype(np.uint64), axis=1)
    return out


def seating_tuple(byte):
    return tuple((int(byte) >> (2 * s)) & 3 for s in range(4))


def sample_tables(dealer, vul_ns, vul_ew, seating, hands):
    """uint64 [K,16]: the empty tables of the deals ``hands`` [K,4]: ``encode`` of no calls, the hand words filled in (word 7 + seat
    holds the hand word << 4, as ``Table.pack`` writes it)"""
    base = R.encode(dealer & 3, [], vul_ns=vul_ns & 1, vul_ew=vul_ew & 1, seating=seating_tuple(seating)).pack()
    out = np.tile(base, (hands.shape[0], 1))
    out[:, 7:11] = hands << np.uint64(4)
    return out


# ---- the weight --------------------------------------------------------------------------------------------------------------------
def legal_words(dealer, calls):
    """[(caller seat, legal word)] of a prefix, by the encoder's rules; asserts that the prefix is legal"""
    t, out = R.Table(dealer), []
    for a in calls:
        assert not t.term
        word = sum(1 << x for x in range(38) if t.legal(x))
        assert (word >> a) & 1
        out.append((t.seat(), word))
        t.step(a)
    return out


def logp64(logits, word, action):
    """(float64 log-probability of ``action`` under the logits masked to ``word``, greedy flag) per row of float logits [m, 38]:
    greedy = the first maximum of the masked logits is the action, and the log-probability is not NaN"""
    cand = np.array([(word >> a) & 1 for a in range(38)], bool)
    lp = cref.log_softmax64(logits, cand)[..., action]
    return lp, (cref.mode64(logits, cand) == action) & ~np.isnan(lp)


def chain64(oracle_tables, step, seat, team_of_seat, dealer, calls, forward, tol_of):
    """The float64 weight of every sample: ``oracle_tables`` are the samples' tables in a host environment whose ``observation``
    and ``legal_action_mask`` fields are read and which ``step(tables, actions)`` advances; ``forward(team, obs)`` gives float64
    logits [m, 38]; ``tol_of(logits)`` a forward's tolerance.  -> (logw float64 [K], weighed calls, tolerance sum, below [K, T]:
    how far the call's logit lies under the largest legal one, gap [K, T]: how far the second largest legal logit does, both in
    units of that forward's tolerance (NaN: a call that is not weighed))"""
    K = len(oracle_tables["observation"])
    logw, tol_sum, weighed = np.zeros(K), 0.0, 0
    below = np.full((K, max(1, len(calls))), np.nan)
    gap = np.full((K, max(1, len(calls))), np.nan)
    for t, ((caller, word), a) in enumerate(zip(legal_words(dealer, calls), calls)):
        mask = np.array([(word >> x) & 1 for x in range(38)], np.uint8)
        assert (oracle_tables["legal_action_mask"] == mask[None, :]).all(), f"call {t}: the legal word"
        if caller != seat:
            lg = forward(team_of_seat(caller), oracle_tables["observation"])
            tol = tol_of(lg)
            lp, _ = logp64(lg, word, a)
            logw += lp
            masked = np.where(mask[None, :] == 1, lg, -np.inf)
            top = np.sort(masked, axis=1)
            below[:, t] = (top[:, -1] - lg[:, a]) / tol
            gap[:, t] = (top[:, -1] - top[:, -2]) / tol
            tol_sum += tol
            weighed += 1
        step(oracle_tables, np.full(K, a, np.int32))
    return logw, weighed, tol_sum, below, gap


# ---- the reduction ---------------------------------------------------------------------------------------------------------------
def features(words):
    """(bits [.., 52] 0/1, hcp [..], lengths [.., 4] by suit C,D,H,S, balanced [..]) of hand words, by book_ref's definitions"""
    w = np.asarray(words, np.uint64)
    bits = ((w[..., None] >> np.arange(52, dtype=np.uint64)) & np.uint64(1)).astype(np.int64)
    by_rank = bits.reshape(bits.shape[:-1] + (13, 4))
    hcp = (by_rank.sum(-1) * np.array(RANK_POINTS)).sum(-1)
    lengths = by_rank.sum(-2)
    shape = np.sort(lengths, axis=-1)
    balanced = np.zeros(hcp.shape, bool)
    for pattern in B.BALANCED:
        balanced |= (shape == np.array(pattern)).all(-1)
    return bits, hcp, lengths, balanced


def reduce64(seat, hands, logw, greedy):
    """one entry as a dict of arrays (the fields of brl_belief_entry) from hands uint64 [K,4], logw float32 [K], greedy [K]"""
    hands, logw, greedy = np.asarray(hands, np.uint64), np.asarray(logw, np.float32), np.asarray(greedy) != 0
    K = len(logw)
    hidden = hands[:, [(seat + 1 + h) & 3 for h in range(3)]]
    bits, hcp, lengths, balanced = features(hidden)
    onehot_hcp = (hcp[..., None] == np.arange(38)).astype(np.int64)                      # [K,3,38]
    onehot_len = (lengths[..., None] == np.arange(14)).astype(np.int64)                  # [K,3,4,14]
    with np.errstate(invalid="ignore"):
        mx = np.float32(np.nan) if np.isnan(logw).any() else logw.max()
        bad = bool(np.isnan(mx) or np.isinf(mx))
        w = np.exp(logw.astype(np.float64) - np.float64(mx))
    tot = lambda x: np.full(x.shape[1:], np.nan) if bad else np.add.reduce(w.reshape((K,) + (1,) * (x.ndim - 1)) * x, axis=0)   # noqa: E731
    g = greedy.astype(np.int64)
    cnt = lambda x: (g.reshape((K,) + (1,) * (x.ndim - 1)) * x).sum(0).astype(np.uint32)      # noqa: E731
    ones = np.ones(K, np.int64)
    return {"wsum": tot(ones[:, None])[0], "wsq": np.nan if bad else float(np.add.reduce(w * w)),
            "max_logw": np.float32(np.nan) if bad else np.float32(mx), "n": K, "consistent": int(g.sum()),
            "card": tot(bits), "hcp": tot(onehot_hcp), "length": tot(onehot_len), "balanced": tot(balanced.astype(np.int64)),
            "g_card": cnt(bits), "g_hcp": cnt(onehot_hcp), "g_length": cnt(onehot_len), "g_balanced": cnt(balanced.astype(np.int64))}


FLOAT_FIELDS = ("wsum", "wsq", "card", "hcp", "length", "balanced")
INT_FIELDS = ("n", "consistent", "g_card", "g_hcp", "g_length", "g_balanced")


def compare_entry(entry, want, K):
    """asserts one device entry (a record of belief.ENTRY_DTYPE) against ``reduce64``'s: integers bit for bit, float64 sums within
    K * 2^-52 relative (reordering only), a NaN block NaN throughout; -> the largest relative difference found"""
    worst = 0.0
    for name in INT_FIELDS:
        assert np.array_equal(np.asarray(entry[name]).astype(np.int64), np.asarray(want[name]).astype(np.int64)), name
    assert entry["reserved"] == 0 and entry["reserved2"] == 0
    if np.isnan(want["wsum"]):
        assert np.isnan(entry["max_logw"]) and all(np.isnan(np.asarray(entry[name])).all() for name in FLOAT_FIELDS)
        return worst
    assert np.float32(entry["max_logw"]) == np.float32(want["max_logw"])
    for name in FLOAT_FIELDS:
        got, ref = np.asarray(entry[name], np.float64), np.asarray(want[name], np.float64)
        assert got.shape == ref.shape and ((ref == 0) == (got == 0)).all(), name
        rel = np.abs(got - ref) / np.where(ref == 0, 1.0, ref)
        worst = max(worst, float(rel.max()))
        assert (rel <= K * 2.0 ** -52).all(), (name, float(rel.max()), K * 2.0 ** -52)
    return worst
