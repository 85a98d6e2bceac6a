"""Python restatement of the beliefs' resample-move stages (include/brl_belief_smc.h) for the tests, in plain numpy: the two-level
cumulative sum and the systematic resampling, the card exchange of a proposal, the acceptance in float64 and the schedule.  It
shares no code with brl_amd/belief.py; the Philox function is tests/belief_ref.py's.  No tests in here."""
import numpy as np

from tests import belief_ref as BR

RESAMPLE_STREAM = 0x42524C53      # BRL_BELIEF_RESAMPLE_STREAM
MOVE_STREAM = 0x42524C4D          # BRL_BELIEF_MOVE_STREAM
SEGMENT = 64                      # BRL_BELIEF_SMC_SEGMENT
DECK = (1 << 52) - 1
PAIRS = ((0, 1), (0, 2), (1, 2))  # the hidden seats (first, second) of mulhi32(w0, 3)


def unit(w):
    """((double)w + 0.5) * 2^-32 of 32-bit words"""
    return (np.asarray(w, np.float64) + 0.5) * 2.0 ** -32


def mulhi(w, n):
    return ((np.asarray(w, np.uint64) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


# ---- resample --------------------------------------------------------------------------------------------------------------------
def cumulative(W):
    """C of the header: serial inside segments of 64, the offsets serial over the segments, one more addition (np.cumsum adds in
    order, one float64 addition per element)"""
    W = np.asarray(W, np.float64)
    K = len(W)
    pad = np.zeros(-(-K // SEGMENT) * SEGMENT)
    pad[:K] = W
    inner = np.cumsum(pad.reshape(-1, SEGMENT), axis=1)
    ends = np.array([inner[s, min(SEGMENT, K - s * SEGMENT) - 1] for s in range(inner.shape[0])])      # I at the segment's last particle
    offsets = np.concatenate([[0.0], np.cumsum(ends)[:-1]])
    return (offsets[:, None] + inner).reshape(-1)[:K]


def offset_u(seed, q, t):
    return float(unit(BR.philox4x32_10(t, 0, RESAMPLE_STREAM, q, seed & 0xFFFFFFFF, seed >> 32)[0]))


def thresholds(K, u, S):
    return ((np.arange(K, dtype=np.float64) + u) * S) / np.float64(K)


def resample(logw, u):
    """(ancestors int64 [K], C [K], x [K]) of one query; ancestors None where the query is left as it is (a NaN, or no finite
    largest logw)"""
    logw = np.asarray(logw, np.float32)
    K = len(logw)
    with np.errstate(invalid="ignore"):
        mx = logw.max()
    if np.isnan(logw).any() or not np.isfinite(mx):
        return None, None, None
    C = cumulative(np.exp(logw.astype(np.float64) - np.float64(mx)))
    x = thresholds(K, u, C[-1])
    return np.minimum(np.searchsorted(C, x, side="right"), K - 1).astype(np.int64), C, x      # the smallest k with C_k > x


# ---- propose ---------------------------------------------------------------------------------------------------------------------
def nth_card(word, i):
    """the i-th set bit of ``word``, ascending, as a one-bit int; 0 if there is none"""
    bits = [b for b in range(52) if (int(word) >> b) & 1]
    return 1 << bits[i] if i < len(bits) else 0


def move_words(seed, q, t, m, ks):
    return BR.philox4x32_10(np.asarray(ks, np.uint64), (t << 8) | m, MOVE_STREAM, q, seed & 0xFFFFFFFF, seed >> 32)


def propose(seat, hands, seed, q, t, m):
    """(proposed hands uint64 [K,4], (pair, i, j) int64 [K,3], w3 uint64 [K]) for the particles 0..K-1 with the hands ``hands``"""
    hands = np.asarray(hands, np.uint64)
    K = hands.shape[0]
    w0, w1, w2, w3 = move_words(seed, q, t, m, np.arange(K))
    pick = np.stack([mulhi(w0, 3), mulhi(w1, 13), mulhi(w2, 13)], axis=1)
    out = hands & np.uint64(DECK)
    for k in range(K):
        first, second = ((seat + 1 + h) & 3 for h in PAIRS[pick[k, 0]])
        x, y = int(out[k, first]), int(out[k, second])
        cx, cy = nth_card(x, pick[k, 1]), nth_card(y, pick[k, 2])
        if cx and cy:
            out[k, first], out[k, second] = np.uint64((x ^ cx) | cy), np.uint64((y ^ cy) | cx)
    return out, pick, w3


# ---- accept ----------------------------------------------------------------------------------------------------------------------
def accept(w3, logl, logl_new):
    """bool [K]: log(v) < (double)logl_new - (double)logl in float64, v = unit(w3); a NaN compares false"""
    with np.errstate(invalid="ignore"):
        return np.log(unit(w3)) < np.asarray(logl_new, np.float32).astype(np.float64) - np.asarray(logl, np.float32).astype(np.float64)


# ---- schedule --------------------------------------------------------------------------------------------------------------------
def stages(seat, dealer, n_calls, resample_every):
    """the call indices after which a query resamples: every ``resample_every``-th call whose caller (dealer + t) & 3 is not ``seat``"""
    hidden = [t for t in range(n_calls) if (dealer + t) & 3 != seat]
    return [t for n, t in enumerate(hidden, 1) if resample_every and n % resample_every == 0]
