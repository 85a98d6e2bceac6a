"""Float64 reference of the policy sampler (categorical<K> in brl_amd/csrc/policy_common.hpp): plain numpy, nothing of
brl_amd.  The reference's distribution is `Categorical(logits=where(mask, logits, -inf))`, src/roll_out.py:27-39; a 16-bit
network output converts to float exactly, so the logits given here are the ROUNDED ones (``tensor.float()``)."""
import numpy as np

NUM_ACTIONS = 38
U24 = 2.0 ** -24          # one step of the 24-bit uniform draw, u = (u32 >> 8) / 2**24
TOP = 1.0 - U24           # the largest draw that exists
BAND = 64 * U24
"""How far the sampler's fp32 inverse CDF may sit from the float64 one, in units of u: a bound worked out from the
arithmetic, not a measurement.  The kernel takes the first action with `cum > u * total`; cum and total are fp32 sums of
at most 38 terms e = expf(l - max) in [0, 1], total in [1, 38].  With eps = 2**-24 (half an ulp), relative to total:
  * summation.  No lane layout adds deeper than K = 8: the 5 terms of a lane (4 additions), 3 Hillis-Steele levels for
    the slots in front (the scan `total` also comes from: 7 eps), then up to 5 more additions for the running cum:
    <= 12 eps on cum, <= 7 eps on total.  A plain sequential 38-term sum would be 37 eps each; no layout does that;
  * expf to 2 ulp = 4 eps per term, hence <= 4 eps on either sum;
  * `u * total` rounds once: 1 eps.
  12 + 7 + 4 + 4 + 1 = 28 eps for the comparison itself;
  * a 24-bit draw cannot resolve a cell narrower than one draw step, and a sampler may pass over such cells (the
    kernel does, see categorical<K>): at most 36 of them (all but the mode and the action returned) in front of the
    action returned, each narrower than eps: <= 36 eps.
28 + 36 = 64 eps."""


def _cand_matrix(cand, shape):
    return np.broadcast_to(np.asarray(cand).astype(bool), shape)


def log_softmax64(logits, cand):
    """log-softmax over the candidates in float64; -inf outside `cand` ([..., 38] 0/1)."""
    l = np.asarray(logits, dtype=np.float64)
    l = np.where(_cand_matrix(cand, l.shape), l, -np.inf)
    with np.errstate(invalid="ignore", over="ignore"):
        m = l.max(axis=-1, keepdims=True)
        return (l - m) - np.log(np.exp(l - m).sum(axis=-1, keepdims=True))


def mode64(logits, cand):
    """the first maximum among the candidates (pi.mode() = argmax)"""
    l = np.asarray(logits, dtype=np.float64)
    return np.where(_cand_matrix(cand, l.shape), l, -np.inf).argmax(axis=-1)


def cdf64(logits, cand):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.cumsum(np.exp(log_softmax64(logits, cand)), axis=-1)


def inverse_cdf64(logits, cand, u):
    """first action whose float64 CDF exceeds u (one row)"""
    return int(np.argmax(cdf64(logits, cand) > u))


def accept_matrix(logits, cand, u24, band=BAND):
    """accept_set for many rows at once: [n, 38] bool, row i for the draw u24[i]"""
    c = cdf64(logits, cand)
    u = np.asarray(u24, dtype=np.float64).reshape(-1, 1) * U24
    lo, hi = np.maximum(0.0, u - band), np.minimum(u + band, TOP)
    below = np.concatenate((np.full(c.shape[:-1] + (1,), -np.inf), c[..., :-1]), axis=-1)
    return (c > below) & (c > lo) & (below <= hi)   # the cell of a is [below[a], c[a]); an empty cell is never first


def accept_set(logits, cand, u24, band=BAND):
    """The actions a sampler may return for the draw u = u24 / 2**24 of ONE row: every a that is `first a with
    cdf64[a] > u'` for some u' in [max(0, u - band), min(u + band, 1 - 2**-24)].  The upper clip is the largest draw
    that exists: a call whose CDF cell lies wholly above it can never be drawn and is never acceptable."""
    row = accept_matrix(np.asarray(logits)[None], np.asarray(cand)[None], [u24], band)[0]
    return set(np.nonzero(row)[0].tolist())
