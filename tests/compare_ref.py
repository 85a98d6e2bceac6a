"""Python restatement of the system diff (include/brl_compare.h) for the tests, in plain numpy float64: the key, the features, the
masked arg-max, the divergences in the header's order of operations (five actions per slot, the eight slot sums in ascending
order), the flags, and the entries' two-level sums over the sorted decisions.  It shares no code with brl_amd/compare.py beyond the
two dtypes.  No tests in here."""
import numpy as np

from brl_amd.boards import ILLEGAL, OK
from tests import belief_ref as BR

ACTIONS, SLOTS, PER_SLOT, BLOCK = 38, 8, 5, 64
VALID, AGREE, X_PLAYED, Y_PLAYED, NONFINITE = 1, 2, 4, 8, 16
LN2 = float(np.log(2.0))


def key(calls, t):
    """the key of decision t of an auction: the book's fields of calls[0..t), t + 1 in the low four bits"""
    return sum((int(c) + 1) << (58 - 6 * j) for j, c in enumerate(calls[:t])) | (t + 1)


def features(hand, team):
    """bits 0..23 of the book's packed features of one hand word, with the team index"""
    _, hcp, lengths, balanced = BR.features(np.uint64(int(hand)))
    return int(hcp) | sum(int(lengths[s]) << (6 + 4 * s) for s in range(4)) | (int(balanced) << 22) | (int(team) << 23)


def legal_bits(legal):
    return ((np.asarray(legal, np.uint64)[:, None] >> np.arange(ACTIONS, dtype=np.uint64)) & np.uint64(1)).astype(bool)


def _seq(x, axis):
    """the sum along ``axis`` in ascending order, added to +0.0"""
    zero = np.zeros_like(np.take(x, [0], axis=axis))
    return np.take(np.cumsum(np.concatenate([zero, x], axis=axis), axis=axis), -1, axis=axis)


def slot_sum(terms):
    """[m, 38] terms (0.0 where an action does not count) -> [m]: per slot k the actions 5 k .. 5 k + 4 in ascending order, then the
    eight slot sums in ascending order"""
    t = np.zeros((terms.shape[0], SLOTS * PER_SLOT), np.float64)
    t[:, :ACTIONS] = terms
    return _seq(_seq(t.reshape(-1, SLOTS, PER_SLOT), 2), 1)


def net(logits, legal):
    """one network on float32 logits [m, 38] and legal words [m] -> (call [m], nonfinite [m], p [m, 38], L = log p [m, 38])"""
    l32 = np.asarray(logits, np.float32)[:, :ACTIONS]
    ok = legal_bits(legal)
    with np.errstate(all="ignore"):
        call = np.argmax(np.where(ok & ~np.isnan(l32), l32, -np.inf), axis=1)          # the first maximum; 0 without one above -inf
        nonfinite = (ok & (np.isnan(l32) | (l32 == np.inf))).any(1) | ~(ok & (l32 > -np.inf)).any(1)
        m = l32[np.arange(len(l32)), call].astype(np.float64)
        x = l32.astype(np.float64) - m[:, None]
        e = np.where(ok, np.exp(x), 0.0)
        S = slot_sum(e)
        return call, nonfinite, e / S[:, None], x - np.log(S)[:, None]


def _g(d):
    """log(0.5 (1 + exp d)), in the header's two forms"""
    ad = np.abs(d)
    sh = np.sinh(0.25 * np.minimum(ad, 1.0))
    return np.where(ad <= 1.0, 0.5 * d + np.log1p(2.0 * (sh * sh)), np.log(0.5 * (1.0 + np.exp(-ad))) + np.maximum(d, 0.0))


def divergences(logits_x, logits_y, legal):
    """-> dict of [m] arrays: call_x, call_y, nonfinite, kl_xy, kl_yx, js (NaN where nonfinite), abs_xy, abs_yx, abs_js: the sums
    of the terms' magnitudes, and Lx, Ly [m, 38]: each network's float64 log-probabilities"""
    cx, bx, px, Lx = net(logits_x, legal)
    cy, by, py, Ly = net(logits_y, legal)
    with np.errstate(all="ignore"):
        t_xy = np.where(px > 0.0, px * (Lx - Ly), 0.0)
        t_yx = np.where(py > 0.0, py * (Ly - Lx), 0.0)
        j_x = np.where(px > 0.0, px * (-_g(Ly - Lx)), 0.0)
        j_y = np.where(py > 0.0, py * (-_g(Lx - Ly)), 0.0)
        out = {"call_x": cx, "call_y": cy, "nonfinite": bx | by, "kl_xy": slot_sum(t_xy), "kl_yx": slot_sum(t_yx),
               "js": 0.5 * (slot_sum(j_x) + slot_sum(j_y)), "abs_xy": np.abs(t_xy).sum(1), "abs_yx": np.abs(t_yx).sum(1),
               "abs_js": 0.5 * (np.abs(j_x).sum(1) + np.abs(j_y).sum(1)), "Lx": Lx, "Ly": Ly}
    for name in ("kl_xy", "kl_yx", "js"):
        out[name] = np.where(out["nonfinite"], np.nan, out[name])
    return out


def flags(d, played):
    """the flag byte of the decisions of ``divergences``' result with the calls ``played``"""
    played = np.asarray(played)
    return (VALID | np.where(d["call_x"] == d["call_y"], AGREE, 0) | np.where(d["call_x"] == played, X_PLAYED, 0)
            | np.where(d["call_y"] == played, Y_PLAYED, 0) | np.where(d["nonfinite"], NONFINITE, 0)).astype(np.uint8)


def reviewable(rec):
    return ((rec["flags"] & OK) != 0) & ((rec["flags"] & ILLEGAL) == 0)


def expected_records(rec, depth, t, rows, logits_x, logits_y, legal, dtype):
    """the decision records (``dtype``: compare.DECISION_DTYPE) of call index t of the records rec[rows] — all zero where there is
    none — with logp_x / logp_y left zero, and the ``divergences`` dict they were made from"""
    out = np.zeros(len(rows), dtype)
    d = divergences(logits_x, logits_y, legal)
    ok = reviewable(rec)
    played = np.zeros(len(rows), np.int64)
    for j, i in enumerate(rows):
        r = rec[i]
        if not ok[i] or t >= min(int(r["n_calls"]), depth) or int(r["calls"][t]) >= ACTIONS:
            continue
        seat = (int(r["dealer"]) + t) & 3
        played[j] = int(r["calls"][t])
        out["key"][j] = key([int(c) for c in r["calls"][:t]], t)
        out["feats"][j] = features(r["hands"][seat], ((int(r["seating"]) >> (2 * seat)) & 3) >> 1)
        out["legal"][j] = legal[j]
        out["played"][j] = played[j]
    live = out["key"] != 0
    fl = flags(d, played)
    for name in ("call_x", "call_y", "kl_xy", "kl_yx", "js"):
        out[name] = np.where(live, d[name], 0)
    out["flags"] = np.where(live, fl, 0)
    d["played"], d["live"] = played, live
    return out, d


def sort_runs(dense):
    """(perm, starts) of dense decisions: the stable sort by key of the dense index, and the runs' bounds of the non-zero keys
    (starts[e] .. starts[e + 1] in sorted order)"""
    keys = dense["key"].reshape(-1)
    perm = np.argsort(keys, kind="stable")
    ks = keys[perm]
    bounds = np.concatenate([[0], np.nonzero(ks[1:] != ks[:-1])[0] + 1, [len(ks)]])
    if len(ks) and ks[0] == 0:
        bounds = bounds[1:]
    return perm, bounds.astype(np.int64)


def reduce(sorted_dec, starts, dtype):
    """(entries ``dtype`` [K], confusion int64 [38, 38]) of sorted decisions: integers exactly, the float64 sums in the header's
    two-level order (blocks of 64 from the run's first decision, ascending inside a block, the block sums ascending)"""
    K = len(starts) - 1
    out = np.zeros(K, dtype)
    confusion = np.zeros((ACTIONS, ACTIONS), np.int64)
    for e in range(K):
        run = sorted_dec[starts[e]:starts[e + 1]]
        if len(run) == 0:
            continue
        fin = (run["flags"] & NONFINITE) == 0
        f = run[fin]
        agree = (f["flags"] & AGREE) != 0
        o = out[e]
        o["key"], o["n"], o["nonfinite"] = run["key"][0], len(run), int((~fin).sum())
        o["agree"], o["x_played"], o["y_played"] = int(agree.sum()), int(((f["flags"] & X_PLAYED) != 0).sum()), int(((f["flags"] & Y_PLAYED) != 0).sum())
        for name, src in (("calls_x", "call_x"), ("calls_y", "call_y"), ("played", "played")):
            o[name] = np.bincount(f[src], minlength=ACTIONS)
        hcp = (f["feats"] & 63).astype(np.int64)
        o["hcp_sum"], o["hcp_sum_disagree"] = int(hcp.sum()), int(hcp[~agree].sum())
        np.add.at(confusion, (f["call_x"].astype(np.int64), f["call_y"].astype(np.int64)), 1)
        pad = -len(run) % BLOCK
        for name, src in (("kl_xy_sum", "kl_xy"), ("kl_yx_sum", "kl_yx"), ("js_sum", "js"), ("logp_x_sum", "logp_x"), ("logp_y_sum", "logp_y")):
            with np.errstate(all="ignore"):
                v = np.concatenate([np.where(fin, run[src].astype(np.float64), 0.0), np.zeros(pad)])
                o[name] = _seq(_seq(v.reshape(-1, BLOCK), 1), 0)
        o["js_max"] = f["js"].max() if len(f) else 0.0
    return out, confusion
