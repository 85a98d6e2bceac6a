"""Python restatement of the position queries (include/brl_positions.h) for the tests, in plain Python and numpy float64: the status
rules, the observation row and the legal mask of a position (DESIGN §3's layout: the vulnerability nibble, the auction history by
relative seat, the 52 own-card bits), and the answer — the masked arg-max, p_a and L_a in the header's two-level order, the
entropy, the ranks and the top list, the non-finite rule.  It shares no code with brl_amd/positions.py.  No tests in here."""
import numpy as np

ACTIONS, OBS, MAX_CALLS, FILL, SLOTS, PER_SLOT = 38, 480, 48, 255, 8, 5
OK, BAD_HEADER, BAD_HAND, ILLEGAL_CALL, FINISHED = 0, 1, 2, 3, 4
NONFINITE = 1
DTYPE = np.dtype([("hand", "<u8"), ("dealer", "u1"), ("vul_ns", "u1"), ("vul_ew", "u1"), ("n_calls", "u1"), ("reserved", "<u4"),
                  ("calls", "u1", MAX_CALLS)])


def pack(hand, dealer, vul_ns, vul_ew, calls, reserved=0, n_calls=None, fill=FILL):
    """one record; ``n_calls`` / ``fill`` / ``reserved`` can be set against the rules"""
    r = np.zeros((), DTYPE)
    r["hand"], r["dealer"], r["vul_ns"], r["vul_ew"], r["reserved"] = hand, dealer, vul_ns, vul_ew, reserved
    r["n_calls"] = len(calls) if n_calls is None else n_calls
    r["calls"] = fill
    r["calls"][:len(calls)] = calls
    return r


class Auction:
    """the auction's rules: who may call what, and when it is over"""

    def __init__(self, dealer):
        self.turn, self.dealer = 0, dealer
        self.last_bid, self.bidder, self.doubled, self.redoubled, self.passes, self.over = None, None, False, False, 0, False
        self.events = []     # (observation bit base, absolute seat): what the history shows

    def seat(self):
        return (self.dealer + self.turn) % 4

    def legal(self, a):
        ours = self.bidder is not None and (self.bidder - self.seat()) % 2 == 0
        if a == 0:
            return True
        if a == 1:
            return self.last_bid is not None and not ours and not self.doubled and not self.redoubled
        if a == 2:
            return self.last_bid is not None and ours and self.doubled and not self.redoubled
        return self.last_bid is None or a - 3 > self.last_bid

    def word(self):
        return sum(1 << a for a in range(ACTIONS) if self.legal(a))

    def call(self, a):
        s = self.seat()
        if a >= 3:
            self.last_bid, self.bidder, self.doubled, self.redoubled = a - 3, s, False, False
            self.events.append((8 + 12 * (a - 3), s))
        elif a == 1:
            self.doubled = True
            self.events.append((8 + 12 * self.last_bid + 4, s))
        elif a == 2:
            self.redoubled = True
            self.events.append((8 + 12 * self.last_bid + 8, s))
        elif self.last_bid is None:
            self.events.append((4, s))     # a pass before the first bid
        self.passes = self.passes + 1 if a == 0 else 0
        self.over = self.passes == (4 if self.last_bid is None else 3)
        self.turn += 1


def row_of(r):
    """(status, observation uint8 [480], mask uint8 [38], legal word) of one record; all zero unless the status is OK"""
    zero = (np.zeros(OBS, np.uint8), np.zeros(ACTIONS, np.uint8), 0)
    n, calls = int(r["n_calls"]), [int(c) for c in r["calls"]]
    if (int(r["dealer"]) > 3 or int(r["vul_ns"]) > 1 or int(r["vul_ew"]) > 1 or n > MAX_CALLS or int(r["reserved"]) != 0
            or any(c >= ACTIONS for c in calls[:n]) or any(c != FILL for c in calls[n:])):
        return (BAD_HEADER,) + zero
    hand = int(r["hand"])
    if hand >> 52 or bin(hand).count("1") != 13:
        return (BAD_HAND,) + zero
    au = Auction(int(r["dealer"]))
    for j, a in enumerate(calls[:n]):
        if au.over:
            return (FINISHED | ((j - 1) << 8),) + zero
        if not au.legal(a):
            return (ILLEGAL_CALL | (j << 8),) + zero
        au.call(a)
    if au.over:
        return (FINISHED | ((n - 1) << 8),) + zero
    me = au.seat()
    obs = np.zeros(OBS, np.uint8)
    we, they = (int(r["vul_ns"]), int(r["vul_ew"])) if me % 2 == 0 else (int(r["vul_ew"]), int(r["vul_ns"]))
    obs[1 if we else 0] = 1
    obs[3 if they else 2] = 1
    for base, s in au.events:
        obs[base + (s - me) % 4] = 1
    for c in range(52):
        obs[428 + c] = (hand >> c) & 1
    word = au.word()
    return OK, obs, np.array([(word >> a) & 1 for a in range(ACTIONS)], np.uint8), word


def rows(arr):
    """(status uint32 [n], obs uint8 [n,480], mask uint8 [n,38], legal uint64 [n]) of records ``arr``"""
    out = [row_of(r) for r in arr.reshape(-1)]
    return (np.array([o[0] for o in out], np.uint32), np.stack([o[1] for o in out]), np.stack([o[2] for o in out]),
            np.array([o[3] for o in out], np.uint64))


def fill_hands(hand, seat):
    """the four hand words by seat of a position's table: the 39 other cards in ascending card id, 13 to each next seat"""
    rest = [c for c in range(52) if not (int(hand) >> c) & 1]
    out = [0, 0, 0, 0]
    out[seat] = int(hand)
    for k in range(3):
        out[(seat + 1 + k) % 4] = sum(1 << c for c in rest[13 * k:13 * k + 13])
    return out


# ---- the answer --------------------------------------------------------------------------------------------------------------------
def _seq(x, axis):
    zero = np.zeros_like(np.take(x, [0], axis=axis))
    return np.take(np.cumsum(np.concatenate([zero, x], axis=axis), axis=axis), -1, axis=axis)


def two_level(terms):
    """[m,38] -> [m]: slot k adds its actions 5 k .. 5 k + 4 in ascending order to +0.0; the eight slot sums in ascending order"""
    t = np.zeros((terms.shape[0], SLOTS * PER_SLOT), np.float64)
    t[:, :ACTIONS] = terms
    return _seq(_seq(t.reshape(-1, SLOTS, PER_SLOT), 2), 1)


def answer(logits, legal, top_k, status=None):
    """dict of arrays for float32 logits [m, >= 38] and legal words [m]: call, n_legal, flags, k, entropy, top_action [m,8],
    top_prob [m,8], probs [m,38], and entropy_scale = the sum of the magnitudes of the entropy's terms.  Rows whose ``status`` is
    not OK: call 255, everything else zero."""
    l32 = np.asarray(logits, np.float32)[:, :ACTIONS]
    m = len(l32)
    ok = ((np.asarray(legal, np.uint64)[:, None] >> np.arange(ACTIONS, dtype=np.uint64)) & np.uint64(1)).astype(bool)
    with np.errstate(all="ignore"):
        call = np.argmax(np.where(ok & ~np.isnan(l32), l32, -np.inf), axis=1)
        bad = (ok & (np.isnan(l32) | (l32 == np.inf))).any(1) | ~(ok & (l32 > -np.inf)).any(1)
        top = l32[np.arange(m), call].astype(np.float64)
        x = l32.astype(np.float64) - top[:, None]
        e = np.where(ok, np.exp(x), 0.0)
        S = two_level(e)
        p = e / S[:, None]
        L = x - np.log(S)[:, None]
        terms = np.where(p > 0.0, p * (-L), 0.0)
        entropy = two_level(terms)
        scale = np.abs(terms).sum(1)
    n_legal = ok.sum(1)
    k = np.where(bad, 0, np.minimum(top_k, n_legal))
    b_idx, a_idx = np.arange(ACTIONS)[None, :, None], np.arange(ACTIONS)[None, None, :]
    with np.errstate(all="ignore"):
        ahead = ok[:, :, None] & ((p[:, :, None] > p[:, None, :]) | ((p[:, :, None] == p[:, None, :]) & (b_idx < a_idx)))
    rank = ahead.sum(1)
    top_action = np.full((m, 8), 255, np.uint8)
    top_prob = np.zeros((m, 8))
    for i in range(m):
        for a in np.nonzero(ok[i])[0]:
            if rank[i, a] < k[i]:
                top_action[i, rank[i, a]], top_prob[i, rank[i, a]] = a, p[i, a]
    probs = np.where(ok, p, 0.0)
    entropy, scale = np.where(bad, np.nan, entropy), np.where(bad, 0.0, scale)
    top_prob[bad], probs[bad] = np.nan, np.nan
    out = {"call": call.astype(np.uint8), "n_legal": n_legal.astype(np.uint8), "flags": np.where(bad, NONFINITE, 0).astype(np.uint8),
           "k": k.astype(np.uint8), "entropy": entropy, "top_action": top_action, "top_prob": top_prob, "probs": probs,
           "entropy_scale": scale}
    if status is not None:
        dead = (np.asarray(status) & 0xFF) != OK
        for name, v in out.items():
            v[dead] = 255 if name == "call" else 0
    return out


# ---- the scripted cases the host and the device tests share ------------------------------------------------------------------------
LONG = [a for b in range(16) for a in (3 + b, 0, 0)]     # 48 calls: sixteen bids, two passes behind each; the auction is still open

SCRIPTED = {     # name: calls from the dealer on
    "three passes": [0, 0, 0],
    "1C": [3], "1C P": [3, 0], "1C P P": [3, 0, 0], "1C X": [3, 1], "1C X P": [3, 1, 0], "1C X P P": [3, 1, 0, 0], "1C X XX": [3, 1, 2],
    "1C X XX P": [3, 1, 2, 0], "1C X XX P P": [3, 1, 2, 0, 0], "1C X XX 1D": [3, 1, 2, 4], "1C X 1D": [3, 1, 4], "1C P 1D X": [3, 0, 4, 1],
    "1C P P X": [3, 0, 0, 1], "1C P P X XX": [3, 0, 0, 1, 2], "P 1NT P P": [0, 7, 0, 0], "P P P 1S": [0, 0, 0, 6],
    "7NT": [37], "7NT X": [37, 1], "7NT X XX": [37, 1, 2], "7NT P P": [37, 0, 0], "7C 7NT": [33, 37],
    "48 calls": LONG, "47 calls": LONG[:47],
}

BAD = {     # name: (calls, status) — what a wrong auction must be told
    "X with no bid": ([1], ILLEGAL_CALL | (0 << 8)),
    "X after passes only": ([0, 0, 1], ILLEGAL_CALL | (2 << 8)),
    "an insufficient bid": ([8, 0, 7], ILLEGAL_CALL | (2 << 8)),
    "the same bid again": ([8, 8], ILLEGAL_CALL | (1 << 8)),
    "XX without X": ([3, 2], ILLEGAL_CALL | (1 << 8)),
    "XX by the doubling side": ([3, 1, 0, 2], ILLEGAL_CALL | (3 << 8)),
    "X of partner's bid": ([3, 0, 1], ILLEGAL_CALL | (2 << 8)),
    "X twice": ([3, 1, 0, 0, 1], ILLEGAL_CALL | (4 << 8)),
    "a call after the closing pass": ([3, 0, 0, 0, 4], FINISHED | (3 << 8)),
    "two calls after a pass-out": ([0, 0, 0, 0, 3, 0], FINISHED | (3 << 8)),
    "a finished auction": ([5, 1, 0, 0, 0], FINISHED | (4 << 8)),
    "a pass-out": ([0, 0, 0, 0], FINISHED | (3 << 8)),
}


def random_hand(rng, cards=13):
    return sum(1 << int(c) for c in rng.choice(52, size=cards, replace=False))


def scripted_records(seed=5):
    """(names, records): every dealer x vulnerability without a call, then every SCRIPTED auction, each with a random hand"""
    rng = np.random.default_rng(seed)
    names, out = [], []
    for dealer in range(4):
        for vul in range(4):
            names.append(f"no call, dealer {dealer}, vul {vul}")
            out.append(pack(random_hand(rng), dealer, vul & 1, vul >> 1, []))
    for i, (name, calls) in enumerate(SCRIPTED.items()):
        names.append(name)
        out.append(pack(random_hand(rng), i % 4, (i >> 2) & 1, (i >> 3) & 1, calls))
    return names, np.array(out, DTYPE)
