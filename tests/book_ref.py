"""Python restatement of the bidding-system book (include/brl_book.h) for the tests: a plain dict from the prefix tuple to
counters over a RECORD_DTYPE array.  It shares no code with brl_amd/book.py: high-card points and suit lengths are counted from
the card NAMES (boards.hand_names), as board_stats.py does."""
import numpy as np

from brl_amd.boards import OK, RECORD_DTYPE, hand_names

POINTS = {"A": 4, "K": 3, "Q": 2, "J": 1}
BALANCED = ([3, 3, 3, 4], [2, 3, 4, 4], [2, 3, 3, 5])


def blank():
    return {"count": 0, "balanced": 0, "hcp": [0] * 38, "length": [[0] * 14 for _ in range(4)], "imp_sum": 0, "imp_sq_sum": 0}


def add_table(book, rec, depth, imp=None, imp_sign=1):
    """adds one table's samples to ``book``: {prefix tuple of action ids: [team 1's counters, team 2's counters]}; returns the
    number of records without the self-check bit"""
    assert rec.dtype == RECORD_DTYPE
    skipped = 0
    for i, r in enumerate(rec):
        if not int(r["flags"]) & OK:
            skipped += 1
            continue
        calls = [int(c) for c in r["calls"][:min(int(r["n_calls"]), depth)]]
        seen = {}
        for p in range(len(calls)):
            seat = (int(r["dealer"]) + p) % 4
            player = (int(r["seating"]) >> (2 * seat)) % 4
            if seat not in seen:
                names = hand_names(r["hands"][seat])
                lengths = [sum(1 for c in names if c[0] == s) for s in "CDHS"]
                seen[seat] = (sum(POINTS.get(c[1], 0) for c in names), lengths, sorted(lengths) in BALANCED)
            hcp, lengths, balanced = seen[seat]
            t = book.setdefault(tuple(calls[:p + 1]), [blank(), blank()])[player // 2]
            t["count"] += 1
            t["balanced"] += int(balanced)
            t["hcp"][hcp] += 1
            for s in range(4):
                t["length"][s][lengths[s]] += 1
            if imp is not None:
                v = int(imp[i]) * imp_sign * (1 if seat % 2 == 0 else -1)
                t["imp_sum"] += v
                t["imp_sq_sum"] += v * v
    return skipped


def book_of(rec_a, rec_b=None, depth=4, imp=None):
    """(book, skipped) of a match: table A's records, table B's (the IMP's sign reversed) when given"""
    book = {}
    skipped = add_table(book, rec_a, depth, imp, 1)
    if rec_b is not None:
        skipped += add_table(book, rec_b, depth, imp, -1)
    return book, skipped


def order(prefix):
    """sort key of the depth-first order of the prefix tree: tuples compare call by call, a prefix before its extensions"""
    return tuple(prefix)


# ---- synthetic records -------------------------------------------------------------------------------------------------------
def hand_word(cards):
    """the hand word of (rank, suit) pairs: bit rank * 4 + suit"""
    return sum(1 << (r * 4 + s) for r, s in cards)


def random_hands(rng):
    """four 13-card hand words of one shuffled deck"""
    deck = rng.permutation(52)
    return [sum(1 << int(b) for b in deck[s * 13:(s + 1) * 13]) for s in range(4)]


def shaped_hand(lengths, top=True):
    """one hand word with the suit lengths C,D,H,S given, taking each suit's highest (``top``) or lowest ranks"""
    assert sum(lengths) == 13
    return hand_word([((12 - k) if top else k, s) for s, n in enumerate(lengths) for k in range(n)])


def make_records(auctions, rng, hands=None, ok=None):
    """RECORD_DTYPE [n]: record i holds auctions[i] (a list of action ids, possibly unfinished or empty), a random dealer and
    seating, random 13-card hands (or hands[i]) and the OK bit (unless ok[i] is False)"""
    from brl_amd.boards import FILL
    n = len(auctions)
    rec = np.zeros(n, RECORD_DTYPE)
    perms = [[0, 1, 2, 3], [1, 0, 3, 2], [2, 3, 0, 1], [3, 2, 1, 0], [0, 3, 2, 1], [2, 1, 0, 3]]
    for i, calls in enumerate(auctions):
        r = rec[i]
        r["n_calls"] = len(calls)
        r["dealer"] = int(rng.integers(0, 4))
        seats = perms[int(rng.integers(0, len(perms)))]
        r["seating"] = sum(p << (2 * s) for s, p in enumerate(seats))
        r["flags"] = OK if ok is None or ok[i] else 0
        r["hands"] = random_hands(rng) if hands is None else hands[i]
        r["calls"][:] = FILL
        r["calls"][:len(calls)] = calls
        r["score_ns"] = int(rng.integers(-2000, 2000))     # (fields the book never reads: anything)
        r["vul_ns"], r["vul_ew"] = int(rng.integers(0, 2)), int(rng.integers(0, 2))
    return rec


def key(prefix):
    """brl_book.h's key, restated: six bits per call, most significant first"""
    return sum((int(c) + 1) << (58 - 6 * j) for j, c in enumerate(prefix))


def arrays(book):
    """the dict as the arrays a SystemBook holds, entries in tuple order: (keys, count, balanced, hcp, length, imp_sum, imp_sq_sum)"""
    prefixes = sorted(book, key=order)
    per = lambda name, dt: np.array([[book[p][t][name] for t in (0, 1)] for p in prefixes], dt).reshape((len(prefixes), 2) + {  # noqa: E731
        "hcp": (38,), "length": (4, 14)}.get(name, ()))
    return (np.array([key(p) for p in prefixes], np.uint64), per("count", np.int64), per("balanced", np.int64), per("hcp", np.int64),
            per("length", np.int64), per("imp_sum", np.int64), per("imp_sq_sum", np.uint64))
