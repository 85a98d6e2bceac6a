"""Python restatement of the call review (include/brl_review.h) for the tests.  No tests in here.

``expand`` builds every branch table with tests/board_records_ref.py's encoder — the table of ``encode(dealer, calls[:t] + [a],
seating=..., tricks=..., hands=...)``, packed — and takes the void pattern from ``Table.legal``; ``values`` and ``summaries`` are
plain numpy written from the header's definitions (value, sign, tie rule), not from the kernel."""
import copy

import numpy as np

from brl_amd.boards import ILLEGAL, OK, RECORD_DTYPE, TERMINATED
from tests import board_records_ref as R

ACTIONS, VOID = 38, -128
# the IMP scale (the laws' table): a difference of at least STEPS[k] is worth k + 1 IMPs
STEPS = (20, 50, 90, 130, 170, 220, 270, 320, 370, 430, 500, 600, 750, 900, 1100, 1300, 1500, 1750, 2000, 2250, 2500, 3000, 3500, 4000)


def conv(diff: int) -> int:
    k = sum(1 for s in STEPS if abs(diff) >= s)
    return k if diff >= 0 else -k


def reviewable(r) -> bool:
    return bool(r["flags"] & OK) and not r["flags"] & ILLEGAL


def seating_of(r):
    return tuple((int(r["seating"]) >> (2 * s)) & 3 for s in range(4))


def empty_table(r, dda_row) -> R.Table:
    return R.Table(int(r["dealer"]), vul_ns=int(r["vul_ns"]), vul_ew=int(r["vul_ew"]), seating=seating_of(r),
                   tricks=np.asarray(dda_row).reshape(4, 5), hands=[int(h) for h in r["hands"]])


def packed_with_rewards(t: R.Table) -> np.ndarray:
    """``Table.pack()`` plus the rewards word table_step leaves on the call that ENDS an auction legally (the encoder keeps no
    rewards): every player gets the score of the side it sits on, int16 by player id"""
    w = t.pack()
    if t.term and not t.illegal:
        score_ns = int(R.decode(w[None, :])[0]["score_ns"])
        for seat, p in enumerate(t.seating):
            w[15] |= np.uint64(((score_ns if seat % 2 == 0 else -score_ns) & 0xFFFF) << (16 * p))
    return w


def counts(rec, depth):
    return np.array([min(int(r["n_calls"]), depth) if reviewable(r) else 0 for r in rec], np.int64)


def expand(rec, dda, depth):
    """-> (decisions: list of (board, t, seat, team, played), tables uint64 [D * 38, 16], void bool [D, 38], skipped).  The child
    of (t, a) is the prefix table of calls[:t] copied and stepped with a: the table of encode(dealer, calls[:t] + [a], ...)."""
    decisions, tables, void, skipped = [], [], [], 0
    for i, r in enumerate(rec):
        if not reviewable(r):
            skipped += 1
            continue
        prefix = empty_table(r, dda[i])
        seating = seating_of(r)
        for t in range(min(int(r["n_calls"]), depth)):
            seat = (int(r["dealer"]) + t) & 3
            played = int(r["calls"][t])
            decisions.append((i, t, seat, seating[seat] >> 1, played))
            row = []
            for a in range(ACTIONS):
                child = copy.copy(prefix)
                child.step(a)
                tables.append(packed_with_rewards(child))
                row.append(not prefix.legal(a))
            void.append(row)
            prefix.step(played)
    tables = np.stack(tables) if tables else np.zeros((0, 16), np.uint64)
    return decisions, tables, np.array(void, bool).reshape(-1, ACTIONS), skipped


def values(final, decisions, other):
    """int8 [D, 38]: ``final`` RECORD_DTYPE [D * 38] — the records of the final branch tables —, ``other`` the other table's records"""
    final = final.reshape(-1, ACTIONS)
    out = np.full((len(decisions), ACTIONS), VOID, np.int64)
    for d, (board, t, seat, team, played) in enumerate(decisions):
        s_o = int(other[board]["score_ns"])
        for a in range(ACTIONS):
            f = final[d, a]
            if f["flags"] & ILLEGAL or not f["flags"] & TERMINATED:
                continue
            imp_ns = conv(int(f["score_ns"]) - s_o)
            out[d, a] = imp_ns if seat % 2 == 0 else -imp_ns
    return out.astype(np.int8)


def summaries(imp, decisions):
    """{played, n_legal, played_imp, best_imp, best, loss} as int64 arrays [D]"""
    D = len(decisions)
    out = {k: np.zeros(D, np.int64) for k in ("played", "n_legal", "played_imp", "best_imp", "best", "loss")}
    for d, (board, t, seat, team, played) in enumerate(decisions):
        row = imp[d].astype(np.int64)
        legal = [a for a in range(ACTIONS) if row[a] != VOID]
        best_imp = max(row[a] for a in legal)
        best = played if row[played] == best_imp else min(a for a in legal if row[a] == best_imp)
        out["played"][d], out["n_legal"][d], out["played_imp"][d] = played, len(legal), row[played]
        out["best_imp"][d], out["best"][d], out["loss"][d] = best_imp, best, best_imp - row[played]
    return out


def as_records(tables_by_calls):
    """RECORD_DTYPE [n] from a list of Table objects"""
    return R.decode(np.stack([t.pack() for t in tables_by_calls])) if tables_by_calls else np.zeros(0, RECORD_DTYPE)
