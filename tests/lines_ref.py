"""Python restatement of the auction lines (include/brl_lines.h) for the tests, in numpy float64.  No tests in here.

Tables are stepped by tests/board_records_ref.py's ``Table`` (the auction rules of table_step) and packed the way
tests/review_ref.py packs a branch (the rewards word of the call that ends an auction); the log-softmax, the candidate order, the
selection, the flags and the K x K sum are written from the header's definition, not from the kernel."""
import copy

import numpy as np

from tests import board_records_ref as R
from tests import review_ref as V

EMPTY, FINISHED, VOID, GREEDY = 1, 2, 4, 8
FILL, ACTIONS = 0xFF, 38


def table_of(w):
    """(``R.Table``, word 14) of a packed LIVE or finished table uint64 [16]"""
    w = [int(v) for v in np.asarray(w).view(np.uint64).reshape(16)]
    sc, sch = w[11] & 0xFFFFFFFF, w[11] >> 32
    nibs = w[13] | (w[12] >> 32) << 64
    tricks = np.zeros((4, 5), np.int64)
    for s in range(4):
        for d in range(5):
            tricks[s, d] = (nibs >> (4 * (s * 5 + 4 - d))) & 15
    t = R.Table(sc & 3, vul_ns=(sc >> 2) & 1, vul_ew=(sc >> 3) & 1, seating=tuple((sc >> (4 + 2 * s)) & 3 for s in range(4)),
                tricks=tricks, hands=[w[7 + s] >> 4 for s in range(4)])
    t.hist = sum(w[k] << (64 * k) for k in range(7))
    t.lb1, t.lbseat, t.x, t.xx, t.npass = (sc >> 12) & 63, (sc >> 18) & 3, (sc >> 20) & 1, (sc >> 21) & 1, (sc >> 22) & 7
    t.term, t.maskall, t.illegal = (sc >> 25) & 1, (sc >> 26) & 1, (sc >> 27) & 1
    t.turn, t.steps, t.fd = sch & 511, (sch >> 9) & 1023, w[12] & 0xFFFFFFFF
    return t, w[14]


def pack(t, w14):
    w = V.packed_with_rewards(t)
    w[14] = np.uint64(w14)
    return w


class Line:
    def __init__(self, table=None, w14=0, calls=(), score=-np.inf, flags=EMPTY):
        self.table, self.w14, self.calls, self.score, self.flags = table, w14, list(calls), np.float64(score), flags

    def packed(self):
        return np.zeros(16, np.uint64) if self.flags & EMPTY else pack(self.table, self.w14)

    def live(self):
        return not self.flags & (EMPTY | FINISHED | VOID)

    def player(self):
        return self.table.seating[self.table.seat()]


def initial_beam(packed, k):
    """step 0's beam of one dealt table (call t of the table's auction is calls[t]: a table that comes with calls already made
    leaves their places at ``FILL``)"""
    t, w14 = table_of(packed)
    return [Line(t, w14, [FILL] * t.steps, 0.0, GREEDY | (FINISHED if t.term else 0))] + [Line() for _ in range(k - 1)]


def log_softmax(logits, legal):
    """(terms float64 [38] (nan where illegal), the greedy call, void) of one float32 row: the header's order of operations"""
    l32 = np.asarray(logits, np.float32)
    mx32, greedy, bad = np.float32(-np.inf), 0, False
    found = False
    for a in range(ACTIONS):
        if legal[a]:
            v = l32[a]
            bad |= bool(np.isnan(v) or v == np.inf)
            if v > mx32:
                mx32, greedy, found = v, a, True
    bad |= not found
    terms = np.full(ACTIONS, np.nan)
    if bad:
        return terms, greedy if found else 0, True
    mx, z = np.float64(mx32), np.float64(0.0)
    with np.errstate(all="ignore"):
        for a in range(ACTIONS):
            if legal[a]:
                z = z + np.exp(np.float64(l32[a]) - mx)
        lz = np.log(z)
        for a in range(ACTIONS):
            if legal[a]:
                terms[a] = (np.float64(l32[a]) - mx) - lz
    return terms, greedy, False


def candidates(beam, logits_of):
    """every candidate of one board's step as (void, score, slot, action, greedy), unsorted; ``logits_of(slot, line)`` -> the
    float32 row of a live line"""
    out = []
    for s, ln in enumerate(beam):
        if ln.flags & EMPTY:
            continue
        if not ln.live():
            out.append((1 if ln.flags & VOID else 0, ln.score, s, -1, bool(ln.flags & GREEDY)))
            continue
        legal = [ln.table.legal(a) for a in range(ACTIONS)]
        terms, greedy, void = log_softmax(logits_of(s, ln), legal)
        if void:
            out.append((1, ln.score, s, -1, bool(ln.flags & GREEDY)))
            continue
        for a in range(ACTIONS):
            if legal[a]:
                with np.errstate(all="ignore"):
                    out.append((0, ln.score + terms[a], s, a, bool(ln.flags & GREEDY) and a == greedy))
    return out


def order(cands):
    """the total order: void lines last, score descending, parent slot ascending, action ascending"""
    return sorted(cands, key=lambda c: (c[0], -c[1], c[2], c[3]))


def separation(cands, k):
    """the smallest gap between two different scores among the candidates that are not void and not -inf, and the gap between the
    k-th and the (k+1)-th candidate (inf when there is none or they are an exact tie broken by slot / action)"""
    sc = sorted({float(c[1]) for c in cands if not c[0] and np.isfinite(c[1])}, reverse=True)
    gaps = [a - b for a, b in zip(sc, sc[1:])]
    o = order(cands)
    edge = np.inf
    if len(o) > k and not o[k - 1][0] and not o[k][0] and o[k - 1][1] != o[k][1]:
        edge = float(o[k - 1][1] - o[k][1])
    return (min(gaps) if gaps else np.inf), edge


def expand(beam, logits_of, k):
    """(the next beam, the candidates) of one board"""
    cands = candidates(beam, logits_of)
    new = []
    for void, score, s, a, greedy in order(cands)[:k]:
        parent = beam[s]
        if a < 0:
            new.append(Line(parent.table, parent.w14, parent.calls, score, (parent.flags & (FINISHED | GREEDY)) | (VOID if void else 0)))
            continue
        t = copy.copy(parent.table)
        t.step(a)
        new.append(Line(t, parent.w14, parent.calls + [a], score, (FINISHED if t.term else 0) | (GREEDY if greedy else 0)))
    return new + [Line() for _ in range(k - len(new))], cands


def beam_arrays(beams, k, max_calls):
    """what the kernels leave for a list of boards' beams: tables uint64 [n*K,16], calls, score, flags, request (board, slot,
    player, team), done"""
    n = len(beams)
    tables = np.zeros((n * k, 16), np.uint64)
    calls = np.full((n * k, max_calls), FILL, np.uint8)
    score = np.full(n * k, -np.inf)
    flags = np.zeros(n * k, np.uint8)
    request = np.zeros((n * k, 4), np.int32)
    done = np.ones(n, np.uint8)
    for b, beam in enumerate(beams):
        for s, ln in enumerate(beam):
            i = b * k + s
            tables[i], score[i], flags[i] = ln.packed(), ln.score, ln.flags
            calls[i, :len(ln.calls)] = ln.calls[:max_calls]
            request[i] = (b, s, ln.player(), ln.player() >> 1) if ln.live() else (-1, s, 0, 0)
            if ln.live():
                done[b] = 0
    return {"tables": tables, "calls": calls, "score": score, "flags": flags, "request": request, "done": done}


def result(ln):
    """the ``RESULT`` fields of a line: board_records_ref's decoder applied to the final table"""
    zero = dict(has_result=0, score_ns=0, level=0, strain=0, doubled=0, declarer=0, tricks=0, score_team1=0)
    if not (ln.flags & FINISHED) or ln.flags & (VOID | EMPTY):
        return zero
    r = R.decode(ln.packed()[None, :])[0]
    seat0 = ln.table.seating.index(0)
    s = int(r["score_ns"])
    return dict(has_result=1, score_ns=s, level=int(r["level"]), strain=int(r["strain"]), doubled=int(r["doubled"]),
                declarer=int(r["declarer"]), tricks=int(r["tricks"]), score_team1=s if seat0 % 2 == 0 else -s)


def observe(t):
    """uint8 [480]: the observation of the player to act at ``R.Table`` t (bridge_device.hpp's emit_obs_row: the history with
    every nibble turned to seats relative to the observer, the vulnerability nibble, the observer's hand from bit 428)"""
    seat = t.seat()
    o = 0
    for q in range(1, 107):
        nib = (t.hist >> (4 * q)) & 15
        o |= (((nib >> seat) | (nib << (4 - seat))) & 15) << (4 * q)
    we, they = (t.vul_ew, t.vul_ns) if seat & 1 else (t.vul_ns, t.vul_ew)
    o |= (2 if we else 1) | (8 if they else 4)
    o |= (t.hands[seat] & ((1 << 52) - 1)) << 428
    return np.array([(o >> i) & 1 for i in range(480)], np.uint8)


def search(packed, forward, k, max_calls, on_step=None):
    """the whole search of one table's dealt tables on the host: ``forward(team, obs uint8 [m,480]) -> float32 [m,38]``;
    -> the boards' final beams.  ``on_step(step, board, candidates)`` sees every board's candidate list."""
    beams = [initial_beam(w, k) for w in packed]
    for step in range(max_calls):
        live = [(b, s) for b, beam in enumerate(beams) for s, ln in enumerate(beam) if ln.live()]
        if not live:
            break
        rows = {}
        for team in (0, 1):
            idx = [(b, s) for b, s in live if beams[b][s].player() >> 1 == team]
            if idx:
                lg = np.asarray(forward(team, np.stack([observe(beams[b][s].table) for b, s in idx])), np.float32)
                rows.update({bs: lg[i] for i, bs in enumerate(idx)})
        for b in range(len(beams)):
            beams[b], cands = expand(beams[b], lambda s, ln, b=b: rows[(b, s)], k)
            if on_step is not None:
                on_step(step, b, cands)
    return beams


def board_sums(pa, ua, pb, ub):
    """(S, c) of one board: ``pa`` / ``pb`` float64 [K] — a finished line's probability, 0.0 for any other slot —, ``ua`` / ``ub``
    their scores from player 0's side; the header's symmetric order"""
    k = len(pa)
    term = lambda i, j: (np.float64(pa[i]) * np.float64(pb[j])) * np.float64(V.conv(int(ua[i]) + int(ub[j])))   # noqa: E731
    S = np.float64(0.0)
    for m in range(k):
        S = S + term(m, m)
        for j in range(m):
            S = S + (term(m, j) + term(j, m))
    ca = cb = np.float64(0.0)
    for s in range(k):
        ca, cb = ca + np.float64(pa[s]), cb + np.float64(pb[s])
    return S, ca * cb


def masses(score, flags, has_result):
    """(covered, open, void) of one table's beam, in slot order"""
    covered = opened = voided = np.float64(0.0)
    for s in range(len(score)):
        f = int(flags[s])
        with np.errstate(all="ignore"):
            p = np.float64(0.0) if f & EMPTY else np.exp(np.float64(score[s]))
        if (f & (EMPTY | FINISHED | VOID)) == FINISHED and has_result[s]:
            covered = covered + p
        if not f & (EMPTY | FINISHED | VOID):
            opened = opened + p
        if f & VOID and not f & EMPTY:
            voided = voided + p
    return covered, opened, voided
