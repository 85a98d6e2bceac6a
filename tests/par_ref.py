"""Two restatements of the double-dummy par (include/brl_par.h holds the definition) for the tests (a helper: no tests in
here).  They share no code with the product and only the scorer with each other:

* ``par_brute`` — a memoised recursion straight from the definition: the value of every position (who holds which bid), the
  root for either first side, and the par contracts by quantifying over every overcall.
* ``par_scan`` — the backward scan over b = 34..0 that carries the two suffix optima, and a second scan for the masks.

Both score with ``contract_matrix.law_score`` (written from the Laws), and both return
``(R, R_alt, mask_ns, mask_ew)`` for a first side (0 = North-South deals, 1 = East-West), the masks under the strict rule.

A trick count of 14 or 15 (what the kernel's ``& 15`` lets through) lies outside the Laws' table: ``score`` extends it
linearly, every trick beyond 13 another overtrick.
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np

from tests.contract_matrix import law_score

NS, EW = 0, 1
PASSED_OUT, DEALER_DEPENDENT = 1, 2        # BRL_PAR_* flags
NO_RESULT = -2 ** 31                       # BRL_PAR_NO_RESULT


def score(strain, level, vul, doubling, tricks):
    if tricks <= 13:
        return law_score(strain, level, vul, doubling, tricks)
    assert doubling == 0                   # 14 tricks make every contract, and a making contract is undoubled here
    overtrick = law_score(strain, 1, vul, 0, 8) - law_score(strain, 1, vul, 0, 7)
    return law_score(strain, level, vul, 0, 13) + (tricks - 13) * overtrick


def side_tricks(table):
    """[side][strain] from the 20 counts [seat * 5 + strain]: the better of the side's two seats"""
    t = [int(v) for v in np.asarray(table).reshape(20)]
    return tuple(tuple(max(t[seat * 5 + d], t[(seat + 2) * 5 + d]) for d in range(5)) for seat in (0, 1))


def outcome(tricks, vul, side, b):
    """o(s, b): North-South's score when ``side`` plays bid ``b``"""
    level, strain = b // 5 + 1, b % 5
    t = tricks[side][strain]
    s = score(strain, level, vul[side], 0 if t >= level + 6 else 1, t)
    return s if side == NS else -s


def better(side, a, b):
    """is ``a`` strictly better than ``b`` for ``side``?"""
    return a > b if side == NS else a < b


def best(side, values):
    return max(values) if side == NS else min(values)


# ---- straight from the definition ------------------------------------------------------------------------------------------------
def par_brute(table, vul_ns, vul_ew, first):
    tricks, vul = side_tricks(table), (int(vul_ns), int(vul_ew))

    @lru_cache(maxsize=None)
    def value(side, b):
        """V(side, b): ``side`` holds ``b``, the other side acts — it passes, or bids any higher contract"""
        other = 1 - side
        options = [outcome(tricks, vul, side, b)] + [value(other, c) for c in range(b + 1, 35)]
        return best(other, options)

    def root(d):
        other = 1 - d
        after_pass = best(other, [value(other, b) for b in range(35)] + [0])
        return best(d, [value(d, b) for b in range(35)] + [after_pass])

    r, r_alt = root(first), root(1 - first)
    masks = []
    for side in (NS, EW):
        other, m = 1 - side, 0
        for b in range(35):
            # every overcall c ends strictly worse for the other side than par — that is, strictly better for this one
            if outcome(tricks, vul, side, b) == r and all(better(side, value(other, c), r) for c in range(b + 1, 35)):
                m |= 1 << b
        masks.append(m)
    return r, r_alt, masks[0], masks[1]


# ---- the backward scan --------------------------------------------------------------------------------------------------------
def par_scan(table, vul_ns, vul_ew, first):
    tricks, vul = side_tricks(table), (int(vul_ns), int(vul_ew))
    inf = 10 ** 9
    o = [[outcome(tricks, vul, side, b) for b in range(35)] for side in (NS, EW)]

    def sweep(r=None):
        top_ns, low_ew = -inf, inf            # max V(NS, b') and min V(EW, b') over b' > b
        m_ns = m_ew = 0
        for b in range(34, -1, -1):
            if r is not None:
                if o[NS][b] == r and low_ew > r:
                    m_ns |= 1 << b
                if o[EW][b] == r and top_ns < r:
                    m_ew |= 1 << b
            v_ns, v_ew = min(o[NS][b], low_ew), max(o[EW][b], top_ns)
            top_ns, low_ew = max(top_ns, v_ns), min(low_ew, v_ew)
        return top_ns, low_ew, m_ns, m_ew

    top_ns, low_ew, _, _ = sweep()
    roots = (max(top_ns, min(low_ew, 0)), min(low_ew, max(top_ns, 0)))
    r, r_alt = roots[first], roots[1 - first]
    _, _, m_ns, m_ew = sweep(r)
    return r, r_alt, m_ns, m_ew


def par_records(dda, dealer, vul_ns, vul_ew, solver=par_scan):
    """what brl_par writes for the boards, as a list of (score_ns, score_ns_alt, flags, contracts_ns, contracts_ew): the table
    is masked ``& 15`` and the dealer ``& 3`` as the kernel masks them"""
    dda = np.asarray(dda).reshape(-1, 20)
    out = []
    for i in range(dda.shape[0]):
        r, r_alt, m_ns, m_ew = solver(dda[i].astype(np.int64) & 15, int(vul_ns[i]) & 1, int(vul_ew[i]) & 1, int(dealer[i]) & 1)
        flags = (PASSED_OUT if r == 0 and not (m_ns | m_ew) else 0) | (DEALER_DEPENDENT if r != r_alt else 0)
        out.append((r, r_alt, flags, m_ns, m_ew))
    return out


# ---- the worked boards ----------------------------------------------------------------------------------------------------------
C, D, H, S, NT = range(5)


def table_of(ns=None, ew=None, fill=6):
    """a 20-count table: ``ns`` / ``ew`` = {strain: tricks} for both seats of the side, every other entry ``fill``"""
    t = np.full((4, 5), fill, np.uint8)
    for seats, given in (((0, 2), ns or {}), ((1, 3), ew or {})):
        for strain, n in given.items():
            for seat in seats:
                t[seat, strain] = n
    return t.reshape(20)


def bid(name):
    """"4S" -> the bid index"""
    return (int(name[0]) - 1) * 5 + ("C", "D", "H", "S", "NT").index(name[1:])


def bits(*names):
    return sum(1 << bid(n) for n in names)


# name: (table, vul_ns, vul_ew, {first side: (R, P(NS), P(EW))})
WORKED = {
    "A": (table_of({S: 10}, {S: 3, H: 8}), 0, 0, {NS: (420, bits("4S"), 0), EW: (420, bits("4S"), 0)}),
    "B": (table_of({S: 10}, {S: 3, H: 9}), 0, 0, {NS: (300, 0, bits("5H")), EW: (300, 0, bits("5H"))}),
    "B'": (table_of({S: 10}, {S: 3, H: 9}), 0, 1, {NS: (420, bits("4S"), 0), EW: (420, bits("4S"), 0)}),
    "C": (table_of({NT: 7}, {NT: 7}), 0, 0, {NS: (90, bits("1NT"), 0), EW: (-90, 0, bits("1NT"))}),
    "D": (table_of(), 0, 0, {NS: (0, 0, 0), EW: (0, 0, 0)}),
    "E": (table_of({C: 10}), 1, 0, {NS: (130, bits("2C", "3C", "4C"), 0), EW: (130, bits("2C", "3C", "4C"), 0)}),
}


def worked_flags(name):
    if name == "C":
        return DEALER_DEPENDENT
    return PASSED_OUT if name == "D" else 0
