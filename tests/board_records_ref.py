"""Python restatement of the board records (include/brl_boards.h) for the tests: a forward encoder (calls -> packed table, the
auction rules of bridge_device.hpp's table_step, illegal calls included) and the decoder (packed table -> record) the kernel
is compared with bit for bit."""
import numpy as np

from brl_amd.boards import FILL, ILLEGAL, MAX_CALLS, OK, PASSED_OUT, RECORD_DTYPE, TERMINATED

M64 = (1 << 64) - 1


class Table:
    """one packed table as Python integers"""

    def __init__(self, dealer=0, vul_ns=0, vul_ew=0, seating=(0, 1, 2, 3), tricks=None, hands=(0, 0, 0, 0)):
        self.hist = 0
        self.dealer, self.vul_ns, self.vul_ew, self.seating = dealer, vul_ns, vul_ew, tuple(seating)
        self.lb1 = self.lbseat = self.x = self.xx = self.npass = self.term = self.maskall = self.illegal = 0
        self.turn = self.steps = 0
        self.fd = 0
        self.tricks = np.zeros((4, 5), np.int64) if tricks is None else np.asarray(tricks, np.int64).reshape(4, 5)
        self.hands = tuple(int(h) for h in hands)

    def seat(self):
        return (self.dealer + self.turn) & 3

    def legal(self, a):
        if self.maskall:
            return True
        own = ((self.lbseat ^ self.seat()) & 1) == 0
        if a == 0:
            return True
        if a == 1:
            return bool(self.lb1 and not own and not self.x and not self.xx)
        if a == 2:
            return bool(self.lb1 and own and self.x and not self.xx)
        return a - 2 > self.lb1

    def step(self, a):
        """table_step: the call is applied whether legal or not; an illegal one ends the table"""
        if self.term:
            return
        bad = not self.legal(a)
        seat = self.seat()
        if a >= 3:
            den = (a - 3) % 5
            slot = (seat & 1) * 15 + den * 3
            if (self.fd >> slot) & 7 == 0:
                self.fd |= (seat + 1) << slot
            self.hist |= 1 << (8 + 12 * (a - 3) + seat)
            self.lb1, self.lbseat, self.x, self.xx = a - 2, seat, 0, 0
        elif a == 0:
            if self.lb1 == 0:
                self.hist |= 1 << (4 + seat)
        else:
            if self.lb1:
                self.hist |= 1 << (8 + 12 * (self.lb1 - 1) + 4 * a + seat)
            if a == 1:
                self.x = 1
            else:
                self.xx = 1
        self.npass = self.npass + 1 if a == 0 else 0
        over = self.npass == (3 if self.lb1 else 4)
        if over:
            self.term = self.maskall = 1
        self.steps += 1
        self.turn += 0 if over else 1
        if bad:
            self.term = self.illegal = self.maskall = 1

    def pack(self):
        w = [(self.hist >> (64 * i)) & M64 for i in range(7)]
        w += [(h << 4) & M64 for h in self.hands]
        shuf = sum(p << (2 * s) for s, p in enumerate(self.seating))
        sc = (self.dealer | self.vul_ns << 2 | self.vul_ew << 3 | shuf << 4 | self.lb1 << 12 | self.lbseat << 18 | self.x << 20
              | self.xx << 21 | self.npass << 22 | self.term << 25 | self.maskall << 26 | self.illegal << 27)
        sch = self.turn | self.steps << 9
        nib = [0] * 20
        for s in range(4):
            for d in range(5):
                nib[s * 5 + (4 - d)] = int(self.tricks[s, d])
        lo = sum(v << (4 * i) for i, v in enumerate(nib[:16]))
        hi = sum(v << (4 * i) for i, v in enumerate(nib[16:]))
        w += [sc | sch << 32, self.fd | hi << 32, lo, 0xFFFFFFFF, 0]
        return np.array(w, np.uint64)


def encode(dealer, calls, **kw):
    t = Table(dealer, **kw)
    for a in calls:
        t.step(int(a))
    return t


def contract_score(den, level, vul, x, xx, trick):
    """duplicate score of the declaring side (contract_score, bridge_device.hpp)"""
    u = level + 6 - trick
    if u > 0:
        if not (x or xx):
            return -(100 if vul else 50) * u
        pen = 300 * u - 100 if vul else (200 * u - 100 if u <= 3 else 300 * u - 400)
        return -(2 * pen if xx else pen)
    per = 20 if den <= 1 else 30
    points = (per * level + (10 if den == 4 else 0)) * (4 if xx else 2 if x else 1)
    sc = points + ((500 if vul else 300) if points >= 100 else 50)
    sc += ((750 if vul else 500) if level == 6 else 0) + ((1500 if vul else 1000) if level == 7 else 0)
    sc += 100 if xx else 50 if x else 0
    ov = ((400 if vul else 200) if xx else (200 if vul else 100) if x else per)
    return sc + (-u) * ov


def calls_of(hist, dealer, lb1, lbseat, dbl, npass, turn, term, illegal):
    """(calls, ok): the sequence of a table's history words — include/brl_boards.h, rule by rule"""
    hist &= ((1 << 428) - 1) & ~0xF
    lost = bool(illegal and not dbl and lb1)
    actor = (dealer + turn - 1) & 3
    if illegal and lb1:
        g = 8 + 12 * (lb1 - 1)
        own = ((actor ^ lbseat) & 1) == 0
        hist &= ~(1 << (g + 8 + actor))
        if own or (hist >> (g + 4 + (actor ^ 2))) & 1:
            hist &= ~(1 << (g + 4 + actor))
    opening = bin((hist >> 4) & 15).count("1")
    calls = [0] * opening
    prev = (dealer + opening - 1) & 3
    ev = hist >> 8
    events = ev != 0
    e = 0
    while ev:
        if ev & 1:
            bid, r = divmod(e, 12)
            kind, seat = r >> 2, r & 3
            calls += [0] * ((seat - prev - 1) & 3) + [3 + bid if kind == 0 else kind]
            prev = seat
        ev >>= 1
        e += 1
    calls += [0] * (((actor - prev - 1) & 3) if illegal else (npass if events else 0))
    want = turn - 1 if illegal else turn + 1 if term else turn
    ok = (not lost) and len(calls) == want and len(calls) < MAX_CALLS
    return ([] if lost else calls[:MAX_CALLS - 1]), ok


def decode(packed):
    """uint64 [n,16] -> RECORD_DTYPE [n]: what brl_board_records writes"""
    packed = np.asarray(packed).view(np.uint64).reshape(-1, 16)
    out = np.zeros(packed.shape[0], RECORD_DTYPE)
    for i, w in enumerate(packed):
        w = [int(v) for v in w]
        hist = sum(w[k] << (64 * k) for k in range(7))
        sc, sch = w[11] & 0xFFFFFFFF, w[11] >> 32
        dealer, vns, vew, shuf = sc & 3, (sc >> 2) & 1, (sc >> 3) & 1, (sc >> 4) & 0xFF
        lb1, lbseat, x, xx, npass = (sc >> 12) & 63, (sc >> 18) & 3, (sc >> 20) & 1, (sc >> 21) & 1, (sc >> 22) & 7
        term, illegal, turn = (sc >> 25) & 1, (sc >> 27) & 1, sch & 511
        calls, ok = calls_of(hist, dealer, lb1, lbseat, x | xx, npass, turn, term, illegal)
        r = out[i]
        r["n_calls"], r["dealer"], r["vul_ns"], r["vul_ew"], r["seating"] = len(calls), dealer, vns, vew, shuf
        r["flags"] = (TERMINATED if term else 0) | (PASSED_OUT if term and not illegal and lb1 == 0 else 0) | \
            (ILLEGAL if illegal else 0) | (OK if ok else 0)
        r["calls"][:] = FILL
        r["calls"][:len(calls)] = calls
        r["hands"] = [w[7 + s] >> 4 for s in range(4)]
        if term and not illegal and lb1:
            level, den = divmod(lb1 - 1, 5)
            level += 1
            side = lbseat & 1
            fd = w[12] & 0xFFFFFFFF
            decl = (((fd >> (side * 15 + den * 3)) & 7) - 1) & 3
            nibs = w[13] | (w[12] >> 32) << 64
            tricks = (nibs >> (4 * (decl * 5 + 4 - den))) & 15
            s = contract_score(den, level, vew if side else vns, x, xx, tricks)
            r["level"], r["strain"], r["doubled"], r["declarer"], r["tricks"] = level, den, 2 if xx else x, decl, tricks
            r["score_ns"] = -s if side else s
    return out


# ---- auctions -----------------------------------------------------------------------------------------------------------------
def longest_auction():
    """the 319 calls: P P P, then every bid followed by P P X P P XX P P, and the final pass"""
    calls = [0, 0, 0]
    for b in range(35):
        calls += [3 + b, 0, 0, 1, 0, 0, 2, 0, 0]
    return calls + [0]


def random_auction(rng, stop=None, p_pass=0.55):
    """a random legal auction from the dealer's first call to the end (or ``stop`` calls): list of action ids"""
    t = Table(0)
    calls = []
    while not t.term and (stop is None or len(calls) < stop):
        legal = [a for a in range(38) if t.legal(a)]
        if rng.random() < p_pass:
            a = 0
        else:
            near = [a for a in legal if a < 3 or a - 2 <= t.lb1 + 2]   # low bids: long auctions
            a = int(rng.choice(near))
        calls.append(a)
        t.step(a)
    return calls
