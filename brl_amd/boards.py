"""Board records: named deals in; auctions, contracts and scores out (include/brl_boards.h).

* ``read_deals(path)`` — a deal file in the shape of the reference's ``wb5/dataset_for_vs_wb5.json`` or in PBN, as the arrays
  ``BridgeBidding.init_from_deals`` takes.  The first bad board is rejected with its number (``sl_data.py``'s style).
* ``board_records(packed)`` — one ``brl_board_records`` launch: the packed tables as fixed-size records.
* ``BoardRecords`` — both tables' records of a match, with named accessors, ``to_json`` and ``to_pbn``.
* ``make_board_match`` — ``make_simple_duplicate_evaluate`` that also returns the records of every board.

Card naming has one home here: ``card_bit`` / ``bit_card`` (``"C6"`` <-> the observation's hand bit rank * 4 + suit,
wb5/utils.py:18-26), used by both directions.
"""
from __future__ import annotations

import json
import re
from typing import NamedTuple

import numpy as np

SEATS = "NESW"
SUITS = "CDHS"              # the observation's suit order
RANKS = "23456789TJQKA"     # and rank order: hand bit = rank * 4 + suit (wb5/utils.py:18-19)
STRAINS = ("C", "D", "H", "S", "NT")
VULS = ("None", "NS", "EW", "Both")   # the dataset's names, indexed by vul_ns + 2 * vul_ew

MAX_CALLS = 320             # BRL_BOARD_MAX_CALLS
FILL = 0xFF                 # BRL_BOARD_FILL
TERMINATED, PASSED_OUT, ILLEGAL, OK = 1, 2, 4, 8   # BRL_BOARD_* flags

RECORD_DTYPE = np.dtype([("n_calls", "<u2"), ("dealer", "u1"), ("vul_ns", "u1"), ("vul_ew", "u1"), ("flags", "u1"),
                         ("level", "u1"), ("strain", "u1"), ("doubled", "u1"), ("declarer", "u1"), ("tricks", "u1"),
                         ("seating", "u1"), ("score_ns", "<i4"), ("hands", "<u8", 4), ("calls", "u1", MAX_CALLS)])
assert RECORD_DTYPE.itemsize == 368

CALL_NAMES = ["P", "X", "XX"] + [f"{lv}{s}" for lv in range(1, 8) for s in STRAINS]


# ---- the one card mapping ------------------------------------------------------------------------------------------------------
def card_bit(name: str) -> int:
    """``"C6"`` -> the hand bit rank * 4 + suit (suits C,D,H,S; ranks 2..A)"""
    if len(name) != 2 or name[0] not in SUITS or name[1] not in RANKS:
        raise ValueError(f"not a card: {name!r}")
    return RANKS.index(name[1]) * 4 + SUITS.index(name[0])


def bit_card(bit: int) -> str:
    return SUITS[bit & 3] + RANKS[bit >> 2]


def hand_names(word: int):
    """one seat's cards from its hand word, ascending by (suit, rank) like the dataset: ["C6", "C8", ...]"""
    w = int(word)
    return sorted((bit_card(b) for b in range(52) if (w >> b) & 1), key=lambda c: (SUITS.index(c[0]), RANKS.index(c[1])))


def pbn_deal(words) -> str:
    """the PBN deal string ``N:spades.hearts.diamonds.clubs E S W`` (ranks high to low) of four hand words"""
    hands = []
    for w in words:
        names = hand_names(w)
        hands.append(".".join("".join(sorted((c[1] for c in names if c[0] == s), key=RANKS.index, reverse=True)) for s in "SHDC"))
    return "N:" + " ".join(hands)


# ---- deals in ------------------------------------------------------------------------------------------------------------------
class Deals(NamedTuple):
    """what ``init_from_deals`` takes: ``env.init_from_deals(d.hand, d.dealer, d.vul_ns, d.vul_ew, [0, 1, 2, 3], d.tricks)``"""
    hand: np.ndarray       # int32 [n,52]: 13 pgx card ids (suit S,H,D,C * 13 + rank A,2..K) per seat N,E,S,W, ascending
    dealer: np.ndarray     # int32 [n]
    vul_ns: np.ndarray     # uint8 [n]
    vul_ew: np.ndarray     # uint8 [n]
    tricks: np.ndarray     # uint8 [n,20]: [declarer seat][C,D,H,S,NT]
    board_id: np.ndarray   # int64 [n]

    @property
    def n(self) -> int:
        return int(self.hand.shape[0])

    def hand_words(self) -> np.ndarray:
        """uint64 [n,4]: the records' form of the hands"""
        bits = _pgx_to_bit(self.hand.astype(np.int64)).reshape(-1, 4, 13).astype(np.uint64)
        return np.bitwise_or.reduce(np.left_shift(np.uint64(1), bits), axis=2)

    def lut_keys(self) -> np.ndarray:
        """int32 [n,4]: the pgx double-dummy table's key of every deal (one word per suit S,H,D,C: 13 base-4 digits, most
        significant first, = the seat that owns card suit * 13 + rank)"""
        n = self.n
        owner = np.zeros((n, 52), np.int64)
        owner[np.arange(n)[:, None], self.hand] = np.repeat(np.arange(4), 13)[None, :]
        return (owner.reshape(n, 4, 13) * (4 ** np.arange(12, -1, -1, dtype=np.int64))).sum(-1).astype(np.int32)

    def lut_values(self) -> np.ndarray:
        """int32 [n,4]: the table's value words (one per declarer seat: 5 hex digits C,D,H,S,NT, most significant first)"""
        t = self.tricks.reshape(-1, 4, 5).astype(np.int64)
        return (t * (16 ** np.arange(4, -1, -1, dtype=np.int64))).sum(-1).astype(np.int32)


def _bit_to_pgx(bit):
    bit = np.asarray(bit)
    return (3 - bit % 4) * 13 + (bit // 4 + 1) % 13


def _pgx_to_bit(card):
    card = np.asarray(card)
    return ((card % 13 + 12) % 13) * 4 + (3 - card // 13)


class MalformedDeals(ValueError):
    pass


def _reject(board, what):
    raise MalformedDeals(f"board {int(board)}: {what}")


def _deals_from_named(boards) -> Deals:
    """boards: list of dicts {board_id, dealer, deal{N,E,S,W: [names]}, vulnerability, dda{seat{strain}}} (the dataset's shape)"""
    n = len(boards)
    if n == 0:
        raise MalformedDeals("no boards")
    hand = np.zeros((n, 52), np.int32)
    dealer = np.zeros(n, np.int32)
    vns, vew = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    tricks = np.zeros((n, 20), np.uint8)
    board_id = np.zeros(n, np.int64)
    for i, b in enumerate(boards):
        deal = b.get("deal")
        if not isinstance(deal, dict) or sorted(deal) != sorted(SEATS):
            _reject(i, "the deal does not name the four seats N, E, S, W")
        seen = set()
        for s, seat in enumerate(SEATS):
            cards = deal[seat]
            if len(cards) != 13:
                _reject(i, f"{seat} holds {len(cards)} cards, not 13")
            try:
                bits = [card_bit(c) for c in cards]
            except ValueError as e:
                _reject(i, str(e))
            seen.update(bits)
            hand[i, s * 13:(s + 1) * 13] = np.sort(_bit_to_pgx(np.array(bits)))
        if len(seen) != 52:
            _reject(i, f"{len(seen)} distinct cards, not 52")
        if b.get("dealer") not in tuple(SEATS):
            _reject(i, f"unknown dealer {b.get('dealer')!r}")
        dealer[i] = SEATS.index(b["dealer"])
        if b.get("vulnerability") not in VULS:
            _reject(i, f"unknown vulnerability {b.get('vulnerability')!r}")
        v = VULS.index(b["vulnerability"])
        vns[i], vew[i] = v & 1, v >> 1
        dda = b.get("dda")
        for s, seat in enumerate(SEATS):
            for d, st in enumerate(STRAINS):
                try:
                    t = dda[seat][st]
                except (KeyError, TypeError):
                    _reject(i, f"double-dummy tricks of {seat} in {st} are missing")
                if not isinstance(t, (int, np.integer)) or not 0 <= t <= 13:
                    _reject(i, f"double-dummy tricks of {seat} in {st} are {t!r}, not 0..13")
                tricks[i, s * 5 + d] = t
        board_id[i] = int(b.get("board_id", i))
    return Deals(hand, dealer, vns, vew, tricks, board_id)


_PBN_TAG = re.compile(r'^\[(\w+)\s+"(.*)"\]\s*$')
_PBN_VUL = {"none": "None", "love": "None", "-": "None", "ns": "NS", "ew": "EW", "all": "Both", "both": "Both"}


def _pbn_games(text):
    """the games of a PBN text as (tags dict, OptimumResultTable rows); games of the closed room (a duplicate board's second
    table, as ``to_pbn`` writes it) are skipped"""
    games, tags, rows, section = [], {}, [], None
    for line in text.split("\n") + [""]:
        line = line.strip()
        if not line:
            if tags:
                games.append((tags, rows))
            tags, rows, section = {}, [], None
            continue
        if line[0] in "%;":
            continue
        m = _PBN_TAG.match(line)
        if m:
            tags[m.group(1)] = m.group(2)
            section = m.group(1)
        elif section == "OptimumResultTable":
            rows.append(line.split())
    return [g for g in games if g[0].get("Room", "Open") != "Closed"]


def _named_from_pbn(text):
    boards = []
    for i, (tags, rows) in enumerate(_pbn_games(text)):
        b = {"board_id": int(tags["Board"]) if tags.get("Board", "").lstrip("-").isdigit() else i, "dealer": tags.get("Dealer"),
             "vulnerability": _PBN_VUL.get(tags.get("Vulnerable", "?").lower(), tags.get("Vulnerable"))}
        deal = tags.get("Deal", "")
        parts = deal[2:].split()
        if len(deal) < 2 or deal[0] not in SEATS or deal[1] != ":" or len(parts) != 4 or any(len(p.split(".")) != 4 for p in parts):
            _reject(i, "the Deal tag is not 'S:spades.hearts.diamonds.clubs x4'")
        first = SEATS.index(deal[0])
        b["deal"] = {SEATS[(first + k) % 4]: [s + r for s, rs in zip("SHDC", p.split(".")) for r in rs] for k, p in enumerate(parts)}
        dda = {}
        if "DoubleDummyTricks" in tags:   # 20 hex digits: declarers N,S,E,W x strains NT,S,H,D,C
            dd = tags["DoubleDummyTricks"]
            if len(dd) == 20 and all(ch in "0123456789abcdefABCDEF" for ch in dd):
                for k, seat in enumerate("NSEW"):
                    dda[seat] = {st: int(dd[k * 5 + j], 16) for j, st in enumerate(("NT", "S", "H", "D", "C"))}
        for row in rows:                  # "N NT 7"
            if len(row) == 3 and row[2].isdigit():
                dda.setdefault(row[0], {})[row[1]] = int(row[2])
        b["dda"] = dda
        boards.append(b)
    return boards


def read_deals(path: str) -> Deals:
    """a deal file -> ``Deals``: JSON in the dataset's shape ``{"logs": [{board_id, dealer, deal, vulnerability, dda}]}`` (what
    ``BoardRecords.to_json`` writes is read back too), or PBN with a ``DoubleDummyTricks`` or ``OptimumResultTable`` tag.
    ``MalformedDeals`` names the first bad board (0-based position in the file)."""
    with open(path) as f:
        text = f.read()
    if text.lstrip().startswith("{"):
        doc = json.loads(text)
        if not isinstance(doc, dict) or not isinstance(doc.get("logs"), list):
            raise MalformedDeals('no {"logs": [...]} list')
        return _deals_from_named(doc["logs"])
    return _deals_from_named(_named_from_pbn(text))


# ---- records out ---------------------------------------------------------------------------------------------------------------
def board_records(packed):
    """uint8 [n,368] on the device: ``brl_board_records`` of the packed tables (int64 [n,16]) — one launch on the current stream,
    no synchronisation"""
    import torch

    from . import _capi
    n = packed.shape[0]
    out = torch.empty((n, RECORD_DTYPE.itemsize), dtype=torch.uint8, device=packed.device)
    _capi.check(_capi.lib().brl_board_records(_capi.device_index(packed), _capi.ptr(packed), n, _capi.ptr(out),
                                              _capi.stream(_capi.device_index(packed))))
    return out


def board_imp(rec_a, rec_b):
    """int32 [n] on the device: ``brl_board_imp`` — per board the IMP of the pair that sits North-South at table A"""
    import torch

    from . import _capi
    n = rec_a.shape[0]
    out = torch.empty(n, dtype=torch.int32, device=rec_a.device)
    _capi.check(_capi.lib().brl_board_imp(_capi.device_index(rec_a), _capi.ptr(rec_a), _capi.ptr(rec_b), n, _capi.ptr(out),
                                          _capi.stream(_capi.device_index(rec_a))))
    return out


def _checked(rec: np.ndarray, what: str) -> np.ndarray:
    bad = np.nonzero((rec["flags"] & OK) == 0)[0]
    if bad.size:
        raise ValueError(f"{what}: record {int(bad[0])} fails the self-check (n_calls against _turn, include/brl_boards.h); "
                         f"{bad.size} of {rec.shape[0]} do: not records of an auction")
    return rec


def _structured(x, what):
    if isinstance(x, np.ndarray):
        rec = x if x.dtype == RECORD_DTYPE else np.ascontiguousarray(x).view(RECORD_DTYPE).reshape(-1)
    else:
        rec = x.detach().cpu().contiguous().numpy().view(RECORD_DTYPE).reshape(-1)
    return _checked(rec, what)


class BoardRecords:
    """The records of a match: table A's and (a duplicate match) table B's, the IMP per board and the deals' full double-dummy
    tables.  ``table_a`` / ``table_b``: uint8 [n,368] device tensors (``board_records``) or numpy structured arrays
    (``RECORD_DTYPE``); ``imp`` int32 [n] (pair sitting North-South at table A); ``dda`` uint8 [n,20]; ``board_id`` int64 [n];
    ``cum_return`` float32 [n]: the evaluator's own per-board return (player 0's IMP), as ``board_match`` accumulated it.
    Everything named is read from ``cpu()``'s arrays, which are copied from the device once and refuse a record whose self-check
    bit is clear.  ``par``: the boards' par records when they are known already (``par.PAR_DTYPE`` [n], or their bytes);
    otherwise ``par()`` computes them from ``dda`` on first use."""

    def __init__(self, table_a, table_b=None, imp=None, dda=None, board_id=None, cum_return=None, par=None):
        self.table_a, self.table_b, self.imp, self.dda, self.board_id = table_a, table_b, imp, dda, board_id
        self.cum_return = cum_return
        self._par = par
        self._host = {}

    def __len__(self):
        return int(self.table_a.shape[0])

    def cpu(self, table: str = "a") -> np.ndarray:
        """the numpy structured array (``RECORD_DTYPE``) of table "a" or "b" """
        if table not in self._host:
            src = {"a": self.table_a, "b": self.table_b}[table]
            if src is None:
                raise ValueError(f"no table {table}")
            self._host[table] = _structured(src, f"table {table}")
        return self._host[table]

    def _np(self, name):
        v = getattr(self, name)
        if v is None:
            return None
        return v if isinstance(v, np.ndarray) else v.detach().cpu().numpy()

    def auction(self, i, table="a"):
        r = self.cpu(table)[i]
        return [CALL_NAMES[c] for c in r["calls"][:int(r["n_calls"])]]

    def contract(self, i, table="a") -> str:
        r = self.cpu(table)[i]
        if r["flags"] & PASSED_OUT:
            return "passed out"
        if r["flags"] & ILLEGAL:
            return "ended by an illegal call"
        if not r["flags"] & TERMINATED:
            return "unfinished"
        return f"{r['level']}{STRAINS[r['strain']]}{'X' * int(r['doubled'])} by {SEATS[r['declarer']]}"

    def hands(self, i, table="a") -> str:
        return pbn_deal(self.cpu(table)[i]["hands"])

    def _table_dict(self, i, table, par=False):
        r = self.cpu(table)[i]
        has = bool(r["flags"] & TERMINATED) and not r["flags"] & (PASSED_OUT | ILLEGAL)
        out = {"auction": self.auction(i, table), "contract": self.contract(i, table),
               "declarer": SEATS[r["declarer"]] if has else None, "tricks": int(r["tricks"]) if has else None,
               "score_ns": int(r["score_ns"])}
        if par:
            from .par import NO_RESULT
            v = int(self.imp_vs_par(table)[i])
            out["imp_vs_par"] = None if v == NO_RESULT else v
        return out

    def _dda(self):
        dda = self._np("dda")
        if dda is None:
            raise ValueError("the deals' double-dummy tables (dda=) are needed to write boards")
        return dda

    def par(self) -> np.ndarray:
        """the boards' par records (``par.PAR_DTYPE`` [n]; include/brl_par.h): one ``brl_par`` launch on first use, from
        ``dda`` and table A's dealer and vulnerability"""
        if "par" not in self._host:
            from . import par as P
            if self._par is None:
                self._dda()
                a = self.table_a
                if isinstance(a, np.ndarray):
                    a = self.cpu("a")
                    self._par = P.par_of(self.dda, a["dealer"], a["vul_ns"], a["vul_ew"])
                else:
                    at = lambda name: a[:, RECORD_DTYPE.fields[name][1]]   # noqa: E731  (the byte columns of the records)
                    self._par = P.par_of(self.dda, at("dealer"), at("vul_ns"), at("vul_ew"))
            self._host["par"] = P.par_array(self._par)
        return self._host["par"]

    def imp_vs_par(self, table="a") -> np.ndarray:
        """int32 [n]: the IMP of the table's North-South score against par; ``par.NO_RESULT`` where the table has no result.
        Records on the device go through ``brl_par_imp``, host arrays through the same arithmetic in numpy."""
        key = "imp_vs_par_" + table
        if key not in self._host:
            from . import par as P
            par = self.par()
            src = {"a": self.table_a, "b": self.table_b}[table]
            if isinstance(src, np.ndarray) or isinstance(self._par, np.ndarray):
                self._host[key] = P.imp_vs_par(self.cpu(table), par)
            else:
                self.cpu(table)   # (refuses a record whose self-check bit is clear)
                self._host[key] = P.par_imp(src.contiguous(), self._par, 1).cpu().numpy()
        return self._host[key]

    def boards(self, par=False):
        """one dict per board: the dataset's fields plus ``table_a`` / ``table_b`` and ``imp``.  ``par=True`` adds
        ``par`` = {score_ns, contracts, dealer_dependent} to each board and ``imp_vs_par`` to each table."""
        a = self.cpu("a")
        dda, ids, imp = self._dda(), self._np("board_id"), self._np("imp")
        if par:
            from .par import DEALER_DEPENDENT, par_contracts
            pr = self.par()
        out = []
        for i in range(len(a)):
            r = a[i]
            b = {"board_id": int(ids[i]) if ids is not None else i, "dealer": SEATS[r["dealer"]],
                 "deal": {seat: hand_names(r["hands"][s]) for s, seat in enumerate(SEATS)},
                 "vulnerability": VULS[int(r["vul_ns"]) + 2 * int(r["vul_ew"])],
                 "dda": {seat: {st: int(dda[i].reshape(4, 5)[s, d]) for d, st in enumerate(STRAINS)} for s, seat in enumerate(SEATS)},
                 "table_a": self._table_dict(i, "a", par)}
            if self.table_b is not None:
                b["table_b"] = self._table_dict(i, "b", par)
            if imp is not None:
                b["imp"] = int(imp[i])
            if par:
                b["par"] = {"score_ns": int(pr[i]["score_ns"]), "contracts": par_contracts(pr[i], dda[i]),
                            "dealer_dependent": bool(pr[i]["flags"] & DEALER_DEPENDENT)}
            out.append(b)
        return out

    def to_json(self, path, par=False):
        with open(path, "w") as f:
            json.dump({"logs": self.boards(par)}, f)

    def to_pbn(self, path, par=False):
        """one game per board and table (the second table in the closed room), standard tags.  ``par=True`` adds
        ``OptimumScore`` and ``ParContract`` (side and contract, the lowest one when several score par; ``Pass`` when par is a
        pass-out)."""
        pbn_call = {"P": "Pass"}
        lines = ["% PBN 2.1", ""]
        for b in self.boards(par):
            dd = "".join(f"{b['dda'][seat][st]:x}" for seat in "NSEW" for st in ("NT", "S", "H", "D", "C"))
            for room, key in (("Open", "table_a"), ("Closed", "table_b")):
                t = b.get(key)
                if t is None:
                    continue
                contract = t["contract"].split(" by ")[0] if t["declarer"] else ("Pass" if t["contract"] == "passed out" else "")
                lines += [f'[Board "{b["board_id"]}"]', f'[Room "{room}"]', f'[Dealer "{b["dealer"]}"]',
                          f'[Vulnerable "{ {"Both": "All"}.get(b["vulnerability"], b["vulnerability"]) }"]',
                          f'[Deal "{pbn_deal([sum(1 << card_bit(c) for c in b["deal"][s]) for s in SEATS])}"]',
                          f'[Declarer "{t["declarer"] or ""}"]', f'[Contract "{contract}"]',
                          f'[Result "{t["tricks"] if t["tricks"] is not None else ""}"]', f'[Score "NS {t["score_ns"]}"]',
                          f'[DoubleDummyTricks "{dd}"]']
                if par:
                    first = b["par"]["contracts"][0].split(" by ") if b["par"]["contracts"] else None
                    lines += [f'[OptimumScore "NS {b["par"]["score_ns"]}"]',
                              f'[ParContract "{first[1] + " " + first[0] if first else "Pass"}"]']
                lines.append(f'[Auction "{b["dealer"]}"]')
                calls = [pbn_call.get(c, c) for c in t["auction"]]
                lines += [" ".join(calls[k:k + 4]) for k in range(0, len(calls), 4)]
                lines.append("")
        with open(path, "w") as f:
            f.write("\n".join(lines))

    def save(self, path, par=False):
        if str(path).lower().endswith(".pbn"):
            self.to_pbn(path, par)
        else:
            self.to_json(path, par)


# ---- a match with its boards ------------------------------------------------------------------------------------------------------
class _KeepA:
    """Table A's final states of a run of boards, and the records of both tables at the end.  Table B's records are taken from the
    final states.  Table A's cannot be: the launch that ends table A re-deals the slot for table B, so its final state never
    reaches memory.  ``brl_board_keep_a`` — one launch behind every step (``after_step``) — keeps it: the state before the step,
    stepped with the call the loop made, by the same device function."""

    def __init__(self, packed, table_a):
        import torch

        from . import _capi
        self.packed, self.table_a = packed, table_a
        self.prev, self.final_a = packed.clone(), torch.zeros_like(packed)
        self.taken = torch.zeros(packed.shape[0], dtype=torch.uint8, device=packed.device)
        self.di = _capi.device_index(packed)

    def after_step(self, action):
        from . import _capi
        _capi.check(_capi.lib().brl_board_keep_a(self.di, _capi.ptr(self.packed), _capi.ptr(self.prev), _capi.ptr(action),
                                                 _capi.ptr(self.table_a.terminated), _capi.ptr(self.taken), _capi.ptr(self.final_a),
                                                 self.packed.shape[0], _capi.stream(self.di)))

    def records(self, who, dda, cum, n, board_id=None):
        """one ``BoardRecords`` per match of n boards (``cum`` [matches, n]); ``who``: the caller, named in the error"""
        if not bool(self.taken.all()):
            raise RuntimeError(f"{who}: a board's table A never ended")
        rec_a, rec_b = board_records(self.final_a), board_records(self.packed)
        imp = board_imp(rec_a, rec_b)
        return [BoardRecords(rec_a[s:s + n], rec_b[s:s + n], imp[s:s + n], dda, board_id, cum[s // n])
                for s in range(0, self.packed.shape[0], n)]


def make_board_match(eval_env, team1_activation, team1_model_type, team2_activation, team2_model_type, num_eval_envs=None):
    """``board_match(team1_params, team2_params, deals | rng_key) -> (log, BoardRecords)``: ``make_simple_duplicate_evaluate``'s
    match — the same loop (``evaluation._eval_loop``), the same ``log`` = (mean IMP, standard error, win rate) bit for bit for
    the same key — and the records of both tables of every board.  With a ``Deals`` the given boards are played
    (``num_eval_envs`` is their number; every board seats players 0, 1, 2, 3 at N, E, S, W at table A).

    Table A's final states are kept by ``_KeepA``, one launch behind every step.  Runs on one rank."""
    import torch

    from .dist import one_rank_only
    from .duplicate import Table_info
    from .evaluation import _eval_loop, _match_stats, _team_forwards
    from .models import make_forward_pass
    fp1 = make_forward_pass(team1_activation, team1_model_type)
    fp2 = make_forward_pass(team2_activation, team2_model_type)

    def board_match(team1_params, team2_params, deals_or_key):
        one_rank_only("board_match")
        dev = eval_env.device
        with torch.no_grad():
            if isinstance(deals_or_key, Deals):
                d = deals_or_key
                state = eval_env.init_from_deals(d.hand, d.dealer, d.vul_ns, d.vul_ew, [0, 1, 2, 3], d.tricks)
                board_id = d.board_id
            else:
                if num_eval_envs is None:
                    raise ValueError("board_match(rng_key) needs make_board_match(num_eval_envs=)")
                state = eval_env.init(deals_or_key, num_envs=num_eval_envs)
                board_id = None
            n = state.num_envs
            dda = state._dds_tricks
            table_a_info, table_b_info = Table_info.from_state(state), Table_info.from_state(state)
            cum_return = torch.zeros(n, dtype=torch.float32, device=dev)
            fwd1, fwd2 = _team_forwards(fp1, team1_params, fp2, team2_params)
            keep = _KeepA(state.packed, table_a_info)   # (_eval_loop advances state.packed in place)
            _eval_loop(eval_env, state, fwd1, fwd2, (table_a_info, table_b_info), None, 0, cum_return, None,
                       after_step=lambda packed, action: keep.after_step(action))
            log = _match_stats(cum_return, n)
            records, = keep.records("board_match", dda, cum_return[None], n, board_id)
        return log, records

    return board_match
