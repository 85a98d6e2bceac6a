"""Hand beliefs: the hidden hands an auction shows, by weighted deals (include/brl_belief.h holds the definition).

Given one seat's thirteen cards and an auction prefix, K deals of the 39 unseen cards are drawn uniformly (``brl_belief_deal``),
every deal is weighted by the probability the two networks give the hidden seats' calls of the prefix (each caller's observation
through its team's ``evaluation._Forward``, ``brl_belief_logp``, the table stepped by ``brl_step``), and the weighted deals are
summed per query (``brl_belief_reduce``): the soft belief (importance weights) beside the greedy one (the deals on which every
hidden call is the network's masked arg-max, the policy the evaluators play).  No sampled deal is scored and nothing is searched.

* ``BeliefQuery(seat, hand, dealer, vul, calls, seating=...)``; ``queries_from_records(records, table, board, call_index)``.
* ``make_hand_belief(eval_env, ...)`` -> ``hand_belief(team1_params, team2_params, queries) -> HandBelief``.
* ``HandBelief`` — numpy arrays on the host, with ``of``, ``to_text``, ``to_json`` / ``from_json``, ``same_as``.

Opt-in (``make_hand_belief(..., resample_every=R, moves=M)``, include/brl_belief_smc.h): a resample-move particle
filter for auctions that starve plain importance sampling.  After every R-th weighed call of a query its deals are resampled in
proportion to their weights (``brl_belief_resample``) and each copy is moved M times: one card exchanged between two hidden hands
(``brl_belief_propose``), the prefix so far replayed on the proposed deal through the same forwards, and the exchange taken by the
likelihood ratio (``brl_belief_accept``).  ``resample_every=0`` is the plain path, call for call.
"""
from __future__ import annotations

import json

import numpy as np

from .boards import CALL_NAMES, MAX_CALLS, RANKS, SEATS, SUITS, VULS, bit_card, hand_names

ACTIONS = 38                      # BRL_BELIEF_ACTIONS
STREAM = 0x42524C42               # BRL_BELIEF_STREAM
ALL_ACTIONS = (1 << ACTIONS) - 1
RESAMPLE_STREAM = 0x42524C53      # BRL_BELIEF_RESAMPLE_STREAM
MOVE_STREAM = 0x42524C4D          # BRL_BELIEF_MOVE_STREAM
MAX_MOVES = 256                   # BRL_BELIEF_SMC_MAX_MOVES
SMC_FIELDS = ("resamples", "proposals", "accepted", "distinct")

QUERY_DTYPE = np.dtype([("hand", "<u8"), ("seat", "u1"), ("dealer", "u1"), ("vul_ns", "u1"), ("vul_ew", "u1"), ("seating", "u1"),
                        ("zero", "u1", 3)])
ENTRY_DTYPE = np.dtype([("wsum", "<f8"), ("wsq", "<f8"), ("max_logw", "<f4"), ("n", "<u4"), ("consistent", "<u4"), ("reserved", "<u4"),
                        ("card", "<f8", (3, 52)), ("hcp", "<f8", (3, 38)), ("length", "<f8", (3, 4, 14)), ("balanced", "<f8", 3),
                        ("g_card", "<u4", (3, 52)), ("g_hcp", "<u4", (3, 38)), ("g_length", "<u4", (3, 4, 14)),
                        ("g_balanced", "<u4", 3), ("reserved2", "<u4")])
assert QUERY_DTYPE.itemsize == 16 and ENTRY_DTYPE.itemsize == 5328     # BRL_BELIEF_ENTRY_BYTES

MAX_ROWS = 1 << 18     # rows (samples) of one batch: the slots' memory is the call review's (review.MAX_BRANCHES)
HONOURS = [b for b in range(52) if b >> 2 >= 9]     # J, Q, K, A of every suit


# ---- queries -------------------------------------------------------------------------------------------------------------------
def _seat(x, what):
    if isinstance(x, str):
        if x not in tuple(SEATS):
            raise ValueError(f"{what}: {x!r} is not one of N, E, S, W")
        return SEATS.index(x)
    if not 0 <= int(x) <= 3:
        raise ValueError(f"{what}: {x!r} is not a seat 0..3")
    return int(x)


def hand_word(hand) -> int:
    """a hand word from a PBN-style string ``spades.hearts.diamonds.clubs`` (``"AQ5.KT93.8.QJ762"``) or from a word itself"""
    if isinstance(hand, str):
        suits = hand.strip().split(".")
        if len(suits) != 4:
            raise ValueError(f"hand {hand!r}: not 'spades.hearts.diamonds.clubs'")
        word = 0
        for suit, ranks in zip("SHDC", suits):
            for r in ranks:
                if r not in RANKS:
                    raise ValueError(f"hand {hand!r}: {r!r} is not a rank")
                bit = 1 << (RANKS.index(r) * 4 + SUITS.index(suit))
                if word & bit:
                    raise ValueError(f"hand {hand!r}: {suit}{r} twice")
                word |= bit
    else:
        word = int(hand)
    if word < 0 or word >> 52 or bin(word).count("1") != 13:
        raise ValueError(f"hand {hand!r}: not thirteen cards")
    return word


def hand_text(word: int) -> str:
    names = hand_names(word)
    return ".".join("".join(sorted((c[1] for c in names if c[0] == s), key=RANKS.index, reverse=True)) for s in "SHDC")


class Auction:
    """the auction rules on the host (csrc/bridge_device.hpp: legal_mask, auction_step), for a prefix's legal words"""

    def __init__(self, dealer: int):
        self.dealer, self.turn = dealer, 0
        self.lb1 = self.lbseat = self.x = self.xx = self.npass = 0
        self.over = False

    def seat(self) -> int:
        return (self.dealer + self.turn) & 3

    def legal_word(self) -> int:
        """bit a: action a is legal for the seat to call; 0 once the auction is over"""
        if self.over:
            return 0
        m = 1 | ((ALL_ACTIONS >> (3 + self.lb1)) << (3 + self.lb1))
        own = ((self.lbseat ^ self.seat()) & 1) == 0
        if self.lb1 and not own and not self.x and not self.xx:
            m |= 2
        if self.lb1 and own and self.x and not self.xx:
            m |= 4
        return m

    def step(self, a: int):
        if a >= 3:
            self.lb1, self.lbseat, self.x, self.xx = a - 2, self.seat(), 0, 0
        elif a == 1:
            self.x = 1
        elif a == 2:
            self.xx = 1
        self.npass = self.npass + 1 if a == 0 else 0
        self.over = self.npass == (3 if self.lb1 else 4)
        self.turn += 1


class BeliefQuery:
    """One question: what do the other three hands look like for ``seat`` holding ``hand`` after ``calls``?

    seat, dealer: 0..3 or "N","E","S","W"; hand: ``"spades.hearts.diamonds.clubs"`` or a hand word (bit = rank * 4 + suit);
    vul: "None", "NS", "EW", "Both" or (vul_ns, vul_ew); calls: names of ``boards.CALL_NAMES`` or action ids, starting at the
    dealer; seating: the player id at N, E, S, W (team = id >> 1; players {0,1} are team 1) or the records' seating byte."""

    def __init__(self, seat, hand, dealer, vul, calls, seating=(0, 1, 2, 3)):
        self.seat, self.dealer = _seat(seat, "seat"), _seat(dealer, "dealer")
        self.hand = hand_word(hand)
        if isinstance(vul, str):
            if vul not in VULS:
                raise ValueError(f"vul {vul!r}: not one of {VULS}")
            self.vul_ns, self.vul_ew = VULS.index(vul) & 1, VULS.index(vul) >> 1
        else:
            self.vul_ns, self.vul_ew = int(bool(vul[0])), int(bool(vul[1]))
        if isinstance(seating, (int, np.integer)):
            seating = [(int(seating) >> (2 * s)) & 3 for s in range(4)]
        if sorted(int(p) for p in seating) != [0, 1, 2, 3]:
            raise ValueError(f"seating {seating!r}: not a permutation of the players 0..3")
        self.seating = sum(int(p) << (2 * s) for s, p in enumerate(seating))
        self.calls = []
        for c in calls:
            if isinstance(c, str):
                if c not in CALL_NAMES:
                    raise ValueError(f"call {c!r}: not one of boards.CALL_NAMES")
                c = CALL_NAMES.index(c)
            self.calls.append(int(c))

    def plan(self, index=0):
        """[(caller seat, legal word, action)] per call; ``ValueError`` names the query and the first illegal call"""
        if len(self.calls) > MAX_CALLS:
            raise ValueError(f"query {index}: {len(self.calls)} calls, more than {MAX_CALLS}")
        auction, out = Auction(self.dealer), []
        for t, a in enumerate(self.calls):
            legal = auction.legal_word()
            if not 0 <= a < ACTIONS or not (legal >> a) & 1:
                name = CALL_NAMES[a] if 0 <= a < ACTIONS else str(a)
                raise ValueError(f"query {index}: call {t} ({name}) is not legal" + (" (the auction is over)" if auction.over else ""))
            out.append((auction.seat(), legal, a))
            auction.step(a)
        return out

    def team_at(self, seat: int) -> int:
        return ((self.seating >> (2 * seat)) & 3) >> 1

    def label(self) -> dict:
        return {"seat": SEATS[self.seat], "hand": hand_text(self.hand), "dealer": SEATS[self.dealer],
                "vul": VULS[self.vul_ns + 2 * self.vul_ew], "calls": [CALL_NAMES[c] for c in self.calls],
                "seating": [(self.seating >> (2 * s)) & 3 for s in range(4)]}

    @classmethod
    def from_label(cls, d):
        return cls(d["seat"], d["hand"], d["dealer"], d["vul"], d["calls"], d["seating"])

    def __eq__(self, other):
        return isinstance(other, BeliefQuery) and self.label() == other.label()

    def __repr__(self):
        return f"BeliefQuery({self.label()})"


def queries_from_records(records, table, board, call_index):
    """the queries of the seat to call at decision ``call_index`` of recorded board ``board`` (row of the records) at ``table``
    ("a" / "b"): its own hand, the calls made before it.  ``board`` and ``call_index`` may be sequences of equal length."""
    rec = records.cpu(table)
    boards_ = np.atleast_1d(np.asarray(board, np.int64))
    calls_ = np.atleast_1d(np.asarray(call_index, np.int64))
    if boards_.shape != calls_.shape:
        boards_, calls_ = np.broadcast_arrays(boards_, calls_)
    out = []
    for i, t in zip(boards_.tolist(), calls_.tolist()):
        r = rec[i]
        if not 0 <= t <= int(r["n_calls"]):
            raise ValueError(f"board {i} table {table}: call index {t} outside 0..{int(r['n_calls'])}")
        seat = (int(r["dealer"]) + t) & 3
        out.append(BeliefQuery(seat, int(r["hands"][seat]), int(r["dealer"]), (int(r["vul_ns"]), int(r["vul_ew"])),
                               [int(c) for c in r["calls"][:t]], int(r["seating"])))
    return out


def resample_stages(query, resample_every: int, index=0) -> list:
    """the call indices after which ``query`` resamples (include/brl_belief_smc.h, schedule): every ``resample_every``-th of the
    calls a hidden seat made; none with ``resample_every`` = 0, a prefix without a hidden call or no prefix at all"""
    R = int(resample_every)
    if R < 0:
        raise ValueError("resample_every >= 0")
    out, weighed = [], 0
    for t, (seat, _, _) in enumerate(query.plan(index)):
        weighed += seat != query.seat
        if R and seat != query.seat and weighed % R == 0:
            out.append(t)
    return out


def query_array(queries) -> np.ndarray:
    q = np.zeros(len(queries), QUERY_DTYPE)
    for i, x in enumerate(queries):
        q[i] = (x.hand, x.seat, x.dealer, x.vul_ns, x.vul_ew, x.seating, (0, 0, 0))
    return q


# ---- the result ------------------------------------------------------------------------------------------------------------------
def _quantile(hist, p):
    cdf = np.cumsum(hist)
    return int(np.argmax(cdf >= p * cdf[-1])) if cdf[-1] > 0 else -1


class HandBelief:
    """The beliefs of Q queries.  ``entries``: what ``brl_belief_reduce`` wrote (``ENTRY_DTYPE`` [Q]); ``queries``: their labels.

      seats [Q,3]: the hidden seats, (seat + 1, 2, 3) & 3;  n, consistent [Q];  ess [Q] = wsum^2 / wsq;  max_logw [Q];
      card_prob [Q,3,52], hcp_hist [Q,3,38], hcp_mean [Q,3], length_hist [Q,3,4,14], length_mean [Q,3,4], balanced [Q,3]:
      the weighted sums over wsum (NaN throughout where the query's weights are not finite);
      greedy_card_prob, greedy_hcp_hist, greedy_hcp_mean, greedy_length_hist, greedy_length_mean, greedy_balanced: the counts over
      the consistent samples divided by ``consistent`` (NaN where it is 0).
      With resampling (``smc``: a dict of the four arrays; all four ``None`` without it): resamples [Q] the resamplings a query
      went through, proposals, accepted [Q] its particles' moves, distinct [Q] the different deals among its final particles.
      ``ess`` then counts only the weight since the last resampling — ``distinct`` is the number that shows degeneracy — and the
      consistent samples are the greedy-consistent ones among the soft particles, not a rejection sample."""

    def __init__(self, entries, queries, samples=None, seed=0, smc=None):
        e = np.ascontiguousarray(entries).view(ENTRY_DTYPE).reshape(-1)
        self.entries, self.queries = e, [q if isinstance(q, dict) else q.label() for q in queries]
        assert len(self.queries) == len(e)
        self.seed = int(seed)
        for name in SMC_FIELDS:
            setattr(self, name, None if smc is None else np.asarray(smc[name], np.int64).reshape(len(e)).copy())
        own = np.array([SEATS.index(q["seat"]) for q in self.queries], np.int64).reshape(-1)
        self.seats = ((own[:, None] + np.arange(1, 4)[None, :]) & 3).astype(np.uint8)
        self.n, self.consistent = e["n"].astype(np.int64), e["consistent"].astype(np.int64)
        self.max_logw = e["max_logw"].copy()
        with np.errstate(invalid="ignore", divide="ignore"):
            self.ess = e["wsum"] ** 2 / e["wsq"]
            ws = e["wsum"]
            self.card_prob = e["card"] / ws[:, None, None]
            self.hcp_hist = e["hcp"] / ws[:, None, None]
            self.length_hist = e["length"] / ws[:, None, None, None]
            self.balanced = e["balanced"] / ws[:, None]
            c = np.where(self.consistent > 0, self.consistent, np.nan)
            self.greedy_card_prob = e["g_card"] / c[:, None, None]
            self.greedy_hcp_hist = e["g_hcp"] / c[:, None, None]
            self.greedy_length_hist = e["g_length"] / c[:, None, None, None]
            self.greedy_balanced = e["g_balanced"] / c[:, None]
        self.hcp_mean = (self.hcp_hist * np.arange(38)).sum(-1)
        self.length_mean = (self.length_hist * np.arange(14)).sum(-1)
        self.greedy_hcp_mean = (self.greedy_hcp_hist * np.arange(38)).sum(-1)
        self.greedy_length_mean = (self.greedy_length_hist * np.arange(14)).sum(-1)

    def __len__(self):
        return len(self.entries)

    def of(self, q: int) -> dict:
        """query q as plain Python: the query's label, n, ess, consistent, and per hidden seat name the soft and the greedy
        {hcp_mean, hcp_range (10 % and 90 % points), length_mean {suit: x}, balanced, cards {name: probability}}"""
        out = dict(self.queries[q], n=int(self.n[q]), ess=float(self.ess[q]), consistent=int(self.consistent[q]), hidden={})
        if self.resamples is not None:
            out.update({name: int(getattr(self, name)[q]) for name in SMC_FIELDS})
        own = hand_word(self.queries[q]["hand"])
        for h in range(3):
            views = {}
            for name, pre in (("soft", ""), ("greedy", "greedy_")):
                hist = getattr(self, pre + "hcp_hist")[q, h]
                ok = bool(np.isfinite(hist).all())
                views[name] = {
                    "hcp_mean": float(getattr(self, pre + "hcp_mean")[q, h]),
                    "hcp_range": (_quantile(hist, 0.1), _quantile(hist, 0.9)) if ok else (-1, -1),
                    "length_mean": {SUITS[s]: float(getattr(self, pre + "length_mean")[q, h, s]) for s in range(4)},
                    "balanced": float(getattr(self, pre + "balanced")[q, h]),
                    "cards": {bit_card(b): float(getattr(self, pre + "card_prob")[q, h, b]) for b in range(52) if not (own >> b) & 1}}
            out["hidden"][SEATS[int(self.seats[q, h])]] = views
        return out

    def to_text(self, q: int, honours: int = 3) -> str:
        """query q for reading: per hidden seat the HCP mean and 10-90 % range, the suit lengths, the share of balanced hands and
        the most and least likely honours, the soft belief with the greedy one beside it after ``|``; the second line holds the
        effective sample size and the consistent count, so that a starved belief shows — with resampling the effective size
        since the last resampling, the resamplings, the distinct deals, the moves taken, and the greedy column's name: the
        greedy-consistent among the soft particles"""
        d = self.of(q)
        lines = [f"belief {q}: {d['seat']} holds {d['hand']}; dealer {d['dealer']}, vul {d['vul']}; "
                 f"auction {' '.join(d['calls']) if d['calls'] else '(none)'}",
                 f"  {d['n']} samples, effective {d['ess']:.1f}, consistent with the greedy policy {d['consistent']}"]
        if self.resamples is not None:
            lines[1] = (f"  {d['n']} particles, {d['resamples']} resamplings, effective {d['ess']:.1f} since the last, distinct deals "
                        f"{d['distinct']}, moves taken {d['accepted']} of {d['proposals']}, greedy among soft particles {d['consistent']}")
        for seat, v in d["hidden"].items():
            s, g = v["soft"], v["greedy"]
            lines.append(f"  {seat}: HCP {s['hcp_mean']:.2f} ({s['hcp_range'][0]}-{s['hcp_range'][1]}) | {g['hcp_mean']:.2f} "
                         f"({g['hcp_range'][0]}-{g['hcp_range'][1]}); lengths "
                         + " ".join(f"{x}{s['length_mean'][x]:.2f}" for x in "SHDC") + " | "
                         + " ".join(f"{x}{g['length_mean'][x]:.2f}" for x in "SHDC")
                         + f"; balanced {100 * s['balanced']:.0f}% | {100 * g['balanced']:.0f}%")
            hon = [bit_card(b) for b in HONOURS if bit_card(b) in s["cards"]]
            order = sorted(hon, key=lambda c: -s["cards"][c] if np.isfinite(s["cards"][c]) else 0.0)
            show = lambda cs: " ".join(f"{c} {100 * s['cards'][c]:.0f}%|{100 * g['cards'][c]:.0f}%" for c in cs)   # noqa: E731
            lines.append(f"     most likely honours {show(order[:honours])}; least likely {show(order[::-1][:honours])}")
        return "\n".join(lines)

    def to_json(self, path):
        e = self.entries
        doc = {"seed": self.seed, "queries": self.queries,
               "entries": [{name: (e[name][i].tolist()) for name in ENTRY_DTYPE.names} for i in range(len(e))],
               "summary": [{"n": int(self.n[i]), "ess": float(self.ess[i]), "consistent": int(self.consistent[i]),
                            "hcp_mean": self.hcp_mean[i].tolist(), "greedy_hcp_mean": self.greedy_hcp_mean[i].tolist()}
                           for i in range(len(e))]}
        if self.resamples is not None:
            doc["smc"] = {name: getattr(self, name).tolist() for name in SMC_FIELDS}
        with open(path, "w") as f:
            json.dump(doc, f)

    @classmethod
    def from_json(cls, path):
        with open(path) as f:
            doc = json.load(f)
        e = np.zeros(len(doc["entries"]), ENTRY_DTYPE)
        for i, row in enumerate(doc["entries"]):
            for name in ENTRY_DTYPE.names:
                e[name][i] = np.asarray(row[name], ENTRY_DTYPE.fields[name][0].base)
        return cls(e, doc["queries"], seed=doc["seed"], smc=doc.get("smc"))

    def same_as(self, other) -> bool:
        """the same bytes (NaN blocks included) for the same queries"""
        return self.queries == other.queries and self.entries.tobytes() == other.entries.tobytes()


# ---- the device path -------------------------------------------------------------------------------------------------------------
def deal(queries_dev, K, seed, q0=0):
    """(tables int64 [Q * K, 16], hands int64 [Q * K, 4]): one ``brl_belief_deal`` launch; queries_dev uint8 [Q,16]"""
    import torch

    from . import _capi
    Q, di = queries_dev.shape[0], _capi.device_index(queries_dev)
    tables = torch.empty((Q * K, 16), dtype=torch.int64, device=queries_dev.device)
    hands = torch.empty((Q * K, 4), dtype=torch.int64, device=queries_dev.device)
    _capi.check(_capi.lib().brl_belief_deal(di, _capi.ptr(queries_dev), Q, int(K), int(seed) & 0xFFFFFFFFFFFFFFFF, int(q0),
                                            _capi.ptr(tables), _capi.ptr(hands), _capi.stream(di)))
    return tables, hands


def logp(logits, rows, query_of, legal, action, logw, greedy):
    """one ``brl_belief_logp`` launch: logw / greedy updated in place for the rows listed"""
    from . import _capi
    di = _capi.device_index(logits)
    assert logits.dtype.is_floating_point and logits.element_size() == 4 and logits.stride(1) == 1
    _capi.check(_capi.lib().brl_belief_logp(di, logits.data_ptr(), logits.stride(0), _capi.ptr(rows), rows.shape[0], _capi.ptr(query_of),
                                            query_of.shape[0], _capi.ptr(legal), _capi.ptr(action), legal.shape[0], _capi.ptr(logw),
                                            _capi.ptr(greedy), _capi.stream(di)))


def reduce(queries_dev, K, hands, logw, greedy):
    """entries uint8 [Q, 5328]: one ``brl_belief_reduce`` launch"""
    import torch

    from . import _capi
    Q, di = queries_dev.shape[0], _capi.device_index(queries_dev)
    entries = torch.empty((Q, ENTRY_DTYPE.itemsize), dtype=torch.uint8, device=queries_dev.device)
    _capi.check(_capi.lib().brl_belief_reduce(di, _capi.ptr(queries_dev), Q, int(K), _capi.ptr(hands), _capi.ptr(logw), _capi.ptr(greedy),
                                              _capi.ptr(entries), _capi.stream(di)))
    return entries


def resample(qlist, stream_of, K, seed, stage, tables, hands, logl, logw, greedy):
    """(tables, hands, logl, logw, greedy, ancestor int32 [Q * K]) of one ``brl_belief_resample`` launch, out of place: only the
    rows of the queries ``qlist`` (int32 [L]) are written, the others are uninitialised; stream_of int64 [Q]"""
    import torch

    from . import _capi
    Q, di = stream_of.shape[0], _capi.device_index(tables)
    out = [torch.empty_like(x) for x in (tables, hands, logl, logw, greedy)]
    ancestor = torch.empty(Q * int(K), dtype=torch.int32, device=tables.device)
    _capi.check(_capi.lib().brl_belief_resample(di, _capi.ptr(qlist), qlist.shape[0], _capi.ptr(stream_of), Q, int(K),
                                                int(seed) & 0xFFFFFFFFFFFFFFFF, int(stage), _capi.ptr(tables), _capi.ptr(hands),
                                                _capi.ptr(logl), _capi.ptr(logw), _capi.ptr(greedy), *[_capi.ptr(x) for x in out],
                                                _capi.ptr(ancestor), _capi.stream(di)))
    return (*out, ancestor)


def propose(queries_dev, qlist, stream_of, K, seed, stage, move, hands, tables_new, hands_new):
    """one ``brl_belief_propose`` launch: the proposals of the queries ``qlist`` into the leading L * K rows of tables_new / hands_new"""
    from . import _capi
    di = _capi.device_index(hands)
    _capi.check(_capi.lib().brl_belief_propose(di, _capi.ptr(queries_dev), _capi.ptr(qlist), qlist.shape[0], _capi.ptr(stream_of),
                                               stream_of.shape[0], int(K), int(seed) & 0xFFFFFFFFFFFFFFFF, int(stage), int(move),
                                               _capi.ptr(hands), _capi.ptr(tables_new), _capi.ptr(hands_new), _capi.stream(di)))


def accept(qlist, stream_of, K, seed, stage, move, tables_new, hands_new, logl_new, greedy_new, tables, hands, logl, greedy, counters):
    """one ``brl_belief_accept`` launch: tables / hands / logl / greedy updated in place, counters int64 [Q, 2] added to"""
    from . import _capi
    di = _capi.device_index(hands)
    _capi.check(_capi.lib().brl_belief_accept(di, _capi.ptr(qlist), qlist.shape[0], _capi.ptr(stream_of), stream_of.shape[0], int(K),
                                              int(seed) & 0xFFFFFFFFFFFFFFFF, int(stage), int(move), _capi.ptr(tables_new),
                                              _capi.ptr(hands_new), _capi.ptr(logl_new), _capi.ptr(greedy_new), _capi.ptr(tables),
                                              _capi.ptr(hands), _capi.ptr(logl), _capi.ptr(greedy), _capi.ptr(counters), _capi.stream(di)))


def make_hand_belief(eval_env, team1_activation, team1_model_type, team2_activation, team2_model_type, samples: int = 4096,
                     seed: int = 0, max_rows: int = MAX_ROWS, resample_every: int = 0, moves: int = 2):
    """``hand_belief(team1_params, team2_params, queries, query_offset=0, rows=None, counts=None) -> HandBelief``.

    ``queries``: ``BeliefQuery`` s; query i draws its ``samples`` deals from stream ``query_offset + i`` of ``seed``, so a list
    split over several calls (with the offsets of its parts) gives the same entries.  The two parameter sets make the calls
    (team 1 = players {0,1}, team 2 = players {2,3}, as everywhere).  Queries are processed in batches of at most ``max_rows``
    rows, a query's rows never in two batches; inside a batch the queries are ordered by the length of their prefix, so that the
    rows still in their auction are always the leading ones.  A query's rows are forwarded as a batch of their own (``samples``
    rows), so the result depends neither on the batches nor on the order nor on the other queries of the call.
    ``rows``: a list that receives per query {"hands" uint64 [K,4], "logw" float32 [K], "greedy" uint8 [K]} as the device left
    them; ``counts``: a dict whose "forwarded" grows by the rows that went through a network.  Runs on one rank.
    ``resample_every`` = R > 0 (include/brl_belief_smc.h): a query resamples after every R-th call a hidden seat made, and every
    resampling is followed by ``moves`` Metropolis moves per particle, each of which replays the prefix so far on the proposed
    deals — the listed queries' rows, again K at a time through the networks, so the batches, the order and the other queries
    still do not matter.  The schedule follows from the prefixes: the loop still reads nothing back.  ``rows`` then also holds
    "logl" float32 [K]; the ``HandBelief`` carries ``resamples``, ``proposals``, ``accepted`` and ``distinct``.  R = 0 (the
    default) is the plain path: the same launches, the same bytes."""
    import torch

    from . import _capi
    from ._capi import OBS_SIZE
    from .dist import one_rank_only
    from .evaluation import _Forward, _team_forwards
    from .models import make_forward_pass
    fp1 = make_forward_pass(team1_activation, team1_model_type)
    fp2 = make_forward_pass(team2_activation, team2_model_type)
    K = int(samples)
    if K < 1 or int(max_rows) < K:
        raise ValueError("samples >= 1 and max_rows >= samples")
    R, M = int(resample_every), int(moves)
    if R < 0 or not 0 <= M <= MAX_MOVES:
        raise ValueError(f"resample_every >= 0 and 0 <= moves <= {MAX_MOVES}")
    per = int(max_rows) // K

    def forward(fwd, obs):
        """logits of one query's K observation rows.  A query's rows always go through the network as one batch of exactly K rows:
        which kernels a forward runs on, and with them the last bits of a logit, depend on the batch's size, so a batch made of
        whatever queries happen to be processed together would make the entries depend on the grouping."""
        assert obs.shape[0] == K
        return _Forward.whole(fwd, obs, eval_env)

    def batch(fwds, qs, plans, q_index, rows, counts):
        """the entries of the queries ``qs`` (already ordered by falling prefix length), stream indices ``q_index``, and with
        resampling their {resamples, proposals, accepted, distinct} (None without)"""
        dev, L = eval_env.device, _capi.lib()
        Q = len(qs)
        n = Q * K
        T = [len(p) for p in plans]
        qdev = torch.from_numpy(query_array(qs).view(np.uint8).reshape(Q, 16)).to(dev)
        # a run of consecutive stream indices is one launch
        runs, a = [], 0
        while a < Q:
            b = a + 1
            while b < Q and q_index[b] == q_index[b - 1] + 1:
                b += 1
            runs.append(deal(qdev[a:b], K, seed, q_index[a]))
            a = b
        tables, hands = runs[0] if len(runs) == 1 else (torch.cat([r[0] for r in runs]), torch.cat([r[1] for r in runs]))
        logw = torch.zeros(n, dtype=torch.float32, device=dev)
        greedy = torch.ones(n, dtype=torch.uint8, device=dev)
        depth = max(T) if T else 0
        smc = R > 0
        if smc:
            stages = [resample_stages(q, R) for q in qs]
            logl = torch.zeros(n, dtype=torch.float32, device=dev)
            unused = torch.ones(n, dtype=torch.uint8, device=dev)          # (the flags of the second logp, the one that adds to logl)
            counters = torch.zeros((Q, 2), dtype=torch.int64, device=dev)
        if depth:
            legal_np, act_np = np.zeros((depth, Q), np.int64), np.zeros((depth, Q), np.int32)
            hidden = [[] for _ in range(depth)]            # per call index: (query, team) of the calls a hidden seat made
            live = np.zeros(depth, np.int64)
            for i, (q, plan) in enumerate(zip(qs, plans)):
                for t, (seat, legal, action) in enumerate(plan):
                    legal_np[t, i], act_np[t, i] = legal, action
                    live[t] += 1
                    if seat != q.seat:
                        hidden[t].append((i, q.team_at(seat)))
            legal_dev, act_dev = torch.from_numpy(legal_np).to(dev), torch.from_numpy(act_np).to(dev)
            query_of = torch.arange(Q, dtype=torch.int32, device=dev).repeat_interleave(K)
            query_of64 = query_of.to(torch.int64)
            row_index = torch.arange(n, dtype=torch.int64, device=dev)
            di = _capi.device_index(tables)

            def step(tb, m, action):
                _capi.check(L.brl_step(eval_env._h, _capi.ptr(tb), _capi.ptr(tb), m, _capi.ptr(action), 0, None, None, None, None, None,
                                       _capi.stream(di)))

            def weigh(tb, m, callers, rows_of, legal, action, sums):
                """one call of the weight on the leading m rows of ``tb``: ``callers`` [(position of the query's K rows, team)],
                every (logw, greedy) pair of ``sums`` receives the call's term"""
                obs = torch.empty((m, OBS_SIZE), dtype=torch.bool, device=dev)
                _capi.check(L.brl_observe(eval_env._h, _capi.ptr(tb), m, None, _capi.ptr(obs), None, _capi.stream()))
                for i, team in callers:
                    lg = forward(fwds[team], obs[i * K:(i + 1) * K])
                    for lw, g in sums:
                        logp(lg, row_index[i * K:(i + 1) * K], rows_of, legal, action, lw, g)
                if counts is not None:
                    counts["forwarded"] = counts.get("forwarded", 0) + len(callers) * K

            if smc and any(stages):
                # everything a stage needs, on the device before the loop: the queries that resample after call t (ascending: all
                # of them are still in their auction), and the query of every row of their compact proposal arrays
                at = {}
                for i, st in enumerate(stages):
                    for t in st:
                        at.setdefault(t, []).append(i)
                stage_dev = {t: (torch.tensor(ids, dtype=torch.int32, device=dev),
                                 torch.tensor(ids, dtype=torch.int32, device=dev).repeat_interleave(K)) for t, ids in at.items()}
                widest = max(len(ids) for ids in at.values()) * K
                stream_of = torch.tensor(q_index, dtype=torch.int64, device=dev)
                tables_new = torch.empty((widest, 16), dtype=torch.int64, device=dev)
                hands_new = torch.empty((widest, 4), dtype=torch.int64, device=dev)
                logl_new = torch.empty(widest, dtype=torch.float32, device=dev)
                greedy_new = torch.empty(widest, dtype=torch.uint8, device=dev)
                team_at = [dict(h) for h in hidden]          # per call index: {query: team} of the hidden callers
            else:
                at = {}

            def resample_move(t):
                ids = at[t]
                qlist, rows_of = stage_dev[t]
                m = len(ids) * K
                out = resample(qlist, stream_of, K, seed, t, tables, hands, logl, logw, greedy)
                a = 0
                while a < len(ids):                          # a run of neighbouring queries is one copy per array
                    b = a + 1
                    while b < len(ids) and ids[b] == ids[b - 1] + 1:
                        b += 1
                    lo, hi = ids[a] * K, (ids[b - 1] + 1) * K
                    for dst, src in zip((tables, hands, logl, logw, greedy), out):
                        dst[lo:hi].copy_(src[lo:hi])
                    a = b
                rows_of64 = rows_of.to(torch.int64)
                for move in range(M):
                    propose(qdev, qlist, stream_of, K, seed, t, move, hands, tables_new, hands_new)
                    logl_new[:m].zero_()
                    greedy_new[:m].fill_(1)
                    for u in range(t + 1):                   # the replay: calls 0..t on the proposed deals, as the live ones went
                        callers = [(p, team_at[u][i]) for p, i in enumerate(ids) if i in team_at[u]]
                        if callers:
                            weigh(tables_new, m, callers, rows_of, legal_dev[u], act_dev[u], [(logl_new, greedy_new)])
                        step(tables_new, m, act_dev[u].index_select(0, rows_of64))
                    accept(qlist, stream_of, K, seed, t, move, tables_new, hands_new, logl_new, greedy_new, tables, hands, logl, greedy,
                           counters)

            for t in range(depth):
                nt = int(live[t]) * K                      # the rows still in their auction: the leading ones
                if hidden[t]:
                    weigh(tables, nt, hidden[t], query_of, legal_dev[t], act_dev[t],
                          [(logw, greedy), (logl, unused)] if smc else [(logw, greedy)])
                step(tables, nt, act_dev[t].index_select(0, query_of64[:nt]))
                if t in at:
                    resample_move(t)
        entries = reduce(qdev, K, hands, logw, greedy)
        if rows is not None or smc:
            h = hands.cpu().numpy().view(np.uint64).reshape(Q, K, 4)
        if rows is not None:
            lw, g = logw.cpu().numpy().reshape(Q, K), greedy.cpu().numpy().reshape(Q, K)
            ll = logl.cpu().numpy().reshape(Q, K) if smc else None
            for i in range(Q):
                rows.append({"hands": h[i].copy(), "logw": lw[i].copy(), "greedy": g[i].copy()})
                if smc:
                    rows[-1]["logl"] = ll[i].copy()
        if not smc:
            return entries, None
        c = counters.cpu().numpy()
        return entries, {"resamples": np.array([len(st) for st in stages], np.int64), "proposals": c[:, 0], "accepted": c[:, 1],
                         "distinct": np.array([len(np.unique(h[i], axis=0)) for i in range(Q)], np.int64)}

    def hand_belief(team1_params, team2_params, queries, query_offset: int = 0, rows=None, counts=None):
        one_rank_only("hand_belief")
        queries = list(queries)
        plans = [q.plan(i) for i, q in enumerate(queries)]          # refuses an illegal prefix before anything is sampled
        if not queries:
            return HandBelief(np.zeros(0, ENTRY_DTYPE), [], seed=seed, smc={name: [] for name in SMC_FIELDS} if R > 0 else None)
        with torch.no_grad():
            fwds = _team_forwards(fp1, team1_params, fp2, team2_params)
            parts, order, taken = [], [], []
            for a in range(0, len(queries), per):
                ids = sorted(range(a, min(len(queries), a + per)), key=lambda i: -len(plans[i]))     # (stable)
                got = [] if rows is not None else None
                parts.append(batch(fwds, [queries[i] for i in ids], [plans[i] for i in ids],
                                   [int(query_offset) + i for i in ids], got, counts))
                order += ids
                if rows is not None:
                    taken += got
            host = torch.cat([p[0] for p in parts]).cpu().numpy().view(ENTRY_DTYPE).reshape(-1)
        entries = np.zeros(len(queries), ENTRY_DTYPE)
        entries[np.asarray(order)] = host
        smc = None
        if R > 0:
            smc = {name: np.zeros(len(queries), np.int64) for name in SMC_FIELDS}
            for name in SMC_FIELDS:
                smc[name][np.asarray(order)] = np.concatenate([p[1][name] for p in parts])
        if rows is not None:
            back = [None] * len(queries)
            for i, r in zip(order, taken):
                back[i] = r
            rows.extend(back)
        return HandBelief(entries, queries, seed=seed, smc=smc)

    return hand_belief
