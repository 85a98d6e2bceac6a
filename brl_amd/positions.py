"""Position queries: what a network calls with a given hand after a given auction (include/brl_positions.h holds the definition;
DESIGN §21) — the reference's ``wb5/model_client_script.py`` (``ModelBiddingSystem.bid``), batched.

A position is thirteen cards, the dealer, the vulnerability and the calls so far; no deal is needed and none is built on the host.
``brl_position_rows`` checks the positions on the device, replays their auctions and writes the observation rows and legal masks in
one launch; the rows go through the network once (``evaluation._Forward``, whose route decision is kept); ``brl_position_answers``
turns the logits into the call (the evaluators' masked arg-max), the top of the policy, its entropy and the value.

* ``Position(hand, dealer, vul, calls)`` — parsed and checked on the host; ``positions_array`` packs them.
* ``positions_from_records(records, table, depth=None)`` — every decision of a ``boards.BoardRecords`` as a position.
* ``make_bidder(activation, model_type, top_k=3)`` -> ``ask(params, positions) -> Answers``; ``Bidder(params, ...)`` with
  ``bid(hand, dealer, vul, auction) -> str`` and ``ask(positions)``.
* ``Answers`` — numpy arrays on the host, with ``of``, ``to_text``, ``to_json`` / ``from_json``, ``same_as``.
* ``quiz_score(answers, expected)`` — a bidding-contest score: several calls of a position may score points.
"""
from __future__ import annotations

import json

import numpy as np

from .belief import ALL_ACTIONS, Auction, _seat, hand_text, hand_word
from .boards import CALL_NAMES, ILLEGAL, OK, SEATS, VULS, BoardRecords

ACTIONS = 38                     # BRL_POS_ACTIONS
MAX_CALLS = 48                   # BRL_POS_MAX_CALLS
FILL = 255                       # BRL_POS_FILL
MAX_TOP = 8                      # BRL_POS_MAX_TOP
POS_OK, BAD_HEADER, BAD_HAND, ILLEGAL_CALL, FINISHED = 0, 1, 2, 3, 4     # BRL_POS_*: the status' low byte
NONFINITE = 1                    # BRL_POS_NONFINITE
STATUS_NAMES = ("ok", "bad header", "bad hand", "illegal call", "finished")
MAX_ROWS = 1 << 18               # positions of one forward

POSITION_DTYPE = np.dtype([("hand", "<u8"), ("dealer", "u1"), ("vul_ns", "u1"), ("vul_ew", "u1"), ("n_calls", "u1"), ("reserved", "<u4"),
                           ("calls", "u1", MAX_CALLS)])
ANSWER_DTYPE = np.dtype([("call", "u1"), ("n_legal", "u1"), ("flags", "u1"), ("k", "u1"), ("value", "<f4"), ("entropy", "<f8"),
                         ("top_action", "u1", MAX_TOP), ("top_prob", "<f8", MAX_TOP), ("reserved", "<u8")])
assert POSITION_DTYPE.itemsize == 64 and ANSWER_DTYPE.itemsize == 96     # brl_position, brl_position_answer

_ALIASES = {"PASS": 0, "P": 0, "X": 1, "DBL": 1, "XX": 2, "RDBL": 2}
_ALIASES.update({n.upper(): a for a, n in enumerate(CALL_NAMES)})
_ALIASES.update({f"{lv}N": 3 + 5 * (lv - 1) + 4 for lv in range(1, 8)})


# ---- positions -------------------------------------------------------------------------------------------------------------------
def call_id(c) -> int:
    """the action 0..37 of a call: an action id, a name of ``boards.CALL_NAMES``, or Pass / P, X / Dbl, XX / Rdbl, 1N / 1NT (any case)"""
    if isinstance(c, str):
        a = _ALIASES.get(c.strip().upper())
        if a is None:
            raise ValueError(f"call {c!r}: not a call (P, X, XX, 1C .. 7NT)")
        return a
    if not 0 <= int(c) < ACTIONS:
        raise ValueError(f"call {c!r}: not an action 0..{ACTIONS - 1}")
    return int(c)


def _vul(vul):
    if isinstance(vul, str):
        names = [v.lower() for v in VULS]
        if vul.lower() not in names:
            raise ValueError(f"vul {vul!r}: not one of {VULS}")
        return names.index(vul.lower()) & 1, names.index(vul.lower()) >> 1
    return int(bool(vul[0])), int(bool(vul[1]))


class Position:
    """One question: what does the seat to call do, holding ``hand``, after ``calls``?

    hand: ``"spades.hearts.diamonds.clubs"`` (``"AKQ.J32.T9.87654"``) or a hand word (bit = rank * 4 + suit); dealer: "N", "E", "S",
    "W" or 0..3; vul: "None", "NS", "EW", "Both" or (vul_ns, vul_ew); calls: a list of names or action ids, or one string
    ``"1C P 1H X"``, starting at the dealer.  ``ValueError`` names the index of the first call that is not legal, or that the
    auction is over (the rules are ``belief.Auction``'s)."""

    def __init__(self, hand, dealer, vul, calls=()):
        self.hand, self.dealer = hand_word(hand), _seat(dealer, "dealer")
        self.vul_ns, self.vul_ew = _vul(vul)
        tokens = calls.replace(",", " ").split() if isinstance(calls, str) else list(calls)
        self.calls = []
        for t, c in enumerate(tokens):
            try:
                self.calls.append(call_id(c))
            except ValueError as e:
                raise ValueError(f"call {t}: {e}") from None
        if len(self.calls) > MAX_CALLS:
            raise ValueError(f"{len(self.calls)} calls, more than {MAX_CALLS}")
        auction = Auction(self.dealer)
        for t, a in enumerate(self.calls):
            if auction.over:
                raise ValueError(f"call {t} ({CALL_NAMES[a]}) follows the end of the auction (call {t - 1} ended it)")
            if not (auction.legal_word() >> a) & 1:
                raise ValueError(f"call {t} ({CALL_NAMES[a]}) is not legal")
            auction.step(a)
        if auction.over:
            raise ValueError(f"call {len(self.calls) - 1} ends the auction: nobody is to call")
        self.legal = auction.legal_word() & ALL_ACTIONS

    @property
    def seat(self) -> int:
        """the caller's seat"""
        return (self.dealer + len(self.calls)) & 3

    def label(self) -> dict:
        return {"hand": hand_text(self.hand), "dealer": SEATS[self.dealer], "vul": VULS[self.vul_ns + 2 * self.vul_ew],
                "auction": " ".join(CALL_NAMES[c] for c in self.calls)}

    @classmethod
    def from_label(cls, d):
        return cls(d["hand"], d["dealer"], d.get("vul", "None"), d.get("auction", d.get("calls", ())))

    def __eq__(self, other):
        return isinstance(other, Position) and self.label() == other.label()

    def __repr__(self):
        return f"Position({self.label()})"


def positions_array(positions) -> np.ndarray:
    """the packed records (``POSITION_DTYPE`` [n]) of ``Position`` objects; an array of that dtype (or its bytes, uint8 [n,64])
    passes through unchecked — the device status is then the only check"""
    if isinstance(positions, np.ndarray):
        a = np.ascontiguousarray(positions)
        if a.dtype == POSITION_DTYPE:
            return a.reshape(-1)
        if a.dtype == np.uint8 and a.ndim == 2 and a.shape[1] == POSITION_DTYPE.itemsize:
            return a.view(POSITION_DTYPE).reshape(-1)
        raise ValueError("positions: POSITION_DTYPE [n] or uint8 [n,64]")
    if isinstance(positions, Position):
        positions = [positions]
    out = np.zeros(len(positions), POSITION_DTYPE)
    out["calls"] = FILL
    for i, p in enumerate(positions):
        out["hand"][i], out["dealer"][i], out["vul_ns"][i], out["vul_ew"][i], out["n_calls"][i] = p.hand, p.dealer, p.vul_ns, p.vul_ew, len(p.calls)
        out["calls"][i, :len(p.calls)] = p.calls
    return out


def positions_from_records(records, table="a", depth=None):
    """(positions ``POSITION_DTYPE`` [m], index int64 [m,2]) of every decision of ``records`` (a ``boards.BoardRecords`` or one
    table's ``RECORD_DTYPE`` array) at ``table``: the caller's own hand and the calls before it, for the call indices
    t < min(n_calls, depth, 49); index[j] = (record, call index).  Records without OK or ended by an illegal call are skipped, as
    ``compare.make_policy_diff`` skips them."""
    rec = records.cpu(table) if isinstance(records, BoardRecords) else records
    limit = MAX_CALLS + 1 if depth is None else min(int(depth), MAX_CALLS + 1)
    ok = ((rec["flags"] & OK) != 0) & ((rec["flags"] & ILLEGAL) == 0)
    cnt = np.where(ok, np.minimum(rec["n_calls"].astype(np.int64), limit), 0)
    which = np.repeat(np.arange(len(rec)), cnt)
    t = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    out = np.zeros(len(which), POSITION_DTYPE)
    seat = (rec["dealer"][which].astype(np.int64) + t) & 3
    out["hand"] = rec["hands"][which, seat]
    out["dealer"], out["vul_ns"], out["vul_ew"], out["n_calls"] = rec["dealer"][which], rec["vul_ns"][which], rec["vul_ew"][which], t
    calls = rec["calls"][which, :MAX_CALLS]
    out["calls"] = np.where(np.arange(MAX_CALLS)[None, :] < t[:, None], calls, FILL)
    return out, np.stack([which, t], axis=1).astype(np.int64)


# ---- the result ------------------------------------------------------------------------------------------------------------------
class Answers:
    """What the network answers to n positions.

      positions            ``POSITION_DTYPE`` [n]
      status               uint32 [n]: the device's check of the position (low byte ``POS_OK`` .. ``FINISHED``, bits 8..15 a call index)
      call                 uint8 [n]: the masked arg-max, what the evaluators play; 255 where the status is not OK
      value, entropy       float32 / float64 [n]: the critic's value; the policy's entropy over the legal actions, in nats
      top_action, top_prob uint8 / float64 [n,8]: the ``k[i]`` most probable legal actions, the rest 255 / 0.0
      probs                float64 [n,38]: the policy, 0.0 on illegal actions
      n_legal, k, flags    uint8 [n]; flags & ``NONFINITE``: the row has no distribution (NaN in entropy, top_prob, probs)"""

    FIELDS = ("status", "call", "n_legal", "flags", "k", "value", "entropy", "top_action", "top_prob", "probs")

    def __init__(self, positions, status, answers, probs, top_k):
        self.positions = positions_array(positions)
        a = np.ascontiguousarray(answers)
        a = (a if a.dtype == ANSWER_DTYPE else a.view(ANSWER_DTYPE)).reshape(-1)
        self.top_k = int(top_k)
        self.status = np.asarray(status, np.uint32).reshape(-1)
        for name in ("call", "n_legal", "flags", "k", "value", "entropy", "top_action", "top_prob"):
            setattr(self, name, a[name].copy())
        self.probs = np.asarray(probs, np.float64).reshape(-1, ACTIONS)
        if not len(self.positions) == len(self.status) == len(self.call) == len(self.probs):
            raise ValueError("the arrays of an Answers hold one row per position")

    def __len__(self):
        return len(self.call)

    def of(self, i: int) -> dict:
        """one answer as plain Python, calls named as ``boards.py`` names them"""
        p, st = self.positions[i], int(self.status[i])
        out = {"hand": hand_text(int(p["hand"])) if bin(int(p["hand"])).count("1") == 13 and not int(p["hand"]) >> 52 else hex(int(p["hand"])),
               "dealer": SEATS[int(p["dealer"]) & 3], "vul": VULS[(int(p["vul_ns"]) & 1) + 2 * (int(p["vul_ew"]) & 1)],
               "auction": " ".join(CALL_NAMES[c] if c < ACTIONS else "?" for c in p["calls"][:min(int(p["n_calls"]), MAX_CALLS)]),
               "status": STATUS_NAMES[st & 0xFF] if (st & 0xFF) < len(STATUS_NAMES) else str(st), "status_index": st >> 8 & 0xFF}
        if st & 0xFF != POS_OK:
            return dict(out, call=None)
        return dict(out, seat=SEATS[(int(p["dealer"]) + int(p["n_calls"])) & 3], call=CALL_NAMES[int(self.call[i])], value=float(self.value[i]),
                    entropy=float(self.entropy[i]), n_legal=int(self.n_legal[i]), nonfinite=bool(self.flags[i] & NONFINITE),
                    top=[(CALL_NAMES[int(a)], float(q)) for a, q in zip(self.top_action[i][:int(self.k[i])], self.top_prob[i][:int(self.k[i])])])

    def to_text(self, i: int) -> str:
        d = self.of(i)
        head = f"{d['hand']}  dealer {d['dealer']}  vul {d['vul']}  auction: {d['auction'] or '(none)'}"
        if d["call"] is None:
            return f"{head}\nno call: {d['status']}" + (f" (call {d['status_index']})" if d["status"] in ("illegal call", "finished") else "")
        top = "  ".join(f"{c} {100 * q:.1f}%" for c, q in d["top"]) or "(no distribution: non-finite logits)"
        return f"{head}\n{d['seat']} calls {d['call']}   top: {top}   value {d['value']:+.4f}   entropy {d['entropy']:.3f} nats"

    def to_json(self, path=None):
        """the arrays themselves as a JSON document (written to ``path`` when given); ``from_json`` reads them back exactly"""
        doc = {"format": "brl_amd.positions/1", "top_k": self.top_k,
               "positions": {n: self.positions[n].tolist() for n in POSITION_DTYPE.names},
               "answers": [self.of(i) for i in range(len(self))]}
        for name in self.FIELDS:
            a = getattr(self, name)
            doc[name] = a.view(f"u{a.itemsize}").tolist() if a.dtype.kind == "f" else a.tolist()     # floats by their bits: NaN survives
        if path is not None:
            with open(path, "w") as f:
                json.dump(doc, f)
        return doc

    @classmethod
    def from_json(cls, src):
        if not isinstance(src, dict):
            with open(src) as f:
                src = json.load(f)
        if src.get("format") != "brl_amd.positions/1":
            raise ValueError("not a document written by Answers.to_json")
        n = len(src["status"])
        pos, ans = np.zeros(n, POSITION_DTYPE), np.zeros(n, ANSWER_DTYPE)
        for name in POSITION_DTYPE.names:
            pos[name] = np.asarray(src["positions"][name], POSITION_DTYPE.fields[name][0].base).reshape(pos[name].shape)
        for name in ("call", "n_legal", "flags", "k", "value", "entropy", "top_action", "top_prob"):
            base = ANSWER_DTYPE.fields[name][0].base
            raw = np.asarray(src[name], f"u{base.itemsize}" if base.kind == "f" else base).reshape(ans[name].shape)
            ans[name] = raw.view(base) if base.kind == "f" else raw
        probs = np.asarray(src["probs"], np.uint64).reshape(n, ACTIONS).view(np.float64)
        return cls(pos, np.asarray(src["status"], np.uint32), ans, probs, src["top_k"])

    def same_as(self, other) -> bool:
        """the same values in every field (NaN equal to NaN)"""
        return (self.top_k == other.top_k and self.positions.tobytes() == other.positions.tobytes()
                and all(np.array_equal(getattr(self, n), getattr(other, n), equal_nan=getattr(self, n).dtype.kind == "f") for n in self.FIELDS))


def quiz_score(answers: Answers, expected) -> dict:
    """A bidding-contest score.  ``expected[i]`` maps call names (any alias) to the points the call earns at position i — several
    calls may score — or is None / empty for a position without a key.  Per scored position: ``points`` of the network's call,
    ``max`` = the most a call earns, ``top_mass`` = the policy's probability on the calls that earn the most, ``expected`` =
    sum_a p_a points_a; ``total`` sums them over the scored positions (``top_mass`` as a mean) with ``positions`` = their number."""
    if len(expected) != len(answers):
        raise ValueError(f"{len(expected)} keys for {len(answers)} positions")
    rows, tot = [], {"points": 0.0, "max": 0.0, "expected": 0.0, "top_mass": 0.0, "positions": 0}
    for i, key in enumerate(expected):
        if not key:
            rows.append(None)
            continue
        if int(answers.status[i]) & 0xFF != POS_OK:
            raise ValueError(f"position {i} has a key but no answer ({STATUS_NAMES[int(answers.status[i]) & 0xFF]})")
        pts = np.zeros(ACTIONS)
        for name, v in key.items():
            pts[call_id(name)] = float(v)
        best = float(pts.max())
        p = answers.probs[i]
        row = {"points": float(pts[int(answers.call[i])]), "max": best, "top_mass": float(p[pts == best].sum()) if best > 0 else 0.0,
               "expected": float((p * pts).sum())}
        rows.append(row)
        for k in ("points", "max", "expected", "top_mass"):
            tot[k] += row[k]
        tot["positions"] += 1
    if tot["positions"]:
        tot["top_mass"] /= tot["positions"]
    return {"per_position": rows, "total": tot}


# ---- the device path -------------------------------------------------------------------------------------------------------------
def position_rows(pos, status=None, tables=False):
    """one ``brl_position_rows`` launch on pos uint8 [n,64] (device): (obs bool [n,480], mask uint8 [n,38], legal int64 [n], status
    int32 [n], tables int64 [n,16] or None); ``status``: an int32 [n] tensor to write into"""
    import torch

    from . import _capi
    n, dev, di = pos.shape[0], pos.device, _capi.device_index(pos)
    obs = torch.empty((n, _capi.OBS_SIZE), dtype=torch.bool, device=dev)
    mask = torch.empty((n, ACTIONS), dtype=torch.uint8, device=dev)
    legal = torch.empty(n, dtype=torch.int64, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev) if status is None else status
    tb = torch.empty((n, 16), dtype=torch.int64, device=dev) if tables else None
    _capi.check(_capi.lib().brl_position_rows(di, _capi.ptr(pos), n, _capi.ptr(obs), _capi.ptr(mask), _capi.ptr(legal), _capi.ptr(status),
                                              _capi.ptr(tb), _capi.stream(di)))
    return obs, mask, legal, status, tb


def position_answers(logits, value, legal, status, top_k, answers, probs=None):
    """one ``brl_position_answers`` launch: logits float32 [n, >= 38] of any row stride, value float32 [n] of any stride or None,
    into answers uint8 [n,96] and probs float64 [n,38] (or None)"""
    from . import _capi
    n, di = legal.shape[0], _capi.device_index(legal)
    assert logits.dtype.is_floating_point and logits.element_size() == 4 and logits.stride(1) == 1 and logits.shape[0] >= n and logits.shape[1] >= ACTIONS
    assert value is None or (value.element_size() == 4 and value.dim() == 1 and value.shape[0] >= n)
    _capi.check(_capi.lib().brl_position_answers(di, logits.data_ptr(), logits.stride(0), None if value is None else value.data_ptr(),
                                                 0 if value is None else value.stride(0), _capi.ptr(legal), _capi.ptr(status), n, int(top_k),
                                                 _capi.ptr(answers), _capi.ptr(probs), _capi.stream(di)))


def _heads(fwd, obs):
    """(logits float32 [m, >= 38], value float32 [m] view) of one network for the rows ``obs``, through ``_Forward``'s own route for
    that many rows; the module itself where ``_Forward`` has no snapshot of it (its forward keeps the value it would drop)"""
    import torch

    from .evaluation import _Forward
    if not fwd.constant and fwd.snap is None:
        logits, value = fwd.fp.apply(fwd.params, obs.to(torch.float32))
        return logits.float().contiguous(), value.reshape(-1).float().contiguous()
    out = _Forward.whole(fwd, obs)
    return out, (out[:, ACTIONS] if out.shape[1] > ACTIONS else None)


def _ask(fwd, positions, top_k, device, max_rows):
    import torch
    arr = positions_array(positions)
    n = len(arr)
    if n == 0:
        return Answers(arr, np.zeros(0, np.uint32), np.zeros(0, ANSWER_DTYPE), np.zeros((0, ACTIONS)), top_k)
    with torch.no_grad():
        pos = torch.from_numpy(arr.view(np.uint8).reshape(n, POSITION_DTYPE.itemsize)).to(device)
        a_bytes, p_bytes = n * ANSWER_DTYPE.itemsize, n * ACTIONS * 8
        out = torch.empty(a_bytes + p_bytes + 4 * n, dtype=torch.uint8, device=device)      # answers | probs | status: one copy back
        answers = out[:a_bytes].view(n, ANSWER_DTYPE.itemsize)
        probs = out[a_bytes:a_bytes + p_bytes].view(torch.float64).view(n, ACTIONS)
        status = out[a_bytes + p_bytes:].view(torch.int32)
        for a in range(0, n, max_rows):
            b = min(n, a + max_rows)
            obs, _, legal, st, _ = position_rows(pos[a:b], status[a:b])
            logits, value = _heads(fwd, obs)
            position_answers(logits, value, legal, st, top_k, answers[a:b], probs[a:b])
        host = out.cpu().numpy()
    return Answers(arr, host[a_bytes + p_bytes:].view(np.uint32), host[:a_bytes].view(ANSWER_DTYPE),
                   host[a_bytes:a_bytes + p_bytes].view(np.float64).reshape(n, ACTIONS), top_k)


def _config(top_k, route_config):
    if not 1 <= int(top_k) <= MAX_TOP:
        raise ValueError(f"top_k is 1 .. {MAX_TOP}")
    max_rows = int(route_config.pop("max_rows", MAX_ROWS))
    if route_config:
        raise TypeError(f"unknown option(s) {sorted(route_config)}: max_rows (the positions of one forward) is the one there is")
    if max_rows < 1:
        raise ValueError("max_rows >= 1")
    return int(top_k), max_rows


def make_bidder(activation, model_type, top_k: int = 3, device=None, **route_config):
    """``ask(params, positions) -> Answers``.

    ``positions``: ``Position`` objects (checked on the host when they were made), or a packed array (``positions_array``), whose
    only check is the device's: a position that fails it has a status other than ``POS_OK`` and no answer.  One
    ``brl_position_rows`` launch, one forward through ``evaluation._Forward`` — which keeps its route decision: the batch size
    selects the forward's kernels, so the last bits of a logit depend on how many positions are asked at once —, one
    ``brl_position_answers`` launch and one copy to the host.  ``max_rows`` (the one ``route_config`` option): the positions of one
    forward; a longer list is asked in chunks.  ``device``: where to run (default: where the parameters are)."""
    top_k, max_rows = _config(top_k, dict(route_config))
    from .models import make_forward_pass
    fp = make_forward_pass(activation, model_type)

    def ask(params, positions):
        from .evaluation import _Forward
        dev = device if device is not None else next(params.parameters()).device
        return _ask(_Forward(fp, params), positions, top_k, dev, max_rows)

    return ask


class Bidder:
    """A network that answers bidding questions — the reference's ``ModelBiddingSystem``.  ``params``: an ``ActorCritic``
    (``checkpoint.load_params``).  The parameters are read when the bidder is made."""

    def __init__(self, params, activation="relu", model_type="DeepMind", top_k: int = 3, device=None, **route_config):
        self.top_k, self.max_rows = _config(top_k, dict(route_config))
        from .evaluation import _Forward
        from .models import make_forward_pass
        self.device = device if device is not None else next(params.parameters()).device
        self.fwd = _Forward(make_forward_pass(activation, model_type), params)

    def ask(self, positions) -> Answers:
        return _ask(self.fwd, positions, self.top_k, self.device, self.max_rows)

    def bid(self, hand, dealer, vul, auction=()) -> str:
        """the call with ``hand`` after ``auction`` (names or action ids from the dealer on), as ``boards.CALL_NAMES`` names it"""
        ans = self.ask([Position(hand, dealer, vul, auction)])
        if int(ans.status[0]) & 0xFF != POS_OK:
            raise ValueError(f"no call: {STATUS_NAMES[int(ans.status[0]) & 0xFF]}")
        return CALL_NAMES[int(ans.call[0])]
