"""Call review: what each call of a duplicate match cost, by policy playouts (include/brl_review.h holds the definition).

At every decision of a recorded auction — (table, board, call index t), t < min(n_calls, depth) — every one of the 38 actions is
tried in place of the call made, both sides then continue with their own network's masked arg-max (``masked_pi.mode()``, the
evaluators' rule), and the result is scored in IMPs against the RECORDED result of the other table, from the side of the seat that
made the call.  This is hindsight on the actual deal under the policies' own continuations — it is not a double-dummy judgement of
the call, and it does not see the deal from the caller's information state.

* ``make_call_review(eval_env, ...)`` -> ``call_review(team1_params, team2_params, records, tables="ab") -> CallReview``:
  ``brl_review_expand`` builds the branch tables, ``evaluation._eval_loop`` plays them out (every inference route, the live-row
  compaction), ``brl_review_reduce`` reads them back.
* ``CallReview`` — numpy arrays on the host, with ``of``, ``team_stats``, ``stats_lines``, ``to_text``, ``to_json`` / ``from_json``.
"""
from __future__ import annotations

import json

import numpy as np

from .boards import CALL_NAMES, ILLEGAL, MAX_CALLS, OK, RECORD_DTYPE, SEATS

ACTIONS = 38            # BRL_REVIEW_ACTIONS
VOID = -128             # BRL_REVIEW_VOID

DECISION_DTYPE = np.dtype([("board", "<i4"), ("call_index", "<u2"), ("seat", "u1"), ("team", "u1"), ("played", "u1"), ("zero", "u1", 7)])
SUMMARY_DTYPE = np.dtype([("played", "u1"), ("n_legal", "u1"), ("played_imp", "i1"), ("best_imp", "i1"), ("best", "u1"), ("loss", "u1"),
                          ("zero", "u1", 2)])
assert DECISION_DTYPE.itemsize == 16 and SUMMARY_DTYPE.itemsize == 8

# slots of one playout batch.  Per slot the loop holds the table (128 B), two observations (2 x 480 B: the one read and the one
# written), the next forward's float32 input (1920 B), two 1024-wide float32 activations (8192 B), both teams' logits (2 x 160 B)
# and ~40 B of flags, calls and live indices: ~11.6 KB, so 2^18 slots take ~3 GB.
MAX_BRANCHES = 1 << 18

_ARRAYS = ("table", "board", "board_id", "call_index", "seat", "team", "played", "n_legal", "imp", "best", "played_imp", "best_imp", "loss")


def _mean_se(x):
    nan = float("nan")
    x = np.asarray(x, np.float64)
    return {"count": int(x.size), "mean": float(x.mean()) if x.size else nan,
            "se": float(x.std(ddof=1) / np.sqrt(x.size)) if x.size > 1 else nan}


class CallReview:
    """The review of a match, one entry per decision, in the order table A's decisions (board by board, call index ascending),
    then table B's:

      table 0 = A / 1 = B, board (row of the records), board_id, call_index, seat (0..3 = N,E,S,W), team (0 = players {0,1}),
      played (action id), n_legal; imp int8 [D,38]: the IMP the caller's side would have won with each action, ``VOID`` (-128)
      where the action was not legal; best, played_imp, best_imp, loss (include/brl_review.h: Summary);
      skipped = {"a": records without a review, "b": ...}; depth.

    Hindsight on the actual deal under the policies' own continuations, not a double-dummy judgement."""

    def __init__(self, depth, skipped, **arrays):
        self.depth, self.skipped = int(depth), {k: int(v) for k, v in skipped.items()}
        for name in _ARRAYS:
            setattr(self, name, np.asarray(arrays[name]))
        self.imp = self.imp.astype(np.int8).reshape(-1, ACTIONS)

    def __len__(self):
        return int(self.board.shape[0])

    def of(self, board: int, table: str = "a"):
        """the decisions of one auction, calls named as ``boards.py`` names them: a list of
        {call_index, seat, team, played, played_imp, best, best_imp, loss, n_legal, imp: {call: IMP of every legal action}}"""
        tb = {"a": 0, "b": 1}[table]
        out = []
        for d in np.nonzero((self.table == tb) & (self.board == board))[0]:
            out.append({"call_index": int(self.call_index[d]), "seat": SEATS[int(self.seat[d])], "team": int(self.team[d]) + 1,
                        "played": CALL_NAMES[int(self.played[d])], "played_imp": int(self.played_imp[d]),
                        "best": CALL_NAMES[int(self.best[d])], "best_imp": int(self.best_imp[d]), "loss": int(self.loss[d]),
                        "n_legal": int(self.n_legal[d]),
                        "imp": {CALL_NAMES[a]: int(v) for a, v in enumerate(self.imp[d]) if v != VOID}})
        return out

    def team_stats(self, largest: int = 5) -> dict:
        """{"team1": S, "team2": S}; S = {"decisions", "best_share": the share of decisions where the call made was (one of) the
        best, "mean_loss": IMP per decision, "loss_per_board": {"count", "mean", "se"} — the team's losses summed per board, both
        tables, over the boards where it had a decision —, "largest": the decisions with the largest loss as
        {board, board_id, table, call_index, played, best, loss}}"""
        out = {}
        for team in (0, 1):
            sel = np.nonzero(self.team == team)[0]
            loss = self.loss[sel].astype(np.int64)
            per_board = np.bincount(np.unique(self.board[sel], return_inverse=True)[1], weights=loss) if sel.size else np.zeros(0)
            order = sel[np.argsort(-loss, kind="stable")[:largest]]
            out[f"team{team + 1}"] = {
                "decisions": int(sel.size), "best_share": float((loss == 0).mean()) if sel.size else float("nan"),
                "mean_loss": float(loss.mean()) if sel.size else float("nan"), "loss_per_board": _mean_se(per_board),
                "largest": [{"board": int(self.board[d]), "board_id": int(self.board_id[d]), "table": "ab"[int(self.table[d])],
                             "call_index": int(self.call_index[d]), "played": CALL_NAMES[int(self.played[d])],
                             "best": CALL_NAMES[int(self.best[d])], "loss": int(self.loss[d])} for d in order if self.loss[d] > 0]}
        return out

    def stats_lines(self):
        """one line per team, as ``python -m brl_amd.eval ... review=1`` prints them"""
        lines = []
        for name, s in self.team_stats(largest=1).items():
            top = s["largest"]
            worst = (f"; largest: board {top[0]['board_id']} table {top[0]['table'].upper()} call {top[0]['call_index']} "
                     f"({top[0]['played']}, best {top[0]['best']}: {top[0]['loss']} IMP)") if top else ""
            b = s["loss_per_board"]
            lines.append(f"review {name}: {s['decisions']} decisions (depth {self.depth}), the call made was best in "
                         f"{100 * s['best_share']:.1f}%, mean loss {s['mean_loss']:.3f} IMP per decision, "
                         f"{b['mean']:.3f} ± {b['se']:.3f} IMP per board over {b['count']} boards{worst}")
        return lines

    def to_text(self, board: int) -> str:
        """both auctions of one board, a line per decision: seat, team, the call made and its IMP, the best call and the loss"""
        lines = []
        for table in "ab":
            rows = self.of(board, table)
            if not rows:
                continue
            lines.append(f"board {board} table {table.upper()}")
            for r in rows:
                mark = "" if r["loss"] == 0 else f"  best {r['best']} {r['best_imp']:+d} (loss {r['loss']})"
                lines.append(f"  {r['call_index']:3d} {r['seat']} team{r['team']} {r['played']:<3} {r['played_imp']:+3d} of {r['n_legal']} legal{mark}")
        return "\n".join(lines)

    def to_json(self, path):
        doc = {"depth": self.depth, "skipped": self.skipped, "teams": self.team_stats()}
        doc.update({name: getattr(self, name).tolist() for name in _ARRAYS})
        with open(path, "w") as f:
            json.dump(doc, f)

    @classmethod
    def from_json(cls, path):
        with open(path) as f:
            doc = json.load(f)
        kinds = {"imp": np.int8, "played_imp": np.int8, "best_imp": np.int8, "board": np.int32, "board_id": np.int64,
                 "call_index": np.uint16}
        return cls(doc["depth"], doc["skipped"], **{name: np.asarray(doc[name], kinds.get(name, np.uint8)) for name in _ARRAYS})

    def same_as(self, other) -> bool:
        return (self.depth, self.skipped) == (other.depth, other.skipped) and all(
            getattr(self, n).dtype == getattr(other, n).dtype and np.array_equal(getattr(self, n), getattr(other, n)) for n in _ARRAYS)


def review_from_parts(depth, skipped, parts, board_id=None) -> CallReview:
    """``parts``: per table reviewed (0 / 1, ``DECISION_DTYPE`` [D], int8 [D,38], ``SUMMARY_DTYPE`` [D]) — what the two kernels wrote"""
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)   # noqa: E731
    dec = [p[1] for p in parts]
    summ = [p[3] for p in parts]
    board = cat([d["board"] for d in dec], np.int32)
    return CallReview(
        depth, skipped, table=cat([np.full(len(p[1]), p[0]) for p in parts], np.uint8), board=board,
        board_id=board.astype(np.int64) if board_id is None else np.asarray(board_id, np.int64)[board],
        call_index=cat([d["call_index"] for d in dec], np.uint16), seat=cat([d["seat"] for d in dec], np.uint8),
        team=cat([d["team"] for d in dec], np.uint8), played=cat([d["played"] for d in dec], np.uint8),
        n_legal=cat([s["n_legal"] for s in summ], np.uint8),
        imp=np.concatenate([p[2].reshape(-1, ACTIONS) for p in parts]).astype(np.int8) if parts else np.zeros((0, ACTIONS), np.int8),
        best=cat([s["best"] for s in summ], np.uint8), played_imp=cat([s["played_imp"] for s in summ], np.int8),
        best_imp=cat([s["best_imp"] for s in summ], np.int8), loss=cat([s["loss"] for s in summ], np.uint8))


# ---- the device path ---------------------------------------------------------------------------------------------------------
def first_decisions(rec, depth: int):
    """(first int64 [n + 1] on the device, reviewable bool [n]): the exclusive prefix sum of min(n_calls, depth) over the
    reviewable records of uint8 [n,368] device records — plain torch on the records' bytes, no synchronisation"""
    import torch
    at = lambda name: rec[:, RECORD_DTYPE.fields[name][1]].to(torch.int64)   # noqa: E731
    n_calls = at("n_calls") | (rec[:, RECORD_DTYPE.fields["n_calls"][1] + 1].to(torch.int64) << 8)
    flags = at("flags")
    ok = ((flags & OK) != 0) & ((flags & ILLEGAL) == 0)
    cnt = torch.where(ok, n_calls.clamp(max=min(int(depth), MAX_CALLS)), torch.zeros_like(n_calls))
    first = torch.zeros(rec.shape[0] + 1, dtype=torch.int64, device=rec.device)
    first[1:] = cnt.cumsum(0)
    return first, ok


def expand(rec, dda, depth, first, d0, d1):
    """(decisions uint8 [d1 - d0, 16], tables int64 [(d1 - d0) * 38, 16]): one ``brl_review_expand`` launch"""
    import torch

    from . import _capi
    nd, di = d1 - d0, _capi.device_index(rec)
    decisions = torch.empty((nd, DECISION_DTYPE.itemsize), dtype=torch.uint8, device=rec.device)
    tables = torch.empty((nd * ACTIONS, 16), dtype=torch.int64, device=rec.device)
    _capi.check(_capi.lib().brl_review_expand(di, _capi.ptr(rec), _capi.ptr(dda), rec.shape[0], int(depth), _capi.ptr(first), d0, d1,
                                              _capi.ptr(decisions), _capi.ptr(tables), _capi.stream(di)))
    return decisions, tables


def reduce(tables, decisions, other):
    """(values int8 [nd,38], summary uint8 [nd,8]): one ``brl_review_reduce`` launch"""
    import torch

    from . import _capi
    nd, di = decisions.shape[0], _capi.device_index(tables)
    values = torch.empty((nd, ACTIONS), dtype=torch.int8, device=tables.device)
    summary = torch.empty((nd, SUMMARY_DTYPE.itemsize), dtype=torch.uint8, device=tables.device)
    _capi.check(_capi.lib().brl_review_reduce(di, _capi.ptr(tables), _capi.ptr(decisions), nd, _capi.ptr(other), other.shape[0],
                                              _capi.ptr(values), _capi.ptr(summary), _capi.stream(di)))
    return values, summary


def _device_records(x, dev):
    import torch
    if x is None:
        return None
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1, RECORD_DTYPE.itemsize))
    return x.to(dev).contiguous()


def make_call_review(eval_env, team1_activation, team1_model_type, team2_activation, team2_model_type, depth: int = 12,
                     max_branches: int = MAX_BRANCHES):
    """``call_review(team1_params, team2_params, records, tables="ab", record=None) -> CallReview``.

    ``records``: the ``BoardRecords`` of a duplicate match with both tables and ``dda`` (``boards.make_board_match``); the two
    parameter sets continue the auctions (team 1 = players {0,1}, team 2 = players {2,3}, as everywhere).  ``tables``: "a", "b"
    or "ab".  Decisions are processed in chunks of at most ``max_branches`` slots (38 per decision); the result does not depend on
    the chunking.  ``record``: a list that receives, per table reviewed, the ``brl_board_record`` s (``RECORD_DTYPE``, on the host)
    of all final branch tables in slot order — one more launch per chunk.  Runs on one rank.

    The value of an action is hindsight on the actual deal under the policies' own greedy continuations, scored against the
    recorded result of the other table; it is not a double-dummy judgement of the call."""
    import torch

    from .boards import board_records
    from .bridge_bidding import State
    from .dist import one_rank_only
    from .evaluation import _eval_loop, _team_forwards
    from .models import make_forward_pass
    fp1 = make_forward_pass(team1_activation, team1_model_type)
    fp2 = make_forward_pass(team2_activation, team2_model_type)
    if int(depth) < 1 or int(max_branches) < ACTIONS:
        raise ValueError("depth >= 1 and max_branches >= 38")
    per = int(max_branches) // ACTIONS

    def call_review(team1_params, team2_params, records, tables="ab", record=None):
        one_rank_only("call_review")
        if records.dda is None:
            raise ValueError("call_review: the records hold no double-dummy tables (dda=)")
        if records.table_b is None:
            raise ValueError("call_review: the records hold no table B (a duplicate match is needed)")
        if tables not in ("a", "b", "ab"):
            raise ValueError(f"tables={tables!r}: 'a', 'b' or 'ab'")
        dev = eval_env.device
        with torch.no_grad():
            recs = {"a": _device_records(records.table_a, dev), "b": _device_records(records.table_b, dev)}
            dda = records.dda if isinstance(records.dda, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(records.dda))
            dda = dda.to(device=dev, dtype=torch.uint8).reshape(-1, 20).contiguous()
            if not (recs["a"].shape[0] == recs["b"].shape[0] == dda.shape[0]):
                raise ValueError("call_review: table A, table B and dda hold different numbers of boards")
            fwd1, fwd2 = _team_forwards(fp1, team1_params, fp2, team2_params)
            skipped, parts = {}, []
            for table in tables:
                rec, other = recs[table], recs["ab"["ba".index(table)]]
                first, ok = first_decisions(rec, depth)
                total, bad = (int(v) for v in torch.stack([first[-1], (~ok).sum()]).tolist())   # the one read: sizes the buffers
                skipped[table] = bad
                dec, val, summ, finals = [], [], [], []
                for d0 in range(0, total, per):
                    d1 = min(total, d0 + per)
                    decisions, branch = expand(rec, dda, depth, first, d0, d1)
                    _eval_loop(eval_env, State(eval_env, branch), fwd1, fwd2, None, None, 0, None, None)
                    v, s = reduce(branch, decisions, other)
                    dec.append(decisions)
                    val.append(v)
                    summ.append(s)
                    if record is not None:
                        finals.append(board_records(branch))
                if total:
                    host = lambda xs, dt: torch.cat(xs).cpu().numpy().view(dt).reshape(-1)   # noqa: E731
                    parts.append((0 if table == "a" else 1, host(dec, DECISION_DTYPE), torch.cat(val).cpu().numpy(),
                                  host(summ, SUMMARY_DTYPE)))
                if record is not None:
                    record.append(torch.cat(finals).cpu().numpy().view(RECORD_DTYPE).reshape(-1) if finals
                                  else np.zeros(0, RECORD_DTYPE))
            board_id = records.board_id
            if board_id is not None and not isinstance(board_id, np.ndarray):
                board_id = board_id.detach().cpu().numpy()
        return review_from_parts(depth, skipped, parts, board_id)

    return call_review
