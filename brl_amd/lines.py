"""Auction lines: the K most probable auctions of every board under the networks' masked softmax, with their probability, and
the expected IMP of the policies as trained with a rigorous bound (include/brl_lines.h holds the definition).

Everything else that evaluates a pair plays the masked arg-max call only.  Here every board's auctions are searched with a beam of
width K at both tables of a duplicate match: per step the lines' tables are observed, every line is forwarded through its caller's
network (``evaluation._Forward``), and ``brl_lines_expand`` keeps the K most probable of the finished lines and the live lines'
children.  The finished lines get their results (``brl_lines_finish``) and ``brl_lines_imp`` turns two beams into
``S`` and the covered mass ``c``: the expected IMP of team 1 lies in ``[S - 24 (1 - c), S + 24 (1 - c)]``.

* ``make_auction_lines(eval_env, ...)`` -> ``auction_lines(team1_params, team2_params, rng_key_or_deals) -> AuctionLines``
* ``AuctionLines`` — numpy arrays on the host, with ``of``, ``summary``, ``summary_lines``, ``to_text``, ``to_json`` / ``from_json``.
"""
from __future__ import annotations

import json

import numpy as np

from .boards import CALL_NAMES, SEATS

MAX_K = 16              # BRL_LINES_MAX_K
MAX_CALLS = 64          # BRL_LINES_MAX_CALLS
FILL = 0xFF             # BRL_LINES_FILL
EMPTY, FINISHED, VOID, GREEDY = 1, 2, 4, 8   # BRL_LINE_* flags
NO_RESULT = 0xFF        # ``contract`` of a line without a result (0 = passed out, 3..37 = the final bid's action id)

REQUEST_DTYPE = np.dtype([("board", "<i4"), ("slot", "<i4"), ("player", "<i4"), ("team", "<i4")])
RESULT_DTYPE = np.dtype([("score_ns", "<i4"), ("has_result", "u1"), ("level", "u1"), ("strain", "u1"), ("doubled", "u1"),
                         ("declarer", "u1"), ("tricks", "u1"), ("zero", "u1", 2), ("score_team1", "<i4")])
BOARD_DTYPE = np.dtype([("imp", "<f8"), ("covered", "<f8"), ("covered_a", "<f8"), ("covered_b", "<f8"), ("open_a", "<f8"),
                        ("open_b", "<f8"), ("void_a", "<f8"), ("void_b", "<f8")])
assert REQUEST_DTYPE.itemsize == 16 and RESULT_DTYPE.itemsize == 16 and BOARD_DTYPE.itemsize == 64

_LINE_ARRAYS = ("calls", "length", "logp", "prob", "finished", "open", "void", "greedy", "contract", "declarer", "doubled", "tricks",
                "score_ns", "score_team1")
_BOARD_ARRAYS = ("covered_a", "covered_b", "open_a", "open_b", "void_a", "void_b", "covered", "imp", "imp_lo", "imp_hi")
_KINDS = {"calls": np.uint8, "length": np.int32, "logp": np.float64, "prob": np.float64, "finished": bool, "open": bool, "void": bool,
          "greedy": bool, "contract": np.uint8, "declarer": np.uint8, "doubled": np.uint8, "tricks": np.uint8, "score_ns": np.int32,
          "score_team1": np.int32}


def _auction(calls, length):
    return [CALL_NAMES[c] if c < len(CALL_NAMES) else "?" for c in calls[:length]]


class AuctionLines:
    """The lines of a search.  Per table, board and slot, arrays ``[2, n, K]`` (table 0 = A, 1 = B; slots in the beam's order,
    most probable first, void lines last):

      calls uint8 [2,n,K,max_calls] (``FILL`` behind the last call), length, logp float64 (-inf for an empty slot), prob =
      exp(logp), finished, open (still live when the search stopped), void, greedy (every call was the evaluators' masked arg-max),
      contract (``NO_RESULT``, 0 = passed out, else the action id of the final bid), declarer, doubled, tricks, score_ns,
      score_team1 (the score from player 0's side).

    Per board, float64 ``[n]``: covered_a / covered_b (mass of the finished lines), open_a / open_b, void_a / void_b, covered =
    covered_a * covered_b, imp (``S``), imp_lo / imp_hi = S -/+ 24 (1 - covered); ``board_id`` int64 [n]; ``k``, ``max_calls``."""

    def __init__(self, k, max_calls, board_id=None, **arrays):
        self.k, self.max_calls = int(k), int(max_calls)
        for name in _LINE_ARRAYS:
            setattr(self, name, np.asarray(arrays[name], _KINDS[name]))
        for name in _BOARD_ARRAYS:
            setattr(self, name, np.asarray(arrays[name], np.float64))
        n = self.imp.shape[0]
        self.board_id = np.arange(n, dtype=np.int64) if board_id is None else np.asarray(board_id, np.int64)

    def __len__(self):
        return int(self.imp.shape[0])

    def of(self, board: int, table: str = "a"):
        """the lines of one board at one table, calls named as ``boards.py`` names them: a list of {slot, auction, logp, prob,
        state ("finished" | "open" | "void"), greedy, contract, declarer, doubled, tricks, score_ns}"""
        tb = {"a": 0, "b": 1}[table]
        out = []
        for s in range(self.k):
            if not (self.finished[tb, board, s] or self.open[tb, board, s] or self.void[tb, board, s]):
                continue
            has = int(self.contract[tb, board, s]) != NO_RESULT
            bid = int(self.contract[tb, board, s])
            out.append({"slot": s, "auction": _auction(self.calls[tb, board, s], int(self.length[tb, board, s])),
                        "logp": float(self.logp[tb, board, s]), "prob": float(self.prob[tb, board, s]),
                        "state": "void" if self.void[tb, board, s] else ("finished" if self.finished[tb, board, s] else "open"),
                        "greedy": bool(self.greedy[tb, board, s]),
                        "contract": None if not has else ("passed out" if bid == 0 else CALL_NAMES[bid] + "X" * int(self.doubled[tb, board, s])),
                        "declarer": SEATS[int(self.declarer[tb, board, s])] if has and bid else None,
                        "doubled": int(self.doubled[tb, board, s]), "tricks": int(self.tricks[tb, board, s]) if has and bid else None,
                        "score_ns": int(self.score_ns[tb, board, s]) if has else None})
        return out

    def summary(self) -> dict:
        """{"boards", "k", "imp": mean S, "imp_bound": mean 24 (1 - covered), "imp_lo", "imp_hi": the means of the bounds,
        "covered": mean covered, "covered_table": mean mass of a table's finished lines, "open_table", "void_table",
        "greedy_mass": mean probability of the greedy line (0 where it fell out of the beam), "greedy_kept": the share of tables
        whose greedy line is in the beam, "top_not_greedy": the share of tables, among those with a finished line, whose most
        probable finished line is not the greedy one, "contract_entropy": mean over the tables with a finished line of the entropy
        (nats) of the distribution of (contract, doubled, declarer) over the finished lines, normalised to their mass}"""
        n = len(self)
        fin = self.finished & ~self.void
        pf = np.where(fin, self.prob, 0.0)
        greedy_mass = np.where(self.greedy & ~self.void, self.prob, 0.0).sum(-1)
        has_fin = fin.any(-1)
        top = np.where(fin, self.prob, -1.0).argmax(-1)                       # (first maximum: the beam's order)
        top_greedy = np.take_along_axis(self.greedy, top[..., None], -1)[..., 0]
        ent = []
        for tb in range(2):
            for b in range(n):
                if not has_fin[tb, b]:
                    continue
                mass = {}
                for s in np.nonzero(fin[tb, b])[0]:
                    key = (int(self.contract[tb, b, s]), int(self.doubled[tb, b, s]), int(self.declarer[tb, b, s]))
                    mass[key] = mass.get(key, 0.0) + float(pf[tb, b, s])
                p = np.array(list(mass.values()), np.float64)
                p = p[p > 0] / p.sum() if p.sum() > 0 else p[:0]
                ent.append(float(-(p * np.log(p)).sum()))
        mean = lambda x: float(np.mean(x)) if np.size(x) else float("nan")   # noqa: E731
        return {"boards": n, "k": self.k, "imp": mean(self.imp), "imp_bound": mean(24.0 * (1.0 - self.covered)),
                "imp_lo": mean(self.imp_lo), "imp_hi": mean(self.imp_hi), "covered": mean(self.covered),
                "covered_table": mean(np.stack([self.covered_a, self.covered_b])),
                "open_table": mean(np.stack([self.open_a, self.open_b])), "void_table": mean(np.stack([self.void_a, self.void_b])),
                "greedy_mass": mean(greedy_mass), "greedy_kept": mean((self.greedy & ~self.void).any(-1)),
                "top_not_greedy": mean(~top_greedy[has_fin]), "contract_entropy": mean(ent)}

    def summary_lines(self):
        """the lines ``python -m brl_amd.eval ... lines=K`` prints"""
        s = self.summary()
        return [f"lines: {s['boards']} boards, beam {s['k']}, at most {self.max_calls} calls: expected IMP {s['imp']:.4f} "
                f"± {s['imp_bound']:.4f} (bound: 24 x the mass not covered), covered mass {s['covered']:.4f} "
                f"({s['covered_table']:.4f} per table, open {s['open_table']:.4f}, void {s['void_table']:.4f})",
                f"lines: the greedy auction carries {s['greedy_mass']:.4f} of the policy's mass on average (in the beam at "
                f"{100 * s['greedy_kept']:.1f}% of the tables); the most probable finished auction is not the greedy one at "
                f"{100 * s['top_not_greedy']:.1f}% of the tables; contract entropy {s['contract_entropy']:.3f} nats"]

    def to_text(self, board=None) -> str:
        """``board=None``: the summary lines; else both tables' lines of one board, a line each: probability, state, the auction
        and the result"""
        if board is None:
            return "\n".join(self.summary_lines())
        out = [f"board {int(self.board_id[board])}: expected IMP {self.imp[board]:+.3f} in [{self.imp_lo[board]:+.3f}, "
               f"{self.imp_hi[board]:+.3f}], covered {self.covered[board]:.4f}"]
        for table in "ab":
            out.append(f" table {table.upper()}")
            for r in self.of(board, table):
                res = "" if r["contract"] is None else (
                    "  passed out" if r["contract"] == "passed out" else
                    f"  {r['contract']} by {r['declarer']}, {r['tricks']} tricks, NS {r['score_ns']:+d}")
                mark = "*" if r["greedy"] else " "
                out.append(f"  {r['prob']:.4f}{mark} {r['state']:<8} {' '.join(r['auction'])}{res}")
        return "\n".join(out)

    def to_json(self, path):
        doc = {"k": self.k, "max_calls": self.max_calls, "board_id": self.board_id.tolist(), "summary": self.summary()}
        for name in _LINE_ARRAYS + _BOARD_ARRAYS:
            x = getattr(self, name)
            doc[name] = [None if not np.isfinite(v) else float(v) for v in x.reshape(-1)] if x.dtype == np.float64 else x.reshape(-1).tolist()
        doc["shape"] = list(self.logp.shape)
        with open(path, "w") as f:
            json.dump(doc, f)

    @classmethod
    def from_json(cls, path):
        with open(path) as f:
            doc = json.load(f)
        tb, n, k = doc["shape"]
        arrays = {}
        for name in _LINE_ARRAYS:
            flat = doc[name]
            if _KINDS[name] is np.float64:
                flat = [-np.inf if v is None else v for v in flat]
            arrays[name] = np.asarray(flat, _KINDS[name]).reshape((tb, n, k, -1) if name == "calls" else (tb, n, k))
        for name in _BOARD_ARRAYS:
            arrays[name] = np.asarray([np.nan if v is None else v for v in doc[name]], np.float64)
        return cls(doc["k"], doc["max_calls"], doc["board_id"], **arrays)

    def same_as(self, other) -> bool:
        return (self.k, self.max_calls) == (other.k, other.max_calls) and np.array_equal(self.board_id, other.board_id) and all(
            getattr(self, n).dtype == getattr(other, n).dtype and np.array_equal(getattr(self, n), getattr(other, n), equal_nan=n in ("logp",))
            for n in _LINE_ARRAYS + _BOARD_ARRAYS)


def lines_from_parts(k, max_calls, parts, boards, board_id=None) -> AuctionLines:
    """``parts``: per table (A, B) a dict of host arrays {tables uint64 [n*K,16], calls uint8 [n*K,max_calls], score float64 [n*K],
    flags uint8 [n*K], results ``RESULT_DTYPE`` [n*K]} — what the kernels wrote; ``boards``: ``BOARD_DTYPE`` [n]"""
    n = boards.shape[0]
    per = {name: [] for name in _LINE_ARRAYS}
    for p in parts:
        flags, res = p["flags"].reshape(n, k), p["results"].reshape(n, k)
        empty, fin, void = (flags & EMPTY) != 0, (flags & FINISHED) != 0, (flags & VOID) != 0
        has = res["has_result"] != 0
        sc = np.asarray(p["tables"]).view(np.uint64).reshape(n, k, 16)[:, :, 11]
        per["calls"].append(p["calls"].reshape(n, k, max_calls))
        per["length"].append(np.where(empty, 0, (sc >> np.uint64(41)) & np.uint64(1023)).astype(np.int32))   # SCH_STEP: calls made
        logp = p["score"].reshape(n, k)
        per["logp"].append(logp)
        with np.errstate(over="ignore"):
            per["prob"].append(np.where(empty, 0.0, np.exp(logp)))
        per["finished"].append(fin & ~void & ~empty)
        per["open"].append(~fin & ~void & ~empty)
        per["void"].append(void & ~empty)
        per["greedy"].append(((flags & GREEDY) != 0) & ~empty)
        per["contract"].append(np.where(has, np.where(res["level"] > 0, 3 + 5 * (res["level"].astype(np.int32) - 1) + res["strain"], 0),
                                        NO_RESULT).astype(np.uint8))
        for name in ("declarer", "doubled", "tricks", "score_ns", "score_team1"):
            per[name].append(res[name])
    arrays = {name: np.stack(v) for name, v in per.items()}
    bound = 24.0 * (1.0 - boards["covered"])
    arrays.update({name: boards[name] for name in BOARD_DTYPE.names})
    arrays.update(imp_lo=boards["imp"] - bound, imp_hi=boards["imp"] + bound)
    return AuctionLines(k, max_calls, board_id, **arrays)


# ---- the device path ---------------------------------------------------------------------------------------------------------
class Beam:
    """one table's beam of n boards x K slots on the device: tables int64 [n*K,16], calls uint8 [n*K,max_calls], score float64
    [n*K], flags uint8 [n*K]; request uint8 [n*K,16] (``REQUEST_DTYPE``) and done uint8 [n] as the launch that made it left them"""

    def __init__(self, n, k, max_calls, device):
        import torch
        self.n, self.k, self.max_calls = n, k, max_calls
        self.tables = torch.empty((n * k, 16), dtype=torch.int64, device=device)
        self.calls = torch.empty((n * k, max_calls), dtype=torch.uint8, device=device)
        self.score = torch.empty(n * k, dtype=torch.float64, device=device)
        self.flags = torch.empty(n * k, dtype=torch.uint8, device=device)
        self.request = torch.empty((n * k, REQUEST_DTYPE.itemsize), dtype=torch.uint8, device=device)
        self.done = torch.empty(n, dtype=torch.uint8, device=device)

    def host(self):
        return {"tables": self.tables.cpu().numpy().view(np.uint64), "calls": self.calls.cpu().numpy(), "score": self.score.cpu().numpy(),
                "flags": self.flags.cpu().numpy(), "request": self.request.cpu().numpy().view(REQUEST_DTYPE).reshape(-1),
                "done": self.done.cpu().numpy()}


def _check_beam(k, max_calls):
    if not 1 <= int(k) <= MAX_K:
        raise ValueError(f"k={k}: a beam holds 1 .. {MAX_K} lines")
    if not 1 <= int(max_calls) <= MAX_CALLS:
        raise ValueError(f"max_calls={max_calls}: 1 .. {MAX_CALLS}")


def lines_init(packed, k, max_calls) -> Beam:
    """step 0's beam of the dealt tables ``packed`` int64 [n,16]: one ``brl_lines_init`` launch"""
    from . import _capi
    _check_beam(k, max_calls)
    n, di = packed.shape[0], _capi.device_index(packed)
    b = Beam(n, int(k), int(max_calls), packed.device)
    _capi.check(_capi.lib().brl_lines_init(di, _capi.ptr(packed), n, b.k, b.max_calls, _capi.ptr(b.tables), _capi.ptr(b.calls),
                                           _capi.ptr(b.score), _capi.ptr(b.flags), _capi.ptr(b.request), _capi.ptr(b.done), _capi.stream(di)))
    return b


def lines_expand(beam: Beam, logits1, logits2, out: Beam = None) -> Beam:
    """the next beam: one ``brl_lines_expand`` launch.  ``logits1`` / ``logits2``: float32 [n*K, >= 38] of team 1's / team 2's
    network (any row stride), row b * K + s for line (b, s); ``out``: a beam of the same shape to write into (not ``beam``)"""
    import torch

    from . import _capi
    for lg in (logits1, logits2):
        if lg.dtype != torch.float32 or lg.dim() != 2 or lg.shape[0] < beam.n * beam.k or lg.shape[1] < 38 or lg.stride(1) != 1:
            raise ValueError("lines_expand: logits are float32 [n * k, >= 38] with unit column stride")
    if out is None:
        out = Beam(beam.n, beam.k, beam.max_calls, beam.tables.device)
    if out is beam or (out.n, out.k, out.max_calls) != (beam.n, beam.k, beam.max_calls):
        raise ValueError("lines_expand: the next beam needs memory of its own, of the same shape")
    di = _capi.device_index(beam.tables)
    _capi.check(_capi.lib().brl_lines_expand(
        di, _capi.ptr(beam.tables), _capi.ptr(beam.calls), _capi.ptr(beam.score), _capi.ptr(beam.flags), beam.n, beam.k, beam.max_calls,
        logits1.data_ptr(), logits1.stride(0), logits2.data_ptr(), logits2.stride(0), _capi.ptr(out.tables), _capi.ptr(out.calls),
        _capi.ptr(out.score), _capi.ptr(out.flags), _capi.ptr(out.request), _capi.ptr(out.done), _capi.stream(di)))
    return out


def lines_finish(tables, flags):
    """uint8 [lines,16] (``RESULT_DTYPE``): one ``brl_lines_finish`` launch"""
    import torch

    from . import _capi
    lines, di = flags.shape[0], _capi.device_index(tables)
    res = torch.empty((lines, RESULT_DTYPE.itemsize), dtype=torch.uint8, device=tables.device)
    _capi.check(_capi.lib().brl_lines_finish(di, _capi.ptr(tables), _capi.ptr(flags), lines, _capi.ptr(res), _capi.stream(di)))
    return res


def lines_imp(score_a, flags_a, res_a, score_b, flags_b, res_b, n, k):
    """float64 [n,8] (``BOARD_DTYPE``): one ``brl_lines_imp`` launch"""
    import torch

    from . import _capi
    di = _capi.device_index(score_a)
    out = torch.empty((n, 8), dtype=torch.float64, device=score_a.device)
    _capi.check(_capi.lib().brl_lines_imp(di, _capi.ptr(score_a), _capi.ptr(flags_a), _capi.ptr(res_a), _capi.ptr(score_b), _capi.ptr(flags_b),
                                          _capi.ptr(res_b), n, int(k), _capi.ptr(out), _capi.stream(di)))
    return out


def swapped_seating(packed):
    """the dealt tables of table B: the same deals with the seats exchanged as ``duplicate_step`` exchanges them ([1, 0, 3, 2])"""
    out = packed.clone()
    sc = packed[:, 11]
    sh = (sc >> 4) & 0xFF
    sw = ((sh >> 2) & 0x03) | ((sh & 0x03) << 2) | ((sh >> 2) & 0x30) | ((sh & 0x30) << 2)
    out[:, 11] = (sc & ~(0xFF << 4)) | (sw << 4)
    return out


def search(env, packed, fwd1, fwd2, k, max_calls, record=None):
    """the beam search of one table's dealt tables ``packed``: (final ``Beam``, steps run, rows forwarded per step).  Every step
    observes the lines' tables, forwards every row through the networks (ONE forward when ``fwd2 is fwd1``) and expands.  The loop
    ends after ``max_calls`` steps or once no board has a live line, watched as ``evaluation._eval_loop`` watches its boards
    (``_DoneWatch``: no blocking read per step; it runs at most two steps past the end, and a step without a live line changes
    nothing).  ``record``: a list that receives {"beam": step 0's beam} and then per step {"logits1", "logits2" float32 [n*K,38],
    "obs" bool [n*K,480], "mask" bool [n*K,38], "request": the requests of the beam the step read, "beam": the beam after the step}
    as host arrays."""
    from .evaluation import _DoneWatch, _Forward
    n = packed.shape[0]
    beam = lines_init(packed, k, max_calls)
    spare = Beam(n, beam.k, beam.max_calls, packed.device)
    if record is not None:
        record.append({"beam": beam.host()})
    watch = _DoneWatch.take(env, n, False)
    steps = 0
    try:
        watch.post(0, beam.done)
        for step in range(1, beam.max_calls + 1):
            polled = watch.poll(step)
            if polled is not None and polled[0] >= n:
                break
            obs, mask = env._observe_raw(beam.tables, None)
            l1, l2 = _Forward.whole_pair(fwd1, fwd2, obs)
            nxt = lines_expand(beam, l1, l2, spare)
            if record is not None:
                record.append({"logits1": l1[:, :38].cpu().numpy(), "logits2": l2[:, :38].cpu().numpy(), "obs": obs.cpu().numpy(),
                               "mask": mask.cpu().numpy(),
                               "request": beam.request.cpu().numpy().view(REQUEST_DTYPE).reshape(-1), "beam": nxt.host()})
            watch.post(step, nxt.done)
            beam, spare = nxt, beam
            steps += 1
    finally:
        watch.release()
    return beam, steps, n * beam.k


def make_auction_lines(eval_env, team1_activation, team1_model_type, team2_activation, team2_model_type, num_eval_envs=None, k: int = 4,
                       max_calls: int = MAX_CALLS, record=None):
    """``auction_lines(team1_params, team2_params, deals | rng_key) -> AuctionLines``.

    The boards come as ``boards.make_board_match`` takes them: a ``Deals`` (``boards.read_deals``), or a key for ``eval_env.init``
    with ``num_eval_envs`` boards.  Table A is the table as dealt, table B the same deal with the seats exchanged, as the
    evaluators play them; team 1 = players {0,1}.  The two tables are searched one after the other.  ``record``: a list that
    receives, per table, the list ``search`` fills.  The result has ``steps`` = (table A's, table B's) and ``rows_per_step``.
    Runs on one rank."""
    import torch

    from .boards import Deals
    from .dist import one_rank_only
    from .evaluation import _team_forwards
    from .models import make_forward_pass
    _check_beam(k, max_calls)
    fp1 = make_forward_pass(team1_activation, team1_model_type)
    fp2 = make_forward_pass(team2_activation, team2_model_type)

    def auction_lines(team1_params, team2_params, deals_or_key):
        one_rank_only("auction_lines")
        with torch.no_grad():
            if isinstance(deals_or_key, Deals):
                d = deals_or_key
                state = eval_env.init_from_deals(d.hand, d.dealer, d.vul_ns, d.vul_ew, [0, 1, 2, 3], d.tricks)
                board_id = d.board_id
            else:
                if num_eval_envs is None:
                    raise ValueError("auction_lines(rng_key) needs make_auction_lines(num_eval_envs=)")
                state = eval_env.init(deals_or_key, num_envs=num_eval_envs)
                board_id = None
            n = state.num_envs
            fwd1, fwd2 = _team_forwards(fp1, team1_params, fp2, team2_params)
            parts, dev, steps = [], [], []
            for packed in (state.packed, swapped_seating(state.packed)):
                rec = None
                if record is not None:
                    rec = []
                    record.append(rec)
                beam, count, rows = search(eval_env, packed, fwd1, fwd2, k, max_calls, rec)
                res = lines_finish(beam.tables, beam.flags)
                dev.append((beam, res))
                steps.append(count)
            boards = lines_imp(dev[0][0].score, dev[0][0].flags, dev[0][1], dev[1][0].score, dev[1][0].flags, dev[1][1], n, k)
            for beam, res in dev:
                h = beam.host()
                h["results"] = res.cpu().numpy().view(RESULT_DTYPE).reshape(-1)
                parts.append(h)
            out = lines_from_parts(int(k), int(max_calls), parts, boards.cpu().numpy().view(BOARD_DTYPE).reshape(-1), board_id)
            out.steps, out.rows_per_step = tuple(steps), n * int(k)
        return out

    return auction_lines
