"""System diff: where two networks call differently, by auction prefix (include/brl_compare.h holds the definition).

Every decision of a recorded match — (table, board, call index t), t < min(n_calls, depth) — is shown to two networks X and Y:
the caller's observation at the table rebuilt from the record (``brl_compare_tables``, ``brl_observe`` / ``brl_step``), each
network's logits through ``evaluation._Forward``, and per decision what each would call, the log-probability each gives the call
that was played and the divergences of the two policies (``brl_compare_rows``).  The decisions are sorted by the prefix that led
to them and summed per prefix (``brl_compare_reduce``).  Both networks see the same hand and the same auction; nothing is sampled
and no double-dummy data is needed.

* ``make_policy_diff(eval_env, ...)`` -> ``policy_diff(x_params, y_params, records, tables="ab", rows=None) -> PolicyDiff``.
* ``PolicyDiff`` — numpy arrays on the host, with ``of``, ``entry``, ``worst``, ``stats_lines``, ``to_text``, ``to_json`` /
  ``from_json``; works without a GPU once built.
* ``key_of("1NT P")`` / ``prefix_of(key)`` — the key of the prefix before a decision, and back.
"""
from __future__ import annotations

import json

import numpy as np

from . import book
from .boards import CALL_NAMES, ILLEGAL, OK, RECORD_DTYPE, BoardRecords

ACTIONS = 38                     # BRL_COMPARE_ACTIONS
MAX_DEPTH = book.MAX_DEPTH       # BRL_BOOK_MAX_DEPTH
BLOCK = 64                       # BRL_COMPARE_BLOCK
VALID, AGREE, X_PLAYED, Y_PLAYED, NONFINITE = 1, 2, 4, 8, 16     # BRL_COMPARE_*
MAX_ROWS = 1 << 18               # records of one chunk: the slots' memory is the call review's (review.MAX_BRANCHES)

DECISION_DTYPE = np.dtype([("key", "<u8"), ("legal", "<u8"), ("feats", "<u4"), ("played", "u1"), ("call_x", "u1"), ("call_y", "u1"),
                           ("flags", "u1"), ("logp_x", "<f4"), ("logp_y", "<f4"), ("kl_xy", "<f8"), ("kl_yx", "<f8"), ("js", "<f8"),
                           ("reserved", "<u8")])
ENTRY_DTYPE = np.dtype([("key", "<u8"), ("n", "<u4"), ("agree", "<u4"), ("x_played", "<u4"), ("y_played", "<u4"), ("nonfinite", "<u4"),
                        ("reserved", "<u4"), ("calls_x", "<u4", ACTIONS), ("calls_y", "<u4", ACTIONS), ("played", "<u4", ACTIONS),
                        ("hcp_sum", "<u8"), ("hcp_sum_disagree", "<u8"), ("kl_xy_sum", "<f8"), ("kl_yx_sum", "<f8"), ("js_sum", "<f8"),
                        ("logp_x_sum", "<f8"), ("logp_y_sum", "<f8"), ("js_max", "<f8"), ("reserved2", "<u8")])
assert DECISION_DTYPE.itemsize == 64 and ENTRY_DTYPE.itemsize == 560     # BRL_COMPARE_DECISION_BYTES, BRL_COMPARE_ENTRY_BYTES


# ---- keys ----------------------------------------------------------------------------------------------------------------------
def key_of(prefix) -> int:
    """the key of a decision whose auction so far is ``prefix`` (``"1NT P"``, call names or action ids; at most 9 calls): the
    book's key fields of the prefix and the call index + 1 in the low four bits — the first call of an auction has key 1"""
    calls = prefix.split() if isinstance(prefix, str) else list(prefix)
    if len(calls) >= MAX_DEPTH:
        raise ValueError(f"a decision has at most {MAX_DEPTH - 1} calls before it, not {len(calls)}")
    return book.key_of(calls) | (len(calls) + 1)


def prefix_of(key: int):
    """(action ids of the prefix before the decision, call index t) of a non-zero key"""
    key = int(key)
    t = (key & 15) - 1
    calls = book.calls_of(key & ~15)
    if not 0 <= t < MAX_DEPTH or len(calls) != t:
        raise ValueError(f"not a key: {key:#x}")
    return calls, t


def name_of(key: int) -> str:
    return " ".join(CALL_NAMES[c] for c in prefix_of(key)[0]) or "(opening)"


# ---- the result ----------------------------------------------------------------------------------------------------------------
class PolicyDiff:
    """The diff of two networks X and Y on a match's records.

      decisions  ``DECISION_DTYPE`` [T, n, depth]: table (in the order of ``tables``), board (row of the records), call index; key 0
                 where there is no decision (t past the auction, or a skipped record)
      entries    ``ENTRY_DTYPE`` [K]: one per prefix, ascending by key (a prefix before its extensions)
      confusion  int64 [38, 38]: cell (call_x, call_y) counts the finite decisions
      skipped    {"a": records without OK or ended by an illegal call, "b": ...}; depth; tables ("a", "b" or "ab")"""

    def __init__(self, decisions, entries, confusion, skipped, depth, tables="ab"):
        self.depth, self.tables = int(depth), str(tables)
        self.skipped = {k: int(v) for k, v in skipped.items()}
        d = np.ascontiguousarray(decisions)
        d = d if d.dtype == DECISION_DTYPE else d.view(DECISION_DTYPE)
        self.decisions = d.reshape(len(self.tables), -1, self.depth)
        e = np.ascontiguousarray(entries)
        self.entries = (e if e.dtype == ENTRY_DTYPE else e.view(ENTRY_DTYPE)).reshape(-1)
        self.confusion = np.asarray(confusion).astype(np.int64).reshape(ACTIONS, ACTIONS)
        if len(self.entries) > 1 and not (self.entries["key"][1:] > self.entries["key"][:-1]).all():
            raise ValueError("the keys of a diff ascend strictly")

    def __len__(self):
        return int((self.decisions["key"] != 0).sum())

    # -- lookups
    def of(self, board: int, table: str = "a", t: int = 0):
        """one decision as plain Python, calls named as ``boards.py`` names them; None where there is none"""
        if table not in self.tables:
            raise ValueError(f"table {table!r} is not among the tables compared ({self.tables!r})")
        if not 0 <= int(t) < self.depth:
            raise ValueError(f"call index {t} outside 0..{self.depth - 1}")
        d = self.decisions[self.tables.index(table), int(board), int(t)]
        if d["key"] == 0:
            return None
        fl = int(d["flags"])
        return {"board": int(board), "table": table, "call_index": int(t), "prefix": name_of(int(d["key"])),
                "team": ((int(d["feats"]) >> 23) & 1) + 1, "hcp": int(d["feats"]) & 63, "played": CALL_NAMES[int(d["played"])],
                "call_x": CALL_NAMES[int(d["call_x"])], "call_y": CALL_NAMES[int(d["call_y"])], "agree": bool(fl & AGREE),
                "nonfinite": bool(fl & NONFINITE), "legal": [CALL_NAMES[a] for a in range(ACTIONS) if (int(d["legal"]) >> a) & 1],
                "logp_x": float(d["logp_x"]), "logp_y": float(d["logp_y"]), "kl_xy": float(d["kl_xy"]), "kl_yx": float(d["kl_yx"]),
                "js": float(d["js"])}

    def _summary(self, i):
        e = self.entries[i]
        n, bad = int(e["n"]), int(e["nonfinite"])
        f = n - bad
        nan = float("nan")
        mean = lambda x: float(x) / f if f else nan     # noqa: E731
        top = lambda h: [(CALL_NAMES[a], int(h[a])) for a in np.argsort(-h.astype(np.int64), kind="stable")[:3] if h[a]]   # noqa: E731
        dis = f - int(e["agree"])
        return {"prefix": name_of(int(e["key"])), "key": int(e["key"]), "call_index": (int(e["key"]) & 15) - 1, "n": n, "nonfinite": bad,
                "agree": int(e["agree"]), "agreement": mean(e["agree"]), "x_played": mean(e["x_played"]), "y_played": mean(e["y_played"]),
                "js_mean": mean(e["js_sum"]), "js_max": float(e["js_max"]), "js_total": float(e["js_sum"]),
                "kl_xy_mean": mean(e["kl_xy_sum"]), "kl_yx_mean": mean(e["kl_yx_sum"]),
                "logp_x_mean": mean(e["logp_x_sum"]), "logp_y_mean": mean(e["logp_y_sum"]),
                "hcp_mean": mean(e["hcp_sum"]), "hcp_mean_disagree": float(e["hcp_sum_disagree"]) / dis if dis else nan,
                "calls_x": top(e["calls_x"]), "calls_y": top(e["calls_y"]), "played": top(e["played"])}

    def entry(self, prefix) -> dict:
        """the entry of the decisions reached by ``prefix`` (a string, calls, or a key): n, the agreement rate, each network's
        agreement with the call played, the mean and largest JS, the mean KLs and log-probabilities of the played call, the callers'
        mean HCP overall and where the networks disagree, the three most frequent calls of X, Y and the players; KeyError without one"""
        key = np.uint64(prefix if isinstance(prefix, (int, np.integer)) else key_of(prefix))
        i = int(np.searchsorted(self.entries["key"], key))
        if i >= len(self.entries) or self.entries["key"][i] != key:
            raise KeyError(f"no entry for {name_of(int(key))!r}")
        return self._summary(i)

    def worst(self, k: int = 10, min_count: int = 1):
        """the ``k`` prefixes with at least ``min_count`` finite decisions where the two networks are furthest apart, ranked by
        n x mean JS (the entry's JS sum), ties by key"""
        e = self.entries
        finite = e["n"].astype(np.int64) - e["nonfinite"].astype(np.int64)
        idx = np.nonzero(finite >= max(1, int(min_count)))[0]
        order = idx[np.argsort(-e["js_sum"][idx], kind="stable")][:int(k)]
        return [self._summary(i) for i in order]

    def totals(self) -> dict:
        e = self.entries
        finite = e["n"].astype(np.int64) - e["nonfinite"].astype(np.int64)
        t_of = (e["key"] & np.uint64(15)).astype(np.int64) - 1
        f = int(finite.sum())
        nan = float("nan")
        by_t = []
        for t in range(self.depth):
            sel = t_of == t
            ft = int(finite[sel].sum())
            by_t.append({"call_index": t, "n": ft, "js_mean": float(np.add.reduce(e["js_sum"][sel])) / ft if ft else nan,
                         "agreement": int(e["agree"][sel].sum()) / ft if ft else nan})
        return {"decisions": int(e["n"].sum()), "finite": f, "nonfinite": int(e["nonfinite"].sum()), "prefixes": len(e),
                "agreement": int(e["agree"].sum()) / f if f else nan, "js_mean": float(np.add.reduce(e["js_sum"])) / f if f else nan,
                "x_played": int(e["x_played"].sum()) / f if f else nan, "y_played": int(e["y_played"].sum()) / f if f else nan,
                "by_call_index": by_t}

    def stats_lines(self, cells: int = 3, min_count: int = 1):
        """the lines ``python -m brl_amd.eval ... diff=1`` prints: the agreement rate and the mean JS overall and by call index, each
        network's agreement with the calls played, the largest off-diagonal confusion cells, the prefix that differs most"""
        s = self.totals()
        lines = [f"diff: {s['finite']} decisions (depth {self.depth}, {s['prefixes']} prefixes, {s['nonfinite']} non-finite, "
                 f"{sum(self.skipped.values())} records skipped), X and Y agree on {100 * s['agreement']:.1f}%, mean JS {s['js_mean']:.4f} nats",
                 "diff by call index: " + "; ".join(f"{b['call_index']}: agree {100 * b['agreement']:.1f}% JS {b['js_mean']:.4f} (n={b['n']})"
                                                    for b in s["by_call_index"] if b["n"]),
                 f"diff played: X calls what was played on {100 * s['x_played']:.1f}%, Y on {100 * s['y_played']:.1f}%"]
        off = self.confusion.copy()
        np.fill_diagonal(off, 0)
        top = [(int(c) // ACTIONS, int(c) % ACTIONS) for c in np.argsort(-off.reshape(-1), kind="stable")[:int(cells)]]
        top = [(x, y) for x, y in top if off[x, y] > 0]
        lines.append("diff confusion: " + ("; ".join(f"X {CALL_NAMES[x]} / Y {CALL_NAMES[y]}: {int(off[x, y])}" for x, y in top) or "none"))
        w = self.worst(1, min_count)
        if w:
            lines.append(f"diff largest: after {w[0]['prefix']} (n={w[0]['n']}) agree {100 * w[0]['agreement']:.1f}%, "
                         f"mean JS {w[0]['js_mean']:.4f}, X mostly {w[0]['calls_x'][0][0]}, Y mostly {w[0]['calls_y'][0][0]}")
        return lines

    # -- text and JSON
    def to_text(self, min_count: int = 1, k=None) -> str:
        """the summary lines, then one line per prefix with at least ``min_count`` finite decisions, the furthest apart first
        (``k``: at most that many)"""
        rows = self.worst(len(self.entries) if k is None else k, min_count)
        lines = self.stats_lines(min_count=min_count)
        for r in rows:
            calls = lambda h: ",".join(f"{c}:{n}" for c, n in h)     # noqa: E731
            lines.append(f"{r['prefix']:<28} n={r['n']:<6} agree {100 * r['agreement']:5.1f}%  JS {r['js_mean']:.4f} (max {r['js_max']:.4f})  "
                         f"KL {r['kl_xy_mean']:.4f}/{r['kl_yx_mean']:.4f}  HCP {r['hcp_mean']:.1f} ({r['hcp_mean_disagree']:.1f} apart)  "
                         f"X {calls(r['calls_x'])}  Y {calls(r['calls_y'])}  played {calls(r['played'])}")
        return "\n".join(lines) + "\n"

    def to_json(self, path=None):
        """the arrays themselves as a JSON document (written to ``path`` when given); ``from_json`` reads them back exactly"""
        field = lambda a, dt: {n: a[n].tolist() for n in dt.names}     # noqa: E731
        doc = {"format": "brl_amd.compare/1", "depth": self.depth, "tables": self.tables, "skipped": self.skipped,
               "boards": int(self.decisions.shape[1]), "totals": self.totals(), "decisions": field(self.decisions, DECISION_DTYPE),
               "entries": field(self.entries, ENTRY_DTYPE), "confusion": self.confusion.tolist()}
        if path is not None:
            with open(path, "w") as f:
                json.dump(doc, f)
        return doc

    @classmethod
    def from_json(cls, src):
        if not isinstance(src, dict):
            with open(src) as f:
                src = json.load(f)
        if src.get("format") != "brl_amd.compare/1":
            raise ValueError("not a diff written by PolicyDiff.to_json")

        def back(d, dt, shape):
            a = np.zeros(shape, dt)
            for name in dt.names:
                a[name] = np.asarray(d[name], dt.fields[name][0].base).reshape(a[name].shape)
            return a

        dec = back(src["decisions"], DECISION_DTYPE, (len(src["tables"]), src["boards"], src["depth"]))
        ent = back(src["entries"], ENTRY_DTYPE, (len(src["entries"]["key"]),))
        return cls(dec, ent, np.asarray(src["confusion"], np.int64), src["skipped"], src["depth"], src["tables"])

    def same_as(self, other) -> bool:
        """the same values in every field (NaN equal to NaN)"""
        def eq(a, b, dt):
            return a.shape == b.shape and all(np.array_equal(a[n], b[n], equal_nan=dt.fields[n][0].kind == "f") for n in dt.names)
        return ((self.depth, self.tables, self.skipped) == (other.depth, other.tables, other.skipped)
                and eq(self.decisions, other.decisions, DECISION_DTYPE) and eq(self.entries, other.entries, ENTRY_DTYPE)
                and np.array_equal(self.confusion, other.confusion))


# ---- the device path -----------------------------------------------------------------------------------------------------------
def compare_tables(rec, rows):
    """(tables int64 [m,16], hands int64 [m,4]): one ``brl_compare_tables`` launch; rec uint8 [n,368], rows int64 [m]"""
    import torch

    from . import _capi
    m, di = rows.shape[0], _capi.device_index(rec)
    tables = torch.empty((m, 16), dtype=torch.int64, device=rec.device)
    hands = torch.empty((m, 4), dtype=torch.int64, device=rec.device)
    _capi.check(_capi.lib().brl_compare_tables(di, _capi.ptr(rec), rec.shape[0], _capi.ptr(rows), m, _capi.ptr(tables), _capi.ptr(hands),
                                               _capi.stream(di)))
    return tables, hands


def compare_rows(rec, rows, t, depth, logits_x, logits_y, legal, decisions):
    """one ``brl_compare_rows`` launch: the decision records of call index t of the records ``rows`` into decisions uint8
    [n * depth, 64]; logits float32 [m, >= 38] of any row stride, legal int64 [m] (the masks' bits)"""
    from . import _capi
    di = _capi.device_index(rec)
    for lg in (logits_x, logits_y):
        assert lg.dtype.is_floating_point and lg.element_size() == 4 and lg.stride(1) == 1 and lg.shape[0] >= rows.shape[0]
    assert decisions.shape[0] == rec.shape[0] * depth
    _capi.check(_capi.lib().brl_compare_rows(di, _capi.ptr(rec), rec.shape[0], _capi.ptr(rows), rows.shape[0], int(t), int(depth),
                                             logits_x.data_ptr(), logits_x.stride(0), logits_y.data_ptr(), logits_y.stride(0),
                                             _capi.ptr(legal), _capi.ptr(decisions), _capi.stream(di)))


def compare_reduce(sorted_decisions, entry_start):
    """(entries uint8 [K,560], confusion int64 [38,38]): one ``brl_compare_reduce`` call; sorted_decisions uint8 [S,64],
    entry_start int64 [K + 1]"""
    import torch

    from . import _capi
    k, di = entry_start.shape[0] - 1, _capi.device_index(sorted_decisions)
    entries = torch.empty((k, ENTRY_DTYPE.itemsize), dtype=torch.uint8, device=sorted_decisions.device)
    confusion = torch.empty((ACTIONS, ACTIONS), dtype=torch.int64, device=sorted_decisions.device)
    _capi.check(_capi.lib().brl_compare_reduce(di, _capi.ptr(sorted_decisions), sorted_decisions.shape[0], _capi.ptr(entry_start), k,
                                               _capi.ptr(entries), _capi.ptr(confusion), _capi.stream(di)))
    return entries, confusion


def sort_and_reduce(decisions):
    """(entries uint8 [K,560], confusion int64 [38,38]) of dense decisions uint8 [D,64] on the device: a stable torch sort of the
    keys (unsigned order), ``unique_consecutive`` for the runs — its sizes are the one host read — and ``brl_compare_reduce``"""
    import torch
    dev = decisions.device
    keys = decisions.view(torch.int64)[:, 0]
    top = torch.tensor(-2 ** 63, dtype=torch.int64, device=dev)
    ordered, perm = torch.sort(torch.bitwise_xor(keys, top), stable=True)     # key 0 becomes the smallest int64
    unique, counts = torch.unique_consecutive(ordered, return_counts=True)
    start = torch.zeros(unique.shape[0] + 1, dtype=torch.int64, device=dev)
    start[1:] = counts.cumsum(0)
    first = int((unique[0] == top).item())                                     # a run of key 0 leads: no entry
    if unique.shape[0] - first == 0:
        return (torch.zeros((0, ENTRY_DTYPE.itemsize), dtype=torch.uint8, device=dev),
                torch.zeros((ACTIONS, ACTIONS), dtype=torch.int64, device=dev))
    return compare_reduce(decisions[perm].contiguous(), start[first:].contiguous())


def _records(x):
    """a record array or tensor as a uint8 [n,368] tensor, wherever it lives; ``ValueError`` for anything else"""
    import torch
    if isinstance(x, np.ndarray):
        if x.dtype != RECORD_DTYPE and not (x.dtype == np.uint8 and x.ndim == 2 and x.shape[1] == RECORD_DTYPE.itemsize):
            raise ValueError("records: RECORD_DTYPE, or uint8 [n,368] (boards.board_records)")
        x = torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1, RECORD_DTYPE.itemsize))
    if not isinstance(x, torch.Tensor) or x.dtype != torch.uint8 or x.dim() != 2 or x.shape[1] != RECORD_DTYPE.itemsize:
        raise ValueError("records: uint8 [n,368] (boards.board_records)")
    return x


def make_policy_diff(eval_env, x_activation, x_model_type, y_activation, y_model_type, depth: int = 4, max_rows: int = MAX_ROWS):
    """``policy_diff(x_params, y_params, records, tables="ab", rows=None) -> PolicyDiff``.

    ``records``: a ``BoardRecords`` (``boards.make_board_match``) or one uint8 [n,368] record tensor (table "a"); ``tables``: "a",
    "b" or "ab".  X and Y are shown every decision of the first ``depth`` calls of every auction, whichever team made the call.
    Records are processed in chunks of at most ``max_rows``; inside a chunk the reviewable records are ordered by falling
    min(n_calls, depth), so the rows still in their auction are always the leading ones.  Per call index the live rows are
    observed, forwarded through X and Y (``evaluation._Forward``: one object and one forward when the parameter sets are the same
    object) and written by ``brl_compare_rows``, then stepped with the recorded call; nothing is read back inside the loop.

    A batch's size selects the forward's kernels, so the last bits of a logit — and with them of ``logp`` and the divergences —
    depend on the record set and the chunking; the integer fields do wherever two legal logits are that close.
    ``rows``: a list that receives per (table, chunk, call index) {"table", "first", "t", "rows" (record indices of the chunk's
    live rows), "logits_x", "logits_y" float32 [m,38], "legal" uint64 [m]} as the device used them.  Runs on one rank."""
    if not 1 <= int(depth) <= MAX_DEPTH:
        raise ValueError(f"depth is 1 .. {MAX_DEPTH}")
    if int(max_rows) < 1:
        raise ValueError("max_rows >= 1")
    depth, max_rows = int(depth), int(max_rows)
    import torch

    from . import _capi
    from ._capi import OBS_SIZE
    from .dist import one_rank_only
    from .evaluation import _Forward, _team_forwards
    from .models import make_forward_pass
    fpx = make_forward_pass(x_activation, x_model_type)
    fpy = make_forward_pass(y_activation, y_model_type)
    off = lambda name: RECORD_DTYPE.fields[name][1]     # noqa: E731

    def chunk(fwdx, fwdy, rec, decisions, taken, label):
        """the decisions of the records ``rec`` into ``decisions`` (zeroed, uint8 [n * depth, 64]); -> the records skipped (a tensor)"""
        dev, L, n = rec.device, _capi.lib(), rec.shape[0]
        n_calls = rec[:, off("n_calls")].to(torch.int64) | (rec[:, off("n_calls") + 1].to(torch.int64) << 8)
        flags = rec[:, off("flags")].to(torch.int64)
        ok = ((flags & OK) != 0) & ((flags & ILLEGAL) == 0)
        cnt = torch.where(ok, n_calls.clamp(max=depth), torch.zeros_like(n_calls))
        order = torch.sort(cnt, descending=True, stable=True)[1]
        live = (cnt[:, None] > torch.arange(depth, device=dev)[None, :]).sum(0).tolist()     # the one read: sizes the loop
        if live[0] == 0:
            return (~ok).sum()
        rows_ = order[:live[0]].contiguous()
        tables, _ = compare_tables(rec, rows_)
        calls = rec[:, off("calls"):off("calls") + depth].index_select(0, rows_).to(torch.int32).t().contiguous()     # [depth, m]
        bit = torch.ones(ACTIONS, dtype=torch.int64, device=dev) << torch.arange(ACTIONS, device=dev)
        for t in range(depth):
            m = live[t]
            if m == 0:
                break
            obs = torch.empty((m, OBS_SIZE), dtype=torch.bool, device=dev)
            mask = torch.empty((m, ACTIONS), dtype=torch.uint8, device=dev)
            _capi.check(L.brl_observe(eval_env._h, _capi.ptr(tables), m, None, _capi.ptr(obs), _capi.ptr(mask), _capi.stream()))
            legal = (mask.to(torch.int64) * bit[None, :]).sum(1)
            lx, ly = _Forward.whole_pair(fwdx, fwdy, obs, eval_env)
            compare_rows(rec, rows_[:m], t, depth, lx, ly, legal, decisions)
            if taken is not None:
                taken.append(dict(label, t=t, rows=rows_[:m], logits_x=lx[:, :ACTIONS].clone(), logits_y=ly[:, :ACTIONS].clone(), legal=legal))
            _capi.check(L.brl_step(eval_env._h, _capi.ptr(tables), _capi.ptr(tables), m, _capi.ptr(calls[t, :m].contiguous()), 0, None,
                                   None, None, None, None, _capi.stream()))
        return (~ok).sum()

    def policy_diff(x_params, y_params, records, tables="ab", rows=None):
        one_rank_only("policy_diff")
        if tables not in ("a", "b", "ab"):
            raise ValueError(f"tables={tables!r}: 'a', 'b' or 'ab'")
        if isinstance(records, BoardRecords):
            if "b" in tables and records.table_b is None:
                raise ValueError("policy_diff: the records hold no table B")
            source = {"a": records.table_a, "b": records.table_b}
        else:
            if tables != "a":
                raise ValueError("policy_diff: one record tensor is table 'a'")
            source = {"a": records}
        recs = [_records(source[tb]) for tb in tables]
        n = recs[0].shape[0]
        if any(r.shape[0] != n for r in recs):
            raise ValueError("policy_diff: the two tables hold different numbers of records")
        dev = eval_env.device
        recs = [r.to(dev).contiguous() for r in recs]
        if n == 0:
            return PolicyDiff(np.zeros((len(tables), 0, depth), DECISION_DTYPE), np.zeros(0, ENTRY_DTYPE), np.zeros((ACTIONS, ACTIONS), np.int64),
                              {tb: 0 for tb in tables}, depth, tables)
        with torch.no_grad():
            fwdx, fwdy = _team_forwards(fpx, x_params, fpy, y_params)
            decisions = torch.zeros((len(tables) * n * depth, DECISION_DTYPE.itemsize), dtype=torch.uint8, device=dev)
            taken = [] if rows is not None else None
            skipped = []
            for k, rec in enumerate(recs):
                bad = torch.zeros((), dtype=torch.int64, device=dev)
                for a in range(0, n, max_rows):
                    b = min(n, a + max_rows)
                    bad += chunk(fwdx, fwdy, rec[a:b], decisions[(k * n + a) * depth:(k * n + b) * depth], taken, {"table": tables[k], "first": a})
                skipped.append(bad)
            entries, confusion = sort_and_reduce(decisions)
            out = PolicyDiff(decisions.cpu().numpy(), entries.cpu().numpy(), confusion.cpu().numpy(),
                             {tb: int(s) for tb, s in zip(tables, skipped)}, depth, tables)
            if rows is not None:
                for r in taken:
                    rows.append({k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in r.items()})
                    rows[-1]["legal"] = rows[-1]["legal"].view(np.uint64)
        if not np.array_equal(out.entries["n"].astype(np.int64).sum(), np.int64(len(out))):
            raise RuntimeError("policy_diff: the entries' counts differ from the decisions written")
        return out

    return policy_diff
