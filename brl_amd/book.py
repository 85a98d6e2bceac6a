"""The bidding-system book: what each call shows, by auction prefix (include/brl_book.h).

* ``system_book(records, depth=4)`` — every call of the first ``depth`` calls of every record, grouped on the device by the
  sequence that led to it: ``brl_book_samples`` per table, a torch sort, ``brl_book_reduce``.  The host receives the table only.
* ``SystemBook`` — numpy arrays of exact integer counters per prefix and team; works without a GPU once built.
* ``key_of("1NT P 2C")`` / ``name_of(key)`` — the prefix key and back, in ``boards.CALL_NAMES``.
"""
from __future__ import annotations

import json
import math

import numpy as np

from .boards import CALL_NAMES, OK, RECORD_DTYPE, BoardRecords

MAX_DEPTH = 10             # BRL_BOOK_MAX_DEPTH
SUITS = "CDHS"             # the order of length_hist's suit axis
TEAM_DTYPE = np.dtype([("count", "<u4"), ("balanced", "<u4"), ("hcp", "<u4", 38), ("length", "<u4", (4, 14)),
                       ("imp_sum", "<i8"), ("imp_sq_sum", "<u8")])
ENTRY_DTYPE = np.dtype([("key", "<u8"), ("reserved", "<u8"), ("team", TEAM_DTYPE, 2)])
assert TEAM_DTYPE.itemsize == 400 and ENTRY_DTYPE.itemsize == 816   # BRL_BOOK_ENTRY_BYTES

_CALL_ID = {name: i for i, name in enumerate(CALL_NAMES)}


# ---- keys ----------------------------------------------------------------------------------------------------------------------
def key_of(prefix) -> int:
    """the key of a prefix: ``"1NT P 2C"``, or a sequence of call names or action ids; the empty prefix is key 0"""
    calls = prefix.split() if isinstance(prefix, str) else list(prefix)
    if len(calls) > MAX_DEPTH:
        raise ValueError(f"a prefix has at most {MAX_DEPTH} calls, not {len(calls)}")
    key = 0
    for j, c in enumerate(calls):
        if isinstance(c, str):
            if c not in _CALL_ID:
                raise ValueError(f"not a call: {c!r}")
            c = _CALL_ID[c]
        c = int(c)
        if not 0 <= c < len(CALL_NAMES):
            raise ValueError(f"not a call: {c}")
        key |= (c + 1) << (58 - 6 * j)
    return key


def calls_of(key: int):
    """the action ids of a key's prefix"""
    key = int(key)
    out = []
    for j in range(MAX_DEPTH):
        f = (key >> (58 - 6 * j)) & 63
        if f == 0:
            break
        if f > len(CALL_NAMES):
            raise ValueError(f"not a key: {key:#x}")
        out.append(f - 1)
    if key & ~(-1 << (64 - 6 * len(out))) & ((1 << 64) - 1):
        raise ValueError(f"not a key: {key:#x}")
    return out


def name_of(key: int) -> str:
    return " ".join(CALL_NAMES[c] for c in calls_of(key))


def key_depth(keys) -> np.ndarray:
    """the number of calls of each key"""
    keys = np.asarray(keys, np.uint64)
    d = np.zeros(keys.shape, np.int64)
    for j in range(MAX_DEPTH):
        d += ((keys >> np.uint64(58 - 6 * j)) & np.uint64(63)) != 0
    return d


# ---- the book ------------------------------------------------------------------------------------------------------------------
def _percentile(hist, q):
    """the q-th percentile of a histogram by nearest rank: the smallest value whose cumulative count reaches ceil(q / 100 * n)"""
    n = int(hist.sum())
    rank = max(1, -(-q * n // 100))
    return int(np.searchsorted(np.cumsum(hist), rank))


class SystemBook:
    """One entry per auction prefix, ascending by key (= depth-first through the prefix tree, a prefix before its extensions).
    The team axis has team 1 (players 0, 1) at index 0 and team 2 at index 1.

      keys uint64 [K]; count, balanced int64 [K,2]; hcp_hist int64 [K,2,38]; length_hist int64 [K,2,4,14] (suits C,D,H,S);
      imp_sum int64 [K,2]; imp_sq_sum uint64 [K,2]; depth: the calls per auction that were sampled; skipped: records without
      the self-check bit, which gave no samples; has_imp: whether the records came with their IMPs."""

    def __init__(self, keys, count, balanced, hcp_hist, length_hist, imp_sum, imp_sq_sum, depth=MAX_DEPTH, skipped=0, has_imp=True):
        self.keys = np.asarray(keys, np.uint64).reshape(-1)
        k = self.keys.shape[0]
        self.count = np.asarray(count, np.int64).reshape(k, 2)
        self.balanced = np.asarray(balanced, np.int64).reshape(k, 2)
        self.hcp_hist = np.asarray(hcp_hist, np.int64).reshape(k, 2, 38)
        self.length_hist = np.asarray(length_hist, np.int64).reshape(k, 2, 4, 14)
        self.imp_sum = np.asarray(imp_sum, np.int64).reshape(k, 2)
        self.imp_sq_sum = np.asarray(imp_sq_sum, np.uint64).reshape(k, 2)
        self.depth, self.skipped, self.has_imp = int(depth), int(skipped), bool(has_imp)
        if k > 1 and not (self.keys[1:] > self.keys[:-1]).all():
            raise ValueError("the keys of a book ascend strictly")

    @classmethod
    def from_entries(cls, entries, **kw):
        """from brl_book_reduce's entries (``ENTRY_DTYPE``, or their bytes as uint8 [K,816])"""
        e = np.ascontiguousarray(entries)
        e = e if e.dtype == ENTRY_DTYPE else e.view(ENTRY_DTYPE).reshape(-1)
        t = e["team"]
        return cls(e["key"], t["count"], t["balanced"], t["hcp"], t["length"], t["imp_sum"], t["imp_sq_sum"], **kw)

    def __len__(self):
        return int(self.keys.shape[0])

    def __eq__(self, other):
        return isinstance(other, SystemBook) and (self.depth, self.skipped, self.has_imp) == (other.depth, other.skipped, other.has_imp) \
            and all(np.array_equal(getattr(self, n), getattr(other, n)) for n in self._ARRAYS)

    _ARRAYS = ("keys", "count", "balanced", "hcp_hist", "length_hist", "imp_sum", "imp_sq_sum")

    # -- lookups
    def index(self, prefix) -> int:
        """the entry of a prefix (a string, a sequence of calls, or a key); KeyError when the book has none"""
        key = np.uint64(prefix if isinstance(prefix, (int, np.integer)) else key_of(prefix))
        i = int(np.searchsorted(self.keys, key))
        if i >= len(self) or self.keys[i] != key:
            raise KeyError(f"no entry for {name_of(int(key))!r}")
        return i

    @staticmethod
    def _teams(team):
        if team not in (None, 1, 2):
            raise ValueError("team is None (both pooled), 1 or 2")
        return slice(None) if team is None else slice(team - 1, team)

    def _summary(self, i, team=None):
        ts = self._teams(team)
        n = int(self.count[i, ts].sum())
        hcp = self.hcp_hist[i, ts].sum(0)
        length = self.length_hist[i, ts].sum(0)
        out = {"prefix": name_of(int(self.keys[i])), "count": n}
        nan = float("nan")
        if n == 0:
            out.update(hcp_mean=nan, hcp_min=None, hcp_max=None, hcp_p5=None, hcp_p95=None, length_mean={s: nan for s in SUITS},
                       length_mode={s: None for s in SUITS}, balanced=nan, imp_mean=None if not self.has_imp else nan,
                       imp_se=None if not self.has_imp else nan)
            return out
        held = np.nonzero(hcp)[0]
        out.update(hcp_mean=float((hcp * np.arange(38)).sum() / n), hcp_min=int(held[0]), hcp_max=int(held[-1]),
                   hcp_p5=_percentile(hcp, 5), hcp_p95=_percentile(hcp, 95),
                   length_mean={s: float((length[k] * np.arange(14)).sum() / n) for k, s in enumerate(SUITS)},
                   length_mode={s: int(length[k].argmax()) for k, s in enumerate(SUITS)},
                   balanced=float(self.balanced[i, ts].sum() / n))
        if self.has_imp:
            total, sq = int(self.imp_sum[i, ts].sum()), int(self.imp_sq_sum[i, ts].astype(object).sum())
            out["imp_mean"] = total / n
            # the standard error of the mean from the exact sums: sqrt(sample variance / n)
            out["imp_se"] = math.sqrt(max(0.0, (sq - total * total / n) / (n - 1)) / n) if n > 1 else nan
        else:
            out["imp_mean"] = out["imp_se"] = None
        return out

    def entry(self, prefix, team=None) -> dict:
        """what the last call of ``prefix`` shows — count; HCP mean, min, max and the 5th / 95th percentile (nearest rank on the
        histogram); per suit the mean and the most frequent length; the balanced ratio; the bidder's-side IMP mean and its
        standard error — over both teams (``team=None``) or team 1 / 2"""
        return self._summary(self.index(prefix), team)

    def continuations(self, prefix="", team=None):
        """the calls made after ``prefix`` (the empty prefix: the openings), by key: [{"call", "count", "share"}], share of
        all continuations; ``team`` counts that team's bidders only"""
        key = key_of(prefix) if not isinstance(prefix, (int, np.integer)) else int(prefix)
        d = len(calls_of(key))
        if d >= MAX_DEPTH:
            return []
        lo = np.searchsorted(self.keys, np.uint64(key), side="right")
        hi = len(self) if d == 0 else np.searchsorted(self.keys, np.uint64(key + (1 << (64 - 6 * d)) - 1), side="right")
        idx = np.arange(lo, hi)
        idx = idx[key_depth(self.keys[idx]) == d + 1]
        counts = self.count[idx][:, self._teams(team)].sum(1)
        total = int(counts.sum())
        return [{"call": CALL_NAMES[calls_of(int(self.keys[i]))[-1]], "count": int(c), "share": int(c) / total if total else float("nan")}
                for i, c in zip(idx, counts) if c > 0]

    # -- text
    def to_text(self, min_count=1, max_depth=None) -> str:
        """an indented tree, one line per entry with at least ``min_count`` samples and at most ``max_depth`` calls:
        ``1NT  n=812  HCP 15.9 (15–17)  S3.1 H3.0 D3.4 C3.5  bal 0.97  IMP +0.21±0.18`` (HCP mean and 5th–95th percentile, the
        mean suit lengths, the balanced ratio, the bidder's-side IMP mean ± standard error), both teams pooled"""
        lines = []
        depths = key_depth(self.keys)
        for i in range(len(self)):
            if (max_depth is not None and depths[i] > max_depth) or self.count[i].sum() < min_count:
                continue
            s = self._summary(i)
            line = (f"{'  ' * (int(depths[i]) - 1)}{s['prefix'].split()[-1]}  n={s['count']}  HCP {s['hcp_mean']:.1f} ({s['hcp_p5']}–{s['hcp_p95']})  "
                    + " ".join(f"{c}{s['length_mean'][c]:.1f}" for c in "SHDC") + f"  bal {s['balanced']:.2f}")
            if self.has_imp:
                line += f"  IMP {s['imp_mean']:+.2f}±{s['imp_se']:.2f}"
            lines.append(line)
        return "\n".join(lines) + ("\n" if lines else "")

    # -- JSON: the counters themselves
    def to_json(self, path=None, min_count=1):
        """the counters as a JSON document (written to ``path`` when given); ``from_json`` reads it back exactly.  Entries with
        fewer than ``min_count`` samples are left out."""
        keep = np.nonzero(self.count.sum(1) >= min_count)[0]
        doc = {"format": "brl_amd.book/1", "depth": self.depth, "skipped": self.skipped, "has_imp": self.has_imp,
               "entries": [{"prefix": name_of(int(self.keys[i])), "key": int(self.keys[i]),
                            "teams": [{"count": int(self.count[i, t]), "balanced": int(self.balanced[i, t]),
                                       "hcp": self.hcp_hist[i, t].tolist(), "length": self.length_hist[i, t].tolist(),
                                       "imp_sum": int(self.imp_sum[i, t]), "imp_sq_sum": int(self.imp_sq_sum[i, t])} for t in (0, 1)]}
                           for i in keep]}
        if path is not None:
            with open(path, "w") as f:
                json.dump(doc, f)
        return doc

    @classmethod
    def from_json(cls, src):
        """a book from ``to_json``'s document or the path of one"""
        if not isinstance(src, dict):
            with open(src) as f:
                src = json.load(f)
        if src.get("format") != "brl_amd.book/1":
            raise ValueError("not a book written by SystemBook.to_json")
        es = src["entries"]
        for e in es:
            if key_of(e["prefix"]) != e["key"]:
                raise ValueError(f"entry {e['prefix']!r}: the key does not match the prefix")
        teams = lambda name: [[e["teams"][t][name] for t in (0, 1)] for e in es]   # noqa: E731
        return cls(np.array([e["key"] for e in es], np.uint64), teams("count"), teams("balanced"), teams("hcp"), teams("length"),
                   teams("imp_sum"), np.array(teams("imp_sq_sum"), np.uint64), depth=src["depth"], skipped=src["skipped"],
                   has_imp=src["has_imp"])

    def save(self, path, min_count=1):
        """``.txt``: the tree; anything else: JSON"""
        if str(path).lower().endswith(".txt"):
            with open(path, "w") as f:
                f.write(self.to_text(min_count=min_count))
        else:
            self.to_json(path, min_count=min_count)


def _empty(depth, skipped, has_imp):
    z = np.zeros((0, 2), np.int64)
    return SystemBook(np.zeros(0, np.uint64), z, z, np.zeros((0, 2, 38), np.int64), np.zeros((0, 2, 4, 14), np.int64), z,
                      np.zeros((0, 2), np.uint64), depth=depth, skipped=skipped, has_imp=has_imp)


# ---- the device path ------------------------------------------------------------------------------------------------------------
def _device_records(x, dev=None):
    import torch
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1, RECORD_DTYPE.itemsize)).to(dev or "cuda")
    if x.dtype != torch.uint8 or x.dim() != 2 or x.shape[1] != RECORD_DTYPE.itemsize or not x.is_cuda:
        raise ValueError("records: uint8 [n,368] on the device (boards.board_records)")
    return x.contiguous()


def book_samples(records, depth, imp=None, imp_sign=1, keys=None, feats=None):
    """one ``brl_book_samples`` launch on the current stream: (keys int64 [n * depth] — the uint64 keys' bits —, feats int32
    [n * depth]) of uint8 [n,368] device records; ``keys`` / ``feats``: where to write them"""
    import torch

    from . import _capi
    n = records.shape[0]
    if keys is None:
        keys = torch.empty(n * depth, dtype=torch.int64, device=records.device)
        feats = torch.empty(n * depth, dtype=torch.int32, device=records.device)
    di = _capi.device_index(records)
    _capi.check(_capi.lib().brl_book_samples(di, _capi.ptr(records), n, _capi.ptr(imp), int(imp_sign), int(depth), _capi.ptr(keys),
                                             _capi.ptr(feats), _capi.stream(di)))
    return keys, feats


def book_reduce(feats, entry_index, entry_keys):
    """one ``brl_book_reduce`` call on the current stream: uint8 [K,816] entries of the sorted samples"""
    import torch

    from . import _capi
    k = entry_keys.shape[0]
    entries = torch.empty((k, ENTRY_DTYPE.itemsize), dtype=torch.uint8, device=feats.device)
    di = _capi.device_index(feats)
    _capi.check(_capi.lib().brl_book_reduce(di, _capi.ptr(feats), _capi.ptr(entry_index), feats.shape[0], _capi.ptr(entry_keys), k,
                                            _capi.ptr(entries), _capi.stream(di)))
    return entries


def system_book(records, depth: int = 4) -> SystemBook:
    """The book of a match's records: a ``BoardRecords`` (both tables, with its ``imp`` when present) or one uint8 [n,368]
    device tensor.  Subsets (one vulnerability, one dealer) are taken by indexing the record tensors before the call.

    Per table one ``brl_book_samples`` launch into its half of one buffer; then torch sorts the keys, ``unique_consecutive``
    numbers the runs — its count of them is the only host synchronisation before the second launch — and the features are
    gathered into key order for ``brl_book_reduce``.  A sentinel sample with key 0 behind the buffer makes key 0 always the
    first run, which gets entry index -1 and is dropped by the kernel."""
    import torch
    if not 1 <= int(depth) <= MAX_DEPTH:
        raise ValueError(f"depth is 1 .. {MAX_DEPTH}")
    depth = int(depth)
    if isinstance(records, BoardRecords):
        tables = [records.table_a] + ([records.table_b] if records.table_b is not None else [])
        imp = records.imp
    else:
        tables, imp = [records], None
    dev = next((t.device for t in tables if not isinstance(t, np.ndarray)), None)
    tables = [_device_records(t, dev) for t in tables]
    dev = tables[0].device
    n = tables[0].shape[0]
    if any(t.shape[0] != n for t in tables):
        raise ValueError("the two tables hold different numbers of records")
    if n == 0:
        return _empty(depth, 0, imp is not None)
    if imp is not None:
        imp = (torch.from_numpy(np.ascontiguousarray(imp)) if isinstance(imp, np.ndarray) else imp).to(device=dev, dtype=torch.int32).contiguous()
        if imp.shape != (n,):
            raise ValueError("imp: one value per board")
    with torch.no_grad():
        per = n * depth
        total = len(tables) * per
        keys = torch.empty(total + 1, dtype=torch.int64, device=dev)
        feats = torch.empty(total + 1, dtype=torch.int32, device=dev)
        keys[total:] = 0
        feats[total:] = 0
        skipped = torch.zeros((), dtype=torch.int64, device=dev)
        for t, rec in enumerate(tables):
            book_samples(rec, depth, imp, 1 if t == 0 else -1, keys[t * per:(t + 1) * per], feats[t * per:(t + 1) * per])
            skipped += ((rec[:, RECORD_DTYPE.fields["flags"][1]] & OK) == 0).sum()
        # int64 order of key ^ 2^63 is the unsigned order of the key; key 0 becomes the smallest int64
        top = torch.tensor(-2 ** 63, dtype=torch.int64, device=dev)
        ordered, perm = torch.sort(torch.bitwise_xor(keys, top))
        unique, inverse, counts = torch.unique_consecutive(ordered, return_inverse=True, return_counts=True)
        k = int(unique.shape[0]) - 1
        if k == 0:
            return _empty(depth, int(skipped), imp is not None)
        entries = book_reduce(feats[perm], (inverse - 1).to(torch.int32), torch.bitwise_xor(unique[1:], top).contiguous())
        book = SystemBook.from_entries(entries.cpu().numpy(), depth=depth, skipped=int(skipped), has_imp=imp is not None)
        if not np.array_equal(book.count.sum(1), counts[1:].cpu().numpy()):
            raise RuntimeError("system_book: an entry's count differs from its run of sorted keys")
    return book
