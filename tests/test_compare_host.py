"""The host side of the system diff (brl_amd/compare.py, include/brl_compare.h) without a GPU: the header against the ctypes binding
and the numpy dtypes, the key, the restatement's own properties (tests/compare_ref.py), and a PolicyDiff built from the
restatement — lookups, ``worst``, the text and the JSON round trip, argument validation."""
import os
import re
import types

import numpy as np
import pytest

from brl_amd import book, compare
from brl_amd.boards import CALL_NAMES, RECORD_DTYPE
from tests import belief_ref as BR
from tests import board_records_ref as R
from tests import book_ref as B
from tests import compare_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "brl_compare.h")).read()
C_TYPES = {"uint64_t": "<u8", "uint32_t": "<u4", "uint8_t": "u1", "float": "<f4", "double": "<f8"}


def _struct(name):
    """[(field, numpy type, count)] of a struct of the header, in order"""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = decl.split(None, 1)
        for nm in names.split(","):
            m = re.match(r"\s*(\w+)(?:\[(\w+)\])?\s*$", nm)
            count = {"BRL_COMPARE_ACTIONS": 38, None: 1}.get(m.group(2), m.group(2))
            out.append((m.group(1), C_TYPES[ctype], int(count)))
    return out


@pytest.mark.parametrize("name,dtype", [("brl_compare_decision", compare.DECISION_DTYPE), ("brl_compare_entry", compare.ENTRY_DTYPE)])
def test_the_headers_structs_are_the_numpy_dtypes(name, dtype):
    fields = _struct(name)
    assert [f[0] for f in fields] == list(dtype.names)
    offset = 0
    for fname, kind, count in fields:
        sub, at = dtype.fields[fname][0], dtype.fields[fname][1]
        assert at == offset and sub.base == np.dtype(kind) and int(np.prod(sub.shape or (1,))) == count, fname
        offset += sub.itemsize
    assert offset == dtype.itemsize and dtype.itemsize % 16 == 0                      # no padding, whole 16-byte pieces
    assert f"#define {name.upper()}_BYTES {dtype.itemsize}" in HEADER


def test_the_headers_constants_and_signatures_are_the_bindings():
    for cname, value in (("ACTIONS", compare.ACTIONS), ("BLOCK", compare.BLOCK), ("VALID", compare.VALID), ("AGREE", compare.AGREE),
                         ("X_PLAYED", compare.X_PLAYED), ("Y_PLAYED", compare.Y_PLAYED), ("NONFINITE", compare.NONFINITE)):
        assert re.search(r"#define BRL_COMPARE_%s %d\b" % (cname, value), HEADER), cname
    assert (CR.ACTIONS, CR.BLOCK, CR.VALID, CR.AGREE, CR.X_PLAYED, CR.Y_PLAYED, CR.NONFINITE) == (38, 64, 1, 2, 4, 8, 16)
    assert compare.MAX_DEPTH == book.MAX_DEPTH == 10


# ---- the key ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", range(10))
def test_key_round_trips_with_the_books(t):
    rng = np.random.default_rng(t)
    for calls in ([0] * 10, [37] * 10, list(rng.integers(0, 38, size=10))):
        calls = [int(c) for c in calls]
        k = compare.key_of(calls[:t])
        assert k == CR.key(calls, t) == compare.key_of(" ".join(CALL_NAMES[c] for c in calls[:t])) and 0 < k < 1 << 64
        assert k & 15 == t + 1 and book.calls_of(k & ~15) == calls[:t] and compare.prefix_of(k) == (calls[:t], t)
        assert k & ~15 == book.key_of(calls[:t])                       # the book's fields of the prefix BEFORE the call
    assert compare.key_of("") == 1 and compare.name_of(1) == "(opening)" and compare.name_of(compare.key_of("1NT P")) == "1NT P"


def test_bad_keys_and_prefixes_are_refused():
    with pytest.raises(ValueError):
        compare.key_of(["P"] * 10)                  # the tenth decision has nine calls before it
    with pytest.raises(ValueError):
        compare.prefix_of(book.key_of("P") | 1)     # one call, but call index 0
    with pytest.raises(ValueError):
        compare.prefix_of(0)


def test_key_order_is_a_prefix_before_its_extensions():
    rng = np.random.default_rng(5)
    prefixes = {()}
    for _ in range(300):
        calls = tuple(int(c) for c in rng.integers(0, 38, size=int(rng.integers(1, 10))))
        prefixes.update(calls[:k] for k in range(len(calls) + 1))
    prefixes = list(prefixes)
    by_key = sorted(prefixes, key=compare.key_of)
    assert by_key == sorted(prefixes)                                   # tuple order: call by call, a prefix before its extensions
    keys = np.array([compare.key_of(p) for p in by_key], np.uint64)
    assert (keys[1:] > keys[:-1]).all() and (keys >> np.uint64(63)).any() and keys[0] == 1


# ---- the restatement's own properties ----------------------------------------------------------------------------------------------
def _random_case(m=400, seed=0, scale=6.0):
    rng = np.random.default_rng(seed)
    lx = (rng.normal(size=(m, 38)) * scale).astype(np.float32)
    ly = (lx + rng.normal(size=(m, 38)) * rng.choice([0.0, 0.01, 1.0, 8.0], size=(m, 1))).astype(np.float32)
    words = [1, 1 | (1 << 37), (1 << 38) - 1, 1 | 2 | (((1 << 38) - 1) >> 9 << 9), 1 | 4 | (((1 << 38) - 1) >> 20 << 20)]
    legal = np.array([words[i % len(words)] for i in range(m)], np.uint64)
    return lx, ly, legal


SLACK = 2.0 ** -50      # a few roundings of sums of at most 38 terms whose magnitudes sum to at most 2 ln 2


def test_kl_of_a_network_with_itself_is_exactly_zero_and_js_is_bounded_and_symmetric():
    lx, ly, legal = _random_case()
    same = CR.divergences(lx, lx, legal)
    for name in ("kl_xy", "kl_yx", "js"):
        assert (same[name] == 0.0).all() and not np.signbit(same[name]).any(), name
    d, swapped = CR.divergences(lx, ly, legal), CR.divergences(ly, lx, legal)
    assert (d["js"] >= -SLACK).all() and (d["js"] <= CR.LN2 + SLACK).all() and d["js"].max() > 0.3
    assert (d["kl_xy"] >= -SLACK).all() and (d["kl_yx"] >= -SLACK).all()
    assert d["js"].tobytes() == swapped["js"].tobytes()
    assert d["kl_xy"].tobytes() == swapped["kl_yx"].tobytes() and d["kl_yx"].tobytes() == swapped["kl_xy"].tobytes()
    assert np.array_equal(d["call_x"], swapped["call_y"]) and not d["nonfinite"].any()
    one = legal == 1                                                     # one legal action: nothing to differ about
    assert one.any() and (d["js"][one] == 0.0).all() and (d["kl_xy"][one] == 0.0).all() and (d["call_x"][one] == 0).all()
    # against the textbook formulas in plain float64
    ok = CR.legal_bits(legal)
    p, q = (np.where(ok, np.exp(v.astype(np.float64) - np.where(ok, v, -np.inf).max(1, keepdims=True)), 0.0) for v in (lx, ly))
    p, q = p / p.sum(1, keepdims=True), q / q.sum(1, keepdims=True)
    with np.errstate(all="ignore"):
        mid = 0.5 * (p + q)
        kl = lambda a, b: np.where(a > 0, a * (np.log(a) - np.log(b)), 0.0).sum(1)     # noqa: E731
        assert np.allclose(d["kl_xy"], kl(p, q), rtol=1e-9, atol=1e-12) and np.allclose(d["js"], 0.5 * kl(p, mid) + 0.5 * kl(q, mid), rtol=1e-9, atol=1e-12)


def test_disjoint_policies_reach_ln_2_and_an_infinite_kl():
    """X puts everything on pass, Y everything on 1C (``_PassOnly``'s -1e30 elsewhere): JS = ln 2 and the KLs are the 1e30 the
    logits say; where Y's logit of X's call is -inf, KL(X||Y) is +inf.  A legal -inf logit is not non-finite."""
    lx = np.full((2, 38), -1e30, np.float32)
    ly = lx.copy()
    lx[:, 0], ly[:, 3] = 0.0, 0.0
    lx[1, 5], ly[1, 0] = -np.inf, -np.inf
    d = CR.divergences(lx, ly, np.array([(1 << 38) - 1] * 2, np.uint64))
    assert np.allclose(d["js"], CR.LN2, rtol=0, atol=SLACK) and d["kl_xy"][0] == d["kl_yx"][0] == np.float64(np.float32(1e30))
    assert d["kl_xy"][1] == np.inf and d["kl_yx"][1] == np.float64(np.float32(1e30))
    assert not d["nonfinite"].any() and d["call_x"].tolist() == [0, 0] and d["call_y"].tolist() == [3, 3]
    assert CR.flags(d, [0, 3]).tolist() == [CR.VALID | CR.X_PLAYED, CR.VALID | CR.Y_PLAYED]


def test_the_non_finite_cases_set_the_flag_and_give_nan():
    nan, inf = np.nan, np.inf
    word = 1 | 2 | (0xFF << 10)                      # legal: 0, 1, 10..17
    base = np.linspace(-3, 3, 38).astype(np.float32)
    rows, want = [], []
    for at, value, bad in ((14, nan, True), (5, nan, False), (14, inf, True), (5, inf, False), (14, -inf, False), (5, -inf, False)):
        row = base.copy()
        row[at] = value
        rows.append(row)
        want.append(bad)
    none = base.copy()
    none[[0, 1] + list(range(10, 18))] = -inf
    rows.append(none)
    want.append(True)
    bad_rows = np.stack(rows)
    good = np.tile(base, (len(rows), 1))
    legal = np.array([word] * len(rows), np.uint64)
    for d in (CR.divergences(bad_rows, good, legal), CR.divergences(good, bad_rows, legal)):
        assert d["nonfinite"].tolist() == want
        for name in ("kl_xy", "kl_yx", "js"):
            assert np.isnan(d[name]).tolist() == want, name
        assert ((CR.flags(d, np.zeros(len(rows), int)) & CR.NONFINITE) != 0).tolist() == want
    d = CR.divergences(bad_rows, good, legal)
    assert d["call_x"][0] == 17 and d["call_x"][2] == 14 and d["call_x"][6] == 0      # NaN is never the maximum; +inf is; none: action 0
    assert np.isinf(d["kl_yx"][4]) and np.isfinite(d["kl_xy"][4]) and np.isfinite(d["js"][4])     # Y has mass where X has none


# ---- a PolicyDiff from the restatement ----------------------------------------------------------------------------------------------
def reference_diff(recs, depth, seed=0, same=False, nan_at=()):
    """a PolicyDiff of the record arrays ``recs`` (one per table) under random logits, by the restatement alone; -> (diff, dense)"""
    rng = np.random.default_rng(seed)
    n = len(recs[0])
    dense = np.zeros((len(recs), n, depth), compare.DECISION_DTYPE)
    for k, rec in enumerate(recs):
        for t in range(depth):
            rows = np.arange(n)
            legal = np.zeros(n, np.uint64)
            for i in rows:
                calls = [int(c) for c in rec["calls"][i][:min(int(rec["n_calls"][i]), t + 1)]]
                if len(calls) > t:
                    legal[i] = BR.legal_words(int(rec["dealer"][i]), calls)[t][1]
            lx = (rng.normal(size=(n, 38)) * 3).astype(np.float32)
            ly = lx if same else (lx + rng.normal(size=(n, 38)) * rng.choice([0.0, 0.5, 4.0], size=(n, 1))).astype(np.float32)
            for i in nan_at:
                lx = lx.copy()
                lx[i, 0] = np.nan
            out, d = CR.expected_records(rec, depth, t, rows, lx, ly, np.where(legal == 0, 1, legal).astype(np.uint64), compare.DECISION_DTYPE)
            out["logp_x"] = np.where(d["live"], d["Lx"][rows, d["played"]], 0).astype(np.float32)
            out["logp_y"] = np.where(d["live"], d["Ly"][rows, d["played"]], 0).astype(np.float32)
            dense[k, :, t] = out
    perm, starts = CR.sort_runs(dense)
    entries, confusion = CR.reduce(dense.reshape(-1)[perm], starts, compare.ENTRY_DTYPE)
    skipped = {tb: int((~CR.reviewable(rec)).sum()) for tb, rec in zip("ab", recs)}
    return compare.PolicyDiff(dense, entries, confusion, skipped, depth, "ab"[:len(recs)]), dense


def _match(n=200, seed=3, skip=()):
    rng = np.random.default_rng(seed)
    auctions = [R.random_auction(rng, p_pass=0.5) for _ in range(n)]
    ok = [i not in skip for i in range(n)]
    return B.make_records(auctions, rng, ok=ok), B.make_records(auctions[::-1], rng)


def test_lookups_read_the_arrays():
    rec_a, rec_b = _match(skip=(4,))
    pd, dense = reference_diff([rec_a, rec_b], 4, nan_at=(7,))
    assert pd.skipped == {"a": 1, "b": 0} and pd.decisions.shape == (2, 200, 4) and (pd.decisions["key"][0, 4] == 0).all()
    assert len(pd) == sum(min(int(r["n_calls"]), 4) for rec in (rec_a, rec_b) for r in rec[CR.reviewable(rec)])
    assert int(pd.entries["n"].sum()) == len(pd) and int(pd.entries["nonfinite"].sum()) == int(((dense["flags"] & CR.NONFINITE) != 0).sum()) > 0
    assert pd.confusion.sum() == len(pd) - int(pd.entries["nonfinite"].sum())
    assert pd.of(4, "a", 0) is None
    d = pd.of(0, "b", 1)
    r = rec_b[0]
    assert d["prefix"] == CALL_NAMES[int(r["calls"][0])] and d["played"] == CALL_NAMES[int(r["calls"][1])] and d["call_index"] == 1
    assert d["played"] in d["legal"] and d["call_x"] in d["legal"] and d["agree"] == (d["call_x"] == d["call_y"])
    seat = (int(r["dealer"]) + 1) & 3
    assert d["hcp"] == int(BR.features(np.uint64(int(r["hands"][seat])))[1]) and d["team"] == (((int(r["seating"]) >> (2 * seat)) & 3) >> 1) + 1
    opening = pd.entry("")
    first = dense[:, :, 0].reshape(-1)
    first = first[(first["key"] != 0)]
    fin = first[(first["flags"] & CR.NONFINITE) == 0]
    assert opening["n"] == len(first) and opening["nonfinite"] == len(first) - len(fin) and opening["call_index"] == 0
    assert opening["agreement"] == pytest.approx(((fin["flags"] & CR.AGREE) != 0).mean()) and opening["js_mean"] == pytest.approx(fin["js"].mean())
    assert opening["js_max"] == fin["js"].max() and opening["hcp_mean"] == pytest.approx((fin["feats"] & 63).mean())
    assert opening["logp_x_mean"] == pytest.approx(fin["logp_x"].astype(np.float64).mean())
    assert pd.entry(compare.key_of("")) == opening and pd.entry([]) == opening
    with pytest.raises(KeyError):
        pd.entry("7NT 7NT")
    with pytest.raises(ValueError):
        pd.of(0, "c")
    with pytest.raises(ValueError):
        pd.of(0, "a", 4)
    t = pd.totals()
    assert t["decisions"] == len(pd) and [b["n"] for b in t["by_call_index"]] == [int(((dense[:, :, k]["key"] != 0) & ((dense[:, :, k]["flags"] & CR.NONFINITE) == 0)).sum()) for k in range(4)]


def test_worst_ranks_by_the_js_sum():
    pd, _ = reference_diff(list(_match()), 4)
    rows = pd.worst(5, min_count=3)
    e = pd.entries
    finite = e["n"].astype(np.int64) - e["nonfinite"]
    want = sorted((i for i in range(len(e)) if finite[i] >= 3), key=lambda i: (-e["js_sum"][i], e["key"][i]))[:5]
    assert [r["key"] for r in rows] == [int(e["key"][i]) for i in want] and len(rows) == 5
    assert all(r["js_total"] == pytest.approx(r["n"] * r["js_mean"]) for r in rows)
    assert pd.worst(3, min_count=10 ** 6) == [] and len(pd.worst(10 ** 6)) == len(e)
    same, _ = reference_diff(list(_match()), 2, same=True)
    assert (same.entries["js_sum"] == 0).all() and (same.entries["agree"] == same.entries["n"]).all()
    assert np.array_equal(same.confusion, np.diag(np.diag(same.confusion)))
    assert "agree on 100.0%" in same.stats_lines()[0] and same.stats_lines()[3] == "diff confusion: none"


def test_text_and_json_round_trip(tmp_path):
    pd, _ = reference_diff(list(_match(n=60, skip=(2,))), 3, nan_at=(1,))
    lines = pd.stats_lines()
    assert lines[0].startswith(f"diff: {pd.totals()['finite']} decisions (depth 3, {len(pd.entries)} prefixes, ") and "1 records skipped" in lines[0]
    assert lines[1].startswith("diff by call index: 0: agree ") and lines[2].startswith("diff played: X calls what was played on ")
    assert lines[3].startswith("diff confusion: X ") and lines[4].startswith("diff largest: after ")
    text = pd.to_text(min_count=2)
    body = text.splitlines()[len(lines):]
    assert text.splitlines()[:4] == lines[:4] and len(body) == len(pd.worst(10 ** 6, min_count=2)) > 0 and all(" JS " in ln for ln in body)
    path = tmp_path / "diff.json"
    pd.to_json(str(path))
    back = compare.PolicyDiff.from_json(str(path))
    assert back.same_as(pd) and pd.same_as(compare.PolicyDiff.from_json(pd.to_json()))
    fin = (pd.decisions["flags"] & CR.NONFINITE) == 0
    for name in compare.DECISION_DTYPE.names:                            # bit for bit, the float fields included, where finite
        assert back.decisions[name][fin].tobytes() == pd.decisions[name][fin].tobytes(), name
    assert back.entries.tobytes() == pd.entries.tobytes() and back.to_text() == pd.to_text()
    assert np.isnan(back.decisions["js"][~fin & (pd.decisions["key"] != 0)]).all()
    other, _ = reference_diff(list(_match(n=60, skip=(2,))), 3, seed=9)
    assert not other.same_as(pd)
    with pytest.raises(ValueError):
        compare.PolicyDiff.from_json({"format": "brl_amd.book/1"})


def test_bad_arguments_are_refused_before_anything_is_launched():
    env = types.SimpleNamespace(device="cpu", _h=None)
    for depth in (0, 11, -1):
        with pytest.raises(ValueError, match="depth"):
            compare.make_policy_diff(env, "relu", "DeepMind", "relu", "DeepMind", depth=depth)
    with pytest.raises(ValueError, match="max_rows"):
        compare.make_policy_diff(env, "relu", "DeepMind", "relu", "DeepMind", max_rows=0)
    policy_diff = compare.make_policy_diff(env, "relu", "DeepMind", "relu", "DeepMind", depth=4)
    rec = np.zeros(3, RECORD_DTYPE)
    with pytest.raises(ValueError, match="tables"):
        policy_diff(None, None, rec, tables="c")
    with pytest.raises(ValueError, match="table 'a'"):
        policy_diff(None, None, rec, tables="ab")                        # one array is one table
    with pytest.raises(ValueError, match="records"):
        policy_diff(None, None, np.zeros((3, 368), np.int32), tables="a")
    with pytest.raises(ValueError, match="records"):
        policy_diff(None, None, np.zeros((3, 367), np.uint8), tables="a")
    import torch
    with pytest.raises(ValueError, match="records"):
        policy_diff(None, None, torch.zeros((3, 368), dtype=torch.int8), tables="a")
    from brl_amd.boards import BoardRecords
    with pytest.raises(ValueError, match="table B"):
        policy_diff(None, None, BoardRecords(rec), tables="ab")


def test_eval_defaults_gained_the_diff_arguments():
    from brl_amd.eval import EVAL_DEFAULTS
    from brl_amd.league import parse
    assert (EVAL_DEFAULTS["diff"], EVAL_DEFAULTS["diff_depth"], EVAL_DEFAULTS["diff_min_count"], EVAL_DEFAULTS["save_diff"]) == (0, 4, 20, None)
    cfg = parse(["diff=1", "diff_depth=6", "diff_min_count=5", "save_diff=d.json"], EVAL_DEFAULTS)
    assert (cfg["diff"], cfg["diff_depth"], cfg["diff_min_count"], cfg["save_diff"]) == (1, 6, 5, "d.json")
