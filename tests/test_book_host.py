"""The host side of the bidding-system book (brl_amd/book.py) without a GPU: keys and names, key order, and a SystemBook built
from the restatement's counters (tests/book_ref.py) — entry, continuations, the text tree and the JSON round trip."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import board_records_ref as R  # noqa: E402
import book_ref as B  # noqa: E402

from brl_amd import book  # noqa: E402
from brl_amd.boards import CALL_NAMES  # noqa: E402


def test_the_header_states_the_layout_the_host_reads():
    text = open(os.path.join(ROOT, "include", "brl_book.h")).read()
    assert f"#define BRL_BOOK_ENTRY_BYTES {book.ENTRY_DTYPE.itemsize}" in text and book.ENTRY_DTYPE.itemsize % 16 == 0
    assert f"#define BRL_BOOK_MAX_DEPTH {book.MAX_DEPTH}" in text
    assert book.ENTRY_DTYPE.fields["team"][1] == 16 and book.TEAM_DTYPE.fields["imp_sum"][1] == 384


@pytest.mark.parametrize("length", range(1, 11))
def test_key_and_name_round_trip(length):
    rng = np.random.default_rng(length)
    for calls in ([0] * length, [37] * length, [0, 37] * 5, [37, 0] * 5, list(rng.integers(0, 38, size=10))):
        calls = [int(c) for c in calls[:length]]
        names = " ".join(CALL_NAMES[c] for c in calls)
        k = book.key_of(names)
        assert k == B.key(calls) == book.key_of(calls) == book.key_of(names.split()) and 0 < k < 1 << 64
        assert book.name_of(k) == names and book.calls_of(k) == calls
        assert int(book.key_depth(np.array([k], np.uint64))[0]) == length
    assert book.key_of("P") == 1 << 58 and book.key_of("7NT") == 38 << 58 and book.key_of("") == 0 and book.name_of(0) == ""


def test_bad_prefixes_and_keys_are_refused():
    with pytest.raises(ValueError):
        book.key_of("1NT 8C")
    with pytest.raises(ValueError):
        book.key_of(["P"] * 11)
    with pytest.raises(ValueError):
        book.name_of(39 << 58)                       # a field past 7NT
    with pytest.raises(ValueError):
        book.name_of((1 << 58) | (1 << 46))          # a call behind the end of the prefix


def test_key_order_is_the_depth_first_order_of_the_prefix_tree():
    rng = np.random.default_rng(7)
    prefixes = set()
    for _ in range(300):
        calls = tuple(int(c) for c in rng.integers(0, 38, size=int(rng.integers(1, 11))))
        prefixes.update(calls[:k] for k in range(1, len(calls) + 1))      # with every prefix of its own
    prefixes = list(prefixes)
    by_key = sorted(prefixes, key=lambda p: book.key_of(p))
    assert by_key == sorted(prefixes, key=B.order)
    keys = np.array([book.key_of(p) for p in by_key], np.uint64)           # and as uint64 in numpy, the top bit included
    assert (keys[1:] > keys[:-1]).all() and (keys >> np.uint64(63)).any()
    for a, b in zip(by_key, by_key[1:]):                                    # a prefix comes before its extensions
        assert not (len(b) < len(a) and a[:len(b)] == b)


def _book(n=300, depth=4, seed=3, with_imp=True):
    rng = np.random.default_rng(seed)
    auctions = [R.random_auction(rng, p_pass=0.5) for _ in range(n)]
    rec_a, rec_b = B.make_records(auctions, rng), B.make_records(auctions[::-1], rng)
    imp = rng.integers(-24, 25, size=n) if with_imp else None
    ref, skipped = B.book_of(rec_a, rec_b, depth, imp)
    return book.SystemBook(*B.arrays(ref), depth=depth, skipped=skipped, has_imp=with_imp), ref


def test_entry_reads_the_counters():
    sb, ref = _book()
    assert len(sb) == len(ref) and sb.depth == 4 and sb.skipped == 0
    for prefix in list(ref)[:50]:
        names = " ".join(CALL_NAMES[c] for c in prefix)
        for team in (None, 1, 2):
            ts = [t for t in (0, 1) if team in (None, t + 1)]
            e = sb.entry(names, team)
            n = sum(ref[prefix][t]["count"] for t in ts)
            assert e["count"] == n and e["prefix"] == names
            if n == 0:
                continue
            hcp = [sum(ref[prefix][t]["hcp"][v] for t in ts) for v in range(38)]
            values = sorted(v for v in range(38) for _ in range(hcp[v]))          # every sample's HCP, written out
            assert e["hcp_mean"] == pytest.approx(sum(values) / n) and (e["hcp_min"], e["hcp_max"]) == (values[0], values[-1])
            assert e["hcp_p5"] == values[max(1, math.ceil(0.05 * n)) - 1] and e["hcp_p95"] == values[max(1, math.ceil(0.95 * n)) - 1]
            for s, suit in enumerate("CDHS"):
                ln = [sum(ref[prefix][t]["length"][s][v] for t in ts) for v in range(14)]
                assert e["length_mean"][suit] == pytest.approx(sum(v * c for v, c in enumerate(ln)) / n)
                assert e["length_mode"][suit] == ln.index(max(ln))
            assert e["balanced"] == pytest.approx(sum(ref[prefix][t]["balanced"] for t in ts) / n)
            assert e["imp_mean"] == pytest.approx(sum(ref[prefix][t]["imp_sum"] for t in ts) / n)
    with pytest.raises(KeyError):
        sb.entry("7NT 7NT")
    with pytest.raises(ValueError):
        sb.entry("P", team=3)


def test_percentiles_and_the_standard_error_on_hand_computed_cases():
    """20 samples with HCP 10 x 1, 12 x 17, 15 x 1, 21 x 1: the 5th percentile is the 1st of 20 (10), the 95th the 19th (15);
    IMPs +3 x 10 and -1 x 10: mean 1, sample variance 80 / 19, standard error sqrt(80 / 19 / 20)"""
    hcp = np.zeros((1, 2, 38), np.int64)
    hcp[0, 0, [10, 12, 15, 21]] = [1, 7, 1, 1]
    hcp[0, 1, 12] = 10
    length = np.zeros((1, 2, 4, 14), np.int64)
    length[0, 0, :, 3], length[0, 1, :, 3] = 10, 10
    length[0, 0, 3, 3], length[0, 0, 3, 4] = 4, 6
    sb = book.SystemBook([book.key_of("1NT")], [[10, 10]], [[9, 10]], hcp, length, [[30, -10]], [[90, 10]], depth=1)
    e = sb.entry("1NT")
    assert (e["count"], e["hcp_min"], e["hcp_max"], e["hcp_p5"], e["hcp_p95"]) == (20, 10, 21, 10, 15)
    assert e["hcp_mean"] == pytest.approx(12.5) and e["balanced"] == pytest.approx(0.95)
    assert e["length_mode"] == {"C": 3, "D": 3, "H": 3, "S": 3} and e["length_mean"]["S"] == pytest.approx(3.3)
    assert e["imp_mean"] == pytest.approx(1.0) and e["imp_se"] == pytest.approx(math.sqrt(80 / 19 / 20))
    one = sb.entry("1NT", team=2)
    assert (one["count"], one["hcp_p5"], one["hcp_p95"], one["imp_mean"], one["imp_se"]) == (10, 12, 12, -1.0, 0.0)
    assert sb.entry("1NT", team=1)["hcp_p95"] == 21 and sb.entry("1NT", team=1)["length_mode"]["S"] == 4
    assert "1NT  n=20  HCP 12.5 (10–15)  S3.3 H3.0 D3.0 C3.0  bal 0.95  IMP +1.00±0.46\n" == sb.to_text()


def test_continuations_share_out_the_next_calls():
    sb, ref = _book()
    for prefix in [()] + [p for p in ref if len(p) < 4][:40]:
        names = " ".join(CALL_NAMES[c] for c in prefix)
        for team in (None, 1, 2):
            ts = [t for t in (0, 1) if team in (None, t + 1)]
            want = {CALL_NAMES[p[-1]]: sum(ref[p][t]["count"] for t in ts) for p in ref if len(p) == len(prefix) + 1 and p[:-1] == prefix}
            want = {c: k for c, k in want.items() if k}
            got = sb.continuations(names, team)
            assert {g["call"]: g["count"] for g in got} == want
            if got:
                assert sum(g["share"] for g in got) == pytest.approx(1.0)
                assert all(g["share"] == pytest.approx(g["count"] / sum(want.values())) for g in got)
    assert sb.continuations(" ".join(["P"] * 10)) == []


def test_json_round_trip_is_exact(tmp_path):
    for with_imp in (True, False):
        sb, _ = _book(seed=11, with_imp=with_imp)
        sb.imp_sq_sum[0, 0] = np.uint64(2 ** 64 - 3)      # the counters' full range survives
        sb.imp_sum[0, 1] = -2 ** 63 + 5
        path = tmp_path / "book.json"
        sb.to_json(str(path))
        back = book.SystemBook.from_json(str(path))
        assert back == sb and back.has_imp == with_imp
        for name in book.SystemBook._ARRAYS:
            a, b = getattr(sb, name), getattr(back, name)
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
        assert book.SystemBook.from_json(sb.to_json()) == sb
    few = book.SystemBook.from_json(sb.to_json(min_count=20))
    assert 0 < len(few) < len(sb) and (few.count.sum(1) >= 20).all()


def test_to_text_honours_min_count_and_max_depth():
    sb, ref = _book()
    depth_of = {book.key_of(p): len(p) for p in ref}
    full = sb.to_text().splitlines()
    assert len(full) == len(ref)
    for line, k in zip(full, sb.keys):
        d = depth_of[int(k)]
        assert line.startswith("  " * (d - 1) + book.name_of(int(k)).split()[-1] + "  n=") and "IMP " in line
    for min_count, max_depth in ((1, 2), (10, None), (25, 3)):
        lines = sb.to_text(min_count=min_count, max_depth=max_depth).splitlines()
        want = [p for p in sorted(ref, key=B.order)
                if ref[p][0]["count"] + ref[p][1]["count"] >= min_count and (max_depth is None or len(p) <= max_depth)]
        assert len(lines) == len(want) and len(lines) > 0
        for line, p in zip(lines, want):
            n = ref[p][0]["count"] + ref[p][1]["count"]
            assert line.startswith("  " * (len(p) - 1) + CALL_NAMES[p[-1]] + f"  n={n}  HCP ")
    assert "IMP" not in _book(with_imp=False)[0].to_text()


def test_eval_defaults_gained_the_book_arguments():
    from brl_amd.eval import EVAL_DEFAULTS
    from brl_amd.league import parse
    assert (EVAL_DEFAULTS["save_book"], EVAL_DEFAULTS["book_depth"], EVAL_DEFAULTS["book_min_count"]) == (None, 4, 20)
    cfg = parse(["save_book=b.txt", "book_depth=6", "book_min_count=5"], EVAL_DEFAULTS)
    assert (cfg["save_book"], cfg["book_depth"], cfg["book_min_count"]) == ("b.txt", 6, 5)
