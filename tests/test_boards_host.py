"""Board records without a GPU: the deal readers against the packed fixture, the JSON / PBN round trips, the rejection of bad
boards, the reconstruction argument (history words -> call sequence) against a forward encoder, and the statistics."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import board_records_ref as R  # noqa: E402

from brl_amd import board_stats, boards  # noqa: E402

NAMED = os.path.join(ROOT, "tests", "golden", "wb5_named_24.json")


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_read_deals_gives_the_packed_fixture_rows(dds):
    d = boards.read_deals(NAMED)
    assert d.n == 24
    assert np.array_equal(d.lut_keys(), dds["keys"][:24])
    assert np.array_equal(d.lut_values(), dds["values"][:24])
    assert np.array_equal(d.tricks.reshape(24, 4, 5), dds["tricks"][:24])
    assert np.array_equal(d.dealer, dds["dealer"][:24])
    assert np.array_equal(d.vul_ns, dds["vul_ns"][:24]) and np.array_equal(d.vul_ew, dds["vul_ew"][:24])
    assert np.array_equal(d.board_id, dds["board_id"][:24])
    assert (np.sort(d.hand, axis=1) == np.arange(52)).all()


def _records_of(d, rng):
    """a hand-written structured array for the deals: random finished auctions, contract fields from the restatement"""
    words = d.hand_words()
    packed = []
    for i in range(d.n):
        calls = R.random_auction(rng) if i else [0, 0, 0, 0]
        t = R.encode(int(d.dealer[i]), calls, vul_ns=int(d.vul_ns[i]), vul_ew=int(d.vul_ew[i]), tricks=d.tricks[i],
                     hands=[int(w) for w in words[i]])
        packed.append(t.pack())
    return R.decode(np.stack(packed))


@pytest.mark.parametrize("ext", ["json", "pbn"])
def test_round_trip_through_the_writers(tmp_path, ext):
    d = boards.read_deals(NAMED)
    rec = _records_of(d, np.random.default_rng(3))
    br = boards.BoardRecords(rec, rec, np.zeros(d.n, np.int32), d.tricks, d.board_id)
    path = str(tmp_path / f"out.{ext}")
    br.save(path)
    back = boards.read_deals(path)
    assert _same(back, d)
    if ext == "json":
        logs = json.load(open(path))["logs"]
        src = json.load(open(NAMED))["logs"]
        for a, b in zip(logs, src):
            assert all(a[k] == b[k] for k in ("board_id", "dealer", "deal", "vulnerability", "dda"))
        assert logs[0]["table_a"]["contract"] == "passed out" and logs[0]["table_a"]["auction"] == ["P"] * 4
        assert set(logs[1]["table_a"]) == {"auction", "contract", "declarer", "tricks", "score_ns"} and "imp" in logs[1]


def test_named_accessors():
    t = R.encode(3, [0, 3 + 18, 1, 0, 0, 0], vul_ew=1, tricks=np.full((4, 5), 9), hands=[0x1111111111111, 0x2222222222222,
                                                                                     0x4444444444444, 0x8888888888888])
    br = boards.BoardRecords(R.decode(t.pack()[None]))
    assert br.auction(0) == ["P", "4S", "X", "P", "P", "P"]
    assert br.contract(0) == "4SX by N"                     # dealer W passes, N bids 4S
    assert br.cpu()[0]["score_ns"] == -100 and br.cpu()[0]["tricks"] == 9
    assert br.hands(0) == "N:...AKQJT98765432 ..AKQJT98765432. .AKQJT98765432.. AKQJT98765432..."
    assert boards.card_bit("C6") == 16 and boards.bit_card(16) == "C6"
    assert all(boards.card_bit(boards.bit_card(b)) == b for b in range(52))


def test_a_record_without_the_self_check_bit_is_refused():
    rec = R.decode(R.encode(0, [0, 3, 0, 0, 0]).pack()[None])
    rec["flags"] &= ~np.uint8(boards.OK)
    with pytest.raises(ValueError, match="record 0 fails the self-check"):
        boards.BoardRecords(rec).auction(0)


def _bad(tmp_path, edit):
    logs = json.load(open(NAMED))["logs"][:6]
    edit(logs[4])
    path = str(tmp_path / "bad.json")
    json.dump({"logs": logs}, open(path, "w"))
    return path


@pytest.mark.parametrize("what, edit", [
    ("51 distinct cards", lambda b: b["deal"]["N"].__setitem__(0, b["deal"]["N"][1])),
    ("S holds 12 cards", lambda b: b["deal"]["S"].pop()),
    ("not a card", lambda b: b["deal"]["E"].__setitem__(3, "Z9")),
    ("unknown dealer", lambda b: b.__setitem__("dealer", "Q")),
    ("unknown vulnerability", lambda b: b.__setitem__("vulnerability", "All of them")),
    ("tricks of W in H are 14", lambda b: b["dda"]["W"].__setitem__("H", 14)),
    ("tricks of E in NT are missing", lambda b: b["dda"]["E"].pop("NT")),
])
def test_bad_boards_are_rejected_with_their_number(tmp_path, what, edit):
    with pytest.raises(boards.MalformedDeals, match=f"board 4: .*{what}"):
        boards.read_deals(_bad(tmp_path, edit))


def test_bad_pbn_board_is_rejected_with_its_number(tmp_path):
    d = boards.read_deals(NAMED)
    rec = _records_of(d, np.random.default_rng(4))
    path = str(tmp_path / "x.pbn")
    boards.BoardRecords(rec, None, None, d.tricks, d.board_id).to_pbn(path)
    text = open(path).read().split("\n")
    k = [i for i, l in enumerate(text) if l.startswith("[DoubleDummyTricks")][2]
    del text[k]
    open(path, "w").write("\n".join(text))
    with pytest.raises(boards.MalformedDeals, match="board 2: .*missing"):
        boards.read_deals(path)


def test_pbn_with_an_optimum_result_table(tmp_path):
    b = json.load(open(NAMED))["logs"][0]
    deal = "N:" + " ".join(".".join("".join(c[1] for c in b["deal"][seat] if c[0] == s) for s in "SHDC") for seat in "NESW")
    rows = [f"{seat} {st} {b['dda'][seat][st]}" for seat in "NESW" for st in ("NT", "S", "H", "D", "C")]
    text = "\n".join(['[Board "5000000"]', f'[Dealer "{b["dealer"]}"]', '[Vulnerable "EW"]', f'[Deal "{deal}"]',
                      '[OptimumResultTable "Declarer;Denomination\\2R;Result\\2R"]'] + rows + [""])
    path = str(tmp_path / "ort.pbn")
    open(path, "w").write(text)
    got, want = boards.read_deals(path), boards.read_deals(NAMED)
    assert all(np.array_equal(x, y[:1]) for x, y in zip(got, want))
    open(path, "w").write(text.replace("W C " + str(b["dda"]["W"]["C"]) + "\n", ""))
    with pytest.raises(boards.MalformedDeals, match="board 0: .*W in C are missing"):
        boards.read_deals(path)


def test_the_decoder_inverts_the_encoder_on_20000_auctions():
    rng = np.random.default_rng(20)
    auctions = [R.longest_auction(), [0, 0, 0, 0]] + [R.random_auction(rng, p_pass=float(rng.uniform(0.05, 0.6))) for _ in range(20000 - 2)]
    stops = rng.integers(0, 30, size=len(auctions))
    lens, passouts, live = [], 0, 0
    for k, calls in enumerate(auctions):
        if k % 5 == 4:                       # an unfinished table: the first `stop` calls only
            calls = calls[:min(int(stops[k]), len(calls) - 1)]
            live += 1
        t = R.encode(k & 3, calls)
        got, ok = R.calls_of(t.hist, t.dealer, t.lb1, t.lbseat, t.x | t.xx, t.npass, t.turn, t.term, t.illegal)
        assert ok and got == list(calls), (k, calls, got)
        lens.append(len(calls))
        passouts += calls == [0, 0, 0, 0]
    assert max(lens) == 319 and passouts >= 20 and live == 4000 and sum(n > 40 for n in lens) > 100


def test_illegal_endings_keep_the_calls_before_the_illegal_one():
    rng = np.random.default_rng(21)
    kinds = 0
    for k in range(4000):
        calls = R.random_auction(rng, stop=int(rng.integers(0, 14)))
        t = R.encode(k & 3, calls)
        if t.term:
            continue
        bad = [a for a in (1, 2) if not t.legal(a)]
        a = int(rng.choice(bad))
        t.step(a)
        assert t.illegal and t.term
        rec = R.decode(t.pack()[None])[0]
        assert rec["flags"] == boards.TERMINATED | boards.ILLEGAL | boards.OK
        assert list(rec["calls"][:rec["n_calls"]]) == calls and rec["n_calls"] == t.turn - 1
        assert rec["level"] == 0 and rec["score_ns"] == 0
        kinds += 1
    assert kinds > 2000
    # an illegal bid overwrites the last bid: no record
    t = R.encode(0, [3 + 10, 0])
    t.step(3 + 4)
    rec = R.decode(t.pack()[None])[0]
    assert rec["flags"] == boards.TERMINATED | boards.ILLEGAL and rec["n_calls"] == 0


def _board(calls, dealer, hands, tricks, **kw):
    words = [sum(1 << boards.card_bit(c) for c in h) for h in hands]
    return R.encode(dealer, calls, tricks=tricks, hands=words, **kw).pack()


def test_board_stats_on_hand_built_boards():
    suits = {s: [s + r for r in boards.RANKS] for s in "CDHS"}
    n_hand, e_hand, s_hand, w_hand = suits["S"], suits["H"], suits["D"], suits["C"]     # 10 HCP each; N/S hold S and D
    hands = [n_hand, e_hand, s_hand, w_hand]
    t = np.zeros((4, 5), np.int64)
    t[0] = t[2] = [0, 13, 0, 13, 6]
    t[1] = t[3] = [13, 0, 13, 0, 6]
    bid = lambda lv, st: 3 + 5 * (lv - 1) + boards.STRAINS.index(st)   # noqa: E731
    rows = [
        _board([0, 0, 0, 0], 0, hands, t),                          # passed out
        _board([0, 0, 0, 0], 1, hands, t),                          # passed out
        _board([bid(4, "S"), 0, 0, 0], 0, hands, t),                # 4S by N: made, longest suit (tie S / D)
        _board([bid(2, "D"), 0, 0, 0], 2, hands, t),                # 2D by S: made, agrees
        _board([bid(1, "C"), 0, 0, 0], 0, hands, t),                # 1C by N: down, disagrees
        _board([bid(3, "NT"), 1, 0, 0, 0], 0, hands, t),            # 3NTX by N: down, no-trump
        _board([0, bid(7, "H"), 1, 2, 0, 0, 0], 0, hands, t),       # 7HXX by E: made, agrees
        _board([bid(1, "S"), bid(2, "S"), 0, 0, 0], 0, hands, t),   # 2S by E: down, disagrees
        _board([bid(6, "D"), 0, 0, 0], 0, hands, t),                # 6D by N: made, agrees
        _board([bid(1, "H"), 0, 0, 0], 1, hands, t),                # 1H by E: made, agrees
        _board([bid(5, "C"), 0, 0, 0], 3, hands, t),                # 5C by W: made, agrees
        _board([bid(2, "NT"), 0, 0, 0], 0, hands, t),               # 2NT by N: down
    ]
    rec = R.decode(np.stack(rows))
    imp = np.array([0, 0, 3, -3, 5, -5, 1, -1, 2, -2, 0, 0])
    s = board_stats.board_stats(boards.BoardRecords(rec).cpu(), imp)
    levels = np.array([4, 2, 1, 3, 7, 2, 6, 1, 5, 2], float)
    assert s["boards"] == 12 and s["contracts"] == 10
    assert s["pass_out_ratio"] == pytest.approx(2 / 12)
    assert s["made_ratio"] == pytest.approx(6 / 10)
    assert s["mean_level"] == pytest.approx(levels.mean())
    assert s["doubled_ratio"] == pytest.approx(2 / 10)
    assert s["strain_agreement"] == pytest.approx(6 / 8)
    assert np.isnan(s["level_hcp_corr"])                           # every side holds 20 points: no variance
    assert s["imp_mean"] == 0.0 and s["imp_se"] == pytest.approx(imp.std(ddof=1) / np.sqrt(12))
    assert board_stats.side_counts(rec[2]["hands"], 0) == (20, {"C": 0, "D": 13, "H": 0, "S": 13})
    # level against points: N/S hold 30 points, E/W the clubs' 10
    strong = [suits["S"], suits["C"][5:] + suits["D"][:5], suits["D"][9:] + suits["H"][9:] + suits["C"][:5], suits["D"][5:9] + suits["H"][:9]]
    rows2 = [_board([bid(6, "S"), 0, 0, 0], 0, strong, t), _board([0, bid(1, "C"), 0, 0, 0], 0, strong, t),
             _board([bid(4, "S"), 0, 0, 0], 0, strong, t), _board([0, bid(2, "C"), 0, 0, 0], 0, strong, t)]
    s2 = board_stats.board_stats(R.decode(np.stack(rows2)))
    assert s2["level_hcp_corr"] == pytest.approx(np.corrcoef([6, 1, 4, 2], [30, 10, 30, 10])[0, 1])
