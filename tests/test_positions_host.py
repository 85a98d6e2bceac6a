"""The position queries on the CPU (brl_amd/positions.py, brl_amd/bid.py, tests/positions_ref.py): parsing and packing, the host's
ValueError against the restatement's status, the restatement's rows against the C oracle's observation of the stepped table,
quiz_score, the Answers document, the command line's argument errors.  The kernels are tests/test_gpu_positions.py's."""
import json
import os

import numpy as np
import pytest

from brl_amd import boards, positions as M
from tests import guarded
from tests import positions_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The memory-contract ledger (tests/guarded.py; tests/test_guarded_host.py holds every `int brl_*(` of include/*.h against it): the two
# entry points of include/brl_positions.h run under the guards in tests/test_gpu_positions.py.  Their entries are made here, when
# the suite is collected, because they arrive with these tests; DESIGN.md's "Memory contract" table lists them too.
guarded.COVERED.update({
    "brl_position_rows": "n in {1, 3, 65, 130}, good positions and every kind of bad one; positions / tables at 16, obs / legal at 8, status at 4, "
                         "mask at 1; tables given and NULL (tests/test_gpu_positions.py)",
    "brl_position_answers": "the same n, on those legal words and statuses; logits at 4 with a row pitch of 40 (NaN padding), value at 4 at stride 2, "
                            "legal / probs at 8, answers at 16; probs given and NULL (tests/test_gpu_positions.py)",
})

QUIZ = os.path.join(ROOT, "tests", "golden", "bidding_quiz_12.json")
HAND = "AKQ.J32.T9.87654"


# ---- the header and the binding --------------------------------------------------------------------------------------------------------
def test_the_header_states_what_the_binding_and_the_host_read():
    import re

    from brl_amd import _capi
    text = open(os.path.join(ROOT, "include", "brl_positions.h")).read()
    for macro, v in (("MAX_CALLS", M.MAX_CALLS), ("FILL", M.FILL), ("ACTIONS", M.ACTIONS), ("MAX_TOP", M.MAX_TOP), ("OK", M.POS_OK),
                     ("BAD_HEADER", M.BAD_HEADER), ("BAD_HAND", M.BAD_HAND), ("ILLEGAL_CALL", M.ILLEGAL_CALL), ("FINISHED", M.FINISHED),
                     ("NONFINITE", M.NONFINITE)):
        assert re.search(rf"#define BRL_POS_{macro} {v}\b", text), macro
    assert (P.OK, P.BAD_HEADER, P.BAD_HAND, P.ILLEGAL_CALL, P.FINISHED, P.NONFINITE) == (0, 1, 2, 3, 4, 1) and P.DTYPE == M.POSITION_DTYPE
    for dt, struct in ((M.POSITION_DTYPE, "brl_position"), (M.ANSWER_DTYPE, "brl_position_answer")):
        body = re.search(r"typedef struct " + struct + r" \{(.*?)\} " + struct, text, re.S).group(1)
        fields = [n for decl in re.findall(r"^\s*\w+ ([^;]+);", body, re.M) for n in re.findall(r"(\w+)(?:\[\w+\])?", decl) if not n.isupper()]
        assert fields == list(dt.names), (struct, fields)
    # the library refuses a misaligned pointer on the host: nothing is launched (the prototypes against the argtypes it binds:
    # tests/test_capi_cpu.py, every header)
    if os.path.exists(_capi.LIB_PATH):
        L = _capi.lib()
        big = 0x7F1234567000      # (never dereferenced: the checks come first)
        assert L.brl_position_rows(0, big + 8, 4, big, big, big, big, None, None) == -1 and b"aligned" in L.brl_last_error()
        assert L.brl_position_answers(0, big, 38, big, 1, big, big, 4, 3, big + 8, big, None) == -1 and b"aligned" in L.brl_last_error()
        assert L.brl_position_answers(0, big, 38, big, 1, big, big, 4, 9, big, big, None) == -1 and b"top_k" in L.brl_last_error()


# ---- parsing and packing -------------------------------------------------------------------------------------------------------------
def test_every_call_name_and_alias():
    for a, name in enumerate(boards.CALL_NAMES):
        assert M.call_id(name) == M.call_id(name.lower()) == M.call_id(a) == a
    assert [M.call_id(x) for x in ("Pass", "P", "pass", "X", "Dbl", "dbl", "XX", "Rdbl", "RDBL")] == [0, 0, 0, 1, 1, 1, 2, 2, 2]
    for lv in range(1, 8):
        assert M.call_id(f"{lv}N") == M.call_id(f"{lv}NT") == 3 + 5 * (lv - 1) + 4 and M.call_id(f"{lv}C") == 3 + 5 * (lv - 1)
    for bad in ("8C", "0NT", "1", "NT", "XXX", "", 38, -1):
        with pytest.raises(ValueError):
            M.call_id(bad)


def test_position_parses_every_form_and_round_trips():
    a = M.Position(HAND, "N", "None", "1C P 1H X")
    b = M.Position(M.hand_word(HAND), 0, (0, 0), [3, "Pass", "1h", "Dbl"])
    assert a == b and a.calls == [3, 0, 5, 1] and a.seat == 0 and a.dealer == 0 and (a.vul_ns, a.vul_ew) == (0, 0)
    assert a.label() == {"hand": HAND, "dealer": "N", "vul": "None", "auction": "1C P 1H X"} and M.Position.from_label(a.label()) == a
    assert M.Position(HAND, "W", "Both", "").seat == 3 and M.Position(HAND, "E", "EW", "P P").seat == 3
    assert M.Position(HAND, 2, "NS", "1N").calls == [7] and (M.Position(HAND, 2, "ns", []).vul_ns, M.Position(HAND, 2, "EW", []).vul_ew) == (1, 1)
    assert bin(a.hand).count("1") == 13 and a.hand == sum(1 << boards.card_bit(s + r) for s, rs in zip("SHDC", HAND.split(".")) for r in rs)
    # the legal word of the seat to call: after 1C P 1H X — pass, redouble, the bids above 1H
    assert a.legal == 1 | 4 | sum(1 << x for x in range(6, 38))
    for bad in (dict(hand="AKQ.J32.T9.8765"), dict(hand="AKQ.J32.T9.876543"), dict(hand="AKQ.J32.T9"), dict(dealer="Q"), dict(dealer=4),
                dict(vul="All"), dict(calls="1C 1Z")):
        kw = dict(dict(hand=HAND, dealer="N", vul="None", calls=""), **bad)
        with pytest.raises(ValueError):
            M.Position(**kw)


def test_packing_is_the_headers_record():
    ps = [M.Position(HAND, "S", "EW", "1C X"), M.Position("7.KQ9843.AJ5.Q62", "E", "NS", P.LONG)]
    arr = M.positions_array(ps)
    assert arr.dtype == M.POSITION_DTYPE == P.DTYPE and arr.dtype.itemsize == 64 and arr.tobytes()[16:19] == bytes([3, 1, 255])
    raw = arr.view(np.uint8).reshape(2, 64)
    assert raw[0, 8:16].tolist() == [2, 0, 1, 2, 0, 0, 0, 0] and int.from_bytes(raw[0, :8].tobytes(), "little") == ps[0].hand
    assert (raw[0, 18:] == 255).all() and raw[1, 11] == 48 and raw[1, 16:].tolist() == P.LONG
    assert M.positions_array(arr) is not None and M.positions_array(raw).tobytes() == arr.tobytes() and M.positions_array(ps[0]).tobytes() == arr[:1].tobytes()
    with pytest.raises(ValueError):
        M.positions_array(np.zeros((2, 63), np.uint8))
    with pytest.raises(ValueError, match="more than 48"):
        M.Position(HAND, "N", "None", P.LONG + [0])
    st, _, _, legal = P.rows(arr)
    assert (st == 0).all() and [int(w) for w in legal] == [p.legal for p in ps]


def test_the_hosts_errors_are_the_restatements_status():
    """every scripted auction is accepted by both, with the same legal word; every bad one is refused by both at the same call"""
    rng = np.random.default_rng(2)
    for name, calls in P.SCRIPTED.items():
        p = M.Position(P.random_hand(rng), 1, "NS", calls)
        st, _, _, word = P.row_of(M.positions_array([p])[0])
        assert st == P.OK and word == p.legal, name
    for name, (calls, status) in P.BAD.items():
        code, index = status & 0xFF, status >> 8
        assert P.row_of(P.pack(P.random_hand(rng), 3, 0, 1, calls))[0] == status, name
        with pytest.raises(ValueError) as e:
            M.Position(P.random_hand(rng), 3, "EW", calls)
        if code == P.ILLEGAL_CALL:
            assert f"call {index} " in str(e.value) and "not legal" in str(e.value), name
        else:
            assert f"call {index} e" in str(e.value), name      # "call 3 ended it" / "call 3 ends the auction"
    for cards, what in ((12, "thirteen"), (14, "thirteen")):
        hand = P.random_hand(rng, cards)
        assert P.row_of(P.pack(hand, 0, 0, 0, []))[0] == P.BAD_HAND
        with pytest.raises(ValueError, match=what):
            M.Position(hand, 0, "None", [])
    assert P.row_of(P.pack(P.random_hand(rng) | (1 << 52), 0, 0, 0, []))[0] in (P.BAD_HAND,)
    for kw in (dict(dealer=4), dict(vul_ns=2), dict(vul_ew=2), dict(reserved=1), dict(fill=0), dict(n_calls=49), dict(calls=[38])):
        args = dict(dict(hand=P.random_hand(rng), dealer=0, vul_ns=0, vul_ew=0, calls=[]), **kw)
        assert P.row_of(P.pack(**args))[0] == P.BAD_HEADER, kw
    # the order of the checks: a bad header before a bad hand before the auction
    assert P.row_of(P.pack(0, 4, 0, 0, [1]))[0] == P.BAD_HEADER and P.row_of(P.pack(0, 0, 0, 0, [1]))[0] == P.BAD_HAND


# ---- the restatement's rows against the oracle -----------------------------------------------------------------------------------------
def _pgx_hands(words):
    hand = np.zeros(52, np.int32)
    for s, w in enumerate(words):
        hand[13 * s:13 * s + 13] = np.sort(boards._bit_to_pgx(np.array([c for c in range(52) if (w >> c) & 1])))
    return hand


def test_the_restatements_rows_are_the_oracles_observation(oracle):
    """every scripted position: the table of the header (the caller's hand, the fill) built in the C oracle and stepped with the
    calls; the oracle's observation and legal mask of the player to act are the restatement's row.  And with another fill."""
    names, rec = P.scripted_records()
    st, obs, mask, legal = P.rows(rec)
    assert (st == P.OK).all() and len({int(r["n_calls"]) for r in rec}) >= 6
    rng = np.random.default_rng(3)
    for fill in ("ascending", "shuffled"):
        hands = []
        for r in rec:
            seat = (int(r["dealer"]) + int(r["n_calls"])) & 3
            words = P.fill_hands(int(r["hand"]), seat)
            if fill == "shuffled":
                rest = rng.permutation([c for c in range(52) if not (int(r["hand"]) >> c) & 1])
                for k in range(3):
                    words[(seat + 1 + k) % 4] = sum(1 << int(c) for c in rest[13 * k:13 * k + 13])
            assert sum(words) == (1 << 52) - 1 and words[seat] == int(r["hand"])
            hands.append(_pgx_hands(words))
        o = oracle.init_explicit(np.stack(hands), rec["dealer"].astype(np.int32), rec["vul_ns"], rec["vul_ew"], [0, 1, 2, 3], np.zeros(20, np.uint8))
        for t in range(48):
            live = np.nonzero(rec["n_calls"] > t)[0]
            if len(live) == 0:
                break
            sub = o[live]
            assert not sub["terminated"].any()
            oracle.step(sub, rec["calls"][live, t].astype(np.int32))
            o[live] = sub
        assert not o["terminated"].any()
        seat = (rec["dealer"].astype(np.int64) + rec["n_calls"]) & 3
        assert np.array_equal(o["current_player"], seat)      # seating is the identity
        got = oracle.observe(o, o["current_player"])
        for i, name in enumerate(names):
            assert np.array_equal(got[i], obs[i]), (fill, name, np.nonzero(got[i] != obs[i])[0])
            assert np.array_equal(o["legal_action_mask"][i].astype(np.uint8), mask[i]), (fill, name)
    assert mask[names.index("7NT")].tolist() == [1, 1] + [0] * 36 and mask[names.index("7NT X XX")].sum() == 1
    assert mask[names.index("48 calls")].sum() == 1 + 1 + 35 - 16      # pass, double (the last bid is the opponents'), 19 bids
    assert mask[names.index("1C X P P")][:3].tolist() == [1, 0, 1]


def test_positions_from_records_takes_every_decision_and_skips_what_compare_skips():
    from tests import book_ref as B
    rng = np.random.default_rng(4)
    auctions = [[3, 0, 0, 0], [0, 0, 0, 0], [7, 1, 2, 0, 0, 0], P.LONG + [0, 0, 0] + [0], [4, 0, 9, 0, 0, 0], [5, 0, 0, 0]]
    auctions[3] = P.LONG + [0]                       # 49 calls, finished: the decisions 0..48 fit a position
    rec = B.make_records(auctions, rng)
    rec["flags"][4] = int(rec["flags"][4]) & (0xFF ^ boards.OK)
    rec["flags"][5] = int(rec["flags"][5]) | boards.ILLEGAL
    arr, index = M.positions_from_records(rec)
    want = [(i, t) for i in range(4) for t in range(len(auctions[i]))]
    assert [tuple(x) for x in index.tolist()] == want and len(arr) == 4 + 4 + 6 + 49
    st, _, _, _ = P.rows(arr)
    assert (st == P.OK).all()
    for j, (i, t) in enumerate(want):
        seat = (int(rec["dealer"][i]) + t) & 3
        assert int(arr["hand"][j]) == int(rec["hands"][i][seat]) and arr["calls"][j][:t].tolist() == auctions[i][:t] and int(arr["n_calls"][j]) == t
        assert (arr["dealer"][j], arr["vul_ns"][j], arr["vul_ew"][j]) == (rec["dealer"][i], rec["vul_ns"][i], rec["vul_ew"][i])
    short, idx = M.positions_from_records(rec, depth=2)
    assert [tuple(x) for x in idx.tolist()] == [(i, t) for i in range(4) for t in range(2)] and short.tobytes() == arr[[want.index(tuple(x)) for x in idx.tolist()]].tobytes()
    both = M.positions_from_records(boards.BoardRecords(rec[:2], rec[2:4]), "b", depth=1)      # (a BoardRecords refuses a record without OK)
    assert both[0].tobytes() == M.positions_from_records(rec[2:4], depth=1)[0].tobytes() and both[1].tolist() == [[0, 0], [1, 0]]


# ---- answers, quiz ---------------------------------------------------------------------------------------------------------------------
def _answers(n=3, top_k=3, seed=7):
    """an Answers made by the restatement from random logits on the quiz's first positions"""
    with open(QUIZ) as f:
        quiz = json.load(f)
    ps = [M.Position.from_label(d) for d in quiz[:n]]
    arr = M.positions_array(ps)
    st, _, _, legal = P.rows(arr)
    lg = np.random.default_rng(seed).normal(size=(n, 38)).astype(np.float32) * 3
    a = P.answer(lg, legal, top_k, st)
    ans = np.zeros(n, M.ANSWER_DTYPE)
    for name in ("call", "n_legal", "flags", "k", "entropy", "top_action", "top_prob"):
        ans[name] = a[name]
    ans["value"] = np.linspace(-0.5, 0.5, n)
    return M.Answers(arr, st, ans, a["probs"], top_k), quiz[:n], ps


def test_quiz_score_arithmetic():
    ans, quiz, ps = _answers(3)
    key = [{"1N": 10, "1D": 4}, None, {"1H": 10, "2H": 3, "Pass": 1}]
    s = M.quiz_score(ans, key)
    assert s["per_position"][1] is None and s["total"]["positions"] == 2 and s["total"]["max"] == 20
    for i, k in ((0, {7: 10, 4: 4}), (2, {5: 10, 10: 3, 0: 1})):
        row, p = s["per_position"][i], ans.probs[i]
        assert row["points"] == k.get(int(ans.call[i]), 0) and row["max"] == 10
        assert row["top_mass"] == pytest.approx(p[[a for a, v in k.items() if v == 10]].sum(), abs=1e-15)
        assert row["expected"] == pytest.approx(sum(p[a] * v for a, v in k.items()), abs=1e-12)
    assert s["total"]["points"] == s["per_position"][0]["points"] + s["per_position"][2]["points"]
    assert s["total"]["expected"] == pytest.approx(s["per_position"][0]["expected"] + s["per_position"][2]["expected"])
    assert s["total"]["top_mass"] == pytest.approx((s["per_position"][0]["top_mass"] + s["per_position"][2]["top_mass"]) / 2)
    forced = M.quiz_score(ans, [{boards.CALL_NAMES[int(c)]: 5} for c in ans.call])
    assert forced["total"]["points"] == forced["total"]["max"] == 15
    with pytest.raises(ValueError):
        M.quiz_score(ans, key[:2])
    with pytest.raises(ValueError):
        M.quiz_score(ans, [{"9C": 1}, None, None])


def test_answers_document_round_trips_with_nan_and_bad_rows(tmp_path):
    ans, _, _ = _answers(4, top_k=8)
    ans.entropy[1], ans.top_prob[1], ans.probs[1], ans.flags[1], ans.k[1], ans.top_action[1] = np.nan, np.nan, np.nan, M.NONFINITE, 0, 255
    ans.status[2], ans.call[2] = M.ILLEGAL_CALL | (1 << 8), 255
    path = tmp_path / "answers.json"
    ans.to_json(path)
    back = M.Answers.from_json(path)
    assert back.same_as(ans) and ans.same_as(back) and len(back) == 4 and back.top_k == 8
    assert back.entropy.tobytes() == ans.entropy.tobytes() and back.probs.tobytes() == ans.probs.tobytes() and back.value.dtype == np.float32
    other = M.Answers.from_json(path)
    other.call[0] ^= 1
    assert not other.same_as(ans)
    with pytest.raises(ValueError):
        M.Answers.from_json({"format": "something else"})
    d = back.of(0)
    assert d["call"] == boards.CALL_NAMES[int(ans.call[0])] and len(d["top"]) == int(ans.k[0]) and d["top"][0][1] >= d["top"][-1][1]
    assert d["hand"] == "AQ5.KJ4.QT92.K83" and d["seat"] == "N" and d["auction"] == ""
    assert back.of(2)["call"] is None and "illegal call (call 1)" in back.to_text(2) and "non-finite" in back.to_text(1)
    text = back.to_text(0)
    assert f"N calls {d['call']}" in text and "value" in text and "%" in text and "(none)" in text


def test_the_quiz_fixture_is_twelve_legal_positions_with_keys():
    from brl_amd import bid
    ps, keys = bid.read_positions(QUIZ)
    assert len(ps) == 12 and all(keys) and len({p.hand for p in ps}) == 12 and {p.dealer for p in ps} == {0, 1, 2, 3}
    for p, k in zip(ps, keys):
        assert all((p.legal >> M.call_id(c)) & 1 for c in k) and max(k.values()) == 10      # every keyed call is a legal one
    assert (P.rows(M.positions_array(ps))[0] == P.OK).all()


# ---- the command line ------------------------------------------------------------------------------------------------------------------
def test_cli_argument_errors(tmp_path):
    from brl_amd import bid
    for argv, what in (([], "model_path"), (["model_path=x.pt"], "either hand="), (["model_path=x.pt", f"hand={HAND}", f"positions_path={QUIZ}"], "either hand="),
                       (["model_path=x.pt", f"hand={HAND}", "save_path=a.json"], "save_path= needs"), (["model_path=x.pt", f"hand={HAND}", "top_k=9"], "top_k"),
                       (["model_path=x.pt", f"hand={HAND}", "auction=1C 1C"], "call 1 "), (["model_path=x.pt", "hand=AKQ.J32.T9.8765"], "thirteen"),
                       (["model_path=x.pt", f"hand={HAND}", "colour=red"], "unknown option")):
        with pytest.raises(SystemExit) as e:
            bid.main(argv, log=lambda *_: None)
        assert what in str(e.value), (argv, e.value)
    bad = tmp_path / "bad.json"
    bad.write_text(json.dumps([{"hand": HAND, "dealer": "N", "vul": "None", "auction": ""}, {"hand": HAND, "dealer": "N", "vul": "None", "auction": "X"}]))
    with pytest.raises(SystemExit, match="position 1: call 0"):
        bid.read_positions(str(bad))
    bad.write_text("{}")
    with pytest.raises(SystemExit, match="JSON list"):
        bid.read_positions(str(bad))
