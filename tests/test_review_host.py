"""CPU: the call review's header against the binding, its Python restatement (tests/review_ref.py) on hand-made cases, and
``CallReview``'s statistics, text and JSON on hand-made arrays."""
import os
import re

import numpy as np
import pytest
import torch

from brl_amd import boards, review
from tests import board_records_ref as R
from tests import review_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, X, XX = 0, 1, 2


def bid(level, strain):
    return 3 + 5 * (level - 1) + "CDHSN".index(strain)


def _rec(dealer, calls, **kw):
    """the record of an auction (the restatement's encoder and decoder)"""
    return R.decode(R.encode(dealer, calls, **kw).pack()[None, :])


def _played_out(rec, dda, depth, tail=lambda t, a: []):
    """the review's branches with every continuation scripted: the prefix, the alternative, ``tail(t, a)``, then passes to the end
    -> (decisions, void, final records)"""
    decisions, tables, void, _ = V.expand(rec, dda, depth)
    finals = []
    for d, (i, t, seat, team, played) in enumerate(decisions):
        for a in range(38):
            tb = V.empty_table(rec[i], dda[i])
            for c in [int(x) for x in rec[i]["calls"][:t]] + [a] + list(tail(t, a)) + [P] * 4:
                tb.step(c)
            finals.append(tb)
    return decisions, void, V.as_records(finals)


# ---- the header and the binding -------------------------------------------------------------------------------------------------
def test_the_header_states_what_the_binding_and_the_host_read():
    text = open(os.path.join(ROOT, "include", "brl_review.h")).read()
    assert f"#define BRL_REVIEW_ACTIONS {review.ACTIONS} " in text and f"#define BRL_REVIEW_VOID ({review.VOID})" in text
    assert "/* 16 bytes, little endian, no padding */" in text and review.DECISION_DTYPE.itemsize == 16
    assert "/* 8 bytes, no padding */" in text and review.SUMMARY_DTYPE.itemsize == 8
    for dt, struct in ((review.DECISION_DTYPE, "brl_review_decision"), (review.SUMMARY_DTYPE, "brl_review_summary")):
        body = re.search(r"typedef struct " + struct + r" \{(.*?)\} " + struct, text, re.S).group(1)
        order = [body.index(f" {name}") for name in dt.names]
        assert order == sorted(order), struct
    assert [review.DECISION_DTYPE.fields[n][1] for n in review.DECISION_DTYPE.names] == [0, 4, 6, 7, 8, 9]
    assert [review.SUMMARY_DTYPE.fields[n][1] for n in review.SUMMARY_DTYPE.names] == [0, 1, 2, 3, 4, 5, 6]
    assert (V.ACTIONS, V.VOID) == (review.ACTIONS, review.VOID)
    assert "brl_review" not in open(os.path.join(ROOT, "include", "brl_hip.h")).read()


# ---- the restatement on hand-made cases -------------------------------------------------------------------------------------------
def test_the_sign_convention_read_off_by_eye():
    """Two boards, nobody vulnerable, every seat takes 7 tricks in no-trumps and 6 in a suit.  Board 0, dealer North: 1NT by North,
    passed out: +90 to North-South.  Board 1, dealer East: 1NT by East, passed out: -90 to North-South.  At the other table both
    boards were passed out (0)."""
    dda = np.tile(np.array([6, 6, 6, 6, 7], np.uint8), (2, 4)).reshape(2, 20)
    kw = [dict(tricks=dda[i].reshape(4, 5), hands=(1, 2, 4, 8)) for i in range(2)]
    sa, sb = (0, 2, 1, 3), (2, 0, 3, 1)      # players 0 and 1 sit North-South at table A, East-West at table B
    ours = np.concatenate([_rec(0, [bid(1, "N"), P, P, P], seating=sa, **kw[0]), _rec(1, [bid(1, "N"), P, P, P], seating=sa, **kw[1])])
    other = np.concatenate([_rec(0, [P] * 4, seating=sb, **kw[0]), _rec(1, [P] * 4, seating=sb, **kw[1])])
    assert ours["score_ns"].tolist() == [90, -90] and other["score_ns"].tolist() == [0, 0]
    for ours_is, a, b in (("a", ours, other), ("b", other, ours)):
        decisions, void, final = _played_out(a, dda, 12)
        imp = V.values(final, decisions, b)
        s = V.summaries(imp, decisions)
        by = {(i, t): d for d, (i, t, _, _, _) in enumerate(decisions)}
        if ours_is == "a":       # the 1NT table against two pass-outs
            assert [dec[:4] for dec in decisions] == [(0, 0, 0, 0), (0, 1, 1, 1), (0, 2, 2, 0), (0, 3, 3, 1),
                                                      (1, 0, 1, 1), (1, 1, 2, 0), (1, 2, 3, 1), (1, 3, 0, 0)]
            # North's 1NT won 90 = 3 IMPs; a pass instead, all pass: 0.  2NT, one down: -50 = -2 IMPs
            d = by[(0, 0)]
            assert (imp[d, bid(1, "N")], imp[d, P], imp[d, bid(2, "N")], imp[d, X], imp[d, XX]) == (3, 0, -2, -128, -128)
            assert (s["played_imp"][d], s["best_imp"][d], s["best"][d], s["loss"][d], s["n_legal"][d]) == (3, 3, bid(1, "N"), 0, 36)
            # East, next to call, passed: 1NT made against it: -3 from East's side.  Doubling: 1NTX made = 180 = 5 IMPs away: -5.
            # 2NT by East instead goes one down: +50 to North-South, -2 for East: the best East can do is 2 of a suit?  Seven
            # tricks short by two: 2C down 2 = -100 for East-West: +100 North-South = 3 IMPs: -3.  So 2NT (-2) is East's best.
            d = by[(0, 1)]
            assert (imp[d, P], imp[d, X], imp[d, bid(2, "N")], imp[d, bid(2, "C")], imp[d, bid(1, "C")]) == (-3, -5, -2, -3, -128)
            assert (s["best"][d], s["best_imp"][d], s["loss"][d]) == (bid(2, "N"), -2, 1)
            # board 1: East opened 1NT and made it: -90 to North-South, +3 from East's side; North's pass behind it: -3
            assert imp[by[(1, 0)], bid(1, "N")] == 3 and imp[by[(1, 3)], P] == -3 and decisions[by[(1, 3)]][2] == 0
        else:                    # the passed-out table against 1NT making: the pass-out costs North-South 90 on board 0
            d = by[(0, 0)]       # North's pass: board passed out, 0 - 90 = -3; opening 1NT makes 90: 0 IMPs
            assert decisions[d][3] == 1                      # player 2 sits North at this table: team 1 (index from 0)
            assert (imp[d, P], imp[d, bid(1, "N")], s["loss"][d], s["best"][d]) == (-3, 0, 3, bid(1, "N"))
            d = by[(0, 1)]       # East (player 0: team 0 here): the pass-out is +3 for East-West; opening 1NT there makes 90: -90 - 90 = +5
            assert decisions[d][2:4] == (1, 0) and (imp[d, P], imp[d, bid(1, "N")]) == (3, 5)
            d = by[(1, 0)]       # board 1, East deals: pass-out 0 against -90: +3 for North-South, -3 for East
            assert decisions[d][2] == 1 and imp[d, P] == -3


def test_the_tie_rule():
    dec = [(0, 0, 0, 0, 5), (0, 1, 1, 1, 5), (0, 2, 2, 0, 0), (0, 3, 3, 1, 9)]
    imp = np.full((4, 38), V.VOID, np.int8)
    imp[0, [0, 3, 5, 7]] = [2, 4, 4, 1]        # the call made ties for best with a lower id: it stays the best
    imp[1, [0, 3, 5, 7]] = [2, 4, 3, 4]        # two others tie above it: the lowest id
    imp[2, [0]] = [-7]                         # one legal action
    imp[3, :] = -24                            # all 38 legal and equal
    s = V.summaries(imp, dec)
    assert s["best"].tolist() == [5, 3, 0, 9] and s["best_imp"].tolist() == [4, 4, -7, -24]
    assert s["loss"].tolist() == [0, 1, 0, 0] and s["n_legal"].tolist() == [4, 4, 1, 38]


def test_pass_outs_final_alternatives_depth_and_skipped_records():
    dda = np.full((5, 20), 8, np.uint8)
    live = [bid(1, "H"), P, bid(2, "H")]
    rec = np.concatenate([
        _rec(2, [P, P, P, P]),                                         # a pass-out
        _rec(3, [bid(1, "N"), X, XX, P, P, P], vul_ns=1),              # doubled and redoubled
        _rec(0, live),                                                 # a live table
        _rec(0, [bid(1, "C"), P, P, P]),                               # (made unreviewable below)
        _rec(0, [bid(2, "C"), P, X]),                                  # ended by an illegal double of the partner's bid
    ])
    rec[3]["flags"] &= 0xFF ^ boards.OK
    assert rec[4]["flags"] & boards.ILLEGAL and rec[2]["flags"] == boards.OK
    for depth, want in ((1, [1, 1, 1, 0, 0]), (3, [3, 3, 3, 0, 0]), (4, [4, 4, 3, 0, 0]), (320, [4, 6, 3, 0, 0])):
        assert V.counts(rec, depth).tolist() == want
        # the host's prefix sum (plain torch on the records' bytes) agrees
        first, ok = review.first_decisions(torch.from_numpy(rec.view(np.uint8).reshape(5, 368)), depth)
        assert first.tolist() == [0] + np.cumsum(want).tolist() and ok.tolist() == [True, True, True, False, False]
    decisions, tables, void, skipped = V.expand(rec, dda, 320)
    assert skipped == 2 and len(decisions) == 13 and tables.shape == (13 * 38, 16)
    assert [d[:3] for d in decisions[:4]] == [(0, 0, 2), (0, 1, 3), (0, 2, 0), (0, 3, 1)] and all(d[4] == P for d in decisions[:4])
    term = lambda d, a: bool((int(tables[d * 38 + a, 11]) >> 25) & 1)      # noqa: E731
    illegal = lambda d, a: bool((int(tables[d * 38 + a, 11]) >> 27) & 1)   # noqa: E731
    # the pass-out's last decision: the pass ends the auction — final at birth —, a bid keeps it alive
    assert term(3, P) and not illegal(3, P) and not term(3, bid(1, "C")) and not term(2, P)
    # every void slot is a table ended by an illegal call, and no other slot is
    for d in range(len(decisions)):
        for a in range(38):
            assert illegal(d, a) == bool(void[d, a]) and (not void[d, a] or term(d, a))
    # doubles: at board 1 the second caller may double, the third redouble, nobody both
    by = {(i, t): d for d, (i, t, _, _, _) in enumerate(decisions)}
    assert not void[by[(1, 1)], X] and void[by[(1, 1)], XX] and not void[by[(1, 2)], XX] and void[by[(1, 2)], X]
    assert void[by[(1, 3)], X] and void[by[(1, 3)], XX] and void[by[(1, 0)], X]
    # the last pass of board 1 ends a redoubled 1NT by West's side (dealer West): the rewards word holds the score by player
    d = by[(1, 5)]
    w = tables[d * 38 + P]
    score = int(R.decode(w[None, :])[0]["score_ns"])
    assert term(d, P) and score != 0 and [(((int(w[15]) >> (16 * p)) & 0xFFFF) ^ 0x8000) - 0x8000 for p in range(4)] == [score, -score, score, -score]
    # every child is the table of encode(dealer, calls[:t] + [a]) — the rewards word apart, which the encoder does not keep
    for d, (i, t, _, _, _) in enumerate(decisions):
        for a in (P, X, XX, bid(1, "C"), bid(2, "H"), bid(7, "N")):
            r = rec[i]
            want = R.encode(int(r["dealer"]), [int(c) for c in r["calls"][:t]] + [a], vul_ns=int(r["vul_ns"]), vul_ew=int(r["vul_ew"]),
                            seating=V.seating_of(r), tricks=dda[i].reshape(4, 5), hands=[int(h) for h in r["hands"]]).pack()
            assert np.array_equal(tables[d * 38 + a, :15], want[:15])
    # a pass-out alternative is worth the other table's score with the sign turned: other +400 -> -9 for North-South
    other = rec.copy()
    other["score_ns"] = 400
    final = R.decode(tables)
    imp = V.values(final, decisions, other)
    assert imp[3, P] == 9 and decisions[3][2] == 1          # (East makes the last pass: -(-9))
    assert (imp[void] == V.VOID).all()
    assert (imp[2, 1:] == V.VOID).all()                     # live branches have no result until they are played out


# ---- CallReview --------------------------------------------------------------------------------------------------------------------
def _hand_made():
    dec = np.zeros(5, review.DECISION_DTYPE)
    dec["board"], dec["call_index"], dec["seat"] = [0, 0, 0, 2, 2], [0, 1, 2, 0, 1], [0, 1, 2, 3, 0]
    dec["team"], dec["played"] = [0, 1, 0, 1, 0], [7, 0, 0, 0, 12]
    imp = np.full((5, 38), review.VOID, np.int8)
    rows = [{7: 3, 0: 0, 8: 5}, {0: -3, 1: -5, 12: -2}, {0: 3}, {0: 0, 3: 11}, {12: -4, 0: -4}]
    summ = np.zeros(5, review.SUMMARY_DTYPE)
    for d, row in enumerate(rows):
        for a, v in row.items():
            imp[d, a] = v
        s = V.summaries(imp[d:d + 1], [(0, 0, 0, 0, int(dec["played"][d]))])
        for k in ("played", "n_legal", "played_imp", "best_imp", "best", "loss"):
            summ[k][d] = s[k][0]
    return review.review_from_parts(12, {"a": 1, "b": 0}, [(0, dec[:3], imp[:3], summ[:3]), (1, dec[3:], imp[3:], summ[3:])],
                                    board_id=np.array([100, 101, 102]))


def test_call_review_statistics_text_and_json(tmp_path):
    rv = _hand_made()
    assert len(rv) == 5 and rv.table.tolist() == [0, 0, 0, 1, 1] and rv.board_id.tolist() == [100, 100, 100, 102, 102]
    assert rv.loss.tolist() == [2, 1, 0, 11, 0] and rv.best.tolist() == [8, 12, 0, 3, 12]
    st = rv.team_stats()
    t1, t2 = st["team1"], st["team2"]
    assert (t1["decisions"], t2["decisions"]) == (3, 2)
    assert t1["best_share"] == 2 / 3 and t1["mean_loss"] == 2 / 3 and t2["best_share"] == 0.0 and t2["mean_loss"] == 6.0
    # team 1 lost 2 on board 0 and 0 on board 2; team 2 lost 1 and 11
    assert t1["loss_per_board"] == pytest.approx({"count": 2, "mean": 1.0, "se": 1.0}) and t2["loss_per_board"] == pytest.approx({"count": 2, "mean": 6.0, "se": 5.0})
    assert t2["largest"][0] == {"board": 2, "board_id": 102, "table": "b", "call_index": 0, "played": "P", "best": "1C", "loss": 11}
    assert [x["loss"] for x in t1["largest"]] == [2]                  # (decisions without a loss are not listed)
    rows = rv.of(0, "a")
    assert [r["played"] for r in rows] == ["1NT", "P", "P"] and rows[0]["imp"] == {"P": 0, "1NT": 3, "2C": 5}
    assert rows[1] == {"call_index": 1, "seat": "E", "team": 2, "played": "P", "played_imp": -3, "best": "2NT", "best_imp": -2, "loss": 1,
                       "n_legal": 3, "imp": {"P": -3, "X": -5, "2NT": -2}}
    assert rv.of(1, "a") == [] and len(rv.of(2, "b")) == 2
    text = rv.to_text(0)
    assert text.splitlines()[0] == "board 0 table A" and "best 2C +5 (loss 2)" in text and len(text.splitlines()) == 4
    lines = rv.stats_lines()
    assert len(lines) == 2 and lines[0].startswith("review team1: 3 decisions (depth 12), the call made was best in 66.7%")
    assert "largest: board 102 table B call 0 (P, best 1C: 11 IMP)" in lines[1]
    rv.to_json(tmp_path / "r.json")
    back = review.CallReview.from_json(tmp_path / "r.json")
    assert back.same_as(rv) and back.stats_lines() == lines and back.to_text(2) == rv.to_text(2)
    back.loss[0] += 1
    assert not back.same_as(rv)
