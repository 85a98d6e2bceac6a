"""CPU: the auction lines' header against the binding and the host's dtypes, the Python restatement (tests/lines_ref.py) on
hand-worked cases, its observation against the oracle's, the closed form of a uniform policy, ``AuctionLines``' statistics, text
and JSON on hand-made arrays, and the command line's arguments."""
import math
import os
import re

import numpy as np
import pytest

from brl_amd import lines
from tests import board_records_ref as R
from tests import lines_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, X, XX = 0, 1, 2
NT7 = 37


def _beam(prefix, k, dealer=0, **kw):
    t = R.encode(dealer, prefix, **kw)
    return [F.Line(t, 0xFFFFFFFF, list(prefix), 0.0, F.GREEDY)] + [F.Line() for _ in range(k - 1)]


def _rows(row):
    return lambda s, ln: np.asarray(row, np.float32)


# ---- the header and the binding -------------------------------------------------------------------------------------------------
def test_the_header_states_what_the_binding_and_the_host_read():
    text = open(os.path.join(ROOT, "include", "brl_lines.h")).read()
    for macro, value in (("BRL_LINES_MAX_K", lines.MAX_K), ("BRL_LINES_MAX_CALLS", lines.MAX_CALLS), ("BRL_LINE_EMPTY", lines.EMPTY),
                         ("BRL_LINE_FINISHED", lines.FINISHED), ("BRL_LINE_VOID", lines.VOID), ("BRL_LINE_GREEDY", lines.GREEDY)):
        assert re.search(r"#define " + macro + r" " + str(value) + r"\b", text), macro
    assert "#define BRL_LINES_FILL 0xFF" in text and lines.FILL == F.FILL == 0xFF
    assert (F.EMPTY, F.FINISHED, F.VOID, F.GREEDY) == (lines.EMPTY, lines.FINISHED, lines.VOID, lines.GREEDY)
    for dt, struct in ((lines.REQUEST_DTYPE, "brl_line_request"), (lines.RESULT_DTYPE, "brl_line_result"), (lines.BOARD_DTYPE, "brl_lines_board")):
        body = re.search(r"typedef struct " + struct + r" \{(.*?)\} " + struct, text, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        order = [re.search(r"\b" + name + r"\b", body).start() for name in dt.names]
        assert order == sorted(order), struct
    assert [lines.RESULT_DTYPE.fields[n][1] for n in lines.RESULT_DTYPE.names] == [0, 4, 5, 6, 7, 8, 9, 10, 12]
    assert "brl_lines" not in open(os.path.join(ROOT, "include", "brl_hip.h")).read()


# ---- the restatement on hand-worked cases -----------------------------------------------------------------------------------------
def test_exact_ties_go_to_the_lower_slot_then_the_lower_action():
    """Equal logits, a fresh deal: the 36 children tie, the beam is Pass, 1C (, 1D).  With K = 2 both lines then have 36 legal
    calls (Pass and 35 bids; Pass, X and 34 bids), so all 72 children tie again: slot 0's two lowest actions win.  With K = 3 the
    line 1D has 35 legal calls, each worth 1/35 instead of 1/36: its three lowest actions win."""
    beam, cands = F.expand(_beam([], 2), _rows(np.zeros(38)), 2)
    assert len(cands) == 36 and [ln.calls for ln in beam] == [[P], [3]]
    assert [float(ln.score) for ln in beam] == [-math.log(36.0)] * 2
    assert [ln.flags for ln in beam] == [F.GREEDY, 0]                          # the arg-max of equal logits is the first legal call
    beam, cands = F.expand(beam, _rows(np.zeros(38)), 2)
    assert len(cands) == 72 and len({float(c[1]) for c in cands}) == 1
    assert [ln.calls for ln in beam] == [[P, P], [P, 3]] and [ln.flags for ln in beam] == [F.GREEDY, 0]
    beam, _ = F.expand(_beam([], 3), _rows(np.zeros(38)), 3)
    assert [ln.calls for ln in beam] == [[P], [3], [4]]
    beam, cands = F.expand(beam, _rows(np.zeros(38)), 3)
    assert len(cands) == 36 + 36 + 35 and [ln.calls for ln in beam] == [[4, P], [4, X], [4, 5]] and not any(ln.flags for ln in beam)


def test_a_finished_line_is_kept_against_live_children():
    """P P P on the table, K = 2, Pass at 0.9: the pass-out finishes with log 0.9 and stays in slot 0, unchanged, while the
    live line's children (0.1 x ...) compete for slot 1."""
    row = np.full(38, -30.0, np.float32)
    row[P], row[3] = math.log(9.0), 0.0                                      # Pass 0.9, 1C 0.1, the rest ~ 1e-13
    beam, _ = F.expand(_beam([P, P, P], 2), _rows(row), 2)
    assert [ln.calls for ln in beam] == [[P, P, P, P], [P, P, P, 3]] and [ln.flags for ln in beam] == [F.FINISHED | F.GREEDY, 0]
    assert abs(float(beam[0].score) - math.log(0.9)) < 1e-7 and abs(float(beam[1].score) - math.log(0.1)) < 1e-7   # (log 9 rounded to float32)
    first = (beam[0].packed().tobytes(), float(beam[0].score))
    beam, cands = F.expand(beam, _rows(row), 2)
    assert (beam[0].packed().tobytes(), float(beam[0].score)) == first and beam[0].flags == F.FINISHED | F.GREEDY
    assert (0, beam[0].score, 0, -1, True) in cands                          # the finished line is action -1 of its own slot
    assert beam[1].calls == [P, P, P, 3, P] and abs(float(beam[1].score) - math.log(0.1)) < 1e-7   # (1C is no longer legal: Pass ~ 1)
    assert F.result(beam[0]) == dict(has_result=1, score_ns=0, level=0, strain=0, doubled=0, declarer=0, tricks=0, score_team1=0)


def test_fewer_candidates_than_slots_leave_empty_slots():
    """after a 7NT opening the next seat has two legal calls, Pass and X: K = 5 keeps both and three empty slots"""
    beam, cands = F.expand(_beam([NT7], 5), _rows(np.arange(38)), 5)
    assert len(cands) == 2 and [ln.calls for ln in beam[:2]] == [[NT7, X], [NT7, P]]
    assert [ln.flags for ln in beam] == [F.GREEDY, 0, F.EMPTY, F.EMPTY, F.EMPTY] and all(ln.score == -np.inf for ln in beam[2:])
    arr = F.beam_arrays([beam], 5, 8)
    assert not arr["tables"][2:].any() and (arr["calls"][2:] == F.FILL).all() and arr["request"][:, 0].tolist() == [0, 0, -1, -1, -1]
    assert arr["calls"][0].tolist() == [NT7, X] + [F.FILL] * 6 and arr["done"].tolist() == [0]


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_a_row_without_a_distribution_voids_the_line(bad):
    """slot 0's row has a NaN (or +inf) on a legal call: the line becomes void — table, calls and score unchanged — and ranks
    behind every other candidate; the same value on an illegal call changes nothing"""
    beam, _ = F.expand(_beam([], 2), _rows(np.zeros(38)), 2)                 # Pass and 1C, both at 1 / 36
    good = np.zeros(38, np.float32)
    rows = {0: good.copy(), 1: good.copy()}
    rows[0][5] = bad                                                         # 1E.. a bid: legal after Pass
    rows[1][3] = bad                                                         # 1C again: NOT legal after 1C
    new, cands = F.expand(beam, lambda s, ln: rows[s], 2)
    assert sum(1 for c in cands if c[0]) == 1 and len(cands) == 1 + 36
    assert [ln.calls for ln in new] == [[3, P], [3, X]] and all(ln.flags == 0 for ln in new)
    # a beam of a live line and a finished one (P P P 1C at 0.9, the pass-out at 0.1), then the bad value on the live line's row
    row = np.full(38, -40.0, np.float32)
    row[P], row[3] = 0.0, 2.0
    beam, _ = F.expand(_beam([P, P, P], 3), _rows(row), 3)
    assert [ln.calls[3:] for ln in beam[:2]] == [[3], [P]] and [ln.flags for ln in beam[:2]] == [F.GREEDY, F.FINISHED]
    rows = {0: good.copy()}
    rows[0][P] = bad
    new3, cands = F.expand(beam, lambda s, ln: rows.get(s, good), 3)
    assert len(cands) == 2 + 35                                              # (slot 2 holds P P P 1D at e-42: Pass, X and 33 bids)
    assert new3[0].flags == F.FINISHED and new3[0].score == beam[1].score    # behind the finished line although it has more mass
    void = [ln for ln in F.expand(beam[:2], lambda s, ln: rows[s], 2)[0] if ln.flags & F.VOID][0]
    assert void.flags == F.VOID | F.GREEDY and void.calls == [P, P, P, 3] and void.score == beam[0].score
    assert void.packed().tobytes() == beam[0].packed().tobytes()
    again, _ = F.expand([void, F.Line()], lambda s, ln: good, 2)             # the void bit stays, the line is not continued
    assert again[0].flags == F.VOID | F.GREEDY and again[0].calls == [P, P, P, 3] and again[1].flags == F.EMPTY
    terms, greedy, void = F.log_softmax(np.full(38, -np.inf), [True] * 38)   # no legal logit above -inf: void, arg-max 0
    assert void and greedy == 0
    row = np.zeros(38, np.float32)
    row[P] = -np.inf                                                         # -inf on a legal call: probability 0, not void
    terms, greedy, void = F.log_softmax(row, [True] + [False, False] + [True] * 35)
    assert not void and terms[P] == -np.inf and greedy == 3 and abs(terms[3] + math.log(35.0)) < 1e-15


def test_the_greedy_call_is_the_evaluators_first_strict_maximum():
    row = np.array([1.0, 9.0, 9.0, 2.0, 5.0, 5.0] + [0.0] * 32, np.float32)
    legal = [True, False, False] + [True] * 35
    assert F.log_softmax(row, legal)[1] == 4                                 # X / XX are not legal; 5.0 first at action 4
    row[7] = np.nan
    assert F.log_softmax(row, legal)[1] == 4 and F.log_softmax(row, legal)[2]   # a NaN is never the maximum (and voids the row)


def test_a_line_still_live_at_the_cap_is_open():
    k, cap = 2, 2
    beam = _beam([], k)
    for _ in range(cap):
        beam, _ = F.expand(beam, _rows(np.zeros(38)), k)
    arr = F.beam_arrays([beam, _beam([P, P, P, P], k)], k, cap)
    res = np.zeros(2 * k, lines.RESULT_DTYPE)
    for i, ln in enumerate(beam + _beam([P, P, P, P], k)):
        for name, v in F.result(ln).items():
            res[i][name] = v
    arr["flags"][k] |= F.FINISHED                                            # (the second board was dealt finished: brl_lines_init's flag)
    res[k]["has_result"] = 1
    boards = np.zeros(2, lines.BOARD_DTYPE)
    al = lines.lines_from_parts(k, cap, [dict(arr, results=res)] * 2, boards)
    assert al.open[0, 0].tolist() == [True, True] and not al.finished[0, 0].any() and al.length[0, 0].tolist() == [2, 2]
    assert al.finished[0, 1].tolist() == [True, False] and not al.open[0, 1].any() and al.contract[0, 1].tolist() == [0, lines.NO_RESULT]
    assert al.contract[0, 0].tolist() == [lines.NO_RESULT] * 2 and al.prob[0, 1].tolist() == [1.0, 0.0]
    assert [r["state"] for r in al.of(0)] == ["open", "open"] and al.of(1)[0]["contract"] == "passed out"


def test_the_restatements_observation_is_the_oracles(oracle, dds):
    rng = np.random.default_rng(7)
    for i in range(12):
        calls = R.random_auction(rng, stop=int(rng.integers(0, 14)))
        hand = oracle.key_to_hand(dds["keys"][i])
        hand = np.sort(hand.reshape(4, 13), axis=1).reshape(52).astype(np.int32)
        seating = [(0, 2, 1, 3), (2, 0, 3, 1), (1, 3, 0, 2), (3, 1, 2, 0)][i & 3]
        st = oracle.init_explicit(hand[None], i & 3, (i >> 2) & 1, (i >> 3) & 1, np.array(seating, np.int32), dds["tricks"][i].reshape(1, 20))
        bits = ((hand % 13 + 12) % 13) * 4 + (3 - hand // 13)
        hands = [sum(1 << int(b) for b in bits[s * 13:(s + 1) * 13]) for s in range(4)]
        t = R.Table(i & 3, vul_ns=(i >> 2) & 1, vul_ew=(i >> 3) & 1, seating=seating, hands=hands)
        for a in calls:
            if t.term:
                break
            assert np.array_equal(F.observe(t), oracle.observe(st, st["current_player"])[0]), (i, calls)
            assert [int(t.legal(x)) for x in range(38)] == st["legal_action_mask"][0].tolist()
            t.step(a)
            oracle.step(st, np.array([a], np.int32))


def test_a_uniform_policy_gives_the_closed_form(oracle, dds):
    """Equal logits everywhere, K = 1: ties go to the lowest action, so the line is Pass four times, with probability
    1 / (L0 L1 L2 L3), the L being the legal counts the oracle reports; the evaluators' arg-max of equal logits is the first legal
    call, Pass, so the line is the greedy one."""
    hand = np.sort(oracle.key_to_hand(dds["keys"][0]).reshape(4, 13), axis=1).reshape(1, 52).astype(np.int32)
    st = oracle.init_explicit(hand, 1, 0, 1, np.array([0, 2, 1, 3], np.int32), dds["tricks"][0].reshape(1, 20))
    counts = []
    while not st["terminated"][0]:
        counts.append(int(st["legal_action_mask"][0].sum()))
        oracle.step(st, np.array([P], np.int32))
    assert counts == [36, 36, 36, 36]
    beam = _beam([], 1, dealer=1, seating=(0, 2, 1, 3))
    for _ in range(6):
        beam, _ = F.expand(beam, _rows(np.full(38, 0.25)), 1)
    ln = beam[0]
    assert ln.calls == [P] * 4 and ln.flags == F.FINISHED | F.GREEDY
    assert abs(math.exp(ln.score) - 1.0 / np.prod(counts)) < 1e-18


def test_the_sum_is_antisymmetric_bit_for_bit_and_bounded():
    rng = np.random.default_rng(3)
    for k in (1, 2, 5, 16):
        pa, pb = rng.dirichlet(np.ones(k + 1))[:k], rng.dirichlet(np.ones(k + 1))[:k]
        ua, ub = rng.integers(-2000, 2000, k) // 10 * 10, rng.integers(-2000, 2000, k) // 10 * 10
        S, c = F.board_sums(pa, ua, pb, ub)
        S2, c2 = F.board_sums(pb, -ub, pa, -ua)                              # the teams exchanged: the beams swap, every score negates
        assert S2 == -S and c2 == c and 0 < c < 1 and abs(S) <= 24 * c
        plain = sum(pa[i] * pb[j] * F.V.conv(int(ua[i] + ub[j])) for i in range(k) for j in range(k))
        assert abs(S - plain) < 1e-12
    assert F.board_sums([0.0, 0.0], [0, 0], [0.5, 0.0], [100, 0]) == (0.0, 0.0)


# ---- AuctionLines ---------------------------------------------------------------------------------------------------------------------
def _synthetic():
    """two boards, K = 2.  Board 0: table A finished lines 1NT by N making 7 (0.6, greedy) and a pass-out (0.3); table B one finished
    line (0.5, not greedy) and an open line (0.4, greedy).  Board 1: table A one void line (0.2) and nothing else; table B empty but
    a pass-out (1.0)."""
    k, mc = 2, 4
    z = lambda dt: np.zeros((2, 2, k), dt)   # noqa: E731
    a = {n: z(lines._KINDS[n]) for n in lines._LINE_ARRAYS if n != "calls"}
    a["calls"] = np.full((2, 2, k, mc), lines.FILL, np.uint8)
    a["calls"][0, 0, 0], a["calls"][0, 0, 1] = [7, P, P, P], [P, P, P, P]
    a["calls"][1, 0, 0], a["calls"][1, 0, 1, :2] = [P, 7, P, P], [P, P]
    a["calls"][0, 1, 0, :1], a["calls"][1, 1, 0] = [P], [P, P, P, P]
    a["length"][:, 0], a["length"][0, 1], a["length"][1, 1] = [[4, 4], [4, 2]], [1, 0], [4, 0]
    a["prob"][:, 0], a["prob"][0, 1], a["prob"][1, 1] = [[0.6, 0.3], [0.5, 0.4]], [0.2, 0.0], [1.0, 0.0]
    with np.errstate(divide="ignore"):
        a["logp"] = np.log(a["prob"])
    a["finished"][:, 0], a["finished"][1, 1] = [[1, 1], [1, 0]], [1, 0]
    a["open"][1, 0, 1], a["void"][0, 1, 0] = True, True
    a["greedy"][0, 0, 0] = a["greedy"][1, 0, 1] = a["greedy"][0, 1, 0] = a["greedy"][1, 1, 0] = True
    a["contract"][:] = lines.NO_RESULT
    a["contract"][0, 0], a["contract"][1, 0, 0], a["contract"][1, 1, 0] = [7, 0], 7, 0
    a["declarer"][1, 0, 0], a["tricks"][0, 0, 0], a["tricks"][1, 0, 0] = 1, 7, 7
    a["score_ns"][0, 0, 0], a["score_ns"][1, 0, 0] = 90, -90
    a["score_team1"][0, 0, 0], a["score_team1"][1, 0, 0] = 90, 90
    b = dict(covered_a=[0.9, 0.0], covered_b=[0.5, 1.0], open_a=[0.0, 0.0], open_b=[0.4, 0.0], void_a=[0.0, 0.2], void_b=[0.0, 0.0])
    b["covered"] = [0.45, 0.0]
    b["imp"] = [0.6 * 0.5 * 5 + 0.3 * 0.5 * 3, 0.0]                           # conv(180) = 5, conv(90) = 3
    b["imp_lo"] = [b["imp"][0] - 24 * 0.55, -24.0]
    b["imp_hi"] = [b["imp"][0] + 24 * 0.55, 24.0]
    return lines.AuctionLines(k, mc, [11, 12], **a, **b)


def test_summary_text_and_json_of_a_synthetic_result(tmp_path):
    al = _synthetic()
    s = al.summary()
    assert s["boards"] == 2 and s["k"] == 2 and abs(s["imp"] - 0.5 * (1.5 + 0.45)) < 1e-15
    assert abs(s["imp_bound"] - 0.5 * 24 * (0.55 + 1.0)) < 1e-12 and abs(s["covered"] - 0.225) < 1e-15
    assert abs(s["covered_table"] - 2.4 / 4) < 1e-15 and abs(s["open_table"] - 0.1) < 1e-15 and abs(s["void_table"] - 0.05) < 1e-15
    assert abs(s["greedy_mass"] - (0.6 + 0.4 + 0.0 + 1.0) / 4) < 1e-15         # a void line's greedy bit carries no mass
    assert s["greedy_kept"] == 0.75
    assert abs(s["top_not_greedy"] - 1 / 3) < 1e-15                          # three tables have a finished line; B of board 0 is not greedy
    h = -(2 / 3) * math.log(2 / 3) - (1 / 3) * math.log(1 / 3)
    assert abs(s["contract_entropy"] - h / 3) < 1e-12                        # the other two tables hold one contract each
    text = al.to_text(0)
    assert "board 11:" in text and "1NT by N, 7 tricks, NS +90" in text and "passed out" in text and "0.6000* finished 1NT P P P" in text
    assert "0.4000* open     P P" in text and al.to_text(1).count("void") == 1
    assert al.to_text() == "\n".join(al.summary_lines()) and len(al.summary_lines()) == 2 and all(ln.startswith("lines: ") for ln in al.summary_lines())
    assert [r["state"] for r in al.of(0, "b")] == ["finished", "open"] and al.of(1, "b")[0]["contract"] == "passed out"
    al.to_json(tmp_path / "lines.json")
    back = lines.AuctionLines.from_json(tmp_path / "lines.json")
    assert back.same_as(al) and back.summary() == s and back.to_text(0) == text


def test_the_command_line_checks_its_arguments():
    from brl_amd import eval as ev
    from brl_amd.league import parse
    cfg = parse(["lines=4", "lines_max_calls=24", "save_lines=x.json"], ev.EVAL_DEFAULTS)
    assert (cfg["lines"], cfg["lines_max_calls"], cfg["save_lines"]) == (4, 24, "x.json")
    assert (ev.EVAL_DEFAULTS["lines"], ev.EVAL_DEFAULTS["lines_max_calls"], ev.EVAL_DEFAULTS["save_lines"]) == (0, 64, None)
    base = ["team1_model_path=a.pt", "team2_model_path=b.pt"]
    for bad in (["lines=17"], ["lines=-1"], ["save_lines=x.json"]):
        with pytest.raises(SystemExit, match="lines=K"):
            ev.main(base + bad, log=lambda *_: None)
    for k, mc in ((0, 64), (17, 64), (4, 0), (4, 65)):
        with pytest.raises(ValueError):
            lines._check_beam(k, mc)
