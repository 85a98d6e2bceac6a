"""Double-dummy par without a GPU: the two restatements (tests/par_ref.py) against each other and on the worked boards, the
header against what brl_amd/par.py reads, par_stats against plain loops, the contract names, and the writers of BoardRecords
with and without par (the par records come from the restatement here; the kernel is compared with it in test_gpu_par.py)."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import board_records_ref as R  # noqa: E402
import par_ref as P  # noqa: E402

from brl_amd import boards, par  # noqa: E402
from tests.contract_matrix import imp as law_imp  # noqa: E402

NAMED = os.path.join(ROOT, "tests", "golden", "wb5_named_24.json")


# ---- the restatements -------------------------------------------------------------------------------------------------------
def test_scan_equals_brute_force_on_the_fixture_tables(dds):
    """the scan on all 1000 tables x 4 vulnerabilities x both first sides; the brute force on every fifth table (200 x 4 x 2):
    it is ten times slower"""
    never_both = True
    for i in range(1000):
        for v in range(4):
            for first in (0, 1):
                s = P.par_scan(dds["tricks"][i], v & 1, v >> 1, first)
                never_both &= not (s[2] and s[3])
                assert s[0] == 0 or s[2] | s[3], (i, v, first, s)            # a par score other than 0 has a par contract
                if i % 5 == 0:
                    assert P.par_brute(dds["tricks"][i], v & 1, v >> 1, first) == s, (i, v, first)
    assert never_both


def test_scan_equals_brute_force_on_random_tables():
    """2000 uniform 0..13 tables with random vulnerability and first side, the brute force on all of them; dealer dependence,
    which the real tables never show, is common here"""
    rng = np.random.default_rng(12)
    dependent = 0
    for k in range(2000):
        t, v, first = rng.integers(0, 14, size=20), int(rng.integers(0, 4)), int(rng.integers(0, 2))
        s = P.par_scan(t, v & 1, v >> 1, first)
        assert P.par_brute(t, v & 1, v >> 1, first) == s, (k, t, v, first)
        assert not (s[2] and s[3]) and (s[0] == 0 or s[2] | s[3])
        # the other first side swaps R and R_alt
        assert P.par_scan(t, v & 1, v >> 1, 1 - first)[:2] == (s[1], s[0])
        dependent += s[0] != s[1]
    assert dependent >= 500


@pytest.mark.parametrize("name", list(P.WORKED))
@pytest.mark.parametrize("solver", [P.par_brute, P.par_scan])
def test_the_worked_boards(name, solver):
    table, vul_ns, vul_ew, want = P.WORKED[name]
    for first in (0, 1):
        r, r_alt, m_ns, m_ew = solver(table, vul_ns, vul_ew, first)
        assert (r, m_ns, m_ew) == want[first], (name, first)
        assert r_alt == want[1 - first][0]
    for dealer in range(4):
        (rec,) = P.par_records(table[None], [dealer], [vul_ns], [vul_ew], solver)
        assert rec[0] == want[dealer & 1][0] and rec[2] == P.worked_flags(name)


def test_what_the_worked_boards_say():
    """B: 2C by East-West also scores 300 (doubled two off) but is not par — North-South overcall it without loss; E: 1C
    scores 130 too but East-West's 1DX -1 costs them only 100"""
    t, vn, ve, _ = P.WORKED["B"]
    tricks = P.side_tricks(t)
    assert P.outcome(tricks, (vn, ve), P.EW, P.bid("2C")) == 300 == P.outcome(tricks, (vn, ve), P.EW, P.bid("5H"))
    assert not P.par_scan(t, vn, ve, 0)[3] & P.bits("2C")
    t, vn, ve, _ = P.WORKED["E"]
    tricks = P.side_tricks(t)
    assert P.outcome(tricks, (vn, ve), P.NS, P.bid("1C")) == 130 and P.outcome(tricks, (vn, ve), P.EW, P.bid("1D")) == 100
    assert not P.par_scan(t, vn, ve, 0)[2] & P.bits("1C")
    # C depends on the dealer's side, not on the seat
    t, vn, ve, _ = P.WORKED["C"]
    assert [r[0] for r in P.par_records(np.stack([t] * 4), [0, 1, 2, 3], [vn] * 4, [ve] * 4)] == [90, -90, 90, -90]


def test_the_score_beyond_thirteen_tricks_is_one_more_overtrick():
    for strain in range(5):
        for vul in (0, 1):
            step = P.score(strain, 3, vul, 0, 13) - P.score(strain, 3, vul, 0, 12)
            assert P.score(strain, 7, vul, 0, 14) - P.score(strain, 7, vul, 0, 13) == step
            assert P.score(strain, 7, vul, 0, 15) - P.score(strain, 7, vul, 0, 13) == 2 * step


# ---- the header and the binding -------------------------------------------------------------------------------------------------
def test_the_header_states_the_layout_the_host_reads():
    text = open(os.path.join(ROOT, "include", "brl_par.h")).read()
    assert "/* 32 bytes = 2 x 16, little endian, no padding */" in text and par.PAR_DTYPE.itemsize == 32
    assert f"#define BRL_PAR_PASSED_OUT {par.PASSED_OUT} " in text and f"#define BRL_PAR_DEALER_DEPENDENT {par.DEALER_DEPENDENT} " in text
    assert "#define BRL_PAR_NO_RESULT INT32_MIN" in text and par.NO_RESULT == -2 ** 31
    assert (par.PASSED_OUT, par.DEALER_DEPENDENT, par.NO_RESULT) == (P.PASSED_OUT, P.DEALER_DEPENDENT, P.NO_RESULT)
    # the fields in the header's order, at the offsets of two 16-byte pieces
    order = [text.index(f" {name};") for name in par.PAR_DTYPE.names]
    assert order == sorted(order)
    assert [par.PAR_DTYPE.fields[n][1] for n in par.PAR_DTYPE.names] == [0, 4, 8, 12, 16, 24]


def test_the_host_imp_scale_is_the_reference_scale():
    diffs = np.array([0, 10, 20, -20, 40, 50, 3990, 4000, -4000, 15200, -15200] + list(range(-4500, 4501, 10)))
    assert [int(x) for x in par.imp_of(diffs)] == [law_imp(int(d)) for d in diffs]


# ---- records with par ------------------------------------------------------------------------------------------------------------
def _match(n_tables=2, seed=3):
    """the 24 named deals with random finished auctions at both tables (board 0 passed out), and their par records from the
    restatement"""
    d = boards.read_deals(NAMED)
    rng = np.random.default_rng(seed)
    words = d.hand_words()
    tables = []
    for t in range(n_tables):
        packed = []
        for i in range(d.n):
            calls = R.random_auction(rng) if i else [0, 0, 0, 0]
            seating = (0, 1, 2, 3) if t == 0 else (2, 3, 0, 1)
            packed.append(R.encode(int(d.dealer[i]), calls, vul_ns=int(d.vul_ns[i]), vul_ew=int(d.vul_ew[i]), tricks=d.tricks[i],
                                   hands=[int(w) for w in words[i]], seating=seating).pack())
        tables.append(R.decode(np.stack(packed)))
    pr = np.zeros(d.n, par.PAR_DTYPE)
    for i, row in enumerate(P.par_records(d.tricks, d.dealer, d.vul_ns, d.vul_ew)):
        pr[i] = (row[0], row[1], row[2], 0, row[3], row[4])
    return d, tables, pr


def _records(d, tables, pr=None):
    imp = np.array([law_imp(int(a) - int(b)) for a, b in zip(tables[0]["score_ns"], tables[-1]["score_ns"])], np.int32)
    return boards.BoardRecords(tables[0], tables[1] if len(tables) > 1 else None, imp, d.tricks, d.board_id, par=pr)


def test_without_par_the_writers_write_what_they_always_wrote(tmp_path):
    d, tables, pr = _match()
    plain, used = _records(d, tables), _records(d, tables, pr)
    used.par()
    used.boards(par=True)
    assert plain.boards() == used.boards() == used.boards(par=False)
    for ext in ("json", "pbn"):
        a, b = str(tmp_path / f"a.{ext}"), str(tmp_path / f"b.{ext}")
        plain.save(a)
        used.save(b, par=False)
        assert open(a).read() == open(b).read() and '"par"' not in open(a).read()
    assert set(plain.boards()[1]["table_a"]) == {"auction", "contract", "declarer", "tricks", "score_ns"}
    assert "OptimumScore" not in open(str(tmp_path / "a.pbn")).read()


def test_boards_with_par_carry_the_par_record(tmp_path):
    d, tables, pr = _match()
    br = _records(d, tables, pr)
    assert br.par() is br.par() and np.array_equal(br.par(), pr)
    plain, with_par = br.boards(), br.boards(par=True)
    for i, (a, b) in enumerate(zip(plain, with_par)):
        assert b["par"] == {"score_ns": int(pr[i]["score_ns"]), "contracts": par.par_contracts(pr[i], d.tricks[i]),
                            "dealer_dependent": bool(pr[i]["flags"] & par.DEALER_DEPENDENT)}
        for key, rec in (("table_a", tables[0]), ("table_b", tables[1])):
            assert b[key]["imp_vs_par"] == law_imp(int(rec[i]["score_ns"]) - int(pr[i]["score_ns"]))
            assert {k: v for k, v in b[key].items() if k != "imp_vs_par"} == a[key]
        assert {k: v for k, v in b.items() if k not in ("par", "table_a", "table_b")} == \
            {k: v for k, v in a.items() if k not in ("table_a", "table_b")}
    path = str(tmp_path / "p.json")
    br.to_json(path, par=True)
    assert json.load(open(path))["logs"] == with_par
    assert all(np.array_equal(x, y) for x, y in zip(boards.read_deals(path), d))           # and it is still a deal file
    path = str(tmp_path / "p.pbn")
    br.save(path, par=True)
    text = open(path).read()
    assert all(np.array_equal(x, y) for x, y in zip(boards.read_deals(path), d))
    for i, b in enumerate(with_par):
        first = b["par"]["contracts"][0].split(" by ") if b["par"]["contracts"] else None
        want = f'[OptimumScore "NS {b["par"]["score_ns"]}"]\n[ParContract "{first[1] + " " + first[0] if first else "Pass"}"]\n[Auction '
        assert text.count(f'[Board "{b["board_id"]}"]') == 2 and want in text
    assert text.count("[OptimumScore ") == text.count("[ParContract ") == 48


def test_par_needs_the_double_dummy_tables():
    d, tables, _ = _match(1)
    br = boards.BoardRecords(tables[0])
    with pytest.raises(ValueError) as e1:
        br.boards()
    with pytest.raises(ValueError) as e2:
        br.par()
    assert str(e1.value) == str(e2.value)


def test_a_table_without_a_result_has_no_imp_against_par():
    live = R.decode(R.encode(0, [3, 0]).pack()[None])                   # 1C P and still open
    t = R.encode(0, [3, 0])
    t.step(2)                                                           # an illegal redouble
    ended = R.decode(t.pack()[None])
    done = R.decode(R.encode(0, [3, 0, 0, 0], tricks=np.full((4, 5), 7)).pack()[None])
    rec = np.concatenate([live, ended, done])
    pr = np.zeros(3, par.PAR_DTYPE)
    pr["score_ns"] = [70, 70, -50]
    assert list(par.imp_vs_par(rec, pr)) == [par.NO_RESULT, par.NO_RESULT, law_imp(70 + 50)]
    br = boards.BoardRecords(rec, dda=np.full((3, 20), 7, np.uint8), par=pr)
    assert [b["table_a"]["imp_vs_par"] for b in br.boards(par=True)] == [None, None, 3]


# ---- names -----------------------------------------------------------------------------------------------------------------------
def test_par_contract_names():
    def row(r, ns=0, ew=0):
        x = np.zeros(1, par.PAR_DTYPE)
        x[0] = (r, r, 0, 0, ns, ew)
        return x[0]
    for name, want in (("A", ["4S by NS"]), ("B", ["5HX by EW"]), ("C", ["1NT by NS"]), ("D", []), ("E", ["2C by NS", "3C by NS", "4C by NS"])):
        table, vn, ve, exp = P.WORKED[name]
        r, m_ns, m_ew = exp[0]
        assert par.par_contracts(row(r, m_ns, m_ew), table) == want == par.par_contracts(row(r, m_ns, m_ew))
    table, vn, ve, exp = P.WORKED["C"]
    assert par.par_contracts(row(-90, 0, P.bits("1NT")), table) == ["1NT by EW"] == par.par_contracts(row(-90, 0, P.bits("1NT")))
    assert par.par_contracts(row(-100, P.bits("7NT")), P.table_of({P.NT: 12})) == ["7NTX by NS"] == par.par_contracts(row(-100, P.bits("7NT")))
    # with and without the table, on everything the restatement finds
    rng = np.random.default_rng(5)
    for _ in range(300):
        t, v, first = rng.integers(0, 14, size=20), int(rng.integers(0, 4)), int(rng.integers(0, 2))
        r, _, m_ns, m_ew = P.par_scan(t, v & 1, v >> 1, first)
        assert par.par_contracts(row(r, m_ns, m_ew), t) == par.par_contracts(row(r, m_ns, m_ew))


# ---- statistics -------------------------------------------------------------------------------------------------------------------
def _loops(tables, pr, seats_ns):
    """par_stats, written out: per table and team the list of (imp, at par, holder) of its results"""
    results = {(t, team): [] for t in range(len(tables)) for team in (0, 1)}
    skipped = [0] * len(tables)
    for t, rec in enumerate(tables):
        for i in range(len(rec)):
            flags = int(rec[i]["flags"])
            if not flags & boards.TERMINATED or flags & boards.ILLEGAL:
                skipped[t] += 1
                continue
            imp_ns = law_imp(int(rec[i]["score_ns"]) - int(pr[i]["score_ns"]))
            ns_team = seats_ns[t][i]
            for team in (0, 1):
                ns = team == ns_team
                if pr[i]["contracts_ns"] == 0 and pr[i]["contracts_ew"] == 0:
                    holder = "passed_par"
                else:
                    holds_ns = pr[i]["contracts_ns"] != 0
                    holder = "own_par" if holds_ns == ns else "their_par"
                results[(t, team)].append((imp_ns if ns else -imp_ns, int(rec[i]["score_ns"]) == int(pr[i]["score_ns"]), holder))
    return results, skipped


def _check(s, rows):
    imps = [r[0] for r in rows]
    n = len(imps)
    assert s["imp"]["count"] == n
    if n:
        mean = sum(imps) / n
        assert s["imp"]["mean"] == pytest.approx(mean) and s["at_par"] == pytest.approx(sum(r[1] for r in rows) / n)
        if n > 1:
            assert s["imp"]["se"] == pytest.approx((sum((x - mean) ** 2 for x in imps) / (n - 1) / n) ** 0.5)
    for holder in ("own_par", "their_par", "passed_par"):
        part = [r[0] for r in rows if r[2] == holder]
        assert s[holder]["count"] == len(part)
        if part:
            assert s[holder]["mean"] == pytest.approx(sum(part) / len(part))
        else:
            assert np.isnan(s[holder]["mean"])


def test_par_stats_against_plain_loops():
    d, tables, pr = _match(seed=9)
    # a live and an illegal-ended record at table B, and mixed seatings at table A
    tables[1][3] = R.decode(R.encode(int(d.dealer[3]), [3, 0], seating=(2, 3, 0, 1)).pack()[None])[0]
    t = R.encode(int(d.dealer[4]), [3, 0], seating=(2, 3, 0, 1))
    t.step(2)
    tables[1][4] = R.decode(t.pack()[None])[0]
    for i in range(0, 24, 3):
        tables[0]["seating"][i] = 2 | 0 << 2 | 3 << 4 | 1 << 6         # team 2's player 2 sits North
    seats_ns = [[(int(r["seating"]) & 3) >> 1 for r in rec] for rec in tables]
    assert {0, 1} == set(seats_ns[0]) and set(seats_ns[1]) == {1}
    s = par.par_stats(_records(d, tables, pr))
    results, skipped = _loops(tables, pr, seats_ns)
    assert s["boards"] == 24 and skipped == [0, 2]
    for t, name in enumerate("ab"):
        tab = s["tables"][name]
        assert tab["skipped"] == skipped[t]
        rows = results[(t, 0)]
        assert tab["abs_imp"] == pytest.approx(sum(abs(r[0]) for r in rows) / len(rows))
        for team in (0, 1):
            _check(tab[f"team{team + 1}"], results[(t, team)])
        # at one table the two teams mirror each other
        assert tab["team1"]["imp"]["mean"] == pytest.approx(-tab["team2"]["imp"]["mean"])
        assert tab["team1"]["own_par"]["count"] == tab["team2"]["their_par"]["count"]
    for team in (0, 1):
        _check(s["teams"][f"team{team + 1}"], results[(0, team)] + results[(1, team)])
    holders = {r[2] for rows in results.values() for r in rows}
    assert {"own_par", "their_par"} <= holders
    lines = par.stats_lines(s)
    assert len(lines) == 2 and lines[0].startswith("par team1: ") and lines[1].startswith("par team2: ")
    # one table only
    one = par.par_stats(_records(d, tables[:1], pr))
    assert list(one["tables"]) == ["a"] and one["teams"]["team1"]["imp"]["count"] == len(results[(0, 0)])


def test_eval_defaults_gained_par():
    from brl_amd.eval import EVAL_DEFAULTS
    from brl_amd.league import parse
    assert EVAL_DEFAULTS["par"] == 0
    assert parse(["par=1"], EVAL_DEFAULTS)["par"] == 1 and parse([], EVAL_DEFAULTS)["par"] == 0
