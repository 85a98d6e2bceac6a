"""-m gpu: the double-dummy par (brl_amd/par.py, include/brl_par.h) against its restatement (tests/par_ref.py), field for field —
real and random tables at the sizes where a wave's edge lies, the worked boards, untrusted input bytes —, brl_par_imp on every
IMP step, the refused arguments, and a duplicate match with the command line end to end.  Every comparison is exact integer
equality."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import board_records_ref as R  # noqa: E402
import par_ref as P  # noqa: E402

from tests.contract_matrix import imp as law_imp  # noqa: E402
from tests.test_oracle_kat import IMP_THRESHOLDS  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMED = os.path.join(ROOT, "tests", "golden", "wb5_named_24.json")
N = 4099
SIZES = [1, 63, 64, 65, N]
WORKED_AT = {name: (64 * k, 64 * k + 63) for k, name in enumerate(P.WORKED)}    # lanes 0 and 63 of wave k
GARBAGE_AT = 5
RANDOM_FROM = 1100                                                              # boards RANDOM_FROM .. N - 1 are random tables

_POOL = {}


def _pool(dds):
    """The one set of N boards and its restatement, built once and only read: the fixture tables under every dealer and
    vulnerability (board i: dealer i % 4, vulnerability i // 4 % 4), uniform 0..13 tables with random dealer and vulnerability
    behind them, the six worked boards at lanes 0 and 63 of the first six waves (both sides dealing), and at GARBAGE_AT one
    board of bytes that are no trick counts, with a dealer and a vulnerability byte of which only the low bits count."""
    if not _POOL:
        rng = np.random.default_rng(2024)
        dda = np.zeros((N, 20), np.uint8)
        dealer, vul = np.zeros(N, np.uint8), np.zeros(N, np.uint8)
        for i in range(RANDOM_FROM):
            dda[i], dealer[i], vul[i] = dds["tricks"][i % 1000].reshape(20), i % 4, i // 4 % 4
        dda[RANDOM_FROM:] = rng.integers(0, 14, size=(N - RANDOM_FROM, 20))
        dealer[RANDOM_FROM:] = rng.integers(0, 4, size=N - RANDOM_FROM)
        vul[RANDOM_FROM:] = rng.integers(0, 4, size=N - RANDOM_FROM)
        for name, (lo, hi) in WORKED_AT.items():
            table, vn, ve, _ = P.WORKED[name]
            for at, d in ((lo, 2), (hi, 3)):
                dda[at], dealer[at], vul[at] = table, d, vn | ve << 1
        # 14 and 15 tricks, and bytes whose high bits must not count: 0xFE -> 14, 0x2F -> 15, 0x35 -> 5, 0xF0 -> 0
        dda[GARBAGE_AT] = [0xFE, 0x2F, 0x35, 0xF0, 0x17, 0x4D, 0x88, 0x0E, 0x93, 0x6F, 0xFF, 0x21, 0x7C, 0xA9, 0x50, 0x3E, 0xB6, 0xC2, 0xDF, 0x6B]
        dealer[GARBAGE_AT], vul[GARBAGE_AT] = 0xFD, 0xF6          # -> dealer 1, East-West vulnerable
        ref = np.zeros(N, _dtype())
        for i, row in enumerate(P.par_records(dda, dealer, vul & 1, (vul >> 1) & 1)):
            ref[i] = (row[0], row[1], row[2], 0, row[3], row[4])
        _POOL.update(dda=dda, dealer=dealer, vul=vul, ref=ref)
    return _POOL


def _dtype():
    from brl_amd import par
    return par.PAR_DTYPE


def test_the_pool_reaches_every_branch(dds):
    from brl_amd import par
    p = _pool(dds)
    ref = p["ref"]
    special = {GARBAGE_AT} | {at for pair in WORKED_AT.values() for at in pair}
    real = [i for i in range(RANDOM_FROM) if i not in special]
    assert {(int(p["dealer"][i]), int(p["vul"][i])) for i in real} == {(d, v) for d in range(4) for v in range(4)}
    rnd = ref[RANDOM_FROM:]
    assert ((rnd["flags"] & par.DEALER_DEPENDENT) != 0).sum() * 4 >= len(rnd)          # at least a quarter
    assert (ref["flags"] & par.PASSED_OUT).any() and (ref["contracts_ns"] != 0).any() and (ref["contracts_ew"] != 0).any()
    assert (ref["score_ns"] < 0).any() and (ref["score_ns"] > 0).any()
    assert int(p["dda"][GARBAGE_AT].max()) > 15 and {14, 15} <= set(int(x) & 15 for x in p["dda"][GARBAGE_AT])
    # the garbage board is scored as its masked table
    masked = P.par_records(p["dda"][GARBAGE_AT:GARBAGE_AT + 1] & 15, [1], [0], [1])[0]
    assert tuple(ref[GARBAGE_AT][k] for k in ("score_ns", "score_ns_alt", "flags", "contracts_ns", "contracts_ew")) == masked
    for name, (lo, hi) in WORKED_AT.items():
        _, _, _, want = P.WORKED[name]
        for at, first in ((lo, 0), (hi, 1)):
            assert (ref[at]["score_ns"], ref[at]["contracts_ns"], ref[at]["contracts_ew"]) == want[first], (name, at)
            assert ref[at]["flags"] == P.worked_flags(name)


@pytest.mark.parametrize("n", SIZES)
def test_par_equals_the_restatement(dds, n):
    """the first n boards: one lane, a wave's edge from either side, a partial last wave behind 64 full ones"""
    from brl_amd import par
    p = _pool(dds)
    got = par.par_of(torch.from_numpy(p["dda"][:n]).to(DEV), p["dealer"][:n], p["vul"][:n] & 1, p["vul"][:n] >> 1)
    assert got.shape == (n, 32) and got.dtype == torch.uint8
    got = par.par_array(got)
    for name in par.PAR_DTYPE.names:
        bad = np.nonzero(got[name] != p["ref"][name][:n])[0]
        assert bad.size == 0, (name, int(bad[0]), got[bad[0]], p["ref"][bad[0]])
    assert not got["zero"].any() and not ((got["contracts_ns"] | got["contracts_ew"]) >> np.uint64(35)).any()
    assert got.tobytes() == p["ref"][:n].tobytes()


@pytest.mark.parametrize("n", SIZES)
def test_nothing_is_written_behind_the_last_record(dds, n):
    """the raw entry point on a buffer with a sentinel behind record n - 1; and the same bytes on a second run"""
    from brl_amd import _capi
    p = _pool(dds)
    dda, dealer, vul = (torch.from_numpy(p[k][:n].copy()).to(DEV) for k in ("dda", "dealer", "vul"))
    runs = []
    for _ in range(2):
        out = torch.full(((n + 4) * 32,), 0xA5, dtype=torch.uint8, device=DEV)
        _capi.check(_capi.lib().brl_par(0, _capi.ptr(dda), _capi.ptr(dealer), _capi.ptr(vul), n, _capi.ptr(out), _capi.stream(0)))
        host = out.cpu().numpy()
        assert (host[n * 32:] == 0xA5).all()
        runs.append(host[:n * 32].tobytes())
    assert runs[0] == runs[1] == p["ref"][:n].tobytes()


def _finished(score_ns, dealer=0):
    """board records of finished auctions (1C P P P) carrying the given North-South scores"""
    one = R.decode(R.encode(dealer, [3, 0, 0, 0], tricks=np.full((4, 5), 7)).pack()[None])
    rec = np.repeat(one, len(score_ns))
    rec["score_ns"] = score_ns
    return rec


def _upload(rec):
    return torch.from_numpy(rec.view(np.uint8).reshape(-1, 368)).to(DEV)


def _par_rows(score_ns):
    pr = np.zeros(len(score_ns), _dtype())
    pr["score_ns"] = score_ns
    return torch.from_numpy(pr.view(np.uint8).reshape(-1, 32)).to(DEV), pr


@pytest.mark.parametrize("sign", [1, -1])
def test_par_imp_reaches_every_step_of_the_scale(sign):
    """differences at each threshold and 10 below it, both directions, around par scores of either sign: 0 .. 24 IMPs"""
    from brl_amd import par
    diffs = [0, 10, -10] + [s * (th - k) for th in IMP_THRESHOLDS for k in (0, 10) for s in (1, -1)]
    pars = [0, 420, -1100, 7600, -7600]
    score = np.array([p + d for p in pars for d in diffs], np.int32)
    base = np.array([p for p in pars for _ in diffs], np.int32)
    rec = _finished(score)
    dev_par, host_par = _par_rows(base)
    got = par.par_imp(_upload(rec), dev_par, sign).cpu().numpy()
    want = np.array([sign * law_imp(int(s) - int(b)) for s, b in zip(score, base)], np.int32)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert set(range(-24, 25)) == set(int(x) for x in got)
    assert np.array_equal(sign * par.imp_vs_par(rec, host_par), want)                 # the host arithmetic agrees


def test_par_imp_gives_no_result_for_a_live_and_an_illegal_ended_record():
    from brl_amd import par
    live = R.decode(R.encode(0, [3, 0]).pack()[None])
    t = R.encode(0, [3, 0])
    t.step(2)                                                                       # an illegal redouble ends the table
    ended = R.decode(t.pack()[None])
    passed = R.decode(R.encode(1, [0, 0, 0, 0]).pack()[None])
    rec = np.concatenate([live, ended, passed, _finished(np.array([-50], np.int32))])
    rec["score_ns"][:2] = 500                                                       # (whatever the score field holds)
    dev_par, host_par = _par_rows(np.array([0, 0, 110, 70], np.int32))
    for sign in (1, -1):
        got = par.par_imp(_upload(rec), dev_par, sign).cpu().numpy()
        assert list(got) == [par.NO_RESULT, par.NO_RESULT, sign * law_imp(-110), sign * law_imp(-120)]
    assert list(par.imp_vs_par(rec, host_par)) == [par.NO_RESULT, par.NO_RESULT, -3, -3]


def test_bad_arguments_are_refused_with_a_message(dds):
    from brl_amd import _capi
    L = _capi.lib()
    p = _pool(dds)
    dda, dealer, vul = (torch.from_numpy(p[k][:64].copy()).to(DEV) for k in ("dda", "dealer", "vul"))
    out = torch.zeros(65 * 32, dtype=torch.uint8, device=DEV)
    a = [_capi.ptr(dda), _capi.ptr(dealer), _capi.ptr(vul), 64, _capi.ptr(out)]

    def refused(fn, args, what):
        rc = fn(0, *args, _capi.stream(0))
        assert rc < 0 and what in L.brl_last_error().decode(), (rc, L.brl_last_error())

    for k in (0, 1, 2, 4):
        refused(L.brl_par, a[:k] + [None] + a[k + 1:], "NULL array")
    for n in (0, -1, 2 ** 31):
        refused(L.brl_par, a[:3] + [n] + a[4:], "n (1 .. 2^31)")
    refused(L.brl_par, a[:4] + [a[4] + 8], "16-byte aligned")
    refused(L.brl_par, [a[0] + 4] + a[1:], "16-byte aligned")
    rec, (dev_par, _) = _upload(_finished(np.zeros(4, np.int32))), _par_rows(np.zeros(4, np.int32))
    imp = torch.full((4,), 77, dtype=torch.int32, device=DEV)
    b = [_capi.ptr(rec), _capi.ptr(dev_par), 4, 1, _capi.ptr(imp)]
    for k in (0, 1, 4):
        refused(L.brl_par_imp, b[:k] + [None] + b[k + 1:], "NULL array")
    for n in (0, 2 ** 31):
        refused(L.brl_par_imp, b[:2] + [n] + b[3:], "n (1 .. 2^31)")
    for sign in (0, 2, -2):
        refused(L.brl_par_imp, b[:3] + [sign] + b[4:], "sign")
    torch.cuda.synchronize()
    assert not out.any() and (imp == 77).all()                                       # a refused call launches nothing


# ---- a duplicate match, end to end ----------------------------------------------------------------------------------------------
def test_the_par_of_a_match_and_the_command_line(tmp_path):
    import brl_amd
    from brl_amd import boards, checkpoint, par
    from brl_amd import eval as eval_cli
    from brl_amd.models import make_forward_pass
    fp = make_forward_pass("relu", "DeepMind")
    nets = [fp.init(60 + k, device=DEV) for k in range(2)]
    for k in range(2):
        checkpoint.save_params(nets[k], str(tmp_path / f"params-{k:08}.pt"))
    base = [f"team1_model_path={tmp_path / 'params-00000000.pt'}", f"team2_model_path={tmp_path / 'params-00000001.pt'}", f"deals_path={NAMED}"]

    # the command line before anything touched par
    before = []
    eval_cli.main(base + [f"save_boards={tmp_path / 'before.json'}"], log=before.append)

    deals = boards.read_deals(NAMED)
    env = brl_amd.BridgeBidding(lut=(deals.lut_keys(), deals.lut_values()), device=DEV)
    _, records = boards.make_board_match(env, "relu", "DeepMind", "relu", "DeepMind")(nets[0], nets[1], deals)
    plain = records.boards()
    named = json.load(open(NAMED))["logs"]
    file_dda = np.array([[b["dda"][seat][st] for seat in "NESW" for st in ("C", "D", "H", "S", "NT")] for b in named], np.uint8)
    file_dealer = ["NESW".index(b["dealer"]) for b in named]
    file_vul = [("None", "NS", "EW", "Both").index(b["vulnerability"]) for b in named]
    want = P.par_records(file_dda, file_dealer, [v & 1 for v in file_vul], [v >> 1 for v in file_vul])
    got = records.par()
    assert got.dtype == par.PAR_DTYPE and records.par() is got
    assert [tuple(int(r[k]) for k in ("score_ns", "score_ns_alt", "flags", "contracts_ns", "contracts_ew")) for r in got] == want
    assert not got["zero"].any()

    with_par = records.boards(par=True)
    assert records.boards() == plain
    for i, b in enumerate(with_par):
        assert b["par"] == {"score_ns": want[i][0], "contracts": par.par_contracts(got[i], file_dda[i]),
                            "dealer_dependent": bool(want[i][2] & P.DEALER_DEPENDENT)}
        assert b["par"]["contracts"] or want[i][2] & P.PASSED_OUT
        for key, table in (("table_a", "a"), ("table_b", "b")):
            assert b[key]["imp_vs_par"] == law_imp(b[key]["score_ns"] - want[i][0])      # (every table of a match has a result)
        assert {k: v for k, v in b.items() if k not in ("par", "table_a", "table_b")} == {k: v for k, v in plain[i].items() if k not in ("table_a", "table_b")}
    # the device's IMPs against par are the host arithmetic's
    for table in ("a", "b"):
        assert np.array_equal(records.imp_vs_par(table), par.imp_vs_par(records.cpu(table), got))
    stats = par.par_stats(records)
    assert stats["boards"] == 24 and stats["tables"]["a"]["skipped"] == 0 == stats["tables"]["b"]["skipped"]
    assert stats["teams"]["team1"]["imp"]["count"] == 48 == stats["teams"]["team2"]["imp"]["count"]
    # a team's pooled mean: the North-South IMP where its player sits at seat 0, the negative where the other team's does
    total = sum(int(np.where((records.cpu(t)["seating"] & 3) < 2, 1, -1) @ records.imp_vs_par(t).astype(np.int64)) for t in "ab")
    assert stats["teams"]["team1"]["imp"]["mean"] == pytest.approx(total / 48) == -stats["teams"]["team2"]["imp"]["mean"]

    # a match on boards the evaluator deals itself: the seatings keep the teams opposite, so the tables seat different teams North
    _, dealt = boards.make_board_match(env, "relu", "DeepMind", "relu", "DeepMind", 65)(nets[0], nets[1], 5)
    ra, rb = dealt.cpu("a"), dealt.cpu("b")
    assert (((ra["seating"] & 3) >> 1) != ((rb["seating"] & 3) >> 1)).all()
    want65 = P.par_records(dealt.dda.cpu().numpy(), ra["dealer"], ra["vul_ns"], ra["vul_ew"])
    assert [tuple(int(r[k]) for k in ("score_ns", "score_ns_alt", "flags", "contracts_ns", "contracts_ew")) for r in dealt.par()] == want65
    s65 = par.par_stats(dealt)
    for t in "ab":
        assert s65["tables"][t]["team1"]["imp"]["count"] == 65 and s65["tables"][t]["team1"]["imp"]["mean"] == pytest.approx(-s65["tables"][t]["team2"]["imp"]["mean"])

    # the command line: par=1 adds the team lines behind the IMP line and writes par with the boards
    said = []
    eval_cli.main(base + [f"save_boards={tmp_path / 'par.json'}", "par=1"], log=said.append)
    assert said[:len(before)] == before[:-2] + [f"boards: {tmp_path / 'par.json'}"] + before[-1:]
    assert said[len(before):] == par.stats_lines(stats) and len(said) == len(before) + 2
    assert said[-2].startswith("par team1: ") and said[-1].startswith("par team2: ")
    assert json.load(open(tmp_path / "par.json"))["logs"] == with_par
    alone = []
    eval_cli.main(base + ["par=1"], log=alone.append)                                  # par=1 alone implies the boards run
    assert alone == before[:-2] + before[-1:] + said[-2:]
    # without par= the lines and the file are what they were before par() was ever called
    after = []
    eval_cli.main(base + [f"save_boards={tmp_path / 'after.json'}"], log=after.append)
    assert after[:-2] == before[:-2] and after[-1] == before[-1] and after[-2] == f"boards: {tmp_path / 'after.json'}"
    assert open(tmp_path / "after.json").read() == open(tmp_path / "before.json").read()
    assert json.load(open(tmp_path / "before.json"))["logs"] == plain
    pbn = tmp_path / "par.pbn"
    records.save(str(pbn), par=True)
    assert open(pbn).read().count("[OptimumScore ") == 48 and all(np.array_equal(x, y) for x, y in zip(boards.read_deals(str(pbn)), deals))
