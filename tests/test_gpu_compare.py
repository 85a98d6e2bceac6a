"""-m gpu: the system diff (brl_amd/compare.py, include/brl_compare.h) — brl_compare_tables, brl_compare_rows and
brl_compare_reduce on synthetic inputs against their Python restatement (tests/compare_ref.py) and brl_belief_logp, and whole
diffs of the bidder pair (tests/bidder_net.py) on a 256-board match: one network against itself, each caller's own network
against the call it played, a copy forced to 1NT, everything against the restatement on the logits the device used, skipped
records, the tables, the chunking, the plane route, the command line."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import belief_ref as BR
from tests import bidder_net as bn
from tests import board_records_ref as R
from tests import book_ref as B
from tests import compare_ref as CR
from tests.test_gpu_belief import LOGP_BOUND
from tests.test_gpu_review import _oracle_tables

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMED = os.path.join(ROOT, "tests", "golden", "wb5_named_24.json")
ALL = (1 << 38) - 1

C_DIV = 256.0
"""|device divergence - restatement| <= C_DIV * 2^-52 * (the sum of the magnitudes of the restatement's terms).  Both sides perform
the same IEEE double operations in the same order; they differ only in exp, log, log1p and sinh (the device's library against
numpy's).  Measured on an MI355X over every case of this file (the tests print it; DESIGN §17): the worst ratio is 84.9, on the
synthetic rows whose two policies differ by 0.05 per logit — there one ulp of log S moves every d_a by 2^-52 while the terms are
twenty times smaller than the probabilities; on the bidder pair's matches it is 5.4.  Four times the worst is 340: C_DIV is the
256 it may be at most."""
EPS = 2.0 ** -52


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _decisions(raw):
    from brl_amd import compare
    return raw.cpu().numpy().view(compare.DECISION_DTYPE).reshape(-1)


def _within(got, ref, scale, what):
    """asserts the float64 divergences ``got`` against the restatement's within C_DIV; -> the worst |difference| / (2^-52 scale)"""
    nan, inf = np.isnan(ref), np.isinf(ref)
    assert np.array_equal(np.isnan(got), nan) and np.array_equal(got[inf], ref[inf]), what
    fin = ~nan & ~inf
    zero = fin & (scale == 0)
    assert (got[zero] == 0).all() and not np.signbit(got[zero]).any(), what           # nothing to add up: exactly +0.0
    some = fin & (scale > 0)
    ratio = np.abs(got[some] - ref[some]) / (EPS * scale[some])
    worst = float(ratio.max()) if some.any() else 0.0
    assert worst <= C_DIV, (what, worst)
    return worst


def _check_against(got, want, d, what):
    """device decision records against ``compare_ref.expected_records``: the integer fields bit for bit, the divergences within
    C_DIV; -> the worst ratio"""
    for name in ("key", "legal", "feats", "played", "call_x", "call_y", "flags", "reserved"):
        assert np.array_equal(got[name], want[name]), (what, name, np.nonzero(got[name] != want[name])[0][:5])
    live = d["live"]
    dead = got[~live]
    assert not dead.view(np.uint8).any(), what                                         # no decision: an all-zero record
    return max(_within(got[name][live], want[name][live], d[scale][live], (what, name))
               for name, scale in (("kl_xy", "abs_xy"), ("kl_yx", "abs_yx"), ("js", "abs_js")))


# ---- brl_compare_tables -------------------------------------------------------------------------------------------------------------
def _auctions(rng, n, long_every=2):
    out = []
    for i in range(n):
        a = R.random_auction(rng, p_pass=0.35)
        while i % long_every == 0 and len(a) < 10:
            a = R.random_auction(rng, p_pass=0.35)
        out.append(a)
    return out


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_tables_are_the_beliefs_empty_tables(n):
    """a wave's 64 rows and one more or less; the rows in no order, one record twice; every dealer, vulnerability and seating"""
    from brl_amd import compare
    rng = np.random.default_rng(n)
    rec = B.make_records(_auctions(rng, n + 2), rng)
    rows = rng.permutation(n + 2)[:n].astype(np.int64)
    if n > 1:
        rows[-1] = rows[0]
    tables, hands = compare.compare_tables(_dev(rec.view(np.uint8).reshape(-1, 368)), _dev(rows))
    tables, hands = tables.cpu().numpy().view(np.uint64), hands.cpu().numpy().view(np.uint64)
    assert tables.shape == (n, 16) and hands.shape == (n, 4)
    for j, i in enumerate(rows):
        r = rec[i]
        assert np.array_equal(hands[j], r["hands"]), j
        want = BR.sample_tables(int(r["dealer"]), int(r["vul_ns"]), int(r["vul_ew"]), int(r["seating"]), r["hands"][None, :].astype(np.uint64))
        assert np.array_equal(tables[j], want[0]), j
    if n >= 63:
        assert len(set(rec["dealer"][rows])) == 4 and len(set(rec["seating"][rows])) >= 4 and len(set(zip(rec["vul_ns"][rows], rec["vul_ew"][rows]))) == 4


# ---- brl_compare_rows ---------------------------------------------------------------------------------------------------------------
def _rows_case(m, ld, t, depth, seed):
    """n = m + 3 records (every second one with ten calls and more; one without OK, one ended by an illegal call), m of them listed
    in no order; per row the legal word of its auction at t, and logits in eight kinds: random; one legal action; tied everywhere;
    the two best tied; _PassOnly's constants against random; legal -inf logits; a legal NaN; a legal +inf"""
    from brl_amd import boards
    rng = np.random.default_rng(seed)
    n = m + 3
    rec = B.make_records(_auctions(rng, n), rng)
    if n > 4:
        rec["flags"][1] = 0
        rec["flags"][3] |= boards.ILLEGAL
    rows = rng.permutation(n)[:m].astype(np.int64)
    legal = np.ones(m, np.uint64)
    lx = (rng.normal(size=(m, ld)) * 4).astype(np.float32)
    ly = (lx + rng.normal(size=(m, ld)) * rng.choice([0.0, 0.05, 2.0], size=(m, 1))).astype(np.float32)
    kinds = np.zeros(m, np.int64)
    for j, i in enumerate(rows):
        calls = [int(c) for c in rec["calls"][i][:int(rec["n_calls"][i])]]
        if t < len(calls):
            legal[j] = BR.legal_words(int(rec["dealer"][i]), calls[:t + 1])[t][1]
        acts = [a for a in range(38) if (int(legal[j]) >> a) & 1]
        kind = kinds[j] = (j + seed) % 8
        if kind == 1 and t < len(calls) and calls[t] == 0:
            legal[j] = 1
        elif kind == 2:
            lx[j, :38] = 1.5
        elif kind == 3 and len(acts) > 1:
            lx[j, acts[-1]] = lx[j, acts[0]] = 30.0
            ly[j, acts[1]] = ly[j, acts[0]] = 30.0
        elif kind == 4:
            lx[j, :38] = -1e30
            lx[j, 0] = 0.0
        elif kind == 5 and len(acts) > 1:
            lx[j, acts[1:3]] = -np.inf
            ly[j, acts[-1]] = -np.inf
        elif kind == 6:
            (lx if j % 2 else ly)[j, acts[len(acts) // 2]] = np.nan
        elif kind == 7:
            (lx if j % 2 else ly)[j, acts[-1]] = np.inf
    return rec, rows, legal, lx, ly, kinds


def _run_rows(rec, rows, t, depth, lx, ly, legal, fill=0):
    from brl_amd import compare
    dec = torch.full((len(rec) * depth, 64), fill, dtype=torch.uint8, device=DEV)
    compare.compare_rows(_dev(rec.view(np.uint8).reshape(-1, 368)), _dev(rows), t, depth, _dev(lx), _dev(ly), _dev(legal.view(np.int64)), dec)
    return _decisions(dec).reshape(len(rec), depth)


@pytest.mark.parametrize("ld", [38, 39])
@pytest.mark.parametrize("m", [1, 7, 8, 9, 511, 512, 513])
def test_rows_equal_the_restatement_and_the_beliefs_logp(m, ld):
    from brl_amd import belief, compare
    worst = 0.0
    for t, depth in ((0, 1), (0, 10), (9, 10)):
        rec, rows, legal, lx, ly, kinds = _rows_case(m, ld, t, depth, 1000 * m + 10 * ld + t + depth)
        dense = _run_rows(rec, rows, t, depth, lx, ly, legal, fill=0xAB)
        listed = np.zeros(len(rec), bool)
        listed[rows] = True
        untouched = np.ones((len(rec), depth), bool)
        untouched[listed, t] = False
        assert (dense.view(np.uint8).reshape(len(rec), depth, 64)[untouched] == 0xAB).all()      # nobody else's records
        got = dense[rows, t]
        want, d = CR.expected_records(rec, depth, t, rows, lx, ly, legal, compare.DECISION_DTYPE)
        worst = max(worst, _check_against(got, want, d, (m, ld, t, depth)))
        live = d["live"]
        if m >= 511:      # every kind of row took part, with and without a decision
            assert set(kinds[live]) == set(range(8)) and (~live).any() and ((got["flags"] & CR.NONFINITE) != 0).sum() >= 10
            assert (got["flags"][live & (kinds == 6)] & CR.NONFINITE).all() and (got["flags"][live & (kinds == 7)] & CR.NONFINITE).all()
            assert not (got["flags"][live & (kinds <= 5)] & CR.NONFINITE).any() and np.isinf(got["kl_xy"][live & (kinds == 5)]).any()
            one = live & (got["legal"] == 1)
            assert one.any() and (got["js"][one] == 0).all() and (got["call_x"][one] == 0).all() and (got["logp_x"][one] == 0).all()
            assert (got["call_x"][live & (kinds == 2)] == [min(a for a in range(38) if (int(w) >> a) & 1) for w in legal[live & (kinds == 2)]]).all()
        # logp: brl_belief_logp on the same logits, legal words and calls, bit for bit
        for name, lg in (("logp_x", lx), ("logp_y", ly)):
            logw, greedy = torch.zeros(m, device=DEV), torch.ones(m, dtype=torch.uint8, device=DEV)
            belief.logp(_dev(lg), torch.arange(m, device=DEV), torch.arange(m, dtype=torch.int32, device=DEV), _dev(legal.view(np.int64)),
                        _dev(d["played"].astype(np.int32)), logw, greedy)
            ref = logw.cpu().numpy()
            a, b = got[name][live], ref[live]
            assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)].view(np.uint32), b[~np.isnan(b)].view(np.uint32)), name
            call = got["call_x" if name == "logp_x" else "call_y"][live]
            assert np.array_equal(greedy.cpu().numpy()[live] != 0, (call == d["played"][live]) & ~np.isnan(a))      # and the arg-max is its
        # the two exact properties
        swapped = _run_rows(rec, rows, t, depth, ly, lx, legal)[rows, t]
        for a, b in (("kl_xy", "kl_yx"), ("kl_yx", "kl_xy"), ("js", "js"), ("logp_x", "logp_y"), ("call_x", "call_y")):
            assert np.array_equal(got[a].view(f"u{got[a].itemsize}"), swapped[b].view(f"u{got[a].itemsize}")), (a, b)
        same = _run_rows(rec, rows, t, depth, lx, lx, legal)[rows, t]
        fin = live & ((same["flags"] & CR.NONFINITE) == 0)
        for name in ("kl_xy", "kl_yx", "js"):
            assert not same[name][fin].view(np.uint64).any(), name                       # +0.0, bit for bit
        assert (same["flags"][fin] & CR.AGREE).all() and np.array_equal(same["logp_x"].view(np.uint32), same["logp_y"].view(np.uint32))
    print(f"rows m={m} ld={ld}: worst |device - restatement| of a divergence = {worst:.2f} x 2^-52 x the sum of its terms' magnitudes (C = {C_DIV})")


# ---- brl_compare_reduce -------------------------------------------------------------------------------------------------------------
def _sorted_case(lengths, seed, zero_run=5):
    """sorted decisions: a leading run of key 0, then one run per length, each with random calls, flags, features and float fields
    spread over thirty orders of magnitude (a sum's bits then depend on its order); every 23rd decision non-finite"""
    from brl_amd import compare
    rng = np.random.default_rng(seed)
    S = zero_run + sum(lengths)
    dec = np.zeros(S, compare.DECISION_DTYPE)
    starts, at = [zero_run], zero_run
    for e, ln in enumerate(lengths):
        dec["key"][at:at + ln] = compare.key_of([e % 38, (e // 38) % 38][:1 + e % 2])
        at += ln
        starts.append(at)
    dec["key"][zero_run:] = np.sort(dec["key"][zero_run:], kind="stable")
    live = dec["key"] != 0
    n = int(live.sum())
    for name in ("kl_xy", "kl_yx", "js"):
        dec[name][live] = np.exp(rng.uniform(-35, 35, size=n))
    dec["kl_xy"][live] = np.where(rng.random(n) < 0.01, np.inf, dec["kl_xy"][live])
    dec["logp_x"][live], dec["logp_y"][live] = -np.exp(rng.uniform(-20, 4, size=(2, n))).astype(np.float32)
    dec["call_x"][live], dec["call_y"][live], dec["played"][live] = rng.integers(0, 38, size=(3, n))
    dec["call_y"][live] = np.where(rng.random(n) < 0.6, dec["call_x"][live], dec["call_y"][live])
    dec["feats"][live] = rng.integers(0, 38, size=n) | (rng.integers(0, 2 ** 18, size=n) << 6)
    fl = CR.VALID | np.where(dec["call_x"] == dec["call_y"], CR.AGREE, 0) | np.where(dec["call_x"] == dec["played"], CR.X_PLAYED, 0) \
        | np.where(dec["call_y"] == dec["played"], CR.Y_PLAYED, 0)
    bad = live & (np.arange(S) % 23 == 7)
    for name in ("kl_xy", "kl_yx", "js"):
        dec[name][bad] = np.nan
    dec["flags"] = np.where(live, fl | np.where(bad, CR.NONFINITE, 0), 0)
    keys = dec["key"][zero_run:]
    bounds = np.concatenate([[0], np.nonzero(keys[1:] != keys[:-1])[0] + 1, [len(keys)]]) + zero_run
    return dec, bounds.astype(np.int64)


REDUCE_RUNS = [1, 63, 64, 65, 1023, 1024, 1025, 3, 256 * 64 + 70, 2, 64, 128, 1]


def test_reduce_equals_the_restatement_bit_for_bit():
    """runs of one decision, around one block of 64, around 16 blocks, one longer than the 256 blocks a workgroup takes at a time
    (256 x 64 + 70), a leading run of key 0; the bytes behind entries[K) stay as they were; twice the same bytes"""
    from brl_amd import _capi, compare
    dec, starts = _sorted_case(REDUCE_RUNS, 11)
    K = len(starts) - 1
    assert K == len(REDUCE_RUNS) and sorted(np.diff(starts).tolist()) == sorted(REDUCE_RUNS) and starts[0] == 5
    want, want_conf = CR.reduce(dec, starts, compare.ENTRY_DTYPE)
    sdev, stdev = _dev(dec.view(np.uint8).reshape(-1, 64)), _dev(starts)
    out = []
    for _ in range(2):
        entries = torch.full((K + 2, 560), 0xCD, dtype=torch.uint8, device=DEV)
        conf = torch.full((38, 38), -1, dtype=torch.int64, device=DEV)
        _capi.check(_capi.lib().brl_compare_reduce(0, _capi.ptr(sdev), sdev.shape[0], _capi.ptr(stdev), K, _capi.ptr(entries), _capi.ptr(conf),
                                                   _capi.stream(0)))
        out.append((entries.cpu().numpy(), conf.cpu().numpy()))
    (raw, conf), again = out
    assert (raw[K:] == 0xCD).all()
    got = raw[:K].reshape(-1).view(compare.ENTRY_DTYPE)
    for name in compare.ENTRY_DTYPE.names:
        assert got[name].tobytes() == want[name].tobytes(), (name, got[name][:3], want[name][:3])
    assert np.array_equal(conf, want_conf) and conf.sum() == int((got["n"] - got["nonfinite"]).sum()) and got["nonfinite"].sum() > 100
    assert raw.tobytes() == again[0].tobytes() and np.array_equal(conf, again[1])
    assert np.isinf(got["kl_xy_sum"]).any() and np.isfinite(got["js_sum"]).all() and (got["js_max"] > 0).all()
    assert int(got["n"].sum()) == sum(REDUCE_RUNS)                                    # the run of key 0 dropped


def test_sort_and_reduce_sorts_stably_by_key():
    """the dense decisions in no order, runs of key 0 scattered among them: the entries are the restatement's of the stable sort"""
    from brl_amd import compare
    dec, _ = _sorted_case([1, 63, 64, 65, 700, 2, 9], 12, zero_run=40)
    dense = dec[np.random.default_rng(3).permutation(len(dec))]
    perm, starts = CR.sort_runs(dense)
    want, want_conf = CR.reduce(dense[perm], starts, compare.ENTRY_DTYPE)
    entries, conf = compare.sort_and_reduce(_dev(dense.view(np.uint8).reshape(-1, 64)))
    assert entries.cpu().numpy().tobytes() == want.tobytes() and np.array_equal(conf.cpu().numpy(), want_conf)
    assert (want["key"][1:] > want["key"][:-1]).all() and int(want["n"].sum()) == len(dec) - 40
    none = compare.sort_and_reduce(torch.zeros((7, 64), dtype=torch.uint8, device=DEV))
    assert none[0].shape == (0, 560) and not none[1].any()


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
BOARDS, DEPTH = 256, 4


@pytest.fixture(scope="module")
def match(dds, oracle):
    """the 256-board match of the bidder pair, its diff team 1 (X) against team 2 (Y) with the logits the device used, and the
    float64 host forward's top-two gap of every decision, computed once"""
    import brl_amd
    from brl_amd import boards, compare
    nets = bn.pair(DEV)
    env = brl_amd.BridgeBidding(lut=(dds["keys"], dds["values"]), device=DEV)
    hand = np.stack([oracle.key_to_hand(k) for k in dds["keys"][:BOARDS]])
    deals = boards.Deals(np.sort(hand.reshape(-1, 4, 13), axis=2).reshape(-1, 52).astype(np.int32), dds["dealer"][:BOARDS], dds["vul_ns"][:BOARDS],
                         dds["vul_ew"][:BOARDS], dds["tricks"][:BOARDS].reshape(-1, 20), dds["board_id"][:BOARDS])
    _, records = boards.make_board_match(env, "relu", "DeepMind", "relu", "DeepMind")(nets[0], nets[1], deals)
    policy_diff = compare.make_policy_diff(env, "relu", "DeepMind", "relu", "DeepMind", depth=DEPTH)
    rows = []
    pd = policy_diff(nets[0], nets[1], records, rows=rows)
    torch.cuda.synchronize()
    return dict(env=env, nets=nets, records=records, policy_diff=policy_diff, diff=pd, rows=rows, rec={tb: records.cpu(tb) for tb in "ab"})


def _check_diff(pd, rows, recs, what):
    """a whole PolicyDiff against the restatement evaluated on the logits ``rows`` holds; -> (worst divergence ratio, worst
    |logp - float64| over its bound)"""
    from brl_amd import compare
    worst, worst_lp, seen = 0.0, 0.0, np.zeros(pd.decisions.shape, bool)
    for r in rows:
        k, rec = pd.tables.index(r["table"]), recs[r["table"]]
        idx = r["first"] + r["rows"]
        got = pd.decisions[k, idx, r["t"]]
        want, d = CR.expected_records(rec, pd.depth, r["t"], idx, r["logits_x"], r["logits_y"], r["legal"], compare.DECISION_DTYPE)
        assert d["live"].all() and not seen[k, idx, r["t"]].any(), what          # only rows still in their auction were forwarded
        seen[k, idx, r["t"]] = True
        worst = max(worst, _check_against(got, want, d, (what, r["table"], r["t"])))
        assert max(float(np.abs(r["logits_x"]).max()), float(np.abs(r["logits_y"]).max())) <= 30.0      # LOGP_BOUND's premise
        j = np.arange(len(idx))
        for name, L in (("logp_x", d["Lx"]), ("logp_y", d["Ly"])):
            err = np.abs(got[name].astype(np.float64) - L[j, d["played"]])
            worst_lp = max(worst_lp, float(err.max() / LOGP_BOUND))
            assert (err <= LOGP_BOUND).all(), (what, name, float(err.max()))
    assert np.array_equal(seen, pd.decisions["key"] != 0) and not pd.decisions[~seen].view(np.uint8).any(), what
    perm, starts = CR.sort_runs(pd.decisions)
    entries, confusion = CR.reduce(pd.decisions.reshape(-1)[perm], starts, compare.ENTRY_DTYPE)
    for name in compare.ENTRY_DTYPE.names:
        assert pd.entries[name].tobytes() == entries[name].tobytes(), (what, name)
    assert np.array_equal(pd.confusion, confusion), what
    return worst, worst_lp


def test_the_whole_diff_is_the_restatements_on_the_devices_logits(match):
    pd = match["diff"]
    worst, worst_lp = _check_diff(pd, match["rows"], match["rec"], "pair")
    want = sum(min(int(r["n_calls"]), DEPTH) for tb in "ab" for r in match["rec"][tb])
    assert len(pd) == want >= 2 * BOARDS * 3 and pd.skipped == {"a": 0, "b": 0} and pd.decisions.shape == (2, BOARDS, DEPTH)
    assert len(match["rows"]) == 2 * DEPTH and [r["t"] for r in match["rows"]] == list(range(DEPTH)) * 2
    assert all(len(r["rows"]) <= BOARDS for r in match["rows"]) and len(match["rows"][0]["rows"]) == BOARDS
    t = pd.totals()
    assert 0.2 < t["agreement"] < 1.0 and t["js_mean"] > 1e-3 and t["nonfinite"] == 0 and len(pd.entries) > 20      # not vacuous
    for line in pd.stats_lines(min_count=5):
        print(line)
    print(f"pair: {len(pd)} decisions, {len(pd.entries)} prefixes; worst divergence ratio {worst:.2f} (C = {C_DIV}), "
          f"worst |logp - float64| = {worst_lp:.3f} of its bound")


def _host_gaps(oracle, nets, rec, dda, depth):
    """per record and call index t < depth: the gap between the two largest legal logits of the caller's own network in the
    float64 host forward on the oracle's observation of the replayed auction (inf with one legal action, NaN without a decision)"""
    o = _oracle_tables(oracle, rec, dda)
    gap = np.full((len(rec), depth), np.nan)
    for t in range(depth):
        live = np.nonzero(rec["n_calls"] > t)[0]
        sub = o[live]
        a = rec["calls"][live, t].astype(np.int32)
        assert (sub["legal_action_mask"][np.arange(len(live)), a] == 1).all()
        for team in (0, 1):
            rows = np.nonzero((sub["current_player"] >> 1) == team)[0]
            if len(rows):
                lg = np.sort(np.where(sub["legal_action_mask"][rows] == 1, bn.host_forward(nets[team], sub["observation"][rows]), -np.inf), axis=1)
                gap[live[rows], t] = lg[:, -1] - lg[:, -2]
        oracle.step(sub, a)
        o[live] = sub
    return gap


def test_each_callers_own_network_calls_what_it_played(oracle, match):
    """X is team 1's network and Y team 2's, the two that played the match: at every decision the caller's own network's call is
    the call played — the observation rebuilt from the record is the one the match showed it.  The evaluators took the arg-max of
    a forward of another batch size, so decisions whose two best legal logits lie within 1e-3 of each other in the float64 host
    forward are left out: at most 1 % of them (on the CPU, with the host forward playing the match: 8 of 2048)."""
    pd, records = match["diff"], match["records"]
    nets = [n.to("cpu") for n in copy.deepcopy(match["nets"])]
    dda = records.dda.cpu().numpy()
    total = out = 0
    for k, tb in enumerate("ab"):
        dec = pd.decisions[k]
        gap = _host_gaps(oracle, nets, match["rec"][tb], dda, DEPTH)
        live = dec["key"] != 0
        assert np.array_equal(live, ~np.isnan(gap))
        team = (dec["feats"] >> 23) & 1
        own = np.where(team == 0, dec["call_x"], dec["call_y"])
        clear = live & (gap >= 1e-3)
        assert (own[clear] == dec["played"][clear]).all(), (tb, np.argwhere(clear & (own != dec["played"]))[:5])
        flag = np.where(team == 0, CR.X_PLAYED, CR.Y_PLAYED)
        assert ((dec["flags"][clear] & flag[clear]) != 0).all()
        assert (team[live] == 0).any() and (team[live] == 1).any()
        total, out = total + int(live.sum()), out + int((live & ~clear).sum())
    print(f"own network against the call played: {total} decisions, {out} left out (top-two gap under 1e-3): {100 * out / total:.2f}%")
    assert out <= 0.01 * total


def test_one_parameter_object_agrees_with_itself_exactly(match, monkeypatch):
    from brl_amd import evaluation
    made = []
    real = evaluation._Forward

    class Counting(real):
        def __init__(self, *a):
            made.append(1)
            super().__init__(*a)

    monkeypatch.setattr(evaluation, "_Forward", Counting)
    pd = match["policy_diff"](match["nets"][0], match["nets"][0], match["records"])
    assert len(made) == 1                                                             # one object, one forward per call index
    d = pd.decisions[pd.decisions["key"] != 0]
    assert len(d) == len(match["diff"]) and (d["flags"] & CR.AGREE).all() and (d["call_x"] == d["call_y"]).all()
    for name in ("kl_xy", "kl_yx", "js"):
        assert not d[name].view(np.uint64).any(), name                                # +0.0, bit for bit
    assert np.array_equal(d["logp_x"].view(np.uint32), d["logp_y"].view(np.uint32))
    e = pd.entries
    assert (e["agree"] == e["n"]).all() and not e["js_sum"].any() and not e["js_max"].any() and np.array_equal(e["calls_x"], e["calls_y"])
    assert np.array_equal(pd.confusion, np.diag(np.diag(pd.confusion))) and pd.confusion.sum() == len(d)
    assert np.array_equal(d["call_x"], match["diff"].decisions[match["diff"].decisions["key"] != 0]["call_x"])      # X is X in both


def test_a_copy_forced_to_1nt_calls_1nt_wherever_it_is_legal(match):
    """Y = X with the actor bias of 1NT (action 7) raised by 64, far above every logit: call_y is 1NT wherever it is legal and
    X's call elsewhere — the masked arg-max is untouched where 1NT is illegal — and the confusion table's column 7 counts them"""
    x = match["nets"][0]
    y = copy.deepcopy(x)
    with torch.no_grad():
        y.actor.bias[7] += 64.0
    pd = match["policy_diff"](x, y, match["records"])
    d = pd.decisions[pd.decisions["key"] != 0]
    can = ((d["legal"] >> np.uint64(7)) & np.uint64(1)) == 1
    assert can.sum() > 100 and (~can).sum() > 50
    assert (d["call_y"][can] == 7).all() and np.array_equal(d["call_y"][~can], d["call_x"][~can]) and (d["flags"][~can] & CR.AGREE).all()
    assert pd.confusion[:, 7].sum() == int(can.sum()) and pd.confusion.sum() == len(d)
    assert np.array_equal(d["call_x"], match["diff"].decisions[match["diff"].decisions["key"] != 0]["call_x"])
    assert (d["js"][can & (d["call_x"] != 7)] > 0).all() and (d["js"][~can] >= 0).all()


def test_skipped_records_leave_key_0_and_one_table_is_the_first_half(match):
    from brl_amd import boards
    pd, policy_diff, nets = match["diff"], match["policy_diff"], match["nets"]
    only_a = policy_diff(nets[0], nets[1], match["records"], tables="a")
    assert only_a.tables == "a" and only_a.decisions.shape == (1, BOARDS, DEPTH) and only_a.skipped == {"a": 0}
    assert only_a.decisions.tobytes() == pd.decisions[0].tobytes()                    # the same chunks, the same batches: the same bytes
    only_b = policy_diff(nets[0], nets[1], match["records"], tables="b")
    assert only_b.decisions.tobytes() == pd.decisions[1].tobytes() and len(only_a) + len(only_b) == len(pd)
    rec = match["rec"]["a"].copy()
    rec["flags"][3] = int(rec["flags"][3]) & (0xFF ^ boards.OK)
    rec["flags"][5] = int(rec["flags"][5]) | boards.ILLEGAL
    rows = []
    cut = policy_diff(nets[0], nets[1], rec, tables="a", rows=rows)
    assert cut.skipped == {"a": 2} and (cut.decisions["key"][0, [3, 5]] == 0).all() and not cut.decisions[0, [3, 5]].view(np.uint8).any()
    assert len(cut) == len(only_a) - min(int(rec["n_calls"][3]), DEPTH) - min(int(rec["n_calls"][5]), DEPTH)
    assert all(3 not in r["rows"] and 5 not in r["rows"] for r in rows) and len(rows[0]["rows"]) == BOARDS - 2
    _check_diff(cut, rows, {"a": rec}, "cut")
    assert cut.of(3, "a", 0) is None and cut.of(4, "a", 0)["played"] == match["records"].auction(4, "a")[0]


def test_chunks_and_the_plane_route(match):
    """three chunks of at most 100 records per table; and table A's records seventeen times over, 4352 rows in one chunk: the
    forwards of 4096 rows and more take the plane route (brl_linear_x3p).  Both against the restatement on their own logits."""
    from brl_amd import compare, evaluation
    from brl_amd.models import make_forward_pass
    env, nets = match["env"], match["nets"]
    rows = []
    small = compare.make_policy_diff(env, "relu", "DeepMind", "relu", "DeepMind", depth=DEPTH, max_rows=100)(nets[0], nets[1], match["records"], rows=rows)
    assert sorted({r["first"] for r in rows}) == [0, 100, 200] and len(small) == len(match["diff"])
    _check_diff(small, rows, match["rec"], "chunks")
    assert np.array_equal(small.decisions["key"], match["diff"].decisions["key"]) and np.array_equal(small.entries["n"], match["diff"].entries["n"])
    many = np.tile(match["rec"]["a"], 17)
    assert evaluation._Forward(make_forward_pass("relu", "DeepMind"), nets[0]).cast(len(many))[0] == torch.bfloat16      # the plane route's input
    rows = []
    big = compare.make_policy_diff(env, "relu", "DeepMind", "relu", "DeepMind", depth=2)(nets[0], nets[1], many, tables="a", rows=rows)
    assert len(rows) == 2 and min(len(r["rows"]) for r in rows) >= 4096
    worst, worst_lp = _check_diff(big, rows, {"a": many}, "planes")
    same_call = big.decisions["call_x"].reshape(17, BOARDS, 2) == match["diff"].decisions["call_x"][0, :, :2][None]
    print(f"planes: {len(big)} decisions, worst divergence ratio {worst:.2f}, worst |logp - float64| = {worst_lp:.3f} of its bound, "
          f"calls equal to the small batch's on {100 * same_call.mean():.2f}%")
    assert same_call.mean() > 0.98


def test_the_command_line_prints_the_diff(tmp_path):
    from brl_amd import checkpoint, compare
    from brl_amd.models import make_forward_pass
    fp = make_forward_pass("relu", "DeepMind")
    for k in range(2):
        checkpoint.save_params(fp.init(60 + k), str(tmp_path / f"params-{k:08}.pt"))
    envv = dict(os.environ, PYTHONPATH=ROOT)
    base = [sys.executable, "-m", "brl_amd.eval", f"team1_model_path={tmp_path / 'params-00000000.pt'}",
            f"team2_model_path={tmp_path / 'params-00000001.pt'}", f"deals_path={NAMED}"]
    out = []
    for extra in ([], ["diff_depth=3", "diff_min_count=2", f"save_diff={tmp_path / 'diff.json'}"]):
        r = subprocess.run(base + extra, cwd=tmp_path, env=envv, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        out.append(r.stdout.splitlines())
    plain, with_diff = out
    start = [i for i, ln in enumerate(with_diff) if ln.startswith("diff: ")]
    assert len(start) == 2 and start[0] == [i for i, ln in enumerate(with_diff) if ln.startswith("IMP: ")][-1] + 1
    assert with_diff[:start[0]] == plain and not any(ln.startswith("diff") for ln in plain)
    back = compare.PolicyDiff.from_json(tmp_path / "diff.json")
    assert with_diff[start[0]:] == back.stats_lines(min_count=2) + [f"diff: {tmp_path / 'diff.json'}"]
    assert back.depth == 3 and back.tables == "ab" and back.decisions.shape == (2, 24, 3) and len(back) > 100
