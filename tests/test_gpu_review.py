"""-m gpu: the call review (brl_amd/review.py, include/brl_review.h) — brl_review_expand and brl_review_reduce against their Python
restatement (tests/review_ref.py) bit for bit, and the whole review of a 64-board match of the bidder pair (tests/bidder_net.py):
every branch replayed through the CPU oracle, every continuation call against the float64 forward, the value table against the
restatement, the played call's branch against the match itself, the chunking, one network on both sides, the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import bidder_net as bn
from tests import board_records_ref as R
from tests import review_ref as V
from tests.nets import forward64
from tests.test_gpu_forward_biases import _tol32

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMED = os.path.join(ROOT, "tests", "golden", "wb5_named_24.json")
P, X, XX = 0, 1, 2
SEATINGS = [(0, 2, 1, 3), (2, 0, 3, 1), (1, 3, 0, 2), (3, 1, 2, 0)]      # team 1 North-South / East-West (seat-swapped), partners swapped


def _host(raw):
    from brl_amd import boards
    return raw.cpu().numpy().view(boards.RECORD_DTYPE).reshape(-1).copy()


# ---- expand ----------------------------------------------------------------------------------------------------------------------
def _auctions(n, seed):
    """n (dealer, calls, keywords) plans: the 319-call auction, a pass-out, a live table, a doubled and redoubled contract, a table
    ended by an illegal call, then random auctions, one in three stopped early; every dealer, vulnerability and seating"""
    rng = np.random.default_rng(seed)
    plans = []
    for i in range(n):
        if i == 0:
            calls = R.longest_auction()
        elif i == 1:
            calls = [P, P, P, P]
        elif i == 2:
            calls = [3 + 6, P, 3 + 11, X]                                   # live, a double on the table
        elif i == 3:
            calls = [P, 3 + 14, X, XX, P, P, P]
        elif i == 4:
            calls = [3 + 5, P, X]                                           # a double of the partner's bid ends the table
        else:
            calls = R.random_auction(rng, stop=None if i % 3 else int(rng.integers(0, 20)), p_pass=float(rng.uniform(0.2, 0.6)))
        kw = dict(vul_ns=(i >> 2) & 1, vul_ew=(i >> 3) & 1, seating=SEATINGS[(i >> 4) & 3], tricks=rng.integers(0, 14, size=(4, 5)),
                  hands=[int(h) for h in rng.integers(0, 1 << 52, size=4)])
        plans.append(((i + (i >> 6)) & 3, calls, kw))
    return plans


def _expand_case(n, seed):
    from brl_amd import boards
    plans = _auctions(n, seed)
    packed = np.stack([R.encode(d, c, **kw).pack() for d, c, kw in plans])
    dda = np.stack([np.asarray(kw["tricks"], np.uint8).reshape(20) for _, _, kw in plans])
    raw = boards.board_records(torch.from_numpy(packed.view(np.int64)).to(DEV))
    if n > 5:
        raw[5, boards.RECORD_DTYPE.fields["flags"][1]] &= 0xFF ^ boards.OK          # a record that is not one of an auction
    return raw, _host(raw), torch.from_numpy(dda).to(DEV), dda


def _check_expand(raw, rec, dda_dev, dda, depth):
    from brl_amd import review
    want_dec, want_tables, want_void, want_skipped = V.expand(rec, dda, depth)
    first, ok = review.first_decisions(raw, depth)
    assert first.cpu().tolist() == [0] + np.cumsum(V.counts(rec, depth)).tolist() and int((~ok).sum()) == want_skipped
    total = int(first[-1])
    assert total == len(want_dec)
    if total == 0:
        return 0
    decisions, tables = review.expand(raw, dda_dev, depth, first, 0, total)
    dec = decisions.cpu().numpy().view(review.DECISION_DTYPE).reshape(-1)
    got = [(int(x["board"]), int(x["call_index"]), int(x["seat"]), int(x["team"]), int(x["played"])) for x in dec]
    assert got == want_dec and not dec["zero"].any()
    tb = tables.cpu().numpy().view(np.uint64).reshape(total, 38, 16)
    sc = tb[:, :, 11].astype(np.int64)
    illegal, term = ((sc >> 27) & 1).astype(bool), ((sc >> 25) & 1).astype(bool)
    assert np.array_equal(illegal, want_void)                          # the void pattern is Table.legal's
    assert term[illegal].all()                                         # a void slot is never forwarded
    keep = ~want_void
    assert np.array_equal(tb[keep], want_tables.reshape(total, 38, 16)[keep])      # every other slot, all 16 words
    # a sub-range writes the same bytes at its own offset, and nothing else
    if total > 3:
        d0, d1 = total // 3, total - 1
        sub_dec, sub_tables = review.expand(raw, dda_dev, depth, first, d0, d1)
        assert torch.equal(sub_dec, decisions[d0:d1]) and torch.equal(sub_tables, tables[d0 * 38:d1 * 38])
    return total


@pytest.mark.parametrize("n", [1, 5, 64, 257])
def test_expand_equals_the_restatement_bit_for_bit(n):
    from brl_amd import boards
    raw, rec, dda_dev, dda = _expand_case(n, 300 + n)
    if n >= 5:
        assert rec[4]["flags"] & boards.ILLEGAL and rec[2]["flags"] == boards.OK and rec[1]["flags"] & boards.PASSED_OUT
        assert rec[3]["doubled"] == 2 and rec[0]["n_calls"] == 319
    if n > 5:
        assert not rec[5]["flags"] & boards.OK
        assert len(set(rec["dealer"].tolist())) == 4 and len(set(zip(rec["vul_ns"].tolist(), rec["vul_ew"].tolist()))) == 4
        assert len(set(rec["seating"].tolist())) == 4
    totals = [_check_expand(raw, rec, dda_dev, dda, depth) for depth in ((4, 12, 320) if n <= 5 else (12,))]
    print(f"expand n={n}: decisions {totals}")
    if n <= 5:
        assert totals[2] >= 319                                        # every call of the longest auction is a decision
    if n == 5:   # double and redouble are legal alternatives somewhere (records 2 and 3)
        _, _, void, _ = V.expand(rec, dda, 320)
        assert (~void[:, X]).any() and (~void[:, XX]).any()


# ---- reduce ----------------------------------------------------------------------------------------------------------------------
def test_reduce_equals_the_restatement_on_scripted_tables():
    """Final tables from a pool of finished auctions (no network).  The other table's scores are set so that the played slots'
    differences sit on and just below every step of the IMP scale, in both signs; callers of every seat; decisions with one legal
    alternative, with 38, with live and with void slots; twice, with the roles of the two tables exchanged."""
    from brl_amd import review
    rng = np.random.default_rng(77)
    pool = []
    while len(pool) < 160:
        calls = R.random_auction(rng, p_pass=float(rng.uniform(0.3, 0.6)))
        pool.append(R.encode(int(rng.integers(0, 4)), calls, vul_ns=int(rng.integers(0, 2)), vul_ew=int(rng.integers(0, 2)),
                             seating=SEATINGS[len(pool) & 3], tricks=rng.integers(0, 14, size=(4, 5))))
    pool.append(R.encode(0, [P, P, P, P]))
    n_done = len(pool)
    pool.append(R.encode(1, [3 + 7, P, X]))                      # void: ended by an illegal call
    pool.append(R.encode(2, [3 + 7, P]))                         # live: no result
    pool_packed = np.stack([t.pack() for t in pool])
    pool_rec = R.decode(pool_packed)
    assert len(set(pool_rec["score_ns"][:n_done].tolist())) > 30
    nb, nd = 100, 257
    targets = [0] + [s * k - off for k in V.STEPS for s in (1, -1) for off in (0, 10 * s)]      # 97 differences
    pick = np.zeros((nd, 38), np.int64)
    decisions = []
    for d in range(nd):
        n_legal = 1 if d % 50 == 7 else 38 if d % 50 == 9 else int(rng.integers(2, 38))
        legal = np.sort(rng.choice(38, size=n_legal, replace=False))
        pick[d] = n_done + (rng.random(38) < 0.2)                # void or live
        pick[d, legal] = rng.integers(0, n_done, size=n_legal) if d % 7 else int(rng.integers(0, n_done))     # (d % 7 == 0: all tie)
        decisions.append((d % nb, int(rng.integers(0, 12)), int(rng.integers(0, 4)), int(rng.integers(0, 2)), int(legal[rng.integers(0, n_legal)])))
    other = np.zeros(nb, pool_rec.dtype)
    other["score_ns"] = rng.integers(-200, 200, size=nb) * 10
    for b, diff in enumerate(targets):                           # decision b is the first on board b
        other["score_ns"][b] = int(pool_rec["score_ns"][pick[b, decisions[b][4]]]) - diff
    dec = np.zeros(nd, review.DECISION_DTYPE)
    for k, name in enumerate(("board", "call_index", "seat", "team", "played")):
        dec[name] = [x[k] for x in decisions]
    tables = torch.from_numpy(pool_packed[pick.reshape(-1)].view(np.int64)).to(DEV)
    dec_dev = torch.from_numpy(dec.view(np.uint8).reshape(nd, 16)).to(DEV)
    final = pool_rec[pick.reshape(-1)]
    for flip in (1, -1):                                         # the other table's scores, then their negatives
        oth = other.copy()
        oth["score_ns"] *= flip
        values, summary = review.reduce(tables, dec_dev, torch.from_numpy(oth.view(np.uint8).reshape(nb, 368)).to(DEV))
        values = values.cpu().numpy()
        summ = summary.cpu().numpy().view(review.SUMMARY_DTYPE).reshape(-1)
        want = V.values(final, decisions, oth)
        assert np.array_equal(values, want)
        ws = V.summaries(want, decisions)
        for k in ("played", "n_legal", "played_imp", "best_imp", "best", "loss"):
            assert np.array_equal(summ[k].astype(np.int64), ws[k]), k
        assert not summ["zero"].any() and (ws["loss"] >= 0).all()
        if flip == 1:
            first = np.array([want[b, decisions[b][4]] for b in range(len(targets))]).astype(np.int64)
            sign = np.array([1 if decisions[b][2] % 2 == 0 else -1 for b in range(len(targets))])
            assert sorted(set((first * sign).tolist())) == list(range(-24, 25))          # every step of the scale, both signs
            assert {1, 38} <= set(ws["n_legal"].tolist()) and (ws["loss"] > 0).any() and (ws["loss"] == 0).any()
            assert ((ws["best"] != ws["played"]) & (ws["loss"] > 0)).any() and (want == V.VOID).any()
    assert {x[2] for x in decisions} == {0, 1, 2, 3}


# ---- end to end --------------------------------------------------------------------------------------------------------------------
DEPTH = 12


@pytest.fixture(scope="module")
def match(dds, oracle):
    """the 64-board match of the bidder pair and its review (depth 12, both tables, branch records on), computed once"""
    import brl_amd
    from brl_amd import boards, review
    nets = bn.pair(DEV)
    env = brl_amd.BridgeBidding(lut=(dds["keys"], dds["values"]), device=DEV)
    hand = np.stack([oracle.key_to_hand(k) for k in dds["keys"][:64]])
    deals = boards.Deals(np.sort(hand.reshape(-1, 4, 13), axis=2).reshape(-1, 52).astype(np.int32), dds["dealer"][:64], dds["vul_ns"][:64],
                         dds["vul_ew"][:64], dds["tricks"][:64].reshape(-1, 20), dds["board_id"][:64])
    _, records = boards.make_board_match(env, "relu", "DeepMind", "relu", "DeepMind")(nets[0], nets[1], deals)
    branch = []
    rv = review.make_call_review(env, "relu", "DeepMind", "relu", "DeepMind", depth=DEPTH)(nets[0], nets[1], records, record=branch)
    torch.cuda.synchronize()
    return dict(env=env, nets=nets, records=records, review=rv, branch=np.concatenate(branch))


def _oracle_tables(oracle, rec, dda):
    from brl_amd import boards
    n = rec.shape[0]
    hand = np.zeros((n, 52), np.int32)
    for s in range(4):
        b = (rec["hands"][:, s][:, None] >> np.arange(52, dtype=np.uint64)[None, :]) & np.uint64(1)
        hand[:, s * 13:(s + 1) * 13] = np.sort(boards._bit_to_pgx(np.nonzero(b)[1].reshape(n, 13)), axis=1)
    shuf = np.stack([(rec["seating"] >> (2 * s)) & 3 for s in range(4)], axis=1).astype(np.int32)
    return oracle.init_explicit(hand, rec["dealer"].astype(np.int32), rec["vul_ns"], rec["vul_ew"], shuf, dda)


def _replay64(oracle, nets, rec, dda, first_checked):
    """Replays every record's calls through the oracle from its own deal.  Every call must be legal; for the calls of index >=
    first_checked[i] the float64 logits of the network to act are formed on the oracle's observation.
    -> (final oracle tables, North-South scores, per record and call index: the call's logit below the largest legal one, the gap
    between the two largest legal logits, both in units of that forward's tol = _tol32)"""
    n = rec.shape[0]
    o = _oracle_tables(oracle, rec, dda)
    score = np.zeros(n, np.int64)
    width = int(rec["n_calls"].max())
    below, gap = np.full((n, width), -np.inf), np.full((n, width), np.inf)
    for k in range(width):
        live = np.nonzero(rec["n_calls"] > k)[0]
        sub = o[live]
        a = rec["calls"][live, k].astype(np.int64)
        assert not sub["terminated"].any(), "a call after the end"
        assert (sub["legal_action_mask"][np.arange(len(live)), a] == 1).all(), f"call {k}: not legal"
        for team, net in enumerate(nets):
            rows = np.nonzero(((sub["current_player"] >> 1) == team) & (k >= first_checked[live]))[0]
            if not len(rows):
                continue
            ref = forward64(net, torch.from_numpy(sub["observation"][rows]).to(DEV))[:, :38]
            tol = _tol32(ref)
            lg = np.where(sub["legal_action_mask"][rows] == 1, ref.cpu().numpy(), -np.inf)
            top = np.sort(lg, axis=1)
            below[live[rows], k] = (top[:, -1] - lg[np.arange(len(rows)), a[rows]]) / tol
            gap[live[rows], k] = (top[:, -1] - top[:, -2]) / tol
        oracle.step(sub, a.astype(np.int32))
        assert not sub["illegal"].any()
        ended = sub["terminated"] != 0
        score[live[ended]] = sub["rewards"][np.arange(len(live)), sub["shuffled_players"][:, 0]][ended].astype(np.int64)
        o[live] = sub
    return o, score, below, gap


def _decisions_by_definition(records, rv):
    """(board, t, seat, team, played) of every decision, from the records and the header's definitions"""
    out = []
    for tb, name in enumerate("ab"):
        rec = records.cpu(name)
        for i, r in enumerate(rec):
            for t in range(min(int(r["n_calls"]), DEPTH)):
                seat = (int(r["dealer"]) + t) & 3
                out.append((i, t, seat, ((int(r["seating"]) >> (2 * seat)) & 3) >> 1, int(r["calls"][t])))
    return out


def _check_review(oracle, records, rv, branch, nets):
    """(i) - (iv) of a review against its branch records; -> the number of branches played"""
    from brl_amd import boards
    dda = records.dda.cpu().numpy()
    decisions = _decisions_by_definition(records, rv)
    D = len(decisions)
    assert len(rv) == D and branch.shape == (D * 38,) and rv.skipped == {"a": 0, "b": 0}
    n_a = int((rv.table == 0).sum())
    assert rv.table.tolist() == [0] * n_a + [1] * (D - n_a)
    got = list(zip(rv.board.tolist(), rv.call_index.tolist(), rv.seat.tolist(), rv.team.tolist(), rv.played.tolist()))
    assert got == decisions
    # the void pattern: Table.legal at the prefix
    for d, (i, t, seat, team, played) in enumerate(decisions):
        r = records.cpu("ab"[int(rv.table[d])])[i]
        prefix = R.encode(int(r["dealer"]), [int(c) for c in r["calls"][:t]])
        assert [rv.imp[d, a] != V.VOID for a in range(38)] == [prefix.legal(a) for a in range(38)], d
    d_of, a_of = np.nonzero(rv.imp != V.VOID)
    slots = d_of * 38 + a_of
    br = branch[slots]
    assert ((br["flags"] & boards.OK) != 0).all() and ((br["flags"] & boards.TERMINATED) != 0).all() and ((br["flags"] & boards.ILLEGAL) == 0).all()
    void = branch[np.setdiff1d(np.arange(D * 38), slots)]
    assert ((void["flags"] & boards.ILLEGAL) != 0).all()
    # (i) the recorded prefix, then the alternative
    t_of = rv.call_index[d_of].astype(np.int64)
    for d, a, t, b in zip(d_of, a_of, t_of, br):
        r = records.cpu("ab"[int(rv.table[d])])[rv.board[d]]
        assert b["n_calls"] > t and np.array_equal(b["calls"][:t], r["calls"][:t]) and b["calls"][t] == a, (d, a)
    for name in ("hands", "dealer", "vul_ns", "vul_ew", "seating"):
        for tb, tname in enumerate("ab"):
            sel = rv.table[d_of] == tb
            assert np.array_equal(br[name][sel], records.cpu(tname)[name][rv.board[d_of][sel]]), name
    # (ii) the auction replays through the oracle from the deal, ends, and scores the same; (iii) every continuation call is a
    # maximum of the float64 logits within 2 tol
    o, score, below, _ = _replay64(oracle, nets, br, dda[rv.board[d_of]], t_of + 1)
    assert (o["terminated"] != 0).all() and np.array_equal(score, br["score_ns"].astype(np.int64))
    checked = np.isfinite(below)
    print(f"continuation calls checked: {int(checked.sum())}, per branch {checked.sum() / len(br):.2f}, at most {int(checked.sum(1).max())}; "
          f"largest distance below the best legal logit: {below[checked].max():.3f} tol")
    assert checked.sum() == (br["n_calls"].astype(np.int64) - t_of - 1).sum() and below[checked].max() <= 2.0
    # (iv) values and summaries are the restatement's, from the branch records and the other table's records
    want = np.concatenate([V.values(branch[:n_a * 38], decisions[:n_a], records.cpu("b")),
                           V.values(branch[n_a * 38:], decisions[n_a:], records.cpu("a"))])
    assert np.array_equal(rv.imp, want)
    ws = V.summaries(want, decisions)
    for k in ("played", "n_legal", "played_imp", "best_imp", "best", "loss"):
        assert np.array_equal(getattr(rv, k).astype(np.int64), ws[k]), k
    assert np.array_equal(rv.board_id, records.board_id[rv.board])
    return len(br), int((br["n_calls"].astype(np.int64) - t_of - 1 > 0).sum())


def test_every_branch_replays_and_every_value_is_the_restatements(oracle, match):
    rv = match["review"]
    branches, played = _check_review(oracle, match["records"], rv, match["branch"], match["nets"])
    lost, none = int((rv.loss > 0).sum()), int((rv.loss == 0).sum())
    print(f"decisions {len(rv)}, branches {branches} ({branches / len(rv):.1f} legal alternatives per decision), continued past the "
          f"alternative {played}; decisions with loss > 0: {lost}, with loss == 0: {none}")
    for line in rv.stats_lines():
        print(line)
    assert branches > 10000 and 5 * lost >= len(rv) and none >= 1          # not vacuous


def test_the_played_calls_branch_is_the_match_itself(oracle, match):
    """Per decision: the branch of the call made either holds the recorded auction — and then its value is the board's recorded IMP
    with the caller's sign — or the float64 forward shows a decision of the recorded auction behind t whose two best legal logits
    are closer than 2 tol.  No other exception."""
    records, rv, branch = match["records"], match["review"], match["branch"]
    dda = records.dda.cpu().numpy()
    imp = records.imp.cpu().numpy().astype(np.int64)
    gaps = {}
    for name in "ab":
        rec = records.cpu(name)
        _, score, _, gap = _replay64(oracle, match["nets"], rec, dda, np.zeros(len(rec), np.int64))
        assert np.array_equal(score, rec["score_ns"].astype(np.int64))
        gaps[name] = gap
    same = near = 0
    for d in range(len(rv)):
        name, i, t = "ab"[int(rv.table[d])], int(rv.board[d]), int(rv.call_index[d])
        r, b = records.cpu(name)[i], branch[d * 38 + int(rv.played[d])]
        if b["n_calls"] == r["n_calls"] and np.array_equal(b["calls"], r["calls"]):
            ns = imp[i] if name == "a" else -imp[i]
            assert rv.played_imp[d] == (ns if rv.seat[d] % 2 == 0 else -ns), d
            same += 1
        else:
            assert (gaps[name][i, t + 1:int(r["n_calls"])] < 2.0).any(), (d, name, i, t)
            near += 1
    print(f"played-call branches equal to the recorded auction: {same}; explained by a near tie of the float64 logits: {near}")
    assert same > 0


def test_the_result_does_not_depend_on_the_chunking(match):
    from brl_amd import review
    branch = []
    small = review.make_call_review(match["env"], "relu", "DeepMind", "relu", "DeepMind", depth=DEPTH, max_branches=4096)(
        match["nets"][0], match["nets"][1], match["records"], record=branch)
    assert len(match["review"]) * 38 > 5 * 4096                       # several chunks per table
    assert small.same_as(match["review"])
    assert np.concatenate(branch).tobytes() == match["branch"].tobytes()


def test_one_network_on_both_sides(oracle, match, monkeypatch):
    from brl_amd import evaluation, review
    made = []
    real = evaluation._Forward

    class Counting(real):
        def __init__(self, *a):
            made.append(1)
            super().__init__(*a)

    monkeypatch.setattr(evaluation, "_Forward", Counting)
    net = match["nets"][0]
    branch = []
    rv = review.make_call_review(match["env"], "relu", "DeepMind", "relu", "DeepMind", depth=DEPTH)(net, net, match["records"], record=branch)
    assert len(made) == 1
    _check_review(oracle, match["records"], rv, np.concatenate(branch), (net, net))
    only_a = review.make_call_review(match["env"], "relu", "DeepMind", "relu", "DeepMind", depth=DEPTH)(net, net, match["records"], tables="a")
    n_a = int((rv.table == 0).sum())
    assert len(only_a) == n_a and np.array_equal(only_a.imp, rv.imp[:n_a]) and only_a.skipped == {"a": 0}


def test_records_that_cannot_be_reviewed_are_refused_or_skipped(match):
    from brl_amd import boards, review
    call_review = review.make_call_review(match["env"], "relu", "DeepMind", "relu", "DeepMind", depth=2)
    records, nets = match["records"], match["nets"]
    with pytest.raises(ValueError, match="dda"):
        call_review(nets[0], nets[1], boards.BoardRecords(records.table_a, records.table_b, records.imp))
    with pytest.raises(ValueError, match="table B"):
        call_review(nets[0], nets[1], boards.BoardRecords(records.table_a, None, None, records.dda))
    raw = records.table_a.clone()
    raw[3, boards.RECORD_DTYPE.fields["flags"][1]] &= 0xFF ^ boards.OK
    rv = call_review(nets[0], nets[1], boards.BoardRecords(raw, records.table_b, records.imp, records.dda), tables="a")
    assert rv.skipped == {"a": 1} and 3 not in rv.board and len(rv) == 2 * 63 and rv.board_id.tolist() == rv.board.tolist()


def test_the_command_line_reviews_a_match(tmp_path):
    from brl_amd import checkpoint, review
    from brl_amd.models import make_forward_pass
    fp = make_forward_pass("relu", "DeepMind")
    for k in range(2):
        checkpoint.save_params(fp.init(60 + k), str(tmp_path / f"params-{k:08}.pt"))
    envv = dict(os.environ, PYTHONPATH=ROOT)
    base = [sys.executable, "-m", "brl_amd.eval", f"team1_model_path={tmp_path / 'params-00000000.pt'}",
            f"team2_model_path={tmp_path / 'params-00000001.pt'}", f"deals_path={NAMED}"]
    out = []
    for extra in ([], ["review=1", "review_depth=6", f"save_review={tmp_path / 'review.json'}"]):
        r = subprocess.run(base + extra, cwd=tmp_path, env=envv, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        out.append(r.stdout.splitlines())
    plain, reviewed = out
    lines = [ln for ln in reviewed if ln.startswith("review")]
    assert [ln.split(":")[0] for ln in lines] == ["review team1", "review team2", "review"]
    assert reviewed.index(lines[0]) == [i for i, ln in enumerate(reviewed) if ln.startswith("IMP: ")][-1] + 1
    assert not any(ln.startswith("review") for ln in plain) and plain == [ln for ln in reviewed if not ln.startswith("review")]
    back = review.CallReview.from_json(tmp_path / "review.json")
    assert back.depth == 6 and len(back) > 24 * 2 * 3 and back.stats_lines() == lines[:2] and set(back.board.tolist()) == set(range(24))
