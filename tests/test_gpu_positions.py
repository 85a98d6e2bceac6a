"""-m gpu: the position queries (brl_amd/positions.py, include/brl_positions.h) — brl_position_rows against brl_observe on the real
deals of a recorded match (the proof that the fill of the hidden hands does not reach the rows) and against the restatement
(tests/positions_ref.py) on scripted auctions and on bad input; brl_position_answers against the float64 restatement; the whole
path on the match's own networks, which must call what they played; both entry points under tests/guarded.py's guards."""
import copy
import json
import os

import numpy as np
import pytest
import torch

from tests import bidder_net as bn
from tests import nonfinite_cases as nf
from tests import positions_ref as P
from tests.guarded import both
from tests.test_gpu_compare import C_DIV, EPS      # what the device's exp / log may differ from numpy's by (tests/test_gpu_compare.py)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMED = os.path.join(ROOT, "tests", "golden", "wb5_named_24.json")
QUIZ = os.path.join(ROOT, "tests", "golden", "bidding_quiz_12.json")
BRL_E_ARG = -1
U8, I32, I64, F32, F64 = torch.uint8, torch.int32, torch.int64, torch.float32, torch.float64


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _rows(arr, tables=True):
    """brl_position_rows on packed records -> (status uint32, obs uint8 [n,480], mask uint8 [n,38], legal uint64, tables uint64 [n,16])"""
    from brl_amd import positions as M
    obs, mask, legal, status, tb = M.position_rows(_dev(arr.view(np.uint8).reshape(-1, 64)), tables=tables)
    torch.cuda.synchronize()
    return (status.cpu().numpy().view(np.uint32), obs.cpu().numpy().view(np.uint8), mask.cpu().numpy(), legal.cpu().numpy().view(np.uint64),
            tb.cpu().numpy().view(np.uint64) if tables else None)


def _answers(logits, legal, top_k, status=None, value=None, probs=True):
    """brl_position_answers -> (ANSWER_DTYPE [n], probs float64 [n,38] or None)"""
    from brl_amd import positions as M
    n = len(legal)
    lg = logits if isinstance(logits, torch.Tensor) else _dev(logits)
    st = _dev((np.zeros(n, np.uint32) if status is None else np.asarray(status, np.uint32)).view(np.int32))
    ans = torch.full((n, 96), 0xAB, dtype=U8, device=DEV)
    pr = torch.full((n, 38), -7.0, dtype=F64, device=DEV) if probs else None
    M.position_answers(lg, None if value is None else _dev(value), _dev(np.asarray(legal, np.uint64).view(np.int64)), st, top_k, ans, pr)
    torch.cuda.synchronize()
    return ans.cpu().numpy().view(M.ANSWER_DTYPE).reshape(-1), (pr.cpu().numpy() if probs else None)


def _check_answers(got, probs, want, what):
    """a device answer against the restatement's: the integer fields exactly, the float64 fields within C_DIV x 2^-52 of the sum
    of the magnitudes of their terms (a probability is its own single term); -> the worst ratio"""
    for name in ("call", "n_legal", "flags", "k", "top_action"):
        assert np.array_equal(got[name], want[name]), (what, name, np.nonzero((got[name] != want[name]).reshape(len(got), -1).any(1))[0][:5])
    assert not got["reserved"].any(), what
    worst = 0.0
    for g, w, scale in ((got["entropy"], want["entropy"], want["entropy_scale"]), (got["top_prob"], want["top_prob"], want["top_prob"]),
                        (probs, want["probs"], want["probs"])):
        if g is None:
            continue
        nan = np.isnan(w)
        assert np.array_equal(np.isnan(g), nan), what
        zero = ~nan & (np.nan_to_num(scale) == 0)
        assert (g[zero] == 0).all() and not np.signbit(g[zero]).any(), what                  # nothing to add up: exactly +0.0
        some = ~nan & ~zero
        if some.any():
            worst = max(worst, float((np.abs(g[some] - w[some]) / (EPS * scale[some])).max()))
    assert worst <= C_DIV, (what, worst)
    return worst


# ---- the match ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def match(dds):
    """the 24 named boards played by the bidder pair at both tables; every decision as a position, and its rows by brl_observe on
    the table rebuilt from the real four hands and stepped with brl_step (as compare.py rebuilds it) — computed once, read only"""
    import brl_amd
    from brl_amd import _capi, boards, compare, positions as M
    nets = bn.pair(DEV)
    env = brl_amd.BridgeBidding(lut=(dds["keys"], dds["values"]), device=DEV)
    deals = boards.read_deals(NAMED)
    _, records = boards.make_board_match(env, "relu", "DeepMind", "relu", "DeepMind")(nets[0], nets[1], deals)
    L = _capi.lib()
    arrs, obs_all, mask_all, team_all, played_all = [], [], [], [], []
    for tb in "ab":
        rec = records.cpu(tb)
        arr, index = M.positions_from_records(records, tb)
        assert len(arr) == int(rec["n_calls"].sum()) and int(rec["n_calls"].max()) <= 48
        where = {(int(i), int(t)): j for j, (i, t) in enumerate(index)}
        obs_t, mask_t = np.zeros((len(arr), 480), np.uint8), np.zeros((len(arr), 38), np.uint8)
        rec_dev = _dev(rec.view(np.uint8).reshape(-1, 368))
        tables, _ = compare.compare_tables(rec_dev, torch.arange(len(rec), device=DEV))
        for t in range(int(rec["n_calls"].max())):
            o = torch.empty((len(rec), 480), dtype=torch.bool, device=DEV)
            m = torch.empty((len(rec), 38), dtype=U8, device=DEV)
            _capi.check(L.brl_observe(env._h, _capi.ptr(tables), len(rec), None, _capi.ptr(o), _capi.ptr(m), _capi.stream()))
            o, m = o.cpu().numpy().view(np.uint8), m.cpu().numpy()
            for i in np.nonzero(rec["n_calls"] > t)[0]:
                obs_t[where[(int(i), t)]], mask_t[where[(int(i), t)]] = o[i], m[i]
            calls = _dev(np.where(rec["n_calls"] > t, rec["calls"][:, t], 0).astype(np.int32))     # (a finished table takes a no-op call)
            _capi.check(L.brl_step(env._h, _capi.ptr(tables), _capi.ptr(tables), len(rec), _capi.ptr(calls), 0, None, None, None, None, None,
                                   _capi.stream()))
        seat = (rec["dealer"][index[:, 0]].astype(np.int64) + index[:, 1]) & 3
        arrs.append(arr), obs_all.append(obs_t), mask_all.append(mask_t)
        team_all.append(((rec["seating"][index[:, 0]].astype(np.int64) >> (2 * seat)) & 3) >> 1)
        played_all.append(rec["calls"][index[:, 0], index[:, 1]])
    torch.cuda.synchronize()
    return dict(env=env, nets=nets, records=records, arr=np.concatenate(arrs), obs=np.concatenate(obs_all), mask=np.concatenate(mask_all),
                team=np.concatenate(team_all), played=np.concatenate(played_all))


@pytest.mark.parametrize("n", [1, 63, 64, 65, None])
def test_rows_equal_brl_observe_on_the_real_deal(match, n):
    """the kernel's table holds other hidden hands than the deal's: equal rows are the proof that the fill does not leak.  And
    brl_observe on the kernel's own tables gives the same rows.  One position, a wave less one, a wave, a wave and one, all."""
    from brl_amd import _capi
    arr = match["arr"] if n is None else match["arr"][7:7 + n]
    want_obs, want_mask = (match["obs"], match["mask"]) if n is None else (match["obs"][7:7 + n], match["mask"][7:7 + n])
    assert len(arr) == (n or len(arr)) and len(match["arr"]) > 200
    st, obs, mask, legal, tables = _rows(arr)
    assert (st == P.OK).all()
    assert np.array_equal(obs, want_obs) and np.array_equal(mask, want_mask)
    assert np.array_equal(legal, (mask.astype(np.uint64) << np.arange(38, dtype=np.uint64)).sum(1))
    # the tables: the header's fill, not the deal — and brl_observe reads the same rows off them
    for j in (0, len(arr) - 1):
        seat = (int(arr["dealer"][j]) + int(arr["n_calls"][j])) & 3
        assert [int(w) >> 4 for w in tables[j, 7:11]] == P.fill_hands(int(arr["hand"][j]), seat) and int(tables[j, 14]) & 0xFFFFFFFF == 0xFFFFFFFF
    o = torch.empty((len(arr), 480), dtype=torch.bool, device=DEV)
    m = torch.empty((len(arr), 38), dtype=U8, device=DEV)
    tb = _dev(tables.view(np.int64))
    _capi.check(_capi.lib().brl_observe(match["env"]._h, _capi.ptr(tb), len(arr), None, _capi.ptr(o), _capi.ptr(m), _capi.stream()))
    assert np.array_equal(o.cpu().numpy().view(np.uint8), obs) and np.array_equal(m.cpu().numpy(), mask)
    without = _rows(arr, tables=False)
    assert all(np.array_equal(a, b) for a, b in zip(without[:4], (st, obs, mask, legal)))


# ---- scripted auctions and bad input ------------------------------------------------------------------------------------------------
def test_scripted_auctions_equal_the_restatement():
    """no call for every dealer x vulnerability, three passes, every double / redouble transition, 7NT, 48 calls; then lengths 0
    and 48 alternating in one wave"""
    names, rec = P.scripted_records()
    for arr in (rec, np.stack([rec[0], rec[names.index("48 calls")]] * 32).reshape(-1)):
        want = P.rows(arr)
        st, obs, mask, legal, tables = _rows(arr)
        assert np.array_equal(st, want[0]) and (st == P.OK).all()
        for i in range(len(arr)):
            assert np.array_equal(obs[i], want[1][i]) and np.array_equal(mask[i], want[2][i]), (names[i] if len(arr) == len(names) else i)
        assert np.array_equal(legal, want[3])
    assert len(arr) == 64 and set(arr["n_calls"]) == {0, 48}


def _bad_batch():
    """64 positions, every fourth one a bad one of its own kind; -> (records, {row: what})"""
    rng = np.random.default_rng(9)
    good = list(P.SCRIPTED.values())
    arr = np.array([P.pack(P.random_hand(rng), i % 4, i & 1, (i >> 1) & 1, good[i % len(good)]) for i in range(64)], P.DTYPE)
    kinds = {}
    bad = [("12 cards", dict(hand=P.random_hand(rng, 12))), ("14 cards", dict(hand=P.random_hand(rng, 14))),
           ("a bit at 52", dict(hand=P.random_hand(rng) | (1 << 52))), ("a bit at 63", dict(hand=P.random_hand(rng, 12) | (1 << 63))),
           ("dealer 4", dict(dealer=4)), ("vul_ns 2", dict(vul_ns=2)), ("vul_ew 2", dict(vul_ew=2)), ("reserved", dict(reserved=1 << 31)),
           ("fill 0", dict(calls=[3, 0], fill=0)), ("n_calls 49", dict(calls=[0], n_calls=49, fill=0)), ("a call above 37", dict(calls=[3, 38])),
           ("n_calls 200 over a full array", dict(calls=P.LONG, n_calls=200))]
    bad += [(name, dict(calls=calls)) for name, (calls, _) in P.BAD.items()]
    assert len(bad) <= 32
    for k, (name, kw) in enumerate(bad):
        args = dict(dict(hand=P.random_hand(rng), dealer=k % 4, vul_ns=0, vul_ew=1, calls=[]), **kw)
        arr[2 * k + 1] = P.pack(**args)
        kinds[2 * k + 1] = name
    return arr, kinds


def test_status_of_bad_positions_and_their_neighbours():
    arr, kinds = _bad_batch()
    want = P.rows(arr)
    st, obs, mask, legal, tables = _rows(arr)
    for i, name in kinds.items():
        assert st[i] == want[0][i] and st[i] & 0xFF != P.OK, (name, hex(st[i]), hex(want[0][i]))
        if name in P.BAD:
            assert st[i] == P.BAD[name][1], name                                                     # the code and the index
        assert not obs[i].any() and not mask[i].any() and legal[i] == 0 and not tables[i].any(), name     # nothing but zeros
    assert {int(st[i]) & 0xFF for i in kinds} == {P.BAD_HEADER, P.BAD_HAND, P.ILLEGAL_CALL, P.FINISHED}
    good = [i for i in range(64) if i not in kinds]
    assert (st[good] == P.OK).all() and np.array_equal(obs[good], want[1][good]) and np.array_equal(legal, want[3])
    for i in good + list(kinds):                 # every row of the wave is what it is alone
        alone = _rows(arr[i:i + 1])
        for a, b in zip(alone, (st, obs, mask, legal, tables)):
            assert np.array_equal(a[0], b[i]), (i, kinds.get(i))


# ---- the answers --------------------------------------------------------------------------------------------------------------------
def _legal_words(rng, m):
    """legal words of real shape: pass, at most one of X / XX, the bids above a level; some with one or two legal actions only"""
    out = np.zeros(m, np.uint64)
    for i in range(m):
        lb = int(rng.integers(0, 36))
        w = 1 | (((1 << 38) - 1) >> (3 + lb) << (3 + lb)) | (int(rng.integers(0, 3)) << 1 if lb else 0) & 6
        out[i] = (1, 3, 1 | 1 << 37)[i % 3] if i % 11 == 0 else w
    return out


@pytest.mark.parametrize("ld", [38, 39])
@pytest.mark.parametrize("top_k", [1, 3, 8])
def test_answers_equal_the_float64_restatement(ld, top_k):
    """random logits; exact ties (bit-equal logits) everywhere, among the best, and across the top_k boundary; legal -inf logits;
    all-equal rows; fewer legal actions than top_k; one row more than a block of 32 and a partial wave; bad-status rows between"""
    rng = np.random.default_rng(100 * ld + top_k)
    m = 32 * 3 + 5
    legal = _legal_words(rng, m)
    lg = (rng.normal(size=(m, ld)) * 4).astype(np.float32)
    for i in range(m):
        acts = [a for a in range(38) if (int(legal[i]) >> a) & 1]
        kind = i % 8
        if kind == 1:
            lg[i, :38] = 1.5                                             # all equal: ranks by index
        elif kind == 2 and len(acts) > top_k:
            lg[i, acts] = np.linspace(-1, 1, len(acts)).astype(np.float32)
            lg[i, acts[:top_k + 1]] = 7.0                                # a tie that straddles the top_k boundary
        elif kind == 3 and len(acts) > 2:
            lg[i, acts[-1]] = lg[i, acts[0]] = 30.0                      # the two best tied, far apart in index
        elif kind == 4 and len(acts) > 2:
            lg[i, acts[1:3]] = -np.inf                                   # legal actions of probability zero
        elif kind == 5:
            lg[i, :38] = -1e30
            lg[i, 0] = 0.0                                               # _PassOnly's constants
        elif kind == 6:
            lg[i, [a for a in range(38) if a not in acts]] = 1e30        # huge illegal logits count for nothing
    status = np.zeros(m, np.uint32)
    status[[3, 40, m - 1]] = [P.BAD_HAND, P.ILLEGAL_CALL | (2 << 8), P.FINISHED | (5 << 8)]
    value = rng.normal(size=m).astype(np.float32)
    got, probs = _answers(lg, legal, top_k, status, value)
    want = P.answer(lg, legal, top_k, status)
    worst = _check_answers(got, probs, want, (ld, top_k))
    dead = (status & 0xFF) != 0
    assert np.array_equal(got["value"], np.where(dead, 0, value).astype(np.float32)) and (got["call"][dead] == 255).all()
    assert not got[dead].view(np.uint8).reshape(-1, 96)[:, 1:].any() and not probs[dead].any()      # all zero but the call
    live = ~dead
    assert not (got["flags"] & P.NONFINITE).any() and (got["n_legal"][live] < top_k).any() == (top_k > 1) and (got["k"][live] >= 1).all()
    assert np.allclose(probs[live].sum(1), 1.0, atol=1e-12) and (got["top_prob"][live, 0] == probs[live].max(1)).all()
    assert (got["call"][live] == got["top_action"][live, 0]).all()                                  # the arg-max is rank 0, ties by index
    without, none = _answers(lg, legal, top_k, status, None, probs=False)
    assert none is None and not without["value"].any()
    for name in ("call", "entropy", "top_action", "top_prob"):
        assert without[name].tobytes() == got[name].tobytes(), name
    print(f"answers ld={ld} top_k={top_k}: worst |device - restatement| = {worst:.2f} x 2^-52 x the terms' magnitudes (C = {C_DIV})")


def test_answers_on_non_finite_rows():
    """the rows of tests/nonfinite_cases.py: a NaN on a legal action, a NaN on an illegal one (which changes nothing), +inf on a
    legal action, no legal logit above -inf, -inf on some legal actions only (finite)"""
    b = nf.loss_batch(16, seed=3)
    legal = (b["mask"].astype(np.uint64) << np.arange(38, dtype=np.uint64)).sum(1)
    lg = b["logits"].copy()
    for i in (1, 5):
        lg[i] = nf.poisoned(b, "nan_legal_logit", i)["logits"][i]
    for i in (2, 6):
        lg[i] = nf.poisoned(b, "nan_illegal_logit", i)["logits"][i]
    acts = lambda i: np.flatnonzero(b["mask"][i])     # noqa: E731
    lg[8, acts(8)[-1]] = np.inf
    lg[9, acts(9)] = -np.inf
    lg[10, acts(10)[1:]] = -np.inf
    lg[11, acts(11)[0]] = np.nan                      # the NaN on the first legal action: never the maximum
    got, probs = _answers(lg, legal, 3)
    want = P.answer(lg, legal, 3)
    _check_answers(got, probs, want, "non-finite")
    bad = (got["flags"] & P.NONFINITE) != 0
    assert np.flatnonzero(bad).tolist() == [1, 5, 8, 9, 11]
    assert np.isnan(got["entropy"][bad]).all() and np.isnan(got["top_prob"][bad]).all() and np.isnan(probs[bad]).all()
    assert (got["top_action"][bad] == 255).all() and (got["k"][bad] == 0).all() and got["call"][9] == 0 and got["call"][8] == acts(8)[-1]
    assert got["call"][11] != acts(11)[0] and got["k"][10] == 3 and got["top_prob"][10, 0] == 1.0 and got["entropy"][10] == 0.0
    clean, _ = _answers(b["logits"], legal, 3)
    assert clean[[2, 6]].tobytes() == got[[2, 6]].tobytes()


def test_answers_on_the_bidder_networks_logits(match):
    """the logits the bidder network gives the match's positions (near-deterministic rows: entropies near zero)"""
    from brl_amd import positions as M
    arr = match["arr"]
    with torch.no_grad():
        obs, _, legal, status, _ = M.position_rows(_dev(arr.view(np.uint8).reshape(-1, 64)))
        out = match["nets"][0](obs.to(F32))
        lg = torch.cat([out[0], out[1].reshape(-1, 1)], dim=1).contiguous()
    got, probs = _answers(lg, legal.cpu().numpy().view(np.uint64), 3, value=out[1].reshape(-1).cpu().numpy())
    want = P.answer(lg.cpu().numpy(), legal.cpu().numpy().view(np.uint64), 3)
    worst = _check_answers(got, probs, want, "bidder")
    assert np.array_equal(got["value"], lg[:, 38].cpu().numpy()) and (got["entropy"] >= 0).all()
    print(f"bidder logits: {len(arr)} positions, worst ratio {worst:.2f}, mean entropy {got['entropy'].mean():.3f} nats")


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
ROUTES = {  # name: (environment, rows asked at once: the set itself, or tiled to at least that many)
    "library": ({}, None), "library_no_views": ({"BRL_SNAPSHOT_VIEWS": "0"}, None), "library_forced": ({"BRL_INFERENCE_GEMM": "library"}, 4096),
    "planes": ({"BRL_INFERENCE_PLANES": "1"}, 4096), "x3": ({"BRL_INFERENCE_PLANES": "0"}, 4096),
}


@pytest.mark.parametrize("route", list(ROUTES))
def test_the_networks_call_what_they_played(match, route, monkeypatch):
    """each team's network asked its own decisions of the match: the call is the recorded one at EVERY decision when the positions
    are asked as they are (the match was played by the same networks' masked arg-max).  Tiled to 4096 rows and more the forward
    runs on the bf16x3 kernels, whose logits differ in the last bits from those the match was played with: there the decisions
    whose two best legal logits lie within 1e-3 of each other in the host forward are left out, as tests/test_gpu_compare.py leaves
    them out, and at most 1 % may be."""
    from brl_amd import boards, evaluation, positions as M
    from brl_amd.models import make_forward_pass
    env_vars, rows = ROUTES[route]
    for name in ("BRL_INFERENCE_GEMM", "BRL_INFERENCE_PLANES", "BRL_SNAPSHOT_VIEWS"):
        monkeypatch.delenv(name, raising=False)
    for name, v in env_vars.items():
        monkeypatch.setenv(name, v)
    ask = M.make_bidder("relu", "DeepMind", top_k=3)
    total = out = 0
    for team in (0, 1):
        sel = np.nonzero(match["team"] == team)[0]
        reps = 1 if rows is None else -(-rows // len(sel))
        arr = np.tile(match["arr"][sel], reps)
        fwd = evaluation._Forward(make_forward_pass("relu", "DeepMind"), match["nets"][team])
        want_route = {"planes": "full_bool"}.get(route, "full_f32")
        assert evaluation._Forward.route(fwd, len(arr), False) == want_route and (fwd.snap.gemm_x3 or route == "library_forced")
        ans = ask(match["nets"][team], arr)
        assert (ans.status == P.OK).all() and len(ans) == len(arr)
        played = np.tile(match["played"][sel], reps)
        if rows is None:
            assert np.array_equal(ans.call, played), np.nonzero(ans.call != played)[0][:5]
        else:
            lg = np.where(match["mask"][sel] == 1, bn.host_forward(copy.deepcopy(match["nets"][team]).to("cpu"), match["obs"][sel]), -np.inf)
            top2 = np.sort(lg, axis=1)[:, -2:]
            clear = np.tile((top2[:, 1] - top2[:, 0]) >= 1e-3, reps)
            assert np.array_equal(ans.call[clear], played[clear])
            total, out = total + len(clear), out + int((~clear).sum())
        assert (ans.top_action[:, 0] == ans.call).all() and np.allclose(ans.probs.sum(1), 1.0, atol=1e-12)
    assert out <= 0.01 * total
    if rows is None and route == "library":
        j = int(np.nonzero(match["team"] == 0)[0][5])
        p = match["arr"][j]
        bidder = M.Bidder(match["nets"][0], "relu", "DeepMind")
        hand = M.hand_text(int(p["hand"]))
        name = bidder.bid(hand, "NESW"[int(p["dealer"])], (int(p["vul_ns"]), int(p["vul_ew"])), [int(c) for c in p["calls"][:int(p["n_calls"])]])
        assert name == boards.CALL_NAMES[int(match["played"][j])]
        with pytest.raises(ValueError):
            bidder.bid(hand, "N", "None", "1C 1C")


def test_the_quiz_through_the_command_line(match, tmp_path, capsys):
    """python -m brl_amd.bid's main on a saved bidder: one position, then the quiz file with its totals and the saved answers"""
    from brl_amd import bid, checkpoint, positions as M
    path = str(tmp_path / "params-00000000.pt")
    checkpoint.save_params(match["nets"][0], path)
    lines = []
    one = bid.main([f"model_path={path}", "hand=AKQ.J32.T9.87654", "dealer=N", "vul=None", "auction=1C P"], log=lines.append)
    lines = "\n".join(lines).split("\n")       # (an answer is logged as one two-line text)
    assert len(one) == 1 and lines[0].startswith("AKQ.J32.T9.87654  dealer N  vul None  auction: 1C P") and "S calls " in lines[1]
    assert len(lines) == 2 and "top: " in lines[1] and "%" in lines[1] and "value " in lines[1]
    lines = []
    ans = bid.main([f"model_path={path}", f"positions_path={QUIZ}", f"save_path={tmp_path / 'a.json'}", "top_k=2"], log=lines.append)
    assert len(lines) == 12 + 2 and lines[:12] == [ans.to_text(i) for i in range(12)]
    assert len(ans) == 12 and (ans.status == 0).all() and lines[-2].startswith("quiz: ") and "on 12 positions" in lines[-2]
    back = M.Answers.from_json(str(tmp_path / "a.json"))
    assert back.same_as(ans) and back.top_k == 2
    with open(QUIZ) as f:
        keys = [d["answers"] for d in json.load(f)]
    assert f"{M.quiz_score(ans, keys)['total']['points']:g} of 120 points" in lines[-2]
    direct = M.Bidder(match["nets"][0]).ask(ans.positions)
    assert np.array_equal(direct.call, ans.call)


# ---- the memory contract ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 65, 130])
def test_both_entry_points_under_the_guards(n):
    """positions / tables / answers at exactly 16 bytes, obs / legal / probs at 8, status / logits / value at 4, mask at 1; logits with
    a row pitch of 40 whose padding is NaN, the value a column two floats apart; tables and probs given and NULL"""
    from brl_amd import _capi
    L = _capi.lib()
    arr, _ = _bad_batch()
    arr = np.tile(arr, 3)[:n]
    rng = np.random.default_rng(n)
    lg = (rng.normal(size=(n, 38)) * 3).astype(np.float32)
    val = rng.normal(size=(n, 1)).astype(np.float32)
    want = P.rows(arr)

    for optional in (True, False):
        def run(mem):
            pos = mem.inp("positions", arr.view(np.uint8).reshape(n, 64), U8, 16)
            obs, mask = mem.out("obs", (n, 480), U8, 8), mem.out("mask", (n, 38), U8, 1)
            legal, status = mem.out("legal", (n,), I64, 8), mem.out("status", (n,), I32, 4)
            tables = mem.out("tables", (n, 16), I64, 16) if optional else None
            _capi.check(L.brl_position_rows(0, pos.data_ptr(), n, obs.data_ptr(), mask.data_ptr(), legal.data_ptr(), status.data_ptr(),
                                            None if tables is None else tables.data_ptr(), _capi.stream(0)))
            logits = mem.inp("logits", lg, F32, 4, ld=40, plain_ld=40)
            value = mem.inp("value", val, F32, 4, ld=2, plain_ld=2)
            answers = mem.out("answers", (n, 12), I64, 16)      # (96 bytes a row; as bytes, a stored 255 would pass for "never written")
            probs = mem.out("probs", (n, 38), F64, 8) if optional else None
            _capi.check(L.brl_position_answers(0, logits.data_ptr(), 40, value.data_ptr(), 2, legal.data_ptr(), status.data_ptr(), n, 3,
                                               answers.data_ptr(), None if probs is None else probs.data_ptr(), _capi.stream(0)))
            out = {"obs": obs, "mask": mask, "legal": legal, "status": status, "answers": answers}
            if optional:
                out.update(tables=tables, probs=probs)
            return out

        _, g, _ = both(run)
        st = g["status"].cpu().numpy().view(np.uint32)
        assert np.array_equal(st, want[0]) and np.array_equal(g["obs"].cpu().numpy(), want[1]) and np.array_equal(g["mask"].cpu().numpy(), want[2])
        from brl_amd import positions as M
        got = np.ascontiguousarray(g["answers"].cpu().numpy()).reshape(-1).view(M.ANSWER_DTYPE)
        ref = P.answer(lg, want[3], 3, st)
        _check_answers(got, g["probs"].cpu().numpy() if optional else None, ref, ("guarded", n, optional))
        assert np.array_equal(got["value"], np.where(st & 0xFF, 0, val[:, 0]).astype(np.float32))


def test_every_alignment_violation_is_refused_before_a_launch():
    from brl_amd import _capi
    L = _capi.lib()
    n = 4
    buf = torch.zeros(1 << 16, dtype=U8, device=DEV)
    base = (buf.data_ptr() + 255) // 256 * 256
    at = lambda k: base + 4096 * k     # noqa: E731  sixteen 256-byte-aligned regions
    torch.cuda.synchronize()
    before = buf.clone()
    rows_ok = dict(positions=at(0), obs=at(1), mask=at(2), legal=at(3), status=at(4), tables=at(5))
    for name, off in (("positions", 8), ("tables", 8), ("obs", 4), ("legal", 4), ("status", 2)):
        a = dict(rows_ok, **{name: rows_ok[name] + off})
        rc = L.brl_position_rows(0, a["positions"], n, a["obs"], a["mask"], a["legal"], a["status"], a["tables"], _capi.stream(0))
        assert rc == BRL_E_ARG and b"aligned" in L.brl_last_error(), name
    ans_ok = dict(logits=at(6), value=at(7), legal=at(3), status=at(4), answers=at(8), probs=at(9))
    for name, off in (("logits", 2), ("value", 2), ("legal", 4), ("status", 2), ("answers", 8), ("probs", 4)):
        a = dict(ans_ok, **{name: ans_ok[name] + off})
        rc = L.brl_position_answers(0, a["logits"], 38, a["value"], 1, a["legal"], a["status"], n, 3, a["answers"], a["probs"], _capi.stream(0))
        assert rc == BRL_E_ARG and b"aligned" in L.brl_last_error(), name
    for kw in (dict(n=0), dict(ld=37), dict(top_k=0), dict(top_k=9), dict(value_stride=-1)):
        a = dict(dict(n=n, ld=38, top_k=3, value_stride=1), **kw)
        assert L.brl_position_answers(0, at(6), a["ld"], at(7), a["value_stride"], at(3), at(4), a["n"], a["top_k"], at(8), at(9), _capi.stream(0)) == BRL_E_ARG, kw
    assert L.brl_position_rows(0, at(0), 0, at(1), at(2), at(3), at(4), None, _capi.stream(0)) == BRL_E_ARG
    assert L.brl_position_rows(0, None, n, at(1), at(2), at(3), at(4), None, _capi.stream(0)) == BRL_E_ARG
    torch.cuda.synchronize()
    assert torch.equal(buf, before)                  # nothing was launched: not a byte changed
