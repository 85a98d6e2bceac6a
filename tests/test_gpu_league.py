"""-m gpu: the batched league evaluation (brl_amd/league.py, csrc/brl_league.hip) — the route against its numpy restatement, the
grouped forward against brl_mlp_forward_rows (bit for bit) and float64, whole leagues replayed through the CPU oracle match by
match, batching, the mirror property, PFSP's league under the trainer and both command lines."""
import copy
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.gpu_util import to_np
from tests.test_league_host import route_numpy

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def env(dds):
    import brl_amd
    return brl_amd.BridgeBidding(lut=(dds["keys"], dds["values"]))


def _route(term, cur, pairs, team, n, num_groups):
    """brl_league_route with one group per network (group id = network id), as route_numpy"""
    from brl_amd import _capi
    from brl_amd.league import team_order
    order, _, _ = team_order(pairs, team)
    group_of = np.asarray(pairs)[order, team].astype(np.int32)
    P = len(pairs)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    rows = torch.full((P * n,), -7, dtype=torch.int64, device="cuda")
    gf = torch.full((num_groups + 1,), -7, dtype=torch.int32, device="cuda")
    work = torch.empty(2 * P, dtype=torch.int32, device="cuda")
    t, c, o, g = d(term), d(cur), d(order), d(group_of)
    _capi.check(_capi.lib().brl_league_route(0, t.data_ptr(), c.data_ptr(), team, n, o.data_ptr(), g.data_ptr(), P, num_groups,
                                             work.data_ptr(), rows.data_ptr(), gf.data_ptr(), _capi.stream()))
    torch.cuda.synchronize()
    return rows, gf


@pytest.mark.parametrize("P,n", [(1, 37), (6, 100), (45, 100), (3, 1000), (1100, 3)])   # (1100: two slots per thread of the scan)
@pytest.mark.parametrize("team", [0, 1])
def test_route_equals_the_numpy_restatement(P, n, team):
    rng = np.random.default_rng(100 * P + n + team)
    M = 1 if P == 1 else (4 if P == 6 else (7 if P == 1100 else 10))
    pairs = np.array([[0, 0]]) if P == 1 else (np.array([(i, j) for i in range(10) for j in range(i + 1, 10)]) if P == 45
                                               else rng.integers(0, M, (P, 2)))
    for case in ("random", "nothing acts"):
        term = (rng.random(P * n) < 0.4).astype(np.uint8)
        cur = rng.integers(0, 4, P * n).astype(np.int32)
        if case == "nothing acts":
            cur[term == 0] = 2 * (1 - team) + (cur[term == 0] & 1)      # every live board waits for the other team
        want_rows, want_gf = route_numpy(term, cur, pairs, team, n, num_groups=M + 2)   # (+ 2: groups that no match names)
        rows, gf = _route(term, cur, pairs, team, n, M + 2)
        R = int(want_gf[-1])
        assert (R == 0) == (case == "nothing acts")
        assert np.array_equal(to_np(gf), want_gf)
        assert np.array_equal(to_np(rows)[:R], want_rows) and (to_np(rows)[R:] == -7).all()


def _nets(fp, seeds):
    """one network per seed, every parameter perturbed with a seed of its own (tests/nets.py): on hk.Linear's zero biases a forward
    that read another network's or another layer's bias would give the same numbers"""
    from tests.nets import perturbed
    return [perturbed(fp.init(s, device="cuda"), 1000 + s) for s in seeds]


def _table(refs):
    from brl_amd.league import _net_record
    return torch.tensor([_net_record(r) for r in refs], dtype=torch.int64, device="cuda")


@pytest.mark.parametrize("activation", ["relu", "tanh"])
@pytest.mark.parametrize("model,M,sizes", [
    ("DeepMind", 1, [130]),
    ("DeepMind", 3, [64, 0, 65]),
    ("DeepMind", 10, [0, 1, 63, 64, 65, 300, 0, 7, 450, 128]),
    ("DeepMind_6", 3, [1, 63, 333]),
])
def test_grouped_forward_equals_forward_rows_bit_for_bit(activation, model, M, sizes):
    """For every group g the rows of `out` the league forward writes equal, bit for bit, brl_mlp_forward_rows of network g on the
    same rows: both run mg::gemm_tile's k-ordered chain per output element and the same heads reduction, and an output row depends
    on its own input row and the weights only.  Also the float64 bound of test_mlp_forward_rows_matches_float64
    (< 2e-4 * max(1, max|logits|) against the module in float64); rows that are not routed keep what they held."""
    from brl_amd import _capi
    from brl_amd.evaluation import _Forward
    from brl_amd.models import make_forward_pass
    fp = make_forward_pass(activation, model)
    nets = _nets(fp, range(11, 11 + M))
    fwds = [_Forward(fp, m) for m in nets]
    assert all(f.ref is not None for f in fwds)
    nlayers, hidden = int(fwds[0].ref.nlayers), int(fwds[0].ref.hidden)
    assert hidden == 1024 and nlayers == (6 if model == "DeepMind_6" else 4)
    R = sum(sizes)
    nboards = R + 200
    g = torch.Generator(device="cuda").manual_seed(R + M)
    obs = torch.rand(nboards, 480, device="cuda", generator=g) < 0.1
    rows = torch.randperm(nboards, device="cuda", generator=g)[:R].contiguous()
    gf = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32, device="cuda")
    table = _table([f.ref for f in fwds])
    for rmax in (R, nboards):   # the bound of R the grids are sized for: tight and loose
        out = torch.full((nboards, 40), 123.0, device="cuda")
        scratch = torch.empty(rmax * (480 + 2 * hidden), device="cuda")
        _capi.check(_capi.lib().brl_league_forward(0, table.data_ptr(), M, nlayers, hidden, 0 if activation == "relu" else 1,
                                                   obs.data_ptr(), rows.data_ptr(), gf.data_ptr(), rmax, scratch.data_ptr(),
                                                   scratch.numel(), out.data_ptr(), 40, _capi.stream()))
        torch.cuda.synchronize()
        want = torch.full((nboards, 40), 123.0, device="cuda")
        for k, f in enumerate(fwds):
            if sizes[k]:
                f.rows(obs, rows[int(gf[k]):int(gf[k + 1])].contiguous(), sizes[k], want, None)
        torch.cuda.synchronize()
        assert torch.equal(out, want)
        untouched = torch.ones(nboards, dtype=torch.bool)
        untouched[rows.cpu()] = False
        assert bool((out.cpu()[untouched] == 123.0).all()) and bool((out[:, 39] == 123.0).all())
    for k in range(M):
        if sizes[k] == 0:
            continue
        idx = rows[int(gf[k]):int(gf[k + 1])][:64]
        net64 = copy.deepcopy(nets[k]).double().cpu()
        assert float(net64.body[0].bias.abs().min()) > 0 and (M == 1 or not torch.equal(net64.critic.bias, nets[(k + 1) % M].critic.bias.double().cpu()))
        with torch.no_grad():
            logits, value = net64(obs[idx].cpu().double())
        got = out[idx].cpu().double()
        scale = max(1.0, float(logits.abs().max()))
        assert float((got[:, :38] - logits).abs().max()) < 2e-4 * scale
        assert float((got[:, 38] - value).abs().max()) < 2e-4 * scale


def _replay_match(oracle, n, seed, calls, logits=None):
    """one match's recorded calls ([iterations][n], -1 = waited) through oracle.duplicate_step, as
    test_simple_duplicate_evaluate_default_loop_replays_through_oracle: who acted and who waited, every call legal, waiting boards
    keep their state; with logits: each call is the arg-max of the logits over the oracle's legal mask"""
    from oracle import Oracle
    ref = oracle.init_random(n, seed=seed)
    oA, oB = Oracle.table_info_from(ref), Oracle.table_info_from(ref)
    cum = np.zeros(n, np.float32)
    rows = np.arange(n)
    for i, act in enumerate(calls):
        idle = act < 0
        live = (ref["terminated"] == 0) & ~idle
        team = ref["current_player"] >> 1
        assert (team[live] == (i & 1)).all() and (team[idle & (ref["terminated"] == 0)] != (i & 1)).all()
        assert not (idle & (ref["terminated"] != 0)).any()        # (a finished board takes its no-op step, never waits)
        assert (ref["legal_action_mask"][rows, np.where(idle, 0, act)][live] == 1).all()
        if logits is not None:
            masked = np.where(ref["legal_action_mask"].astype(bool), logits[i], -np.inf)
            assert np.array_equal(act[live], masked.argmax(1)[live])
        keep = (ref[idle].copy(), oA[idle].copy(), oB[idle].copy())
        oracle.duplicate_step(ref, np.where(idle, 0, act).astype(np.int32), oA, oB)
        ref[idle], oA[idle], oB[idle] = keep
        cum[~idle] += ref["rewards"][~idle, 0]
    assert ref["terminated"].all() and oA["terminated"].all() and oB["terminated"].all()
    return cum, oA, oB


@pytest.mark.parametrize("M,n", [(4, 100), (3, 640)])
def test_league_replays_through_the_oracle(env, oracle, M, n):
    from brl_amd.league import all_pairs, league_matrices, make_league_evaluate
    from brl_amd.models import make_forward_pass
    fp = make_forward_pass("relu", "DeepMind")
    nets = _nets(fp, range(3, 3 + M))
    pairs = all_pairs(M)
    record = {"logits": True}
    ev = make_league_evaluate(env, "relu", "DeepMind", n, record=record)
    imp, se, win, cum = ev(nets, pairs, 99)
    torch.cuda.synchronize()
    assert ev.last_method == "batched" and len(record["batches"]) == 1
    b = record["batches"][0]
    assert b["matches"] == (0, len(pairs)) and cum.shape == (len(pairs), n)
    actions = np.stack([to_np(a) for a in b["action"]]).reshape(len(b["action"]), len(pairs), n)
    logits = np.stack([to_np(x)[:, :38] for x in b["logits"]]).reshape(len(b["logits"]), len(pairs), n, 38)
    # the route of every iteration: the boards that made a call are the rows, grouped as the restatement says
    from brl_amd.league import team_order
    for i, (rows, gf) in enumerate(zip(b["rows"], b["group_first"])):
        R = int(gf[-1])
        called = np.nonzero(actions[i].reshape(-1) >= 0)[0]
        live_rows = np.sort(to_np(rows)[:R])
        assert np.isin(live_rows, called).all()                       # (`called` also holds the finished boards' no-op steps)
        order, group_of, netsT = team_order(pairs, i & 1)
        sizes = np.diff(to_np(gf))
        for k, first in enumerate(to_np(gf)[:-1]):
            assert (pairs[to_np(rows)[first:first + sizes[k]] // n, i & 1] == netsT[k]).all()
    for p in range(len(pairs)):
        want, oA, oB = _replay_match(oracle, n, 99, actions[:, p], logits[:, p])
        sl = slice(p * n, (p + 1) * n)
        for T, oT in ((b["table_a"], oA), (b["table_b"], oB)):
            for f in ("terminated", "rewards", "last_bid", "last_bidder", "call_x", "call_xx"):
                assert np.array_equal(to_np(getattr(T, f))[sl].astype(np.float64), oT[f].astype(np.float64)), (p, f)
        assert np.array_equal(to_np(cum[p]), want)
        assert abs(float(imp[p]) - want.mean()) < 1e-5
        assert abs(float(se[p]) - want.std(ddof=1) / np.sqrt(n)) < 1e-5
        assert abs(float(win[p]) - (want > 0).mean()) < 1e-6
    wl, clip, dis = league_matrices(to_np(imp), pairs, M)
    assert np.array_equal(wl, -wl.T) and wl[1][0] == float(imp[0])


def test_batching_changes_nothing_and_a_network_ties_with_itself(env):
    from brl_amd.league import make_league_evaluate
    from brl_amd.models import make_forward_pass
    fp = make_forward_pass("relu", "DeepMind")
    nets = _nets(fp, [3, 4, 5])
    n = 100
    pairs = [(0, 1), (1, 1), (2, 0), (1, 2), (0, 0), (2, 1), (0, 2)]
    outs = []
    for max_boards, nbatches in ((65536, 1), (300, 3)):
        record = {}
        ev = make_league_evaluate(env, "relu", "DeepMind", n, max_boards=max_boards, record=record)
        outs.append([t.clone() for t in ev(nets, pairs, 7)])
        assert len(record["batches"]) == nbatches and ev.last_method == "batched"
    torch.cuda.synchronize()
    assert torch.equal(outs[0][3], outs[1][3]) and bool(outs[0][3].any())
    for a, b in zip(outs[0][:3], outs[1][:3]):
        assert torch.equal(a, b)
    cum = outs[0][3]
    assert not bool(cum[1].any()) and not bool(cum[4].any())          # match (i, i): 0 IMP on every board
    # ... and the loop (one evaluation per pair, the existing evaluator's loop) plays the same matches.  Its full-batch forwards
    # go through the library's GEMM, not the exact chain: an arg-max between two logits closer than the products' rounding may
    # fall the other way (gaps of neighbouring logits are ~1e-2, the rounding ~1e-6: a few boards in 10^4 at most), whereas a
    # loop that played other deals or other pairs would agree on almost none — hence 98 %, as
    # test_policy_rollout_draw_counter_wraps_mod_2_32 argues
    loop = make_league_evaluate(env, "relu", "DeepMind", n, method="loop")
    got = loop(nets, pairs, 7)
    torch.cuda.synchronize()
    assert loop.last_method == "loop" and got[3].shape == cum.shape
    assert float((got[3] == cum).float().mean()) >= 0.98


def test_mirror(env):
    """With (i, j) and (j, i) in one league, cum_return[(j, i)] == -cum_return[(i, j)] board by board: table A of one match is
    table B of the other (the same deal, the same networks in the same seats).  The property holds on the CPU oracle with a
    stand-in policy per network (tests/test_league_host.py::test_mirror_property_on_the_cpu_oracle), so it is asserted here."""
    from brl_amd.league import make_league_evaluate
    from brl_amd.models import make_forward_pass
    fp = make_forward_pass("relu", "DeepMind")
    nets = _nets(fp, [3, 4, 5])
    pairs = [(0, 1), (1, 0), (2, 1), (0, 2), (1, 2), (2, 0)]
    cum = make_league_evaluate(env, "relu", "DeepMind", 256)(nets, pairs, 31)[3]
    torch.cuda.synchronize()
    assert bool(cum.any())
    assert torch.equal(cum[1], -cum[0]) and torch.equal(cum[4], -cum[2]) and torch.equal(cum[5], -cum[3])


def test_one_vs_many_is_the_league_of_the_pairs_0_k(env):
    from brl_amd.league import make_league_evaluate, one_vs_many
    from brl_amd.models import make_forward_pass
    fp = make_forward_pass("relu", "DeepMind")
    nets = _nets(fp, [3, 4, 5, 6])
    imp = one_vs_many(nets[0], nets[1:], env, "relu", "DeepMind", 100, rng_key=12)
    want = make_league_evaluate(env, "relu", "DeepMind", 100)(nets, [(0, 1), (0, 2), (0, 3)], 12)[0]
    torch.cuda.synchronize()
    assert imp.shape == (3,) and torch.equal(imp, want)
    # a FAIR league is played as a loop (the batched path takes DeepMind MLPs), with the same interface
    fair = make_forward_pass("relu", "FAIR")
    ev = make_league_evaluate(env, "relu", "FAIR", 64)
    out = ev([fair.init(1, device="cuda"), fair.init(2, device="cuda")], [(0, 1)], 12)
    assert ev.last_method == "loop" and out[3].shape == (1, 64)


@pytest.mark.parametrize("league_eval", ["batched", "loop"])
def test_train_runs_pfsp_with_either_league(tmp_path, league_eval):
    """Two iterations of the trainer with a prioritised draw from a pool of 3 saved checkpoints, the league of the learner against
    the pool played as one batch or as a loop: both run to the end.  (They are not required to draw the same opponent: a
    near-tied arg-max may fall differently between the library's GEMM and the exact chain.)"""
    from brl_amd import checkpoint
    from brl_amd.models import make_forward_pass
    from brl_amd.train import DEFAULTS, train
    fp = make_forward_pass("relu", "DeepMind")
    cfg = dict(DEFAULTS, num_envs=256, num_steps=8, total_timesteps=256 * 8 * 2, minibatch_size=512, update_epochs=1,
               num_eval_envs=64, num_prioritized_envs=64, lut_len=2000, log_path=str(tmp_path), exp_name="pfsp", save_model=False,
               prioritized_fictitious=True, ratio_model_zoo=1.0, threshold_model_zoo=-1e9, league_eval=league_eval)
    pool = os.path.join(cfg["log_path"], cfg["exp_name"], cfg["save_model_path"])
    os.makedirs(pool)
    for k in range(3):
        checkpoint.save_params(fp.init(20 + k), os.path.join(pool, f"params-{k + 1:08}.pt"))
    lines = []
    _, history = train(cfg, log=lines.append)
    assert len(history) == 2
    assert all(h["opponent"] in ("params-00000001.pt", "params-00000002.pt", "params-00000003.pt") for h in history)


def test_both_command_lines(tmp_path, dds):
    from brl_amd import checkpoint
    from brl_amd.models import make_forward_pass
    fp = make_forward_pass("relu", "DeepMind")
    run = tmp_path / "models" / "run"
    run.mkdir(parents=True)
    for k in range(3):
        checkpoint.save_params(fp.init(30 + k), str(run / f"params-{100 * k:08}.pt"))
    checkpoint.save_params(fp.init(40), str(run / "params-00000150.pt"))     # (filtered out: not a multiple of skip_interval)
    lut = tmp_path / "lut.npy"
    np.save(lut, np.stack([dds["keys"], dds["values"]]))
    envv = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "brl_amd.league", f"models_directory={tmp_path / 'models'}", "exp_name=run",
                        "num_eval_envs=64", f"dds_path={lut}", f"save_fig_directory_path={tmp_path}"], cwd=tmp_path, env=envv,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    files = sorted(glob.glob(str(tmp_path / "win_lose_*.npy")))
    assert [os.path.basename(f) for f in files] == ["win_lose_clip_run.npy", "win_lose_dis_run.npy", "win_lose_run.npy"]
    for f in files:
        m = np.load(f)
        assert m.shape == (3, 3) and np.array_equal(m, -m.T)
    r = subprocess.run([sys.executable, "-m", "brl_amd.eval", f"team1_model_path={run / 'params-00000000.pt'}",
                        f"team2_model_path={run / 'params-00000100.pt'}", "num_eval_envs=64", f"dds_path={lut}"], cwd=tmp_path,
                       env=envv, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("IMP: ")][-1]
    imp, se = (float(x) for x in line[len("IMP: "):].split(" ± "))
    assert se >= 0.0 and np.isfinite(imp)
    r = subprocess.run([sys.executable, "-m", "brl_amd.league", "boards=3"], cwd=tmp_path, env=envv, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode != 0 and "unknown option boards" in r.stderr
