"""The supervised pre-trainer on the GPU (brl_amd/sl.py, include/brl_sl.h): the replay against the oracle, the device sampler
against its numpy restatement, the loss against float64, graph replays against one-step replays and the eager composition,
learning a synthetic teacher, and `python -m brl_amd.sl` end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sl_teacher as T  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _set(n, seed, kind="random"):
    from brl_amd import sl, sl_data
    ts = sl_data.parse_trajectories(T.random_file(n, seed, kind))
    return ts, sl.DeviceSet(ts, DEV)


def test_replay_matches_the_oracle_at_every_decision_point(oracle):
    from brl_amd import sl, sl_data
    ts, data = _set(2000, seed=11)
    nc = ts.n_calls()
    assert nc.max() == 319 and (nc == 4).sum() >= 10 and (ts.calls == 2).sum() > 0
    traj, pos = sl_data.decision_points(ts)
    b = sl.Batch(traj.size, DEV)
    sl.sl_replay(data, torch.from_numpy(traj).to(DEV), torch.from_numpy(pos).to(DEV), b.obs, b.mask, b.label)
    obs, mask, label = b.obs.cpu().numpy(), b.mask.cpu().numpy(), b.label.cpu().numpy()
    assert np.array_equal(label, ts.calls.astype(np.int32))
    # the oracle: the converted deal (seat k % 4 holds chance action k), dealer 0, nobody vulnerable, identity seating
    lines = T.random_file(2000, seed=11).strip().split("\n")
    deal = np.array([[int(t) for t in ln.split()[:52]] for ln in lines])
    hand = np.concatenate([sl_data.openspiel_to_pgx_card(deal[:, s::4]) for s in range(4)], axis=1)
    st = oracle.init_explicit(hand, 0, 0, 0, [0, 1, 2, 3], np.zeros((ts.n, 20), np.uint8))
    for k in range(int(nc.max())):
        live = np.nonzero(k < nc)[0]
        rows = ts.offsets[live] + k
        sub = st[live]
        want_obs = oracle.observe(sub, sub["current_player"])
        assert np.array_equal(obs[rows], want_obs.astype(np.float32)), f"obs differs at call {k}"
        assert np.array_equal(mask[rows], sub["legal_action_mask"]), f"mask differs at call {k}"
        act = np.zeros(ts.n, np.int32)
        act[live] = ts.calls[rows]
        oracle.step(st, act)
    assert st["terminated"].all()


def test_device_sampler_equals_the_numpy_restatement():
    from brl_amd import sl
    ts, data = _set(1000, seed=12)
    b = sl.Batch(ts.n + 37, DEV)
    counter = torch.zeros(1, dtype=torch.int64, device=DEV)
    for start in (0, ts.n - 20, 5 * ts.n + 3):
        counter.fill_(start)
        sl.sl_sample(data, counter, 42, b.traj, b.pos)
        t, p = T.sample(ts.offsets, 42, start, ts.n + 37)
        assert np.array_equal(b.traj.cpu().numpy(), t) and np.array_equal(b.pos.cpu().numpy(), p)
    counter.zero_()
    sl.sl_sample(data, counter, 42, b.traj, b.pos)
    assert sorted(b.traj[:ts.n].cpu().tolist()) == list(range(ts.n))    # each trajectory once in the first epoch


@pytest.mark.parametrize("ent_coef", [0.0, 0.01])
def test_loss_matches_float64(ent_coef):
    from brl_amd import sl
    rng = np.random.default_rng(3)
    B = 777
    z = rng.normal(0, 4, (B, 38)).astype(np.float32)
    z[:32] = rng.choice([-60.0, 60.0], (32, 38)) * rng.random((32, 38))
    mask = rng.random((B, 38)) < 0.4
    mask[:, 0] = True
    mask[40:50] = False
    mask[40:50, 0] = True
    label = np.array([rng.choice(np.nonzero(m)[0]) if i % 7 else rng.integers(0, 38) for i, m in enumerate(mask)], np.int32)
    want, dwant = T.loss64(z.astype(np.float64), label, mask, ent_coef)
    zs = torch.zeros((B, 40), device=DEV)            # a row stride larger than 38
    zs[:, :38] = torch.from_numpy(z)
    lt, mt = torch.from_numpy(label).to(DEV), torch.from_numpy(mask.astype(np.uint8)).to(DEV)
    out, out2 = torch.zeros(5, device=DEV), torch.zeros(5, device=DEV)
    d = torch.zeros((B, 38), device=DEV)
    sl.sl_loss(zs[:, :38], lt, mt, ent_coef, d, out)
    sl.sl_loss(zs[:, :38], lt, mt, ent_coef, None, out2)
    got, dgot = out.cpu().double().numpy(), d.cpu().double().numpy()
    assert np.allclose(got, want, rtol=1e-6, atol=1e-7), (got, want)
    assert np.abs(dgot - dwant).max() <= 1e-6 * np.abs(dwant).max()
    assert torch.equal(out, out2)


def _make(model, seed, data, S, graph, lr=1e-3, B=128):
    from brl_amd import sl
    from brl_amd.models import make_forward_pass
    net = make_forward_pass("relu", model).init(seed, device=DEV)
    opt = sl.make_optimizer(net, lr)
    return net, sl.SLStep(net, opt, data, B, seed, 0.01, steps_per_graph=S, graph=graph)


@pytest.mark.parametrize("model", ["DeepMind", "FAIR"])
def test_graph_replay_equals_one_step_replays_and_eager(model):
    _, data = _set(500, seed=13, kind="teacher")
    net0, _ = _make(model, 1, data, 8, graph=False)
    nets, rows = [], []
    for mode in ("graph8", "graph1", "eager"):
        net, st = _make(model, 1, data, 8, graph=(mode != "eager"))
        if mode == "graph8":
            r = torch.cat([st.run(8).clone() for _ in range(2)])
        elif mode == "graph1":
            r = torch.cat([st.run(1).clone() for _ in range(16)])
        else:
            r = st.eager(16)
        torch.cuda.synchronize()
        nets.append(net)
        rows.append(r.cpu())
        assert int(st.counter.item()) == 16 * 128
    for net, r in zip(nets[1:], rows[1:]):
        assert torch.equal(r, rows[0])
        for a, b in zip(nets[0].parameters(), net.parameters()):
            assert torch.equal(a, b)
    for net in nets:   # the value head gets no gradient
        assert torch.equal(net.critic.weight, net0.critic.weight) and torch.equal(net.critic.bias, net0.critic.bias)
        assert not torch.equal(net.actor.weight, net0.actor.weight)


@pytest.mark.parametrize("model, steps, floor", [("DeepMind", 500, 0.9), ("FAIR", 300, 0.85)])
def test_it_learns_a_synthetic_teacher(model, steps, floor):
    from brl_amd import sl
    _, train = _set(2000, seed=14, kind="teacher")
    _, test = _set(500, seed=15, kind="teacher")
    net, st = _make(model, 0, train, 8, graph=True)
    before = sl.evaluate_all(net, test)["accuracy"]
    for _ in range(steps // 8):
        st.run(8)
    after = sl.evaluate_all(net, test)
    assert before < 0.2 and after["accuracy"] >= floor, (before, after)


def test_cli_end_to_end(tmp_path):
    from brl_amd import checkpoint, sl
    data_dir, save = tmp_path / "data", tmp_path / "save"
    data_dir.mkdir()
    (data_dir / "train.txt").write_text(T.random_file(300, seed=16, kind="teacher"))
    (data_dir / "test.txt").write_text(T.random_file(100, seed=17, kind="teacher"))
    args = [f"data_path={data_dir}", f"save_path={save}", "iterations=40", "eval_every=20", "train_batch=64", "eval_batch=256",
            "num_examples=1"]
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "brl_amd.sl"] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(os.listdir(save)) == ["params-20.pkl", "params-40.pkl"]
    for key in ("train/total_loss", "train/target_loss", "train/entropy", "train/train_accuracy", "test/test_accuracy",
                "test/total_loss", "test/target_loss", "test/entropy", "test/illegal_actions_prob", "Ground truth"):
        assert key in r.stdout, key
    from brl_amd.train import parse_cli
    cfg = parse_cli(args, defaults=sl.SL_DEFAULTS)
    net = sl.train_sl(cfg, log=lambda m: None)
    loaded = checkpoint.load_params(str(save / "params-40.pkl"), "relu", "DeepMind", DEV)
    x = (torch.rand((64, 480), device=DEV) < 0.1).float()
    with torch.no_grad():
        assert torch.allclose(loaded(x)[0], net(x)[0], rtol=1e-6, atol=1e-6)
