"""Policy distillation on the GPU (brl_amd/distill.py, include/brl_distill.h): the two kernels against the float64 restatement
(tests/distill_ref.py), their exact properties, non-finite inputs, graph replays against one-step replays and the eager
composition, the kernel path's gradients against torch autograd, learning the bidder, an ensemble of two, and
`python -m brl_amd.distill` end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import distill_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C_POL, C_VAL = 1.0, 0.5


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _run(z, u, t, v, w, mask, tau, layout="stride40", grad=True, c_pol=C_POL, c_val=C_VAL):
    """both kernels on host arrays -> dict of numpy arrays (q, vstar, hq, dz, du, metrics).  ``layout``: "stride40" — logits in rows
    of 40 floats, the values apart —, or "heads" — the [K, n, 39] stack of ``teacher_heads`` and an [n, 39] student."""
    from brl_amd import distill
    K, B = t.shape[0], t.shape[1]
    if layout == "heads":
        th = torch.zeros((K, B, 39), device=DEV)
        th[:, :, :38], th[:, :, 38] = _dev(t), _dev(v)
        tl, tv = th[:, :, :38], th[:, :, 38]
        sh = torch.zeros((B, 39), device=DEV)
        sh[:, :38], sh[:, 38] = _dev(z), _dev(u)
        zz, uu = sh[:, :38], sh[:, 38]
    else:
        tl = torch.zeros((K, B, 40), device=DEV)
        tl[:, :, :38] = _dev(t)
        tl, tv = tl[:, :, :38], _dev(v)
        zz = torch.zeros((B, 40), device=DEV)
        zz[:, :38] = _dev(z)
        zz, uu = zz[:, :38], _dev(u)
    mk = _dev(mask.astype(np.uint8))
    f = lambda *s: torch.full(s, 7.0, dtype=torch.float32, device=DEV)     # noqa: E731
    q, vstar, hq, dz, du, out = f(B, 38), f(B), f(B), f(B, 38), f(B), f(8)
    distill.distill_targets(tl, tv, _dev(w), mk, tau, q, vstar, hq)
    if grad:
        distill.distill_loss(zz, uu, q, vstar, hq, mk, tau, c_pol, c_val, dz, du, out)
    else:
        distill.distill_loss(zz, uu, q, vstar, hq, mk, tau, c_pol, c_val, None, None, out)
    torch.cuda.synchronize()
    return {k: x.cpu().numpy() for k, x in dict(q=q, vstar=vstar, hq=hq, dz=dz, du=du, metrics=out).items()}


def _want(z, u, t, v, w, mask, tau, c_pol=C_POL, c_val=C_VAL):
    w64 = w.astype(np.float64)
    return (R.restate(z, u, t, v, w64, mask, tau, c_pol, c_val, np.float64),
            R.restate(z, u, t, v, w, mask, tau, c_pol, c_val, np.float32))


def _check(got, want64, want32, where, names=("q", "vstar", "hq", "dz", "du")):
    """max |device - float64| of each quantity and each metric against ``distill_ref.tolerance``; -> the largest error / bound"""
    worst = 0.0
    for name in names:
        err, tol = float(np.abs(got[name].astype(np.float64) - want64[name]).max()), R.tolerance(want64[name], want32[name])
        print(f"{where} {name}: error {err:.3e}, bound {tol:.3e}")
        assert err <= tol, (where, name, err, tol)
        worst = max(worst, err / tol if tol else 0.0)
    for i, name in enumerate(R.METRICS):
        err, tol = abs(float(got["metrics"][i]) - want64["metrics"][i]), R.tolerance(want64["metrics"][i], want32["metrics"][i])
        print(f"{where} {name}: error {err:.3e}, bound {tol:.3e}")
        assert err <= tol, (where, name, err, tol)
    assert got["metrics"][7] == 0.0
    return worst


# ---- the kernels against float64 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 777])
def test_kernels_match_float64(B, K):
    """q, vstar, hq, dz, du and every metric at tau 0.5, 1 and 2, in both layouts (logits in rows of 40 floats; the [K, n, 39]
    heads), on N(0, 4) logits with 32 rows of +-60 logits, rows with only Pass legal and an all-legal row, unequal weights.
    The bound (``distill_ref.tolerance``): 4 x the error of the float32 restatement of the same formulas against float64 on the same
    inputs, never less than 4 * 2^-24 * max |want|.  Also: dz on illegal calls is exactly 0.0, the metrics-only call gives the
    gradient call's bits, a second run gives the same bits, and swapping two teachers with their weights moves q and vstar by no
    more than the bound.  Largest errors measured: DESIGN §19."""
    z, u, t, v, w, mask = R.inputs(B, K, seed=100 + B + K)
    for tau in (0.5, 1.0, 2.0):
        want64, want32 = _want(z, u, t, v, w, mask, tau)
        got = _run(z, u, t, v, w, mask, tau, "stride40")
        _check(got, want64, want32, f"B={B} K={K} tau={tau}")
        assert (got["dz"][~mask] == 0.0).all()
        heads = _run(z, u, t, v, w, mask, tau, "heads")
        again = _run(z, u, t, v, w, mask, tau, "stride40")
        only = _run(z, u, t, v, w, mask, tau, "stride40", grad=False)
        for name in got:
            assert np.array_equal(got[name], heads[name]) and np.array_equal(got[name], again[name]), name
        assert np.array_equal(got["metrics"], only["metrics"]) and (only["dz"] == 7.0).all() and (only["du"] == 7.0).all()
        if K > 1:
            order = [1, 0] + list(range(2, K))
            swapped = _run(z, u, t[order], v[order], w[order], mask, tau, "stride40")
            _check(swapped, want64, want32, f"B={B} K={K} tau={tau} swapped", names=("q", "vstar"))


@pytest.mark.parametrize("tau", [0.5, 1.0, 2.0])
def test_one_teacher_and_the_same_logits_give_exact_zeros(tau):
    """K = 1 and z equal to t_0 bit for bit: L_pol == 0.0 and dz == 0 exactly on every row, agreement 1 (both kernels form lsm and
    the sum over the legal calls through one device function, in one order)"""
    z, u, t, v, _, mask = R.inputs(777, 1, seed=5)
    got = _run(t[0], u, t, v, np.ones(1, np.float32), mask, tau)
    assert got["metrics"][1] == 0.0 and (got["dz"] == 0.0).all() and got["metrics"][5] == 1.0
    rows = _run(t[0][:1], u[:1], t[:, :1], v[:, :1], np.ones(1, np.float32), mask[:1], tau)     # one row: its own L_pol
    assert rows["metrics"][1] == 0.0
    for b in (5, 41, 300, 776):
        one = _run(t[0][b:b + 1], u[b:b + 1], t[:, b:b + 1], v[:, b:b + 1], np.ones(1, np.float32), mask[b:b + 1], tau)
        assert one["metrics"][1] == 0.0 and (one["dz"] == 0.0).all(), b


# ---- non-finite inputs ----------------------------------------------------------------------------------------------------------
def _same_nonfinite(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    assert np.array_equal(np.isinf(got), np.isinf(want)), what


@pytest.mark.parametrize("case", ["nan_teacher", "nan_student", "neginf_teacher", "all_neginf_teacher", "nan_value"])
def test_nonfinite_inputs_follow_the_written_semantics(case):
    """300 rows, K = 2, one poisoned row: its q / hq / vstar / dz / du and the metrics are NaN where the float64 restatement's are
    (include/brl_distill.h, "Non-finite inputs"), a -inf legal teacher logit gives that teacher probability 0 there and everything
    stays finite, and every other row's q, vstar, hq, dz and du are bit for bit those of the clean run (the same 1 / B)"""
    B, row = 300, 121
    z, u, t, v, w, mask = R.inputs(B, 2, seed=6)
    legal = np.nonzero(mask[row])[0]
    assert len(legal) >= 2
    j = int(legal[1])
    clean = _run(z, u, t, v, w, mask, 1.0)
    assert all(np.isfinite(x).all() for x in clean.values())
    z2, u2, t2, v2 = z.copy(), u.copy(), t.copy(), v.copy()
    if case == "nan_teacher":
        t2[1, row, j] = np.nan
    elif case == "nan_student":
        z2[row, j] = np.nan
    elif case == "neginf_teacher":
        t2[0, row, j] = -np.inf
    elif case == "all_neginf_teacher":
        t2[0, row, legal] = -np.inf
    else:
        v2[1, row] = np.nan
    got = _run(z2, u2, t2, v2, w, mask, 1.0)
    want64, want32 = _want(z2, u2, t2, v2, w, mask, 1.0)
    for name in ("q", "vstar", "hq", "dz", "du"):
        _same_nonfinite(got[name], want64[name], f"{case}: {name}")
    keep = [0, 1, 2, 3, 4, 6]
    _same_nonfinite(got["metrics"][keep], want64["metrics"][keep], f"{case}: metrics")
    others = np.arange(B) != row
    for name in ("q", "vstar", "hq", "dz", "du"):
        assert np.array_equal(got[name][others], clean[name][others]), f"{case}: {name} of the other rows"
    assert (got["dz"][~mask] == 0.0).all()
    if case in ("nan_teacher", "all_neginf_teacher"):
        assert np.isnan(got["q"][row][mask[row]]).all() and np.isnan(got["dz"][row][mask[row]]).all() and np.isnan(got["hq"][row])
        assert np.isnan(got["metrics"][[0, 1, 3]]).all() and np.isfinite(got["du"]).all()
    elif case == "nan_student":
        assert np.array_equal(got["q"], clean["q"]) and np.isnan(got["dz"][row][mask[row]]).all() and np.isnan(got["metrics"][[0, 1, 4]]).all()
    elif case == "nan_value":
        assert np.isnan(got["vstar"][row]) and np.isnan(got["du"][row]) and np.isnan(got["metrics"][[0, 2]]).all()
        assert np.isfinite(got["dz"]).all() and np.isfinite(got["metrics"][1])
    else:
        _check(got, want64, want32, case)
        one = _run(z2, u2, t2[:1], v2[:1], np.ones(1, np.float32), mask, 1.0)
        assert one["q"][row, j] == 0.0 and np.isfinite(one["metrics"]).all()


# ---- the step -------------------------------------------------------------------------------------------------------------------
N_ENVS, N_STEPS, BATCH, S = 256, 8, 128, 8
ROLL_CFG = dict(num_steps=N_STEPS, reward_scale=7600.0, game_mode="competitive", actor_illegal_action_mask=True)


@pytest.fixture(scope="module")
def table(dds):
    """the bidder as the teacher, the positions it reaches at the table (256 envs x 8 steps) from two seeds — train and held-out —
    and the train positions' targets at tau 1; shared by the tests below and left unchanged"""
    import brl_amd
    from brl_amd import distill
    from brl_amd.models import make_forward_pass
    from tests.bidder_net import bidder
    teacher = bidder(seed=1, device=DEV)
    fp = make_forward_pass("relu", "DeepMind")
    sets = {}
    for name, seed in (("train", 21), ("held", 22)):
        env = brl_amd.BridgeBidding(lut=(dds["keys"], dds["values"]), device=DEV)
        roll = brl_amd.make_roll_out(ROLL_CFG, env, fp, fp)
        st = env.init(seed, num_envs=N_ENVS)
        _, traj = roll((teacher, None, st, st.observation, 0, 0), teacher)
        sets[name] = (traj.obs.reshape(-1, 480).clone(), traj.legal_action_mask.reshape(-1, 38).clone())
    obs, mask = sets["train"]
    n = obs.shape[0]
    w = torch.ones(1, device=DEV)
    q, vstar, hq = torch.empty((n, 38), device=DEV), torch.empty(n, device=DEV), torch.empty(n, device=DEV)
    heads = distill.ensemble_targets([teacher], w, obs, mask, 1.0, q, vstar, hq)
    torch.cuda.synchronize()
    return dict(teacher=teacher, train=sets["train"], held=sets["held"], q=q, vstar=vstar, hq=hq, heads=heads, n=n)


def _student(model, seed=1):
    from brl_amd.models import make_forward_pass
    return make_forward_pass("relu", model).init(seed, device=DEV)


def _step(table, model, graph, lr=1e-3):
    from brl_amd import distill, sl
    net = _student(model)
    st = distill.DistillStep(net, sl.make_optimizer(net, lr), BATCH, table["n"], 1.0, C_POL, C_VAL, steps_per_graph=S, graph=graph)
    st.load(*table["train"], table["q"], table["vstar"], table["hq"])
    return net, st


def _torch_loss(logits, value, heads, w, mask, tau, c_pol, c_val):
    """the plain torch composition of the same loss in float32: masked log_softmax, the mixture, kl_div, mse_loss (no kernel of
    include/brl_distill.h)"""
    F = torch.nn.functional
    neg = torch.finfo(torch.float32).min
    lsm = lambda x: torch.log_softmax(torch.where(mask, x / tau, torch.full_like(x, neg)), dim=-1)     # noqa: E731
    q = sum(w[k] * lsm(heads[k, :, :38]).exp() for k in range(heads.shape[0])) * mask
    vstar = sum(w[k] * heads[k, :, 38] for k in range(heads.shape[0]))
    kl = F.kl_div(lsm(logits), q, reduction="none").sum(-1)
    return c_pol * tau * tau * kl.mean() + c_val * F.mse_loss(value, vstar)


@pytest.mark.parametrize("model", ["DeepMind", "FAIR"])
def test_graph_replay_equals_one_step_replays_and_eager(table, model):
    """16 steps of B = 128 as two 8-step replays, sixteen 1-step replays and eagerly: bit-equal parameters and metrics rows; the
    critic head has moved (both heads learn, unlike the supervised pre-trainer)"""
    net0 = _student(model)
    nets, rows = [], []
    for mode in ("graph8", "graph1", "eager"):
        net, st = _step(table, model, graph=(mode != "eager"))
        assert st.shuffle(table["n"], torch.Generator(device=DEV).manual_seed(5)) == table["n"] // BATCH == 16
        if mode == "graph8":
            r = torch.cat([st.run(8).clone() for _ in range(2)])
        elif mode == "graph1":
            r = torch.cat([st.run(1).clone() for _ in range(16)])
        else:
            r = st.eager(16)
        torch.cuda.synchronize()
        nets.append(net)
        rows.append(r.cpu())
        assert int(st.cursor.item()) == 16 * BATCH
    assert bool(torch.isfinite(rows[0]).all()) and float(rows[0][:, 1].min()) > 0.0
    for net, r in zip(nets[1:], rows[1:]):
        assert torch.equal(r, rows[0])
        for a, b in zip(nets[0].parameters(), net.parameters()):
            assert torch.equal(a, b)
    for net in nets:
        assert not torch.equal(net.critic.weight, net0.critic.weight) and not torch.equal(net.critic.bias, net0.critic.bias)
        assert not torch.equal(net.actor.weight, net0.actor.weight)


@pytest.mark.parametrize("model", ["DeepMind", "FAIR"])
def test_one_steps_parameter_gradients_match_torch_autograd(table, model):
    """brl_distill_loss's dz / du pushed through torch's layers against torch autograd of the plain float32 composition of the
    same loss on the same batch: within 1e-5 of the largest gradient entry, per tensor"""
    from brl_amd import distill
    obs, mask = table["train"]
    x, mk = obs[:BATCH].float(), mask[:BATCH]
    w = torch.ones(1, device=DEV)
    net = _student(model, seed=3)
    logits, value = net(x)
    dz, du, out = torch.zeros((BATCH, 38), device=DEV), torch.zeros(BATCH, device=DEV), torch.zeros(8, device=DEV)
    distill.distill_loss(logits, value, table["q"][:BATCH], table["vstar"][:BATCH], table["hq"][:BATCH], mk, 1.0, C_POL, C_VAL, dz, du, out)
    torch.autograd.backward([logits, value], [dz, du])
    ours = [p.grad.clone() for p in net.parameters()]
    net.zero_grad(set_to_none=True)
    logits, value = net(x)
    loss = _torch_loss(logits, value, table["heads"][:, :BATCH], w, mk, 1.0, C_POL, C_VAL)
    loss.backward()
    assert abs(float(loss.detach()) - float(out[0])) <= 1e-5 * abs(float(loss.detach()))
    for (name, p), g in zip(net.named_parameters(), ours):
        err, top = float((p.grad - g).abs().max()), float(p.grad.abs().max())
        print(f"{model} {name}: error {err:.3e}, largest entry {top:.3e}")
        assert top > 0.0 and err <= 1e-5 * top, (name, err, top)


LEARN_STEPS = 400


def test_it_learns_the_bidder(table):
    """A FAIR student on the 2048 positions the bidder reaches (B = 128, Adam 1e-3, 400 steps = 25 epochs), judged on the positions
    of a rollout with another seed: mean L_pol falls to a quarter or less, and the held-out agreement is no more than 0.02 below
    what the plain torch-autograd composition reaches from the same initial network with the same permutations and steps.
    Measured (MI355X): held-out mean L_pol 2.766 before, 0.0168 after; agreement 0.093 before, 0.949 after; the torch composition
    reaches L_pol 0.0169 and agreement 0.947."""
    from brl_amd import distill, sl
    teacher, (hobs, hmask) = table["teacher"], table["held"]
    ev = lambda net: distill.distill_evaluate(net, [teacher], hobs, hmask, None, 1.0, C_POL, C_VAL)     # noqa: E731
    net, st = _step(table, "FAIR", graph=True)
    before = ev(net)
    gen = torch.Generator(device=DEV).manual_seed(11)
    epochs = LEARN_STEPS // (table["n"] // BATCH)
    for _ in range(epochs):
        st.epoch(table["n"], gen)
    after = ev(net)
    # the yardstick: the same training by torch autograd alone
    ref = _student("FAIR")
    opt = sl.make_optimizer(ref, 1e-3)
    obs, mask = table["train"]
    w = torch.ones(1, device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(11)
    for _ in range(epochs):
        perm = torch.randperm(table["n"], generator=gen, device=DEV)
        for i in range(table["n"] // BATCH):
            idx = perm[i * BATCH:(i + 1) * BATCH]
            logits, value = ref(obs[idx].float())
            loss = _torch_loss(logits, value, table["heads"][:, idx], w, mask[idx], 1.0, C_POL, C_VAL)
            opt.zero_grad(set_to_none=False)
            loss.backward()
            opt.step()
    yard = ev(ref)
    print(f"held-out before {before}\nafter {after}\ntorch composition {yard}")
    assert after["policy_loss"] <= 0.25 * before["policy_loss"], (before, after)
    assert after["agreement"] >= yard["agreement"] - 0.02, (after, yard)


# ---- ensemble and CLI -----------------------------------------------------------------------------------------------------------
def test_an_ensemble_of_two(table, dds):
    """K = 2, the bidder and a freshly initialised network at 0.75 / 0.25: the targets of the teachers' own heads equal the
    restatement's, teachers that are one object share a forward, and one ``train_distill`` iteration runs"""
    from brl_amd import distill
    teacher, other = table["teacher"], _student("DeepMind", seed=9)
    obs, mask = table["held"]
    obs, mask = obs[:777], mask[:777]
    w = distill.mixture_weights("0.75,0.25", 2)
    q, vstar, hq = torch.empty((777, 38), device=DEV), torch.empty(777, device=DEV), torch.empty(777, device=DEV)
    heads = distill.ensemble_targets([teacher, other], _dev(w), obs, mask, 2.0, q, vstar, hq)
    h = heads.cpu().numpy()
    m = mask.cpu().numpy()
    want64, want32 = (R.targets(h[:, :, :38], h[:, :, 38], w.astype(dt), m, 2.0, dt) for dt in (np.float64, np.float32))
    for got, a, b, name in zip((q, vstar, hq), want64, want32, ("q", "vstar", "hq")):
        err, tol = float(np.abs(got.cpu().numpy().astype(np.float64) - a).max()), R.tolerance(a, b)
        print(f"ensemble {name}: error {err:.3e}, bound {tol:.3e}")
        assert err <= tol, (name, err, tol)
    twice = distill.teacher_heads([teacher, other, teacher], obs)
    assert torch.equal(twice[0], twice[2]) and torch.equal(twice[:2], heads)
    logs = []
    cfg = dict(type_of_model="FAIR", num_envs=N_ENVS, num_steps=N_STEPS, minibatch_size=BATCH, iterations=1, update_epochs=1, eval_every=0,
               teacher_weights="0.75,0.25", learning_rate=1e-3, rng_seed=3)
    net = distill.train_distill(cfg, log=logs.append, teachers=[teacher, other], lut=(dds["keys"], dds["values"]))
    assert logs[0]["steps"] == 16 and all(np.isfinite(logs[0]["train/" + k]) for k in distill.METRICS) and logs[0]["train/policy_loss"] > 0.0
    assert all(bool(torch.isfinite(p).all()) for p in net.parameters())


def test_cli_end_to_end(table, dds, tmp_path):
    from brl_amd import checkpoint, distill
    from brl_amd.train import parse_cli
    teacher_path, save, lut = tmp_path / "teacher.pt", tmp_path / "save", tmp_path / "lut.npy"
    checkpoint.save_params(table["teacher"], str(teacher_path))
    np.save(lut, np.stack([dds["keys"], dds["values"]]))
    args = [f"teacher_model_path={teacher_path}", f"save_path={save}", f"dds_path={lut}", "iterations=2", "eval_every=1", "type_of_model=FAIR",
            f"num_envs={N_ENVS}", f"num_steps={N_STEPS}", f"minibatch_size={BATCH}", "num_eval_envs=64", "learning_rate=0.001"]
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "brl_amd.distill"] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(os.listdir(save)) == ["params-1.pkl", "params-2.pkl"]
    for key in ("train/policy_loss", "train/agreement", "test/policy_loss", "test/agreement", "test/imp", "IMP vs teacher 0"):
        assert key in r.stdout, key
    net = distill.train_distill(parse_cli(args, defaults=distill.DISTILL_DEFAULTS), log=lambda m: None)
    loaded = checkpoint.load_params(str(save / "params-2.pkl"), "relu", "FAIR", DEV)
    x = table["held"][0][:64].float()
    with torch.no_grad():
        for a, b in zip(loaded(x), net(x)):
            assert torch.allclose(a, b, rtol=1e-6, atol=1e-6)
    r = subprocess.run([sys.executable, "-m", "brl_amd.eval", f"team1_model_path={save / 'params-2.pkl'}", "team1_model_type=FAIR",
                        f"team2_model_path={teacher_path}", "num_eval_envs=64", f"dds_path={lut}"], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert [ln for ln in r.stdout.splitlines() if ln.startswith("IMP: ")]
