"""PPO update (src/update.py) on CPU: loss values against an independent numpy restatement, one
optimiser step, and the world_size-2 gloo gradient all-reduce."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from brl_amd.models import make_forward_pass
from brl_amd.roll_out import Transition
from brl_amd.update import allreduce_gradients, make_optimizer, make_update_step, ppo_loss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = {"lr": 1e-3, "clip_eps": 0.2, "ent_coef": 0.001, "vf_coef": 0.5, "value_clipping": True,
       "global_gradient_clipping": True, "max_grad_norm": 0.5, "update_epochs": 2, "minibatch_size": 64,
       "actor_illegal_action_mask": True, "illegal_action_l2norm_coef": 0.0, "reward_scaling": False}


def fake_batch(T, N, seed=0):
    g = torch.Generator().manual_seed(seed)
    mask = torch.rand(T, N, 38, generator=g) < 0.4
    mask[..., 0] = True
    action = torch.multinomial(mask.reshape(-1, 38).float(), 1, generator=g).reshape(T, N).int()
    nl = mask.sum(-1).float()
    tb = Transition(done=torch.rand(T, N, generator=g) < 0.1, action=action, value=torch.randn(T, N, generator=g) * 0.1,
                    reward=torch.randn(T, N, generator=g) * 0.05, log_prob=-torch.log(nl),
                    obs=torch.rand(T, N, 480, generator=g) < 0.1, legal_action_mask=mask)
    return tb, torch.randn(T, N, generator=g), torch.randn(T, N, generator=g)


def numpy_loss(cfg, logits, value, b, gae, tgt):
    """src/update.py:90-167 restated with numpy in float64."""
    logits, value, gae, tgt = (np.asarray(x, np.float64) for x in (logits, value, gae, tgt))
    mask = np.asarray(b.legal_action_mask)
    ml = np.where(mask, logits, -1e30)
    ml = ml - ml.max(1, keepdims=True)
    lsm = ml - np.log(np.exp(ml).sum(1, keepdims=True))
    a = np.asarray(b.action, np.int64)
    lp = lsm[np.arange(len(a)), a]
    old_v, old_lp = np.asarray(b.value, np.float64), np.asarray(b.log_prob, np.float64)
    vc = old_v + np.clip(value - old_v, -cfg["clip_eps"], cfg["clip_eps"])
    vl = 0.5 * np.maximum((value - tgt) ** 2, (vc - tgt) ** 2).mean()
    ratio = np.exp(lp - old_lp)
    la = -np.minimum(ratio * gae, np.clip(ratio, 1 - cfg["clip_eps"], 1 + cfg["clip_eps"]) * gae).mean()
    p = np.exp(lsm)
    ent = -(np.where(mask, p * lsm, 0.0)).sum(1).mean()
    ul = logits - logits.max(1, keepdims=True)
    probs = np.exp(ul) / np.exp(ul).sum(1, keepdims=True)
    ill = np.linalg.norm(probs * ~mask, ord=2) / 2          # src/update.py:136-141 (2-D ord=2: largest singular value)
    total = la + cfg["vf_coef"] * vl - cfg["ent_coef"] * ent + cfg.get("illegal_action_l2norm_coef", 0.0) * ill
    return total, vl, la, ent, ill


def test_loss_matches_numpy_restatement():
    tb, adv, tgt = fake_batch(4, 32)
    flat = Transition(*[x.reshape((128,) + x.shape[2:]) for x in tb])
    fp = make_forward_pass("relu", "DeepMind")
    net = fp.init(0)
    with torch.no_grad():
        logits, value = fp.apply(net, flat.obs.float())
        total, aux = ppo_loss(CFG, logits, value, flat, adv.reshape(-1), tgt.reshape(-1))
    want = numpy_loss(CFG, logits, value, flat, adv.reshape(-1), tgt.reshape(-1))
    assert abs(float(total) - want[0]) < 1e-5   # fp32 vs fp64
    assert abs(float(aux[0]) - want[1]) < 1e-5 and abs(float(aux[1]) - want[2]) < 1e-5 and abs(float(aux[2]) - want[3]) < 1e-5
    # the illegal-action norm is logged whatever its coefficient (src/update.py:136-141): SVD-free estimate, 1e-4 relative
    assert abs(float(aux[5]) - want[4]) < 1e-4 * want[4] and want[4] > 0
    cfg = dict(CFG, illegal_action_l2norm_coef=0.3)  # with a coefficient: the exact, differentiable norm joins the loss
    total2, aux2 = ppo_loss(cfg, logits, value, flat, adv.reshape(-1), tgt.reshape(-1))
    want2 = numpy_loss(cfg, logits, value, flat, adv.reshape(-1), tgt.reshape(-1))
    assert abs(float(total2) - want2[0]) < 1e-5 and abs(float(aux2[5]) - want2[4]) < 1e-5


def test_spectral_norm_without_svd():
    from brl_amd.update import spectral_norm_nonneg
    g = torch.Generator().manual_seed(1)
    for shape in ((1024, 38), (64, 38), (5, 38)):
        a = torch.rand(shape, generator=g) * (torch.rand(shape, generator=g) < 0.6)
        want = float(torch.linalg.matrix_norm(a.double(), ord=2))
        assert abs(float(spectral_norm_nonneg(a)) - want) < 1e-4 * want
    assert float(spectral_norm_nonneg(torch.zeros(8, 38))) == 0.0


def test_update_step_shapes_and_progress():
    tb, adv, tgt = fake_batch(4, 64)
    fp = make_forward_pass("relu", "FAIR")
    net = fp.init(1)
    cfg = dict(CFG)
    upd = make_update_step(cfg, fp)
    before = [p.clone() for p in net.parameters()]
    rs, (total, aux) = upd((net, None, None, None, 0, 7), tb, adv, tgt)
    assert total.shape == (2, 4) and len(aux) == 6 and aux[0].shape == (2, 4)
    assert any(not torch.equal(a, b) for a, b in zip(before, net.parameters()))
    assert torch.isfinite(total).all() and rs[5] == 8
    # value loss on the SAME data goes down over epochs of a larger-lr run
    cfg2 = dict(CFG, lr=3e-3, update_epochs=6, ent_coef=0.0)
    net2 = fp.init(2)
    _, (_, aux2) = make_update_step(cfg2, fp)((net2, None, None, None, 0, 3), tb, adv, tgt)
    assert float(aux2[0][-1].mean()) < float(aux2[0][0].mean())


def check_update_against_numpy(device, graph, T=4, N=256, seed=0):
    """One PPO minibatch step (minibatch = the whole batch, one epoch, fresh Adam) of brl_amd.update on `device` vs
    the float64 numpy restatement tests/ppo_numpy.py: losses, every weight and bias gradient, the pre-clip gradient norm, and
    every parameter after the step.  Tolerances: fp32 GEMMs vs fp64 — loss terms 2e-5 absolute, gradients 2e-5 of the largest
    one (the bound of the FAIR step's check); a parameter moves by lr * g / (|g| + 1e-5) on its first Adam step, so 2 % of lr
    bounds the effect of a 1e-3 relative gradient error.  The gradients left behind: FusedMinibatch keeps the pre-clip ones in its
    flat buffer (its sweep scales them in registers) and reports the pre-clip norm; the eager path's clip_grad_norm_ scales `.grad`
    in place by min(1, max_norm / (norm + 1e-6)) — against float64's own factor, which checks the norm."""
    from brl_amd.update import FusedStep
    from tests.ppo_numpy import adam_first_step, loss_and_grads, params_of
    tb, adv, tgt = fake_batch(T, N, seed=seed)
    B = T * N
    cfg = dict(CFG, minibatch_size=B, update_epochs=1, lr=1e-3, graph_update=graph)
    fp = make_forward_pass("relu", "DeepMind")
    net = fp.init(4, device=device)
    P0 = params_of(net)
    flat = Transition(*[x.reshape((B,) + x.shape[2:]) for x in tb])
    perm = torch.randperm(B, generator=torch.Generator(device=device).manual_seed(9 & 0x7FFFFFFF), device=device).cpu()
    # (the loss is a mean over the minibatch: the permutation only changes the summation order)
    want_total, want_aux, G = loss_and_grads(cfg, P0, flat.obs.numpy(), flat.legal_action_mask.numpy(),
                                             flat.action.numpy().astype(np.int64), flat.value.double().numpy(),
                                             flat.log_prob.double().numpy(), adv.reshape(-1).double().numpy(),
                                             tgt.reshape(-1).double().numpy())
    P1, gn = adam_first_step(cfg, P0, G)
    tbd = Transition(*[x.to(device) for x in tb])
    rs, (total, aux) = make_update_step(cfg, fp)((net, None, None, None, 0, 9), tbd, adv.to(device), tgt.to(device))
    if graph:
        assert rs[1].get("graphed"), rs[1].get("graph_error")
    assert abs(float(total[0, 0]) - want_total) < 2e-5
    for k in range(5):
        assert abs(float(aux[k][0, 0]) - want_aux[k]) < 2e-5, k
    fused = rs[1].get("graphed")
    if isinstance(fused, FusedStep):
        assert abs(float(fused.norm[0]) - gn) < 1e-4 * gn, (float(fused.norm[0]), gn)
        clip = 1.0
    else:
        clip = min(1.0, cfg["max_grad_norm"] / (gn + 1e-6))
    scale = max(np.abs(gw).max() for gw, _ in G) * clip
    lins = list(net.body) + [net.actor, net.critic]
    for k, (lin, (gw, gb)) in enumerate(zip(lins, G)):
        assert np.abs(lin.weight.grad.detach().cpu().double().numpy() - clip * gw).max() < 2e-5 * scale + 1e-9, ("dW", k)
        assert np.abs(lin.bias.grad.detach().cpu().double().numpy() - clip * gb).max() < 2e-5 * scale + 1e-9, ("db", k)
    got = params_of(net)
    worst = max(max(np.abs(a - c).max(), np.abs(b - d).max()) for (a, b), (c, d) in zip(got, P1))
    moved = max(np.abs(a - c).max() for (a, _), (c, _) in zip(P0, P1))
    assert worst < 0.02 * cfg["lr"] and moved > 0.5 * cfg["lr"], (worst, moved, gn)
    return perm


def test_update_step_matches_numpy_restatement_cpu():
    check_update_against_numpy("cpu", graph=False, T=2, N=128)


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    fp = make_forward_pass("relu", "FAIR")
    net = fp.init(5)                      # same initial weights on every rank
    tb, adv, tgt = fake_batch(2, 64, seed=100 + rank)   # different data shard per rank
    upd = make_update_step(dict(CFG, update_epochs=1), fp)
    upd((net, None, None, None, 0, 1), tb, adv, tgt)
    flat = torch.cat([p.detach().reshape(-1) for p in net.parameters()])
    gathered = [torch.empty_like(flat) for _ in range(world)]
    dist.all_gather(gathered, flat)
    if rank == 0:
        torch.save(gathered, os.path.join(out_dir, "params.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_gradient_allreduce_keeps_ranks_in_sync(tmp_path):
    mp.start_processes(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True, start_method="spawn")
    g = torch.load(tmp_path / "params.pt")
    assert torch.equal(g[0], g[1])        # identical parameters after all-reduced updates on different shards


def test_allreduce_is_noop_without_process_group():
    fp = make_forward_pass("relu", "FAIR")
    net = fp.init(0)
    for p in net.parameters():
        p.grad = torch.ones_like(p)
    allreduce_gradients(net)
    assert all(bool((p.grad == 1).all()) for p in net.parameters())


def test_inference_snapshot_matches_module_cpu():
    """models.InferenceSnapshot (fused bias+ReLU epilogue, merged heads) == the module's own forward; refresh()
    re-reads updated weights into the same tensors (their addresses are baked into captured graphs).  On a network whose biases
    are not hk.Linear's zeros, "updated" by a second perturbation (scaling would leave a zero bias zero)."""
    import torch
    from brl_amd.models import InferenceSnapshot, make_forward_pass
    from tests.nets import perturbed
    fp = make_forward_pass("relu", "DeepMind")
    net = perturbed(fp.init(5), 31)
    x = (torch.rand(64, 480) < 0.1)
    snap = InferenceSnapshot.make(net)
    assert snap is not None
    with torch.no_grad():
        lg, v = net(x.float())
        lg2, v2 = snap(x)
    assert lg2.shape == (64, 38) and v2.shape == (64,)
    assert torch.allclose(lg, lg2, atol=1e-5) and torch.allclose(v, v2, atol=1e-5)
    ptrs = [w.data_ptr() for w, _ in snap.body] + [snap.head_w.data_ptr()]
    with torch.no_grad():
        perturbed(net, 32)
        snap.refresh(net)
        lg3, v3 = net(x.float())
        lg4, v4 = snap(x)
    assert torch.allclose(lg3, lg4, atol=1e-5) and torch.allclose(v3, v4, atol=1e-5)
    assert float((lg3 - lg).abs().max()) > 1e-2 and float((v3 - v).abs().max()) > 1e-2     # (the update did move the outputs)
    assert ptrs == [w.data_ptr() for w, _ in snap.body] + [snap.head_w.data_ptr()]
    assert InferenceSnapshot.make(make_forward_pass("relu", "FAIR").init(0)) is None  # not covered: callers fall back


@pytest.mark.parametrize("activation", ["relu", "tanh"])
def test_fair_numpy_restatement_matches_autograd_in_float64(activation):
    """tests/ppo_numpy.py's FAIR forward / backward (the checker of brl_amd.fused_update.FusedFair) against torch autograd through
    the module itself, both in float64: every gradient to 1e-12."""
    from brl_amd.update import ppo_loss
    from tests.ppo_numpy import fair_loss_and_grads, fair_params_of
    net = make_forward_pass(activation, "FAIR").init(3).double()
    tb, adv, tgt = fake_batch(2, 64, seed=1)
    B = 128
    flat = Transition(*[x.reshape((B,) + x.shape[2:]) for x in tb])
    logits, value = net(flat.obs.double())
    b64 = Transition(flat.done, flat.action, flat.value.double(), flat.reward, flat.log_prob.double(), flat.obs, flat.legal_action_mask)
    total, _ = ppo_loss(dict(CFG), logits, value, b64, adv.reshape(-1).double(), tgt.reshape(-1).double())
    total.backward()
    wt, _, G = fair_loss_and_grads(dict(CFG), fair_params_of(net), flat.obs.numpy(), flat.legal_action_mask.numpy(),
                                   flat.action.numpy().astype(np.int64), flat.value.double().numpy(), flat.log_prob.double().numpy(),
                                   adv.reshape(-1).double().numpy(), tgt.reshape(-1).double().numpy(), activation=activation)
    assert abs(float(total.detach()) - wt) < 1e-12
    for lin, (gw, gb) in zip(list(net.l) + [net.actor, net.critic], G):
        assert np.abs(lin.weight.grad.numpy() - gw).max() < 1e-12 and np.abs(lin.bias.grad.numpy() - gb).max() < 1e-12


def _batch64(B, seed):
    """(flat batch, its float64 copy for ppo_loss, numpy arguments of the restatement) of one B-sample minibatch"""
    tb, adv, tgt = fake_batch(1, B, seed=seed)
    flat = Transition(*[x.reshape((B,) + x.shape[2:]) for x in tb])
    b64 = Transition(flat.done, flat.action, flat.value.double(), flat.reward, flat.log_prob.double(), flat.obs, flat.legal_action_mask)
    args = (flat.obs.numpy(), flat.legal_action_mask.numpy(), flat.action.numpy().astype(np.int64), flat.value.double().numpy(),
            flat.log_prob.double().numpy(), adv.reshape(-1).double().numpy(), tgt.reshape(-1).double().numpy())
    return flat, b64, adv.reshape(-1).double(), tgt.reshape(-1).double(), args


def _perturb(net, seed):
    """hk.Linear's zero biases would hide a bias mix-up: every parameter moved a little (tests/nets.py)"""
    from tests.nets import perturbed
    perturbed(net, seed)


# the switches of the PPO step (src/update.py): each one changes the loss or its gradient
SWITCHES = {"defaults": {}, "unmasked": {"actor_illegal_action_mask": False}, "no_value_clipping": {"value_clipping": False},
            "reward_scaling": {"reward_scaling": True}, "illegal_coef": {"illegal_action_l2norm_coef": 0.5},
            "all": {"actor_illegal_action_mask": False, "value_clipping": False, "reward_scaling": True, "illegal_action_l2norm_coef": 0.3}}


@pytest.mark.parametrize("activation,model,switch", [
    ("relu", "DeepMind", "defaults"), ("tanh", "DeepMind", "defaults"), ("relu", "DeepMind_6", "defaults"), ("relu", "DeepMind_8", "defaults"),
    ("relu", "DeepMind", "unmasked"), ("relu", "DeepMind", "no_value_clipping"), ("relu", "DeepMind", "reward_scaling"),
    ("relu", "DeepMind", "illegal_coef"), ("tanh", "DeepMind", "illegal_coef"), ("tanh", "DeepMind_6", "all")])
def test_deepmind_numpy_restatement_matches_autograd_in_float64(activation, model, switch):
    """tests/ppo_numpy.py's DeepMind forward / `head_loss` / backward (the checker of brl_amd.fused_update.FusedMinibatch) against
    torch autograd through the module and brl_amd.update.ppo_loss, both in float64: the loss, the six logged terms and every
    gradient to 1e-12, for every activation, depth and switch of the step."""
    from brl_amd.update import ppo_loss
    from tests.ppo_numpy import loss_and_grads, params_of
    cfg = dict(CFG, **SWITCHES[switch])
    net = make_forward_pass(activation, model).init(3).double()
    _perturb(net, 5)
    flat, b64, adv, tgt, args = _batch64(96, seed=2)
    logits, value = net(flat.obs.double())
    total, aux = ppo_loss(cfg, logits, value, b64, adv, tgt)
    total.backward()
    wt, waux, G = loss_and_grads(cfg, params_of(net), *args, activation=activation)
    assert abs(float(total.detach()) - wt) < 1e-12
    for k in range(6):
        # (clipfrac is a mean of fp32 0/1 flags; without a coefficient the logged norm is the SVD-free estimate)
        tol = {4: 1e-7, 5: 1e-12 if cfg["illegal_action_l2norm_coef"] else 1e-4 * waux[5]}.get(k, 1e-12)
        assert abs(float(aux[k]) - waux[k]) < tol, k
    lins = list(net.body) + [net.actor, net.critic]
    assert len(G) == len(lins) == (int(model.split("_")[1]) if "_" in model else 4) + 2
    for k, (lin, (gw, gb)) in enumerate(zip(lins, G)):
        assert np.abs(lin.weight.grad.numpy() - gw).max() < 1e-12 and np.abs(lin.bias.grad.numpy() - gb).max() < 1e-12, k


def test_deepmind_restatement_gate_override():
    """loss_and_grads' gate_fn (how a checker of a fp32 step takes that step's own ReLU gates): the default gate given back changes
    nothing; one flipped gate changes that unit's bias gradient"""
    from tests.ppo_numpy import loss_and_grads, params_of
    net = make_forward_pass("relu", "DeepMind").init(3).double()
    _perturb(net, 5)
    _, _, _, _, args = _batch64(32, seed=4)
    P = params_of(net)
    _, _, G0 = loss_and_grads(dict(CFG), P, *args)
    _, _, G1 = loss_and_grads(dict(CFG), P, *args, gate_fn=lambda k, z, h: z > 0)
    assert all(np.array_equal(a, c) and np.array_equal(b, d) for (a, b), (c, d) in zip(G0, G1))

    def flip(k, z, h):
        g = z > 0
        if k == 2:
            g[7, 11] = ~g[7, 11]
        return g
    _, _, G2 = loss_and_grads(dict(CFG), P, *args, gate_fn=flip)
    assert abs(G0[2][1][11] - G2[2][1][11]) > 1e-9


@pytest.mark.parametrize("activation,switch", [("relu", "illegal_coef"), ("tanh", "all")])
def test_fair_numpy_restatement_with_switches_matches_autograd_in_float64(activation, switch):
    """the FAIR checker through `head_loss` with the step's switches (the illegal-action term included) against autograd, float64"""
    from brl_amd.update import ppo_loss
    from tests.ppo_numpy import fair_loss_and_grads, fair_params_of
    cfg = dict(CFG, **SWITCHES[switch])
    net = make_forward_pass(activation, "FAIR").init(3).double()
    _perturb(net, 6)
    flat, b64, adv, tgt, args = _batch64(128, seed=1)
    logits, value = net(flat.obs.double())
    total, _ = ppo_loss(cfg, logits, value, b64, adv, tgt)
    total.backward()
    wt, _, G = fair_loss_and_grads(cfg, fair_params_of(net), *args, activation=activation)
    assert abs(float(total.detach()) - wt) < 1e-12
    for lin, (gw, gb) in zip(list(net.l) + [net.actor, net.critic], G):
        assert np.abs(lin.weight.grad.numpy() - gw).max() < 1e-12 and np.abs(lin.bias.grad.numpy() - gb).max() < 1e-12


def test_fair_restatement_gate_override():
    """fair_loss_and_grads' gate_fn (how a checker of a fp32 step takes that step's own ReLU gates): it is asked at the twelve
    activation sites in order, with the linear layer behind each and the shortcut at the two residual sums; the default gate given
    back reproduces gate_fn=None bit for bit and still equals autograd in float64; one flipped gate at a residual sum changes the
    gradients upstream of it"""
    from brl_amd.update import ppo_loss
    from tests.ppo_numpy import fair_loss_and_grads, fair_params_of
    net = make_forward_pass("relu", "FAIR").init(3).double()
    _perturb(net, 6)
    flat, b64, adv, tgt, args = _batch64(48, seed=3)
    P = fair_params_of(net)
    t0, a0, G0 = fair_loss_and_grads(dict(CFG), P, *args)
    seen = []

    def default(site, z, layer, h_in, shortcut):
        seen.append((site, layer, shortcut is not None))
        pre = h_in @ P[layer][0].T + P[layer][1]
        assert np.array_equal(z, pre if shortcut is None else np.maximum(pre, 0.0) + shortcut)
        return z > 0
    t1, a1, G1 = fair_loss_and_grads(dict(CFG), P, *args, gate_fn=default)
    assert seen == [(s, l, s in (3, 9)) for s, l in enumerate((0, 1, 2, 2, 3, 4, 6, 7, 8, 8, 9, 10))]
    assert t0 == t1 and a0 == a1
    assert all(np.array_equal(a, c) and np.array_equal(b, d) for (a, b), (c, d) in zip(G0, G1))
    logits, value = net(flat.obs.double())
    total, _ = ppo_loss(dict(CFG), logits, value, b64, adv, tgt)
    total.backward()
    assert abs(float(total.detach()) - t1) < 1e-12
    for lin, (gw, gb) in zip(list(net.l) + [net.actor, net.critic], G1):
        assert np.abs(lin.weight.grad.numpy() - gw).max() < 1e-12 and np.abs(lin.bias.grad.numpy() - gb).max() < 1e-12

    def flip(site, z, layer, h_in, shortcut):
        g = z > 0
        if site == 3:
            g[7, 11] = ~g[7, 11]
        return g
    _, _, G2 = fair_loss_and_grads(dict(CFG), P, *args, gate_fn=flip)
    assert np.abs(G0[0][1] - G2[0][1]).max() > 1e-9 and np.array_equal(G0[5][0], G2[5][0]) is False
    # (tanh has no gate: the hook is not consulted)
    assert fair_loss_and_grads(dict(CFG), P, *args, activation="tanh", gate_fn=flip)[0] == fair_loss_and_grads(dict(CFG), P, *args, activation="tanh")[0]


def _fair_case_names():
    from tests.test_gpu_update_float64 import FAIR_CASES
    return list(FAIR_CASES)


@pytest.mark.parametrize("case", _fair_case_names())
def test_fair_float64_cases_meet_their_input_conditions(case):
    """tests/test_gpu_update_float64.test_fused_fair_step_matches_float64 caps, per step, the ReLU pre-activations inside their fp32
    rounding band (where it takes the GPU step's own gate) at 1e-4 of all and the samples at PPO's clip kinks at 2 of each kind.
    Both are properties of the case's inputs — its seeded network and batches — so they are checked here in float64 alone, with
    z > 0 in place of the stored gates and the parameters of steps 2 and 3 from the float64 Adam step rounded to fp32: a seed that
    misses a cap is changed here, before the case ever runs on a GPU."""
    from tests.ppo_numpy import adam_step, fair_loss_and_grads, fair_params_of
    from tests.test_gpu_update_float64 import AMBIGUOUS_CAP, FAIR_SITES, KINK_CAP, LR, fair_case, fair_input_conditions
    activation, B, cfg, _, seed, _, net = fair_case(case, "cpu")
    P = fair_params_of(net)
    M = [(np.zeros_like(W), np.zeros_like(b)) for W, b in P]
    V = [(np.zeros_like(W), np.zeros_like(b)) for W, b in P]
    for t in (1, 2, 3):
        _, _, _, _, args = _batch64(B, seed=seed + t)
        lr_t = LR * (1.0 - (t - 1) / cfg["num_updates"]) if cfg.get("anneal_lr") else LR
        n_amb, n_ratio, n_value, gate_fn = fair_input_conditions(cfg, P, args, activation)
        assert n_ratio <= KINK_CAP and n_value <= KINK_CAP, (t, n_ratio, n_value)
        assert n_amb <= AMBIGUOUS_CAP * B * len(FAIR_SITES) * P[0][0].shape[0], (t, n_amb)
        _, _, G = fair_loss_and_grads(cfg, P, *args, activation=activation, gate_fn=gate_fn)
        P, M, V, _ = adam_step(cfg, t, P, M, V, G, lr=lr_t)
        P = [tuple(x.astype(np.float32).astype(np.float64) for x in pair) for pair in P]


def _deepmind_case_names():
    from tests.test_gpu_update_float64 import CASES
    return list(CASES)


@pytest.mark.parametrize("case", _deepmind_case_names())
def test_deepmind_float64_cases_meet_their_input_conditions(case):
    """The twin of test_fair_float64_cases_meet_their_input_conditions for tests/test_gpu_update_float64.test_fused_deepmind_step_matches_float64,
    whose cases start from a perturbed network (deepmind_case): per step, the ReLU pre-activations inside their fp32 rounding band at
    most 1e-4 of all, the samples at PPO's clip kinks at most 2 of each kind — in float64 alone, z > 0 in place of the stored gates,
    the parameters of steps 2 and 3 from the float64 Adam step rounded to fp32.  A seed that misses a cap is changed in
    DEEPMIND_BATCH_SEEDS, never the cap."""
    from tests.ppo_numpy import adam_step, loss_and_grads, params_of
    from tests.test_gpu_update_float64 import AMBIGUOUS_CAP, KINK_CAP, LR, deepmind_case, deepmind_input_conditions
    activation, _, B, cfg, seed, _, net = deepmind_case(case, "cpu")
    P = params_of(net)
    nl, H = len(P) - 2, P[0][0].shape[0]
    assert all(np.abs(b).min() > 0 for _, b in P)
    M = [(np.zeros_like(W), np.zeros_like(b)) for W, b in P]
    V = [(np.zeros_like(W), np.zeros_like(b)) for W, b in P]
    for t in (1, 2, 3):
        _, _, _, _, args = _batch64(B, seed=seed + t)
        lr_t = LR * (1.0 - (t - 1) / cfg["num_updates"]) if cfg.get("anneal_lr") else LR
        n_amb, n_ratio, n_value, gate_fn, _ = deepmind_input_conditions(cfg, P, args, activation)
        assert n_ratio <= KINK_CAP and n_value <= KINK_CAP, (t, n_ratio, n_value)
        assert n_amb <= AMBIGUOUS_CAP * B * H * nl, (t, n_amb)
        _, _, G = loss_and_grads(cfg, P, *args, activation=activation, gate_fn=gate_fn)
        P, M, V, _ = adam_step(cfg, t, P, M, V, G, lr=lr_t)
        P = [tuple(x.astype(np.float32).astype(np.float64) for x in pair) for pair in P]


@pytest.mark.parametrize("clipping,max_norm", [(True, 0.5), (True, 1e3), (False, 0.5)])
def test_adam_step_matches_torch_adam_in_float64(clipping, max_norm):
    """tests/ppo_numpy.adam_step — steps 1, 2 and 3 (bias-corrected, not sign-like after the first) — against
    torch.nn.utils.clip_grad_norm_ + torch.optim.Adam(eps=1e-5) in float64: parameters and both moments to 1e-15 relative of the
    parameters' scale; the pre-clip norm to 1e-12 relative.  max_norm 0.5 clips, 1e3 does not."""
    from tests.ppo_numpy import adam_step
    cfg = dict(CFG, global_gradient_clipping=clipping, max_grad_norm=max_norm, lr=3e-3)
    g = torch.Generator().manual_seed(7)
    shapes = [((16, 8), (16,)), ((3, 16), (3,))]
    P = [tuple(torch.randn(s, generator=g, dtype=torch.float64) for s in pair) for pair in shapes]
    tp = [torch.nn.Parameter(x.clone()) for pair in P for x in pair]
    opt = torch.optim.Adam(tp, lr=cfg["lr"], eps=1e-5)
    Pn = [tuple(x.numpy().copy() for x in pair) for pair in P]
    Mn = [tuple(np.zeros_like(x) for x in pair) for pair in Pn]
    Vn = [tuple(np.zeros_like(x) for x in pair) for pair in Pn]
    for t in (1, 2, 3):
        grads = [tuple(torch.randn(x.shape, generator=g, dtype=torch.float64) * (0.3 if t == 2 else 1.0) for x in pair) for pair in P]
        for q, gr in zip(tp, [x for pair in grads for x in pair]):
            q.grad = gr.clone()
        want_norm = float(torch.nn.utils.clip_grad_norm_(tp, max_norm)) if clipping else None
        opt.step()
        Pn, Mn, Vn, gn = adam_step(cfg, t, Pn, Mn, Vn, [tuple(x.numpy() for x in pair) for pair in grads])
        if clipping:
            assert abs(gn - want_norm) < 1e-12 * want_norm
        flat = lambda L: np.concatenate([x.reshape(-1) for pair in L for x in pair])   # noqa: E731
        assert np.abs(flat(Pn) - np.concatenate([q.detach().numpy().reshape(-1) for q in tp])).max() < 1e-15 * 10
        assert np.abs(flat(Mn) - np.concatenate([opt.state[q]["exp_avg"].numpy().reshape(-1) for q in tp])).max() < 1e-15
        assert np.abs(flat(Vn) - np.concatenate([opt.state[q]["exp_avg_sq"].numpy().reshape(-1) for q in tp])).max() < 1e-15


def test_fused_step_program_has_one_runner_for_both_strategies():
    """brl_amd.fused_update: the step program of kernel groups ("k"), collectives ("c") and waits ("w") has ONE interpreter.  The
    form of a backend that cannot be captured (every run of kernel groups = one graph, blocking collectives between the replays)
    calls the same stubs in the same order as the captured form; a blocking collective that hands back a work object all the same
    is waited for exactly once, at once; nothing is left in `_works`."""
    from brl_amd.fused_update import FusedStep, _graph_kernel_runs
    calls, works = [], []

    class Work:
        def __init__(self, key):
            self.key, self.waits = key, 0

        def wait(self):
            self.waits += 1
            calls.append(("wait", self.key))

    def k(name):
        return ("k", lambda: calls.append(("k", name)))

    def c(key):
        def issue(async_op):
            calls.append(("c", key))
            works.append(Work(key))
            return works[-1]
        return ("c", key, issue)

    # (the shape of the sharded program: parameters gathered by the step before, gradients reduced bucket by bucket)
    program = [("w", "ag1"), k("fwd0"), ("w", "ag0"), k("fwd1"), k("heads"), k("dw1"), c("rs0"), k("dz1"), k("dw0"), c("rs1"),
               ("w", "rs0"), ("w", "rs1"), k("norm"), c("agn"), ("w", "agn"), k("adam"), c("ag1"), c("ag0")]
    launches = lambda: [x for x in calls if x[0] != "wait"]   # noqa: E731
    fs = FusedStep.__new__(FusedStep)
    fs._works = {}
    for _ in range(2):
        fs._run_program(program, True)
    fs._drain()
    captured = launches()
    assert captured == 2 * [("k", "fwd0"), ("k", "fwd1"), ("k", "heads"), ("k", "dw1"), ("c", "rs0"), ("k", "dz1"), ("k", "dw0"), ("c", "rs1"),
                            ("k", "norm"), ("c", "agn"), ("k", "adam"), ("c", "ag1"), ("c", "ag0")]
    assert [w.waits for w in works] == [1] * 10 and fs._works == {}
    assert calls.index(("wait", "ag1")) > calls.index(("c", "ag0"))        # (waited for by the NEXT step, not at once)

    class Graph:                             # stands for a captured run of kernel groups
        def __init__(self, fn):
            self.replay = fn

    eager = _graph_kernel_runs(program, lambda fns: [Graph(fn) for fn in fns])
    assert [item[0] for item in eager] == ["w", "w", "k", "c", "k", "c", "w", "w", "k", "c", "w", "k", "c", "c"]
    assert [item[1] for item in eager if item[0] != "k"] == ["ag1", "ag0", "rs0", "rs1", "rs0", "rs1", "agn", "agn", "ag1", "ag0"]
    del calls[:], works[:]
    for _ in range(2):
        fs._run_program(eager, False)
        assert fs._works == {}
    assert launches() == captured
    assert [w.waits for w in works] == [1] * 10
    for i, x in enumerate(calls):
        if x[0] == "c":
            assert calls[i + 1] == ("wait", x[1])
    # the kernel groups alone (the constructor's first launches): the same runner over the "k" items
    del calls[:]
    fs._run_program([item for item in program if item[0] == "k"], False)
    assert calls == [x for x in captured[:13] if x[0] == "k"]


def test_fused_step_table_builders_hold_addresses_strides_and_shapes():
    """brl_amd.fused_update._gemm_group_tables: the nine arrays of a grouped weight-gradient launch, element for element, from
    views with row strides of their own; _segment_tables: tensors and raw addresses mixed"""
    from brl_amd.fused_update import _gemm_group_tables, _segment_tables
    x, y, z = torch.zeros(5, 7), torch.zeros(6, 9), torch.zeros(4, 10)
    w = torch.zeros(3, 2, 5)
    a = [x[:, :3], y[1:, 2:6]]               # [5, 3] rows 7 apart; [5, 4] rows 9 apart, 9 + 2 floats into y
    b = [z[:, 4:], w[1]]                     # [4, 6] rows 10 apart, 4 floats into z; [2, 5] contiguous, 10 floats into w
    c = [y[:3, :6], w[2].t()[:, :1]]         # [3, 6] rows 9 apart; [5, 1]: rows 1 apart, 20 floats into w
    t = _gemm_group_tables(a, b, c, 5)
    assert len(t) == 9 and all(len(arr) == 2 for arr in t)
    assert [list(arr) for arr in t] == [[x.data_ptr(), y.data_ptr() + 4 * 11], [7, 9],
                                        [z.data_ptr() + 4 * 4, w.data_ptr() + 4 * 10], [10, 5],
                                        [y.data_ptr(), w.data_ptr() + 4 * 20], [9, 1],
                                        [3, 5], [6, 1], [5, 5]]
    import ctypes
    assert [arr._type_ for arr in t] == [ctypes.c_void_p, ctypes.c_int64] * 3 + [ctypes.c_int64] * 3
    parts, cols, tiles, outs = _segment_tables([x, y.data_ptr() + 8, z[2:]], [7, 9, 10], [5, 6, 2], [w.data_ptr(), w[1], w.data_ptr() + 80])
    assert list(parts) == [x.data_ptr(), y.data_ptr() + 8, z.data_ptr() + 4 * 20] and list(cols) == [7, 9, 10]
    assert list(tiles) == [5, 6, 2] and list(outs) == [w.data_ptr(), w.data_ptr() + 40, w.data_ptr() + 80]
    assert [arr._type_ for arr in (parts, cols, tiles, outs)] == [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p]
