"""The fused PPO minibatch steps against float64, gradient by gradient and Adam step by Adam step.

``FusedMinibatch`` (the default step of the DeepMind MLPs, brl_amd/fused_update.py) writes its backward pass out by hand: the head's
dW / db ride in extra workgroups of the dz chain, the weight gradients are one grouped bf16x3 launch, the bias gradients are tile sums
that the clip + Adam launch finishes.  ``FusedFair`` (the FAIR residual net's step) is the other hand-written backward pass: forward,
loss and the whole backward chain of 16 rows per workgroup out of LDS (brl_fair_chain), the twelve weight gradients as one grouped
launch, one launch for every bias gradient; or, by minibatch size and switch, the same launch by launch on brl_mlp_gemm or on library
products.  Here every gradient either step leaves in its flat buffer, its pre-clip norm, its logged losses and the parameters / moments
after three successive Adam steps are compared with the float64 restatement tests/ppo_numpy.py (itself checked against torch autograd
in float64 by tests/test_update_cpu.py), for every switch and minibatch size that changes the code path inside the step
(test_fused_deepmind_step_matches_float64, test_fused_fair_step_matches_float64).  Also: the FAIR network's inference forward
(brl_fair_forward) after updates on each update path."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LR = 1e-3

# one parametrization per line of the step's code paths: (activation, model, minibatch, config overrides)
CASES = {
    "relu_defaults": ("relu", "DeepMind", 1024, {}),                       # bf16x3 dW (brl_mlp_gemm_x3_group), own GEMM dz chain
    "dw_library": ("relu", "DeepMind", 1024, {"dw_gemm": "library"}),     # torch.bmm + torch.mm weight gradients
    "no_own_gemm": ("relu", "DeepMind", 1024, {"own_gemm": False}),      # torch.mm + brl_act_bwd_colsum[_heads_dw]
    "own_gemm_fwd": ("relu", "DeepMind", 1024, {"own_gemm_fwd": True}),  # forward layers on brl_mlp_gemm too
    "tanh_x3": ("tanh", "DeepMind", 1024, {}),
    "DeepMind_6": ("relu", "DeepMind_6", 1024, {}),
    "DeepMind_8": ("relu", "DeepMind_8", 1024, {}),                        # 8 weight gradients: a full x3 group
    "reward_scaling": ("relu", "DeepMind", 1024, {"reward_scaling": True}),
    "unmasked": ("relu", "DeepMind", 1024, {"actor_illegal_action_mask": False}),
    "no_value_clipping": ("relu", "DeepMind", 1024, {"value_clipping": False}),
    "no_global_clipping": ("relu", "DeepMind", 1024, {"global_gradient_clipping": False}),
    "illegal_coef": ("relu", "DeepMind", 1024, {"illegal_action_l2norm_coef": 0.5}),   # brl_ppo_stats_gram + brl_ppo_illegal_grad
    "anneal_lr": ("relu", "DeepMind", 1024, {"anneal_lr": True, "num_minibatches": 1, "num_updates": 4}),
    "B96": ("relu", "DeepMind", 96, {}),       # bf16x3 on, a partial 64-row tile of the bias sums
    "B100": ("relu", "DeepMind", 100, {}),     # bf16x3 off (B % 32), own GEMM on (B % 4 == 0)
    "B333": ("relu", "DeepMind", 333, {}),     # both off, odd B
}


DEEPMIND_PERTURB_SEED = 22
# the seed of a case's batches (step t draws fake_batch(1, B, seed + t)): 200 unless that misses a cap of the input conditions
DEEPMIND_BATCH_SEEDS = {}
DEEPMIND_GATE_BAND = 4e-6   # of |h| |W| + |b|: the fp32 products' rounding band of a ReLU pre-activation


def deepmind_case(case, device):
    """-> (activation, model, B, cfg, seed of its batches, forward pass, its network on `device`): `init(4)` with N(0, 0.01) added to
    every weight and N(0, 0.1) to every bias, as `fair_case` — at hk.Linear's zero biases the step's first forward adds no bias at
    all and the later ones biases of magnitude lr.  (Drawn on the host, so the CPU check of the cases' inputs sees the same network.)"""
    from brl_amd.models import make_forward_pass
    from tests.nets import perturbed
    from tests.test_update_cpu import CFG
    activation, model, B, over = CASES[case]
    cfg = dict(CFG, lr=LR, minibatch_size=B, update_epochs=1, graph_update=True, **over)
    fp = make_forward_pass(activation, model)
    net = perturbed(fp.init(4), DEEPMIND_PERTURB_SEED)
    return activation, model, B, cfg, DEEPMIND_BATCH_SEEDS.get(case, 200), fp, net.to(device)


def deepmind_gate_fn(P, stored, ambiguous):
    """a gate_fn for tests/ppo_numpy.forward: z > 0, except where |z| is within DEEPMIND_GATE_BAND of the magnitude sum behind it —
    there the gate is stored[k] (the fp32 step's own; None: z > 0 all the same) and ambiguous[0] counts the entry"""
    def gate_fn(k, z, h_in):
        band = DEEPMIND_GATE_BAND * (np.abs(h_in) @ np.abs(P[k][0]).T + np.abs(P[k][1]))
        amb = np.abs(z) < band
        gate = z > 0
        if amb.any():
            ambiguous[0] += int(amb.sum())
            if stored is not None:
                gate[amb] = stored[k][amb]
        return gate
    return gate_fn


def deepmind_input_conditions(cfg, P, args, activation, stored=None):
    """the two conditions on a step's INPUTS, from float64 alone where stored is None -> (ambiguous ReLU entries, samples at the
    ratio kink, samples at the value kink, the gate_fn for the gradient pass with its counter)"""
    from tests.ppo_numpy import forward
    ambiguous = [0]
    gate_fn = deepmind_gate_fn(P, stored, ambiguous) if activation == "relu" else None
    logits, value, _, _, _ = forward(P, args[0].astype(np.float64), activation, gate_fn)
    n_ratio, n_value = _ppo_kinks(cfg, logits, value, args[1].astype(bool), args[2], args[3], args[4])
    return ambiguous[0], n_ratio, n_value, gate_fn, ambiguous


def _np(t):
    return t.detach().cpu().double().numpy()


def _ppo_kinks(cfg, logits, value, mask, action, old_value, old_lp, rel=1e-5):
    """samples whose ratio sits within `rel` of PPO's clip boundaries 1 +- clip_eps, or whose value change sits within `rel` of the
    value clip: there the derivative jumps, and a fp32 step may fall on the other side than float64"""
    eps = cfg["clip_eps"]
    masked = cfg.get("actor_illegal_action_mask", True)
    lg = np.where(mask, logits, -np.inf) if masked else logits
    lg = lg - lg.max(1, keepdims=True)
    lsm = lg - np.log(np.exp(lg).sum(1, keepdims=True))
    ratio = np.exp(lsm[np.arange(len(action)), action] - old_lp)
    n_ratio = int((np.minimum(np.abs(ratio - (1 - eps)), np.abs(ratio - (1 + eps))) < rel).sum())
    n_value = int((np.abs(np.abs(value - old_value) - eps) < rel).sum()) if cfg.get("value_clipping", True) else 0
    return n_ratio, n_value


@pytest.mark.parametrize("case", list(CASES))
def test_fused_deepmind_step_matches_float64(case):
    """Three successive update_step calls, each ONE minibatch step (batch = minibatch, update_epochs = 1), through FusedMinibatch, from
    a network whose every parameter is perturbed (deepmind_case: no bias is hk.Linear's zero, at the first step either); the
    float64 reference of step t starts from the GPU's own parameters and moments before it (copied to the host), so errors do not
    build up.  After each call:
      * the five logged losses within 2e-5 of float64 (with the illegal-action term the total also carries the fp32 Gram's 2e-6 relative
        error of sigma_1);
      * every weight and bias gradient left in the flat buffer (the `.grad` views), the [39, H] head included, within 2e-5 max|g| + 1e-9
        — the FAIR step's bound; the pre-clip norm (fm.norm) within 1e-4 relative;
      * parameters and both moments after step t against tests/ppo_numpy.adam_step(t) on the float64 gradients.  Parameters: 0.02 lr_t.
        A gradient error d moves a parameter by about lr_t d (1 - b1) / (1 - b1^t) / (sqrt(v_hat) + eps); at t = 1 that is lr d / (|g| +
        eps) (test_update_cpu.check_update_against_numpy's bound); at t = 2, 3 the factor (1 - b1) / (1 - b1^t) is 0.53 / 0.37 and
        sqrt(v_hat) >= |g_t| sqrt((1 - b2) / (1 - b2^t)) >= |g_t| / sqrt(3) — no more than 0.92 x the first step's sensitivity to the
        same gradient error, so the first step's bound holds for the later, bias-corrected ones too.  m: (1 - b1) x the gradient's
        bound, 2e-5 of the largest clipped gradient (biases included); v: (1 - b2) 2 |g| x that bound = 4e-8 of its square, + 1e-6 max|v|
        (fp32 rounding of v).
    ReLU gates: where a float64 pre-activation is within 4e-6 of its |h||W| + |b| sum (the fp32 products' rounding) of 0, the gate is the
    step's own (fm.hs[l] > 0, rows in the step's permuted order); such entries must be fewer than 1e-4 of all.  Samples at PPO's clip
    kinks (ratio at 1 +- clip_eps, value change at clip_eps, within 1e-5) are counted: at most 2 per step — conditions on the inputs,
    which tests/test_update_cpu.py checks for every case's seeds without a GPU."""
    from brl_amd.roll_out import Transition
    from brl_amd.update import FusedMinibatch, make_optimizer, make_update_step
    from tests.ppo_numpy import adam_step, loss_and_grads, params_of
    from tests.test_update_cpu import fake_batch
    activation, model, B, cfg, seed, fp, net = deepmind_case(case, "cuda")
    opt_state = make_optimizer(cfg, net)
    rs = (net, opt_state, None, None, 0, 9)
    nl = len(net.body)
    upd = make_update_step(cfg, fp)
    for t in (1, 2, 3):
        tb, adv, tgt = fake_batch(1, B, seed=seed + t)
        lr_t = LR * (1.0 - (t - 1) / cfg["num_updates"]) if cfg.get("anneal_lr") else LR
        assert abs(opt_state["opt"].param_groups[0]["lr"] - lr_t) < 1e-12
        P = params_of(net)
        lins = list(net.body) + [net.actor, net.critic]
        st = opt_state["opt"].state
        M = [tuple(_np(st[q]["exp_avg"]) if q in st else np.zeros(tuple(q.shape)) for q in (l.weight, l.bias)) for l in lins]
        V = [tuple(_np(st[q]["exp_avg_sq"]) if q in st else np.zeros(tuple(q.shape)) for q in (l.weight, l.bias)) for l in lins]
        rs, (total, aux) = upd(rs, Transition(*[x.cuda() for x in tb]), adv.cuda(), tgt.cuda())
        opt_state = rs[1]
        fm = opt_state.get("graphed")
        assert isinstance(fm, FusedMinibatch), opt_state.get("graph_error")
        if case == "B96":
            assert fm.dw_x3 and fm.own_gemm
        elif case == "B100":
            assert not fm.dw_x3 and fm.own_gemm
        elif case == "B333":
            assert not fm.dw_x3 and not fm.own_gemm
        elif case in ("relu_defaults", "tanh_x3", "DeepMind_8"):
            assert fm.dw_x3 and fm.own_gemm
        assert fm.own_gemm == (case not in ("no_own_gemm", "B333")) and fm.dw_x3 == (case not in ("dw_library", "B100", "B333"))
        assert abs(float(fm.lr_dev[0]) - lr_t) < 1e-9
        assert {int(s_["step"]) for s_ in opt_state["opt"].state.values()} == {t}
        # the minibatch in the order the step gathered it (its stored activations are in that order)
        perm = fm.perm[:B].cpu()
        flat = Transition(*[x.reshape((B,) + x.shape[2:])[perm] for x in tb])
        args = (flat.obs.numpy(), flat.legal_action_mask.numpy(), flat.action.numpy().astype(np.int64), flat.value.double().numpy(),
                flat.log_prob.double().numpy(), adv.reshape(-1)[perm].double().numpy(), tgt.reshape(-1)[perm].double().numpy())
        stored = [(fm.hs[l] > 0).cpu().numpy() for l in range(nl)] if activation == "relu" else None
        _, n_ratio, n_value, gate_fn, ambiguous = deepmind_input_conditions(cfg, P, args, activation, stored)
        assert n_ratio <= 2 and n_value <= 2, (t, n_ratio, n_value)
        ambiguous[0] = 0
        want_total, want_aux, G = loss_and_grads(cfg, P, *args, activation=activation, gate_fn=gate_fn)
        assert ambiguous[0] <= 1e-4 * B * net.body[0].weight.shape[0] * nl, (t, ambiguous[0])
        ill = float(cfg.get("illegal_action_l2norm_coef", 0.0))
        assert abs(float(total[0, 0]) - want_total) < 2e-5 + ill * 2e-6 * want_aux[5], (t, float(total[0, 0]), want_total)
        for k in range(5):
            assert abs(float(aux[k][0, 0]) - want_aux[k]) < 2e-5, (t, k, float(aux[k][0, 0]), want_aux[k])
        assert abs(float(aux[5][0, 0]) - want_aux[5]) < 1e-4 * want_aux[5], (t, float(aux[5][0, 0]), want_aux[5])
        # every gradient the step left in the flat buffer (the sweep scales them in registers only)
        gmax = max(np.abs(gw).max() for gw, _ in G)
        for k, (lin, (gw, gb)) in enumerate(zip(lins, G)):
            ew = np.abs(_np(lin.weight.grad) - gw).max()
            eb = np.abs(_np(lin.bias.grad) - gb).max()
            assert ew < 2e-5 * gmax + 1e-9 and eb < 2e-5 * gmax + 1e-9, (t, k, ew, eb, gmax)
        P1, M1, V1, gn = adam_step(cfg, t, P, M, V, G, lr=lr_t)
        assert abs(float(fm.norm[0]) - gn) < 1e-4 * gn, (t, float(fm.norm[0]), gn)
        clip = min(1.0, cfg["max_grad_norm"] / (gn + 1e-6)) if cfg.get("global_gradient_clipping", True) else 1.0
        gc = clip * max(max(np.abs(gw).max(), np.abs(gb).max()) for gw, gb in G)    # the largest clipped gradient, biases included
        vmax = max(np.abs(v_).max() for pair in V1 for v_ in pair)
        got = params_of(net)
        worst_p = worst_m = worst_v = moved = 0.0
        for lin, p1, m1, v1, p0, p_ in zip(lins, P1, M1, V1, P, got):
            for q, a, mm, vv, a0, b_ in zip((lin.weight, lin.bias), p1, m1, v1, p0, p_):
                worst_p = max(worst_p, np.abs(b_ - a).max())
                worst_m = max(worst_m, np.abs(_np(opt_state["opt"].state[q]["exp_avg"]) - mm).max())
                worst_v = max(worst_v, np.abs(_np(opt_state["opt"].state[q]["exp_avg_sq"]) - vv).max())
                moved = max(moved, np.abs(a - a0).max())
        assert worst_p < 0.02 * lr_t and moved > 0.3 * lr_t, (t, worst_p, moved, lr_t, gn)
        assert worst_m < 2e-5 * gc + 1e-12, (t, worst_m, gc)
        assert worst_v < 4e-8 * gc * gc + 1e-6 * vmax, (t, worst_v, gc, vmax)


# ---------------------------------------------------------------------------------------------------------------
# FusedFair: (activation, minibatch, config overrides, (fm.chain, fm.own_gemm) the case must run on, seed of its batches)
# ---------------------------------------------------------------------------------------------------------------
FAIR_CASES = {
    "relu_chain": ("relu", 1024, {}, (True, True), 500),                       # brl_fair_chain, 64 workgroups
    "tanh_chain": ("tanh", 1024, {}, (True, True), 500),
    "B16": ("relu", 16, {}, (True, True), 510),                                # one workgroup
    "B48": ("relu", 48, {}, (True, True), 520),                                # 3 workgroups, under one 64-row tile
    "B1008": ("relu", 1008, {}, (True, True), 530),                            # 63 workgroups, a K tail of the grouped dW launch
    "launches": ("relu", 1024, {"fair_chain": False}, (False, True), 500),     # launch by launch, brl_mlp_gemm GATE_COLSUM
    "B100": ("relu", 100, {}, (False, True), 540),                             # B % 16: no chain; B % 4 == 0: own GEMM
    "B1000_tanh": ("tanh", 1000, {}, (False, True), 550),
    "B333": ("relu", 333, {}, (False, False), 560),                            # library products, brl_act_bwd_colsum
    "no_own_gemm": ("relu", 1024, {"fair_chain": False, "own_gemm": False}, (False, False), 500),
    "reward_scaling": ("relu", 1024, {"reward_scaling": True}, (True, True), 500),
    "unmasked": ("relu", 1024, {"actor_illegal_action_mask": False}, (True, True), 500),
    "no_value_clipping": ("relu", 1024, {"value_clipping": False}, (True, True), 500),
    "no_global_clipping": ("relu", 1024, {"global_gradient_clipping": False}, (True, True), 500),
    "illegal_coef": ("relu", 1024, {"illegal_action_l2norm_coef": 0.5}, (False, True), 500),
    "anneal_lr": ("relu", 1024, {"anneal_lr": True, "num_minibatches": 1, "num_updates": 4}, (True, True), 500),
}
# the twelve activation outputs in the order of tests/ppo_numpy.fair_forward's sites; FusedFair keeps every one (fair_stored_gates)
FAIR_SITES = ("h0", "h1", "h2", "g1", "h3", "h4", "h6", "h7", "h8", "g3", "h9", "h10")
FAIR_PERTURB_SEED = 21
AMBIGUOUS_CAP = 1e-4      # of B x 12 x 200 activations per step
KINK_CAP = 2              # samples per step, of each kind


def fair_case(case, device):
    """-> (activation, B, cfg, expected (chain, own_gemm), seed, forward pass, its network on `device`): `init(4)` with N(0, 0.01)
    added to every weight and N(0, 0.1) to every bias — under ReLU too: hk.Linear's zero biases would hide a bias the step never
    adds, or adds from the wrong layer.  (Drawn on the host, so the CPU check of the cases' inputs sees the same network.)"""
    from brl_amd.models import make_forward_pass
    from tests.nets import perturbed
    from tests.test_update_cpu import CFG
    activation, B, over, path, seed = FAIR_CASES[case]
    cfg = dict(CFG, lr=LR, minibatch_size=B, update_epochs=1, graph_update=True, **over)
    fp = make_forward_pass(activation, "FAIR")
    net = perturbed(fp.init(4), FAIR_PERTURB_SEED)
    return activation, B, cfg, path, seed, fp, net.to(device)


def fair_gate_fn(P, stored, ambiguous):
    """a gate_fn for tests/ppo_numpy.fair_forward (its docstring derives the bands): z > 0, except where |z| is within 4e-6 of the
    magnitude sum behind it — there the gate is stored[site] (the fp32 step's own; None: z > 0 all the same) and ambiguous[0]
    counts the entry"""
    def gate_fn(site, z, layer, h_in, shortcut):
        band = np.abs(h_in) @ np.abs(P[layer][0]).T + np.abs(P[layer][1])
        if shortcut is not None:
            band = band + np.abs(shortcut)
        amb = np.abs(z) < 4e-6 * band
        gate = z > 0
        if amb.any():
            ambiguous[0] += int(amb.sum())
            if stored is not None:
                gate[amb] = stored[site][amb]
        return gate
    return gate_fn


def fair_stored_gates(fm):
    """the step's own ReLU gates, one [B, 200] bool array per site of FAIR_SITES, rows in the step's permuted order: h0, h1, g1, h3,
    h6, h7, g3, h9 are inputs of square layers (the stacked `inp` buffer, fm.t[...]); h2, h4, h8, h10 are fm.gates on the chain
    path and fm.t[...] launch by launch"""
    chain_gates = {"h2": 0, "h4": 1, "h8": 2, "h10": 3}
    return [((fm.gates[chain_gates[name]] if fm.chain and name in chain_gates else fm.t[name]) > 0).cpu().numpy() for name in FAIR_SITES]


def fair_input_conditions(cfg, P, args, activation, stored=None):
    """the two conditions on a step's INPUTS, from float64 alone where stored is None -> (ambiguous ReLU entries, samples at the
    ratio kink, samples at the value kink, the gate_fn for the gradient pass)"""
    from tests.ppo_numpy import fair_forward
    ambiguous = [0]
    gate_fn = fair_gate_fn(P, stored, ambiguous) if activation == "relu" else None
    logits, value, _, _ = fair_forward(P, args[0], activation, gate_fn)
    n_ratio, n_value = _ppo_kinks(cfg, logits, value, args[1].astype(bool), args[2], args[3], args[4])
    return ambiguous[0], n_ratio, n_value, gate_fn


@pytest.mark.parametrize("case", list(FAIR_CASES))
def test_fused_fair_step_matches_float64(case):
    """The twin of test_fused_deepmind_step_matches_float64 for FusedFair: three successive update_step calls, each ONE minibatch step,
    the float64 reference (tests/ppo_numpy.fair_loss_and_grads + adam_step) of step t starting from the GPU's own parameters and
    moments before it, rows in the step's own order (fm.perm).  One case per line of the step's code paths — the one-launch chain
    at 64, 1, 3 and 63 workgroups (B = 16: a single workgroup; 48: less than one 64-row tile; 1008: the grouped dW launch sums over
    a K tail and brl_bias_finalize_rows finishes a workgroup count that is no multiple of 4), launch by launch on brl_mlp_gemm
    (B % 16 != 0 or fair_chain=False), library products (B % 4 != 0 or own_gemm=False), every switch of the loss and of the sweep —
    and each asserts the path it ran on.  EVERY case perturbs every parameter (fair_case), ReLU included, so no bias is zero.
    After each call, with the project's bounds (the DeepMind test's docstring derives them):
      * the five logged losses within 2e-5 (+ coef 2e-6 sigma_1 with the illegal-action term), the logged norm / 2 within 1e-4 relative;
      * all thirteen (W, b) gradients left in the flat buffer (the `.grad` views; on the chain path the heads also as the [39, 200]
        block the grouped launch writes) within 2e-5 max|gW| + 1e-9; fm.norm within 1e-4 relative;
      * every step counter t; lr_dev and the optimizer's rate lr_t;
      * parameters within 0.02 lr_t of adam_step(t) (and moved by > 0.3 lr_t), exp_avg within 2e-5 gc + 1e-12, exp_avg_sq within
        4e-8 gc^2 + 1e-6 max|v|, gc the largest clipped gradient: a moment slot mapped to another parameter of FAIR's flat layout
        (square layers, W0, W6, heads, biases), or a wrong bias correction at t >= 2, fails here.
    ReLU gates: where a float64 pre-activation is within its fp32 rounding band of 0 (fair_gate_fn) the gate is the step's own
    (fair_stored_gates, read with > 0); such entries are at most 1e-4 of B x 12 x 200, samples at PPO's clip kinks at most 2 of each
    kind per step — conditions on the inputs, which tests/test_update_cpu.py checks for every case's seeds without a GPU."""
    from brl_amd.roll_out import Transition
    from brl_amd.update import FusedFair, make_optimizer, make_update_step
    from tests.ppo_numpy import adam_step, fair_loss_and_grads, fair_params_of
    from tests.test_update_cpu import fake_batch
    activation, B, cfg, (want_chain, want_own), seed, fp, net = fair_case(case, "cuda")
    opt_state = make_optimizer(cfg, net)
    rs = (net, opt_state, None, None, 0, 9)
    lins = list(net.l) + [net.actor, net.critic]
    H = lins[0].weight.shape[0]
    upd = make_update_step(cfg, fp)
    for t in (1, 2, 3):
        tb, adv, tgt = fake_batch(1, B, seed=seed + t)
        lr_t = LR * (1.0 - (t - 1) / cfg["num_updates"]) if cfg.get("anneal_lr") else LR
        assert abs(opt_state["opt"].param_groups[0]["lr"] - lr_t) < 1e-12
        P = fair_params_of(net)
        st = opt_state["opt"].state
        M = [tuple(_np(st[q]["exp_avg"]) if q in st else np.zeros(tuple(q.shape)) for q in (l.weight, l.bias)) for l in lins]
        V = [tuple(_np(st[q]["exp_avg_sq"]) if q in st else np.zeros(tuple(q.shape)) for q in (l.weight, l.bias)) for l in lins]
        rs, (total, aux) = upd(rs, Transition(*[x.cuda() for x in tb]), adv.cuda(), tgt.cuda())
        opt_state = rs[1]
        fm = opt_state.get("graphed")
        assert isinstance(fm, FusedFair), opt_state.get("graph_error")
        assert (fm.chain, fm.own_gemm) == (want_chain, want_own), (fm.chain, fm.own_gemm)
        if fm.chain:
            assert fm.group_dw and fm.cpartials.shape[0] == B // 16 == {"B16": 1, "B48": 3, "B1008": 63}.get(case, 64)
        assert abs(float(fm.lr_dev[0]) - lr_t) < 1e-9
        assert {int(s_["step"]) for s_ in opt_state["opt"].state.values()} == {t}
        # the minibatch in the order the step gathered it (its stored activations are in that order)
        perm = fm.perm[:B].cpu()
        flat = Transition(*[x.reshape((B,) + x.shape[2:])[perm] for x in tb])
        args = (flat.obs.numpy(), flat.legal_action_mask.numpy(), flat.action.numpy().astype(np.int64), flat.value.double().numpy(),
                flat.log_prob.double().numpy(), adv.reshape(-1)[perm].double().numpy(), tgt.reshape(-1)[perm].double().numpy())
        stored = fair_stored_gates(fm) if activation == "relu" else None
        n_amb, n_ratio, n_value, gate_fn = fair_input_conditions(cfg, P, args, activation, stored)
        assert n_ratio <= KINK_CAP and n_value <= KINK_CAP, (t, n_ratio, n_value)
        assert n_amb <= AMBIGUOUS_CAP * B * len(FAIR_SITES) * H, (t, n_amb)
        want_total, want_aux, G = fair_loss_and_grads(cfg, P, *args, activation=activation, gate_fn=gate_fn)
        ill = float(cfg.get("illegal_action_l2norm_coef", 0.0))
        # every gradient the step left in the flat buffer (the sweep scales them in registers only)
        gmax = max(np.abs(gw).max() for gw, _ in G)
        errs = [(np.abs(_np(lin.weight.grad) - gw).max(), np.abs(_np(lin.bias.grad) - gb).max()) for lin, (gw, gb) in zip(lins, G)]
        print(f"{case} t={t}: {n_amb} ambiguous gates, kinks {n_ratio}/{n_value}, total off by {abs(float(total[0, 0]) - want_total):.2e}, "
              f"worst gradient error {max(max(e) for e in errs):.2e} of {2e-5 * gmax + 1e-9:.2e}")
        assert abs(float(total[0, 0]) - want_total) < 2e-5 + ill * 2e-6 * want_aux[5], (t, float(total[0, 0]), want_total)
        for k in range(5):
            assert abs(float(aux[k][0, 0]) - want_aux[k]) < 2e-5, (t, k, float(aux[k][0, 0]), want_aux[k])
        assert abs(float(aux[5][0, 0]) - want_aux[5]) < 1e-4 * want_aux[5], (t, float(aux[5][0, 0]), want_aux[5])
        for k, (ew, eb) in enumerate(errs):
            assert ew < 2e-5 * gmax + 1e-9 and eb < 2e-5 * gmax + 1e-9, (t, k, ew, eb, gmax)
        if fm.chain:
            eh = np.abs(_np(fm.GWh) - np.concatenate([G[11][0], G[12][0]])).max()
            assert fm.GWh.shape == (39, H) and eh < 2e-5 * gmax + 1e-9, (t, eh, gmax)
        P1, M1, V1, gn = adam_step(cfg, t, P, M, V, G, lr=lr_t)
        assert abs(float(fm.norm[0]) - gn) < 1e-4 * gn, (t, float(fm.norm[0]), gn)
        clip = min(1.0, cfg["max_grad_norm"] / (gn + 1e-6)) if cfg.get("global_gradient_clipping", True) else 1.0
        gc = clip * max(max(np.abs(gw).max(), np.abs(gb).max()) for gw, gb in G)    # the largest clipped gradient, biases included
        vmax = max(np.abs(v_).max() for pair in V1 for v_ in pair)
        got = fair_params_of(net)
        worst_p = worst_m = worst_v = moved = 0.0
        for lin, p1, m1, v1, p0, p_ in zip(lins, P1, M1, V1, P, got):
            for q, a, mm, vv, a0, b_ in zip((lin.weight, lin.bias), p1, m1, v1, p0, p_):
                worst_p = max(worst_p, np.abs(b_ - a).max())
                worst_m = max(worst_m, np.abs(_np(opt_state["opt"].state[q]["exp_avg"]) - mm).max())
                worst_v = max(worst_v, np.abs(_np(opt_state["opt"].state[q]["exp_avg_sq"]) - vv).max())
                moved = max(moved, np.abs(a - a0).max())
        print(f"{case} t={t}: parameters off by {worst_p / lr_t:.4f} lr_t (moved {moved / lr_t:.2f}), exp_avg by {worst_m:.2e} of "
              f"{2e-5 * gc + 1e-12:.2e}, exp_avg_sq by {worst_v:.2e} of {4e-8 * gc * gc + 1e-6 * vmax:.2e}")
        assert worst_p < 0.02 * lr_t and moved > 0.3 * lr_t, (t, worst_p, moved, lr_t, gn)
        assert worst_m < 2e-5 * gc + 1e-12, (t, worst_m, gc)
        assert worst_v < 4e-8 * gc * gc + 1e-6 * vmax, (t, worst_v, gc, vmax)


@pytest.mark.parametrize("path", ["graphed", "fused", "eager"])
def test_fair_inference_forward_follows_the_updated_parameters(path):
    """FAIR's inference forward (`net(x)` under no_grad: brl_fair_forward through ActorCritic._fair_forward) after each of two updates,
    with a forward between them as a rollout does, against the module's CURRENT parameters in float64 (test_fair_forward_matches_float64's
    bound).  graphed = the autograd step captured in a hipGraph (GraphedMinibatch): its replayed Adam step writes the parameters without
    touching their version counters; fused = FusedFair (the heads one block of its flat buffer); eager = the autograd step."""
    from brl_amd.models import make_forward_pass
    from brl_amd.roll_out import Transition
    from brl_amd.update import FusedFair, GraphedMinibatch, make_optimizer, make_update_step
    from tests.test_update_cpu import CFG, fake_batch
    fp = make_forward_pass("relu", "FAIR")
    net = fp.init(3, device="cuda")
    cfg = dict(CFG, lr=1e-2, minibatch_size=256, update_epochs=1, graph_update=path != "eager", fused_update=path == "fused")
    rs = (net, make_optimizer(cfg, net), None, None, 0, 5)
    g = torch.Generator(device="cuda").manual_seed(1)
    x = (torch.rand((1000, 480), device="cuda", generator=g) < 0.12).float()
    upd = make_update_step(cfg, fp)
    for it in range(2):
        with torch.no_grad():
            net(x)                                   # the rollout's forwards between updates
        tb, adv, tgt = fake_batch(4, 256, seed=60 + it)
        rs, _ = upd(rs, Transition(*[t_.cuda() for t_ in tb]), adv.cuda(), tgt.cuda())
        if path != "eager":
            assert isinstance(rs[1].get("graphed"), FusedFair if path == "fused" else GraphedMinibatch), rs[1].get("graph_error")
        with torch.no_grad():
            lg, v = net(x)
            ref = fp.init(3, device="cpu").double()
            ref.load_state_dict({k: t_.double().cpu() for k, t_ in net.state_dict().items()})
            lg64, v64 = ref(x.double().cpu())
        scale = max(1.0, float(lg64.abs().max()))
        el, ev = float((lg.double().cpu() - lg64).abs().max()), float((v.double().cpu() - v64).abs().max())
        assert el < 2e-5 * scale and ev < 2e-5 * scale, (it, el, ev, scale)
