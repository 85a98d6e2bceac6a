"""float64 numpy restatement of ONE PPO minibatch step of the reference (src/update.py:86-178 + the optax chain of
ppo.py:195-211) for the "DeepMind" MLPs (src/models.py:23-33, wb5/models.py:34-88) and the "FAIR" residual net (src/models.py:34-69): forward,
`_loss_fn`, hand-derived backward, clip_by_global_norm, Adam(eps=1e-5) at any step.  TEST INFRASTRUCTURE — the checker for brl_amd/update.py
and brl_amd/fused_update.py on CPU and GPU."""
import numpy as np


def params_of(net):
    """[(W [out,in], b [out])] for body layers, actor head, critic head — float64 copies."""
    lins = list(net.body) + [net.actor, net.critic]
    return [(l.weight.detach().cpu().double().numpy().copy(), l.bias.detach().cpu().double().numpy().copy()) for l in lins]


def _act(activation):
    """-> (act, act' as a function of the activation's OUTPUT)"""
    if activation == "relu":
        return (lambda z: np.maximum(z, 0.0)), (lambda out: (out > 0).astype(np.float64))
    return np.tanh, (lambda out: 1.0 - out * out)


def forward(params, x, activation="relu", gate_fn=None):
    """the DeepMind MLP of any depth (src/models.py:23-33, wb5/models.py:34-88) -> (logits, value, hs, zs, dacts): hs[k] = the input of
    hidden layer k (hs[0] = x), zs[k] its pre-activation, dacts[k] = act'(zs[k]).  gate_fn(k, z, h_in) (ReLU only): the 0/1 gate
    of layer k instead of z > 0 — a checker of a fp32 step takes the step's own gate where z is within its rounding of 0."""
    act, dact = _act(activation)
    hs, zs, dacts = [x], [], []
    for k, (W, b) in enumerate(params[:-2]):
        z = hs[-1] @ W.T + b
        zs.append(z)
        if activation == "relu" and gate_fn is not None:
            gate = np.asarray(gate_fn(k, z, hs[-1]), dtype=bool)
            h = np.where(gate, z, 0.0)
            dacts.append(gate.astype(np.float64))
        else:
            h = act(z)
            dacts.append(dact(h))
        hs.append(h)
    logits = hs[-1] @ params[-2][0].T + params[-2][1]
    value = (hs[-1] @ params[-1][0].T + params[-1][1])[:, 0]
    return logits, value, hs, zs, dacts


def head_loss(cfg, logits, value, mask, action, old_value, old_log_prob, gae, tgt):
    """`_loss_fn` on given network outputs (float64) -> (total, (value_loss, loss_actor, entropy, approx_kl, clipfrac, illegal norm / 2),
    dlogits, dvalue): the derivative w.r.t. the outputs, hand-derived.  cfg["actor_illegal_action_mask"] False = the unmasked policy
    for the log-prob (src/update.py:18-21); the entropy is always the masked policy's (:132-135); cfg["reward_scaling"]: gae
    normalised first (src/update.py:31-44, ddof 0); cfg["illegal_action_l2norm_coef"] = c: + c * sigma_1(P * ~mask) / 2 with P the
    softmax of the UNMASKED logits (src/update.py:136-152), its gradient c / 2 * (u_1 v_1^T * ~mask) pushed back through that
    softmax (u_1, v_1 from the SVD)."""
    B = logits.shape[0]
    eps = cfg["clip_eps"]
    mask = mask.astype(bool)
    if cfg.get("reward_scaling", False):
        gae = (gae - gae.mean()) / (gae.std() + 1e-8)
    masked = cfg.get("actor_illegal_action_mask", True)
    ml = np.where(mask, logits, -np.inf)
    ml = ml - ml.max(1, keepdims=True)
    lsm = ml - np.log(np.exp(ml).sum(1, keepdims=True))
    p = np.exp(lsm)
    ul = logits - logits.max(1, keepdims=True)
    lsm_u = ul - np.log(np.exp(ul).sum(1, keepdims=True))
    p_u = np.exp(lsm_u)
    idx = np.arange(B)
    lsel, psel = (lsm, p) if masked else (lsm_u, p_u)
    lp = lsel[idx, action]
    logratio = lp - old_log_prob
    ratio = np.exp(logratio)
    if cfg.get("value_clipping", True):
        vc = old_value + np.clip(value - old_value, -eps, eps)
        l1, l2 = (value - tgt) ** 2, (vc - tgt) ** 2
        value_loss = 0.5 * np.maximum(l1, l2).mean()
        dv = np.where(l1 >= l2, value - tgt, (vc - tgt) * (np.abs(value - old_value) < eps))
    else:
        value_loss = 0.5 * ((value - tgt) ** 2).mean()
        dv = value - tgt
    dv = dv / B * cfg["vf_coef"]
    a1, a2 = ratio * gae, np.clip(ratio, 1 - eps, 1 + eps) * gae
    loss_actor = -np.minimum(a1, a2).mean()
    inside_r = (ratio > 1 - eps) & (ratio < 1 + eps)
    dlp = -np.where((a1 < a2) | inside_r, gae, 0.0) / B * ratio
    plogp = np.where(mask, p * np.where(mask, lsm, 0.0), 0.0)
    ent_i = -plogp.sum(1)
    entropy = ent_i.mean()
    onehot = np.zeros_like(p)
    onehot[idx, action] = 1.0
    dlogits = dlp[:, None] * (onehot - psel)
    if masked:
        dlogits = np.where(mask, dlogits, 0.0)
    dH = -np.where(mask, p * (np.where(mask, lsm, 0.0) + ent_i[:, None]), 0.0)
    dlogits = dlogits - cfg["ent_coef"] * dH / B
    # the illegal-action term: sigma_1 of the illegal probabilities of the unmasked policy (logged whatever its coefficient)
    if np.isfinite(p_u).all():
        u, s, vt = np.linalg.svd(p_u * ~mask, full_matrices=False)
        illegal = s[0] / 2
    else:        # jnp.linalg.norm of a matrix holding a NaN is NaN (LAPACK's SVD refuses it instead)
        u, vt = np.full((B, 1), np.nan), np.full((1, p_u.shape[1]), np.nan)
        illegal = np.nan
    coef = float(cfg.get("illegal_action_l2norm_coef", 0.0) or 0.0)
    total = loss_actor + cfg["vf_coef"] * value_loss - cfg["ent_coef"] * entropy + coef * illegal
    if coef:
        dP = coef / 2 * np.outer(u[:, 0], vt[0]) * ~mask                  # d sigma_1 / dA = u_1 v_1^T (the sign of the pair cancels)
        dlogits = dlogits + p_u * (dP - (dP * p_u).sum(1, keepdims=True))  # back through the softmax
    approx_kl = ((ratio - 1) - logratio).mean()
    clipfrac = (np.abs(ratio - 1.0) > eps).mean()
    return total, (value_loss, loss_actor, entropy, approx_kl, clipfrac, illegal), dlogits, dv


def loss_and_grads(cfg, params, obs, mask, action, old_value, old_log_prob, gae, tgt, activation="relu", gate_fn=None):
    """the DeepMind MLP (any depth, either activation) -> (total, (value_loss, loss_actor, entropy, approx_kl, clipfrac, illegal norm
    / 2), grads like params): `head_loss` on the forward pass and the backward pass written out."""
    logits, value, hs, zs, dacts = forward(params, obs.astype(np.float64), activation, gate_fn)
    total, aux, dlogits, dv = head_loss(cfg, logits, value, mask, action, old_value, old_log_prob, gae, tgt)
    return total, aux, backward(params, dlogits, dv, hs, dacts)


def backward(params, dlogits, dvalue, hs, dacts):
    """the DeepMind MLP's backward pass written out: d loss / d logits [B, 38], d loss / d value [B] and `forward`'s tape (hs, dacts)
    -> grads like params"""
    grads = [None] * len(params)
    h = hs[-1]
    grads[-2] = (dlogits.T @ h, dlogits.sum(0))
    grads[-1] = (dvalue[None, :] @ h, np.array([dvalue.sum()]))
    dh = dlogits @ params[-2][0] + dvalue[:, None] * params[-1][0]
    for k in range(len(params) - 3, -1, -1):
        dz = dh * dacts[k]
        grads[k] = (dz.T @ hs[k], dz.sum(0))
        dh = dz @ params[k][0]
    return grads


def global_norm(grads):
    return float(np.sqrt(sum((gw ** 2).sum() + (gb ** 2).sum() for gw, gb in grads)))


def adam_step(cfg, t, params, m, v, grads, lr=None, eps=1e-5, clip=None):
    """step t (1, 2, ...) of clip_by_global_norm(max_grad_norm) + Adam(eps=1e-5) (ppo.py:195-211) with torch's arithmetic
    (torch.nn.utils.clip_grad_norm_: coef = max_norm / (norm + 1e-6) clamped to 1; torch.optim.Adam: m <- m + (g - m)(1 - b1),
    v <- b2 v + (1 - b2) g^2, p <- p - lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)).  params / m / v / grads: lists of
    (W, b) pairs -> (params, m, v, pre-clip global norm).  eps: Adam's; clip: None = as cfg says, False = no clipping (cfg may
    then be None with lr given) — brl_amd.sl.make_optimizer is adam_step(None, t, ..., lr=lr, eps=1e-8, clip=False)."""
    lr = cfg["lr"] if lr is None else lr
    b1, b2 = 0.9, 0.999
    gn = global_norm(grads)
    clip = cfg.get("global_gradient_clipping", True) if clip is None else clip
    # (np.minimum, as torch.clamp and jnp.minimum: a NaN norm gives a NaN factor; Python's min(1.0, nan) is 1.0)
    scale = float(np.minimum(1.0, cfg["max_grad_norm"] / (gn + 1e-6))) if clip else 1.0
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    P, M, V = [], [], []
    for pp, mm, vv, gg in zip(params, m, v, grads):
        outs = [[], [], []]
        for x, m_, v_, g in zip(pp, mm, vv, gg):
            g = g * scale
            m_ = m_ + (g - m_) * (1.0 - b1)
            v_ = v_ * b2 + g * g * (1.0 - b2)
            outs[0].append(x - lr / bc1 * m_ / (np.sqrt(v_) / np.sqrt(bc2) + eps))
            outs[1].append(m_)
            outs[2].append(v_)
        P.append(tuple(outs[0])); M.append(tuple(outs[1])); V.append(tuple(outs[2]))
    return P, M, V, gn


def adam_first_step(cfg, params, grads):
    """`adam_step` from a fresh state -> (params, pre-clip global norm)"""
    zeros = [(np.zeros_like(W), np.zeros_like(b)) for W, b in params]
    P, _, _, gn = adam_step(cfg, 1, params, zeros, zeros, grads)
    return P, gn


# ---------------------------------------------------------------------------------------------------------------
# the FAIR network (src/models.py:34-69), written as the reference writes it: x = L(x); shortcut = x; x = act(x); ...
# ---------------------------------------------------------------------------------------------------------------
def fair_params_of(net):
    lins = list(net.l) + [net.actor, net.critic]
    return [(l.weight.detach().cpu().double().numpy().copy(), l.bias.detach().cpu().double().numpy().copy()) for l in lins]


def fair_forward(params, obs, activation="relu", gate_fn=None):
    """the FAIR forward pass in the reference's statement order -> (logits, value, x, tape): x = the heads' input, tape = the
    (kind, ...) entries `fair_loss_and_grads` differentiates in reverse.

    gate_fn(site, z, layer, h_in, shortcut) (ReLU only) returns the 0/1 gate of activation site `site` instead of z > 0; the
    activation's output is then z * gate and its derivative the gate itself.  A checker of a fp32 step takes the step's own gate
    where z is within the step's rounding of 0.  The twelve sites are the twelve `activate(...)` calls below, in order:

        site   0   1   2   3*  4   5   6   7   8   9*  10  11
        layer  0   1   2   2   3   4   6   7   8   8   9   10      (the output the FusedFair step keeps of it:
        output h0  h1  h2  g1  h3  h4  h6  h7  h8  g3  h9  h10      tests/test_gpu_update_float64.FAIR_SITES)

    What the rounding band of a site needs comes with the call.  Behind a linear layer (every site but 3 and 9) z = h_in W^T + b
    with (W, b) = params[layer], h_in that layer's input (layer 6: [z5 | obs]) and shortcut None: a fp32 product sum is off by a
    small multiple of 2^-24 of the sum of its terms' magnitudes, so the band is c (|h_in| |W|^T + |b|); the checkers use c = 4e-6,
    ~70 ulp, as for the DeepMind MLP.  At the residual sums (*) z = act(h_in W^T + b) + shortcut, with `layer` the linear layer
    FEEDING the sum (2: h2 = act(h1 W_2^T + b_2), 8: h8 likewise), h_in its input and shortcut the pre-activation z0 / z6 taken
    right behind layer 0 / 6.  ReLU is 1-Lipschitz, so h2 carries no more error than its pre-activation, c (|h_in| |W|^T + |b|);
    the shortcut arrives with a relative error of the same few ulp, c |shortcut|, and the fp32 addition rounds by 2^-24 (|h2| +
    |shortcut|), which both terms already cover.  Band of the sum: c (|h_in| |W|^T + |b| + |shortcut|).  (The shortcut's own
    accumulation error — 48 or so terms of a 0/1 observation, ~1e-7 absolute — is far below the first term, a 200-term sum of
    O(1) magnitude.)"""
    act, _ = _act(activation)
    gated = activation == "relu" and gate_fn is not None
    x = obs.astype(np.float64)
    inp = x
    tape = []
    site = [0]
    last = [None, None]      # (layer, input) of the last linear layer

    def lin(k, v):
        tape.append(("lin", k, v))
        last[0], last[1] = k, v
        return v @ params[k][0].T + params[k][1]

    def activate(v, shortcut=None):
        if gated:
            gate = np.asarray(gate_fn(site[0], v, last[0], last[1], shortcut), dtype=bool)
            out = np.where(gate, v, 0.0)
            tape.append(("act", out, gate.astype(np.float64)))
        else:
            out = act(v)
            tape.append(("act", out, None))
        site[0] += 1
        return out

    x = lin(0, x); s1 = x
    x = activate(x); x = lin(1, x); x = activate(x); x = lin(2, x); x = activate(x)
    x = x + s1; tape.append(("add", "s1")); s2 = x
    x = activate(x, s1); x = lin(3, x); x = activate(x); x = lin(4, x); x = activate(x)
    x = x + s2; tape.append(("add", "s2"))
    x = lin(5, x)
    x = np.concatenate([x, inp], axis=-1); tape.append(("cat", 200))
    x = lin(6, x); s3 = x
    x = activate(x); x = lin(7, x); x = activate(x); x = lin(8, x); x = activate(x)
    x = x + s3; tape.append(("add", "s3")); s4 = x
    x = activate(x, s3); x = lin(9, x); x = activate(x); x = lin(10, x); x = activate(x)
    x = x + s4; tape.append(("add", "s4"))
    assert site[0] == 12
    logits = x @ params[11][0].T + params[11][1]
    value = (x @ params[12][0].T + params[12][1])[:, 0]
    return logits, value, x, tape


def fair_loss_and_grads(cfg, params, obs, mask, action, old_value, old_log_prob, gae, tgt, activation="relu", gate_fn=None):
    """-> (total, aux, grads like params): the loss of `head_loss` on the FAIR forward pass (`fair_forward`; gate_fn: see there)
    and its gradient by reverse-mode differentiation of the reference's own statement order (a tape of (kind, ...) entries; no
    shared code with the build)."""
    logits, value, x, tape = fair_forward(params, obs, activation, gate_fn)
    total, aux, dlogits, dv = head_loss(cfg, logits, value, mask, action, old_value, old_log_prob, gae, tgt)
    return total, aux, fair_backward(params, dlogits, dv, x, tape, activation)


def fair_backward(params, dlogits, dvalue, x, tape, activation="relu"):
    """the FAIR net's backward pass: d loss / d logits [B, 38], d loss / d value [B], the heads' input x and `fair_forward`'s tape
    -> grads like params"""
    _, dact = _act(activation)
    grads = [None] * len(params)
    grads[11] = (dlogits.T @ x, dlogits.sum(0))
    grads[12] = (dvalue[None, :] @ x, np.array([dvalue.sum()]))
    d = dlogits @ params[11][0] + dvalue[:, None] * params[12][0]
    # the shortcuts were taken right AFTER the linear layers 0 and 6 (s1, s3) and after the first / third block's sum (s2, s4):
    # a pending shortcut gradient is added where its value was defined
    pending = {}
    defined_after = {"s4": ("add", "s3"), "s2": ("add", "s1")}     # s4 = the value after `add s3`, s2 = the value after `add s1`
    for entry in reversed(tape):
        if entry[0] == "add":
            name = entry[1]
            pending[name] = d.copy()                                 # x = x + s: the gradient flows to both
            for later, where in defined_after.items():
                if where == entry and later in pending:              # this sum's OUTPUT was also taken as shortcut `later`
                    d = d + pending.pop(later)
                    pending[name] = d.copy()
        elif entry[0] == "act":
            d = d * (dact(entry[1]) if entry[2] is None else entry[2])
        elif entry[0] == "cat":
            d = d[:, :entry[1]]
        else:
            _, k, v = entry
            if k == 6 and "s3" in pending:
                d = d + pending.pop("s3")
            if k == 0 and "s1" in pending:
                d = d + pending.pop("s1")
            grads[k] = (d.T @ v, d.sum(0))
            d = d @ params[k][0]
    assert not pending
    return grads
