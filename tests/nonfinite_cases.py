"""Inputs with ONE non-finite number, and what the float64 / eager references make of them ("Non-finite values").
TEST INFRASTRUCTURE shared by tests/test_nonfinite_host.py (which pins the references on the CPU) and tests/test_gpu_nonfinite.py.

`loss_batch` is a `_loss_fn` minibatch in numpy (float32 where the kernels read float32), `poisoned` a copy of it with one sample
poisoned in one of the six ways of POISONS, `loss_reference` the float64 restatement (tests/ppo_numpy.head_loss) on it.  The
statistics come back in the order of the kernels' log row: total, value_loss, loss_actor, entropy, approx_kl, clipfrac, illegal norm / 2."""
import numpy as np

LOSS_CFG = {"clip_eps": 0.2, "vf_coef": 0.5, "ent_coef": 0.001, "value_clipping": True, "actor_illegal_action_mask": True,
            "reward_scaling": False, "illegal_action_l2norm_coef": 0.0}
POISONS = ("nan_value", "inf_value", "nan_legal_logit", "nan_illegal_logit", "nan_old_logp", "nan_adv")
STATS = ("total", "value_loss", "loss_actor", "entropy", "approx_kl", "clipfrac", "illegal")
# what each poison turns NaN (+inf for inf_value) in the float64 restatement with the masked policy: the statistics, and of the
# poisoned sample's derivatives "v" = dvalue, "legal" = dlogits on its legal actions (its illegal ones stay 0)
EXPECTED = {
    "nan_value": ({"total", "value_loss"}, {"v"}),
    "inf_value": ({"total", "value_loss"}, {"v"}),
    "nan_legal_logit": ({"total", "loss_actor", "entropy", "approx_kl", "illegal"}, {"legal"}),
    "nan_illegal_logit": ({"total", "illegal"}, set()),          # (total: + 0 x NaN, src/update.py:146-151)
    "nan_old_logp": ({"total", "loss_actor", "approx_kl"}, {"legal"}),
    "nan_adv": ({"total", "loss_actor"}, {"legal"}),
}


def _log_prob64(logits, mask, action):
    ml = np.where(mask, logits.astype(np.float64), -np.inf)
    ml = ml - ml.max(1, keepdims=True)
    lsm = ml - np.log(np.exp(ml).sum(1, keepdims=True))
    return lsm[np.arange(len(action)), action]


def loss_batch(B, seed=0):
    """-> dict: logits [B, 38], value, old_value, old_log_prob, gae, tgt [B] float32, mask [B, 38] bool (action 0 legal, action 37
    illegal, the rest drawn), action [B] int32 (legal).  old_log_prob = the current log-prob + N(0, 0.1): most ratios inside the clip
    range, some outside."""
    rng = np.random.default_rng(seed)
    logits = rng.standard_normal((B, 38)).astype(np.float32)
    mask = rng.random((B, 38)) < 0.5
    mask[:, 0], mask[:, 37] = True, False
    action = (rng.random((B, 38)) * mask).argmax(1).astype(np.int32)
    f = lambda s: (rng.standard_normal(B) * s).astype(np.float32)   # noqa: E731
    value, old_value, tgt, gae = f(0.3), f(0.3), f(0.3), f(1.0)
    old_lp = (_log_prob64(logits, mask, action) + rng.standard_normal(B) * 0.1).astype(np.float32)
    return {"logits": logits, "value": value, "mask": mask, "action": action, "old_value": old_value, "old_log_prob": old_lp,
            "gae": gae, "tgt": tgt}


def settle(batch, i):
    """sample i's ratio put at exp(0.01): well inside the clip range, where a NaN advantage gives a NaN derivative in float32 and in
    float64 alike; in place -> batch"""
    lp = _log_prob64(batch["logits"][i:i + 1], batch["mask"][i:i + 1], batch["action"][i:i + 1])[0]
    batch["old_log_prob"][i] = np.float32(lp - 0.01)
    return batch


def poisoned(batch, kind, i):
    """a copy of `batch` with sample i poisoned"""
    b = {k: v.copy() for k, v in batch.items()}
    if kind == "nan_value":
        b["value"][i] = np.nan
    elif kind == "inf_value":
        b["value"][i] = np.inf
    elif kind == "nan_legal_logit":
        legal = np.flatnonzero(b["mask"][i])
        others = legal[legal != b["action"][i]]
        b["logits"][i, others[-1] if len(others) else legal[0]] = np.nan
    elif kind == "nan_illegal_logit":
        b["logits"][i, 37] = np.nan
    elif kind == "nan_old_logp":
        b["old_log_prob"][i] = np.nan
    elif kind == "nan_adv":
        b["gae"][i] = np.nan
    else:
        raise KeyError(kind)
    return b


def loss_reference(cfg, b, logits=None, value=None):
    """tests/ppo_numpy.head_loss in float64 on the batch (logits / value: other network outputs than the batch's own)
    -> (stats [7] float64, dlogits [B, 38], dvalue [B])"""
    from tests.ppo_numpy import head_loss
    d = lambda x: np.asarray(x, np.float64)   # noqa: E731
    with np.errstate(all="ignore"):
        total, aux, dlogits, dv = head_loss(cfg, d(b["logits"] if logits is None else logits), d(b["value"] if value is None else value),
                                            b["mask"], b["action"].astype(np.int64), d(b["old_value"]), d(b["old_log_prob"]),
                                            d(b["gae"]), d(b["tgt"]))
    return np.array([total, *aux], np.float64), dlogits, dv


def nonfinite_pattern(x):
    """0 finite, 1 NaN, 2 +inf, 3 -inf, elementwise"""
    x = np.asarray(x, np.float64)
    return np.isnan(x) * 1 + np.isposinf(x) * 2 + np.isneginf(x) * 3


def assert_same_nonfinite(got, want, what=""):
    """`got` is NaN exactly where `want` is, +inf where it is +inf, -inf where it is -inf"""
    g, w = nonfinite_pattern(got), nonfinite_pattern(want)
    assert np.array_equal(g, w), f"{what}: non-finite pattern differs at {np.argwhere(g != w)[:5].tolist()}: got {g[g != w][:5]}, want {w[g != w][:5]}"


def gae_numpy32(done, value, reward, last_val, gamma, gae_lambda):
    """src/gae.py:28-29, 39 in float32 numpy, statement by statement (gamma * gae_lambda: a Python-float product rounded once)"""
    T, N = done.shape
    f = np.float32
    gamma32, gl = f(gamma), f(float(gamma) * float(gae_lambda))
    gae, next_value = np.zeros(N, f), np.asarray(last_val, f).copy()
    adv = np.zeros((T, N), f)
    with np.errstate(all="ignore"):
        for t in range(T - 1, -1, -1):
            nd = f(1.0) - done[t].astype(f)
            delta = reward[t] + gamma32 * next_value * nd - value[t]
            gae = delta + gl * nd * gae
            adv[t] = gae
            next_value = value[t]
        return adv, adv + value


def gae_inputs(T, N, seed):
    """done / value / reward [T, N] and last_val [N] with NaN, +inf and -inf scattered over value, reward and last_val — some of them
    right behind a `done`, where the scan multiplies them by 0"""
    rng = np.random.default_rng(seed)
    done = rng.random((T, N)) < 0.15
    value = rng.standard_normal((T, N)).astype(np.float32)
    reward = (rng.standard_normal((T, N)) * 0.2).astype(np.float32)
    last = rng.standard_normal(N).astype(np.float32)
    specials = (np.nan, np.inf, -np.inf)
    for k in range(9):
        arr = (value, reward, value)[k % 3]
        arr[rng.integers(T), rng.integers(N)] = specials[k % 3 if k < 6 else (k + 1) % 3]
    last[[1, N // 2, N - 1]] = (np.inf, np.nan, -np.inf)
    done[T - 1, 1] = True            # an inf `last_val` behind a done: inf x 0
    if T > 2:
        t, n = np.argwhere(np.isinf(value))[0]
        done[max(t - 1, 0), n] = True
    return done, value, reward, last
