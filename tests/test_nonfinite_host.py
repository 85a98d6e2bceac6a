"""Non-finite values, the references first (no GPU): what tests/test_gpu_nonfinite.py holds the kernels to is pinned here on the CPU.

DESIGN.md, "Non-finite values": an output is NaN wherever its float64 / eager reference is NaN and non-finite wherever it is +-inf.
The references are tests/ppo_numpy.py (float64 `_loss_fn`, clip_by_global_norm + Adam), torch's own clip_grad_norm_ + Adam, the eager
`make_update_step`, and the oracle's GAE scan."""
import numpy as np
import pytest
import torch

from tests import nonfinite_cases as nc
from tests.ppo_numpy import adam_first_step, adam_step, fair_loss_and_grads, fair_params_of, global_norm

ADAM_CFG = {"lr": 1e-3, "max_grad_norm": 0.5, "global_gradient_clipping": True}


def _params(seed=0, sizes=((7, 5), (3, 7))):
    rng = np.random.default_rng(seed)
    mk = lambda: [(rng.standard_normal(s), rng.standard_normal(s[0])) for s in sizes]   # noqa: E731
    return mk(), mk()


def _flat(P):
    return np.concatenate([x.reshape(-1) for pair in P for x in pair])


@pytest.mark.parametrize("B", [17, 256])
@pytest.mark.parametrize("kind", nc.POISONS)
def test_head_loss_reports_a_poisoned_sample(kind, B):
    """tests/ppo_numpy.head_loss on a batch with one poisoned sample: exactly the statistics of nonfinite_cases.EXPECTED are NaN
    (+inf for an infinite value), the sample's own derivatives are NaN / +inf where listed and 0 on its illegal actions, and every
    other sample's derivatives are those of the clean batch."""
    i = B // 3
    clean = nc.settle(nc.loss_batch(B, seed=B), i)
    st0, dl0, dv0 = nc.loss_reference(nc.LOSS_CFG, clean)
    assert np.isfinite(st0).all() and np.isfinite(dl0).all() and np.isfinite(dv0).all()
    b = nc.poisoned(clean, kind, i)
    st, dl, dv = nc.loss_reference(nc.LOSS_CFG, b)
    bad_stats, bad_d = nc.EXPECTED[kind]
    want = 2 if kind == "inf_value" else 1
    for k, name in enumerate(nc.STATS):
        assert nc.nonfinite_pattern(st[k]) == (want if name in bad_stats else 0), (name, st[k])
    legal = b["mask"][i]
    assert (nc.nonfinite_pattern(dl[i][legal]) == (1 if "legal" in bad_d else 0)).all()
    assert (dl[i][~legal] == 0).all()
    assert nc.nonfinite_pattern(dv[i]) == (want if "v" in bad_d else 0)
    others = np.arange(B) != i
    assert np.array_equal(dl[others], dl0[others]) and np.array_equal(dv[others], dv0[others])


def test_fair_loss_and_grads_reports_a_poisoned_sample():
    """the FAIR restatement: a NaN `old_log_prob` of one sample gives a NaN total / loss_actor / approx_kl and NaN gradients of every
    layer and of the actor head's rows of that sample's legal actions (d logits^T x sums over the samples)"""
    from brl_amd.models import make_forward_pass
    B = 17
    net = make_forward_pass("relu", "FAIR").init(3)
    b = nc.poisoned(nc.loss_batch(B, seed=5), "nan_old_logp", 4)
    obs = (np.random.default_rng(1).random((B, 480)) < 0.1).astype(np.float64)
    with np.errstate(all="ignore"):
        total, aux, grads = fair_loss_and_grads(nc.LOSS_CFG, fair_params_of(net), obs, b["mask"], b["action"].astype(np.int64),
                                                b["old_value"].astype(np.float64), b["old_log_prob"].astype(np.float64),
                                                b["gae"].astype(np.float64), b["tgt"].astype(np.float64))
    assert np.isnan(total) and np.isnan(aux[1]) and np.isnan(aux[3]) and np.isfinite(aux[0]) and np.isfinite(aux[2])
    assert all(np.isnan(gw).all() and np.isnan(gb).all() for gw, gb in grads[:11])      # every layer: d logits W_actor is NaN in row 4
    legal = b["mask"][4]                                                              # the actor head: the sample's legal actions
    assert np.isnan(grads[11][0][legal]).all() and np.isnan(grads[11][1][legal]).all()
    assert np.isfinite(grads[11][0][~legal]).all() and np.isfinite(grads[11][1][~legal]).all()
    assert np.isfinite(grads[12][0]).all() and np.isfinite(grads[12][1]).all()        # the critic head: dvalue is clean


def test_adam_step_clamps_with_a_nan_propagating_minimum():
    """tests/ppo_numpy.adam_step: the clip factor is min(1, max_norm / (norm + 1e-6)) as torch.clamp / jnp.minimum take it — the same
    numbers as before on finite gradients (above and below the threshold), NaN everywhere for one NaN gradient element, NaN at an
    infinite element only (factor 0: 0 x inf) with the other parameters finite and unmoved."""
    P, G = _params()
    for scale in (1.0, 1e-3):                               # clipped / not clipped
        Gs = [(gw * scale, gb * scale) for gw, gb in G]
        gn = global_norm(Gs)
        P1, want_gn = adam_first_step(ADAM_CFG, P, Gs)
        assert want_gn == gn and (gn > 0.5) == (scale == 1.0)
        c = min(1.0, 0.5 / (gn + 1e-6))
        for (w1, b1), (w0, b0), (gw, gb) in zip(P1, P, Gs):     # a first Adam step: p - lr g / (|g| + eps)
            for x1, x0, g in ((w1, w0, gw), (b1, b0, gb)):
                assert np.allclose(x1, x0 - 1e-3 * (c * g) / (np.abs(c * g) + 1e-5), rtol=1e-9, atol=0)
    Gn = [(gw.copy(), gb.copy()) for gw, gb in G]
    Gn[1][0][2, 3] = np.nan
    Pn, gn = adam_first_step(ADAM_CFG, P, Gn)
    assert np.isnan(gn) and np.isnan(_flat(Pn)).all()
    Gi = [(gw.copy(), gb.copy()) for gw, gb in G]
    Gi[0][1][4] = np.inf
    with np.errstate(all="ignore"):
        Pi, M, V, gn = adam_step(ADAM_CFG, 1, P, [(np.zeros_like(w), np.zeros_like(b)) for w, b in P],
                                 [(np.zeros_like(w), np.zeros_like(b)) for w, b in P], Gi)
    assert np.isposinf(gn)
    want_nan = np.zeros(_flat(P).shape, bool)
    want_nan[7 * 5 + 4] = True
    for X in (Pi, M, V):
        assert np.array_equal(np.isnan(_flat(X)), want_nan) and np.isfinite(_flat(X)[~want_nan]).all()
    assert np.array_equal(_flat(Pi)[~want_nan], _flat(P)[~want_nan])


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_torch_clip_and_adam_agree_with_the_numpy_restatement(bad):
    """torch.nn.utils.clip_grad_norm_ + torch.optim.Adam(eps=1e-5) on the host, one step: the NaN positions of the parameters and of
    Adam's moments equal tests/ppo_numpy.adam_step's (all of them for a NaN element, that element alone for an infinite one) and the
    finite parameters agree to 1e-6"""
    P, G = _params(seed=2)
    G[1][0][1, 1] = bad
    zeros = [(np.zeros_like(w), np.zeros_like(b)) for w, b in P]
    with np.errstate(all="ignore"):
        P1, M1, V1, gn = adam_step(ADAM_CFG, 1, P, zeros, zeros, G)
    ts = [torch.nn.Parameter(torch.tensor(x, dtype=torch.float32)) for pair in P for x in pair]
    for t, g in zip(ts, [x for pair in G for x in pair]):
        t.grad = torch.tensor(g, dtype=torch.float32)
    opt = torch.optim.Adam(ts, lr=1e-3, eps=1e-5)
    norm = torch.nn.utils.clip_grad_norm_(ts, 0.5)
    opt.step()
    nc.assert_same_nonfinite(float(norm), gn, "norm")
    got = np.concatenate([t.detach().numpy().reshape(-1) for t in ts])
    want = _flat(P1)
    nc.assert_same_nonfinite(got, want, "parameters")
    assert np.isnan(want).all() if np.isnan(bad) else int(np.isnan(want).sum()) == 1
    ok = ~np.isnan(want)
    assert np.abs(got[ok] - want[ok]).max(initial=0.0) < 1e-6
    for key, ref in (("exp_avg", M1), ("exp_avg_sq", V1)):
        state = np.concatenate([opt.state[t][key].numpy().reshape(-1) for t in ts])
        nc.assert_same_nonfinite(state, _flat(ref), key)


def test_eager_update_step_goes_nan_with_the_critic():
    """the eager `make_update_step` on the CPU with critic.weight[0, 5] = NaN: every minibatch's total and value_loss are NaN and
    every parameter is NaN afterwards (clip_grad_norm_'s NaN factor) — what the fused steps are held to on the GPU"""
    from brl_amd.models import make_forward_pass
    from brl_amd.update import make_update_step
    from tests.test_update_cpu import CFG, fake_batch
    fp = make_forward_pass("relu", "DeepMind")
    net = fp.init(4)
    with torch.no_grad():
        net.critic.weight[0, 5] = float("nan")
    tb, adv, tgt = fake_batch(2, 64)
    _, (total, aux) = make_update_step(dict(CFG), fp)((net, None, None, None, 0, 7), tb, adv, tgt)
    assert torch.isnan(total).all() and torch.isnan(aux[0]).all()
    assert all(bool(torch.isnan(p).all()) for p in net.parameters())


def test_eager_loss_keeps_nan_in_entropy_and_total():
    """brl_amd.update.ppo_loss (the eager `_loss_fn`) against tests/ppo_numpy.head_loss on every poison: the same statistics are NaN
    / +inf — a NaN legal logit reaches the entropy, a NaN illegal-action norm reaches the total through its zero coefficient"""
    from brl_amd.roll_out import Transition
    from brl_amd.update import ppo_loss
    B, i = 17, 5
    clean = nc.settle(nc.loss_batch(B, seed=B), i)
    for kind in nc.POISONS:
        b = nc.poisoned(clean, kind, i)
        want, _, _ = nc.loss_reference(nc.LOSS_CFG, b)
        t = lambda k: torch.from_numpy(b[k])   # noqa: E731
        flat = Transition(done=None, action=t("action"), value=t("old_value"), reward=None, log_prob=t("old_log_prob"), obs=None,
                          legal_action_mask=t("mask"))
        total, aux = ppo_loss(nc.LOSS_CFG, t("logits"), t("value"), flat, t("gae"), t("tgt"))
        nc.assert_same_nonfinite(np.array([float(total)] + [float(a) for a in aux]), want, kind)


@pytest.mark.parametrize("T,N", [(7, 130), (33, 64)])
def test_oracle_gae_on_non_finite_inputs(oracle, T, N):
    """oracle.gae on values, rewards and a last value holding NaN, +inf and -inf (an infinite value right behind a `done`: inf x 0)
    equals the float32 numpy restatement of src/gae.py:28-29, 39, NaN for NaN"""
    done, value, reward, last = nc.gae_inputs(T, N, seed=T)
    adv, tgt = oracle.gae(done.astype(np.uint8), value, reward, last, 0.99, 0.95)
    wa, wt = nc.gae_numpy32(done, value, reward, last, 0.99, 0.95)
    assert np.isnan(wa).any() and np.isinf(wa).any() and np.isfinite(wa).any()
    assert np.array_equal(adv, wa, equal_nan=True) and np.array_equal(tgt, wt, equal_nan=True)


def test_cpu_shim_keeps_nan_like_the_kernels():
    """the CPU shim's restatements of the device entry points (oracle/brl_shim.c) follow the same rule: brl_mlp_gemm's bias + ReLU
    epilogue keeps a NaN column (and turns a -inf one into 0), brl_adam_shard_apply turns every parameter NaN for one NaN gradient"""
    import ctypes
    import oracle as oracle_pkg
    from brl_amd._capi import ShardGeom
    from oracle.binding import shim_path
    oracle_pkg.build()
    shim = ctypes.CDLL(shim_path())
    f32, vp, i32, i64 = ctypes.c_float, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    ptr = lambda a: a.ctypes.data_as(vp)   # noqa: E731
    rng = np.random.default_rng(0)
    M, N, K = 5, 8, 12
    a, b = rng.standard_normal((M, K)).astype(np.float32), rng.standard_normal((N, K)).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    bias[2], bias[5] = np.nan, -np.inf
    c = np.zeros((M, N), np.float32)
    shim.brl_mlp_gemm.argtypes = [i32, i32, i32, vp, i64, vp, i64, vp, i64, i64, i64, i64, i32, vp, vp, i64, vp, vp, vp]
    assert shim.brl_mlp_gemm(0, 0, 1, ptr(a), K, ptr(b), K, ptr(c), N, M, N, K, 0, ptr(bias), None, 0, None, None, None) == 0
    keep = np.ones(N, bool)
    keep[[2, 5]] = False
    assert np.isnan(c[:, 2]).all() and (c[:, 5] == 0).all()
    assert np.allclose(c[:, keep], np.maximum(a @ b.T + bias, 0)[:, keep], atol=1e-5)
    shim.brl_adam_shard_norm.argtypes = [i32, vp, ctypes.POINTER(ShardGeom), i32, i32, f32, vp, vp, vp, vp]
    shim.brl_adam_shard_apply.argtypes = [i32, vp, vp, vp, vp, ctypes.POINTER(ShardGeom), i32, i32, vp, vp, f32, vp, f32, f32, f32, f32, f32, vp,
                                          vp, i64, vp]
    geom = ShardGeom()
    geom.nbuckets, geom.world, geom.nsub = 1, 2, 2
    geom.off[0], geom.len[0] = 0, 16
    n = 32
    p, g = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    g[3] = np.nan
    m, v, part = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(4, np.float32)
    step, norm = np.zeros(1, np.float32), np.zeros(1, np.float32)
    assert shim.brl_adam_shard_norm(0, ptr(g), ctypes.byref(geom), 0, 2, f32(1.0), ptr(part), ptr(step), None, None) == 0
    assert shim.brl_adam_shard_apply(0, ptr(p), ptr(g), ptr(m), ptr(v), ctypes.byref(geom), 0, 2, ptr(part), ptr(step), f32(1e-3), None,
                                     f32(0.9), f32(0.999), f32(1e-5), f32(0.5), f32(1.0), ptr(norm), None, 0, None) == 0
    assert np.isnan(norm[0]) and np.isnan(p).all() and np.isnan(m).all() and np.isnan(v).all()
