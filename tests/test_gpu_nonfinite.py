"""-m gpu: non-finite values through every device path, against the float64 / eager semantics ("Non-finite values").

An output is NaN wherever its reference is NaN and non-finite (on the one-product entry points: with the same sign) wherever it is
+-inf; every other output is what the same launch gives on clean data, bit for bit.  The references themselves are pinned on the CPU
by tests/test_nonfinite_host.py; the poisoned inputs are tests/nonfinite_cases.py's.

  a  brl_mlp_gemm, brl_mlp_gemm_x3, brl_linear_x3p (fp32 rows and planes), brl_linear_act (bf16, fp16): bias + ReLU with a NaN, a
     +inf and a -inf bias and with one NaN weight;
  b  whole forwards with one NaN in a layer-0 weight: every InferenceSnapshot backend, brl_mlp_forward_rows, brl_league_forward,
     brl_fair_forward;
  c  make_roll_out with such an actor;
  d  the loss kernels with one poisoned sample: brl_ppo_loss, brl_ppo_heads_loss_split, brl_fair_chain; brl_sl_loss;
  e  clip + Adam: brl_adam_clip_fin_gather, brl_adam_shard_norm / _apply;
  f  whole update steps with a NaN critic weight;
  g  the GAE scans.
No tolerance here is new: finite outputs are compared bit for bit with a clean launch, or with the bound of the test named."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import nonfinite_cases as nc
from tests.nets import forward64

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
J_NAN, J_PINF, J_NINF, J_W = 5, 33, 70, 41       # the poisoned columns (70: in the second 64-column tile of every entry point)


@pytest.fixture(scope="module")
def env(dds):
    import brl_amd
    return brl_amd.BridgeBidding(lut=(dds["keys"], dds["values"]))


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _all_nan(t):
    return bool(torch.isnan(t.float()).all())


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------------------------------------------
# a: one product, bias + ReLU
# ---------------------------------------------------------------------------------------------------------------
def _check_bias_and_weight(run, w, bias, planes=False, linear=None):
    """run(w, bias[, relu]) -> [M, N] output (planes: [3, M, N] bf16 planes whose sum is the output).  Bias NaN / +inf / -inf at
    columns J_NAN / J_PINF / J_NINF: those columns are all NaN / all +inf / all 0 and every other column is bit for bit the launch
    on the clean bias; one NaN weight in output column J_W: that column all NaN, the rest bit-identical.  linear: the entry point's
    relu = 0 form — the NaN column stays NaN, the infinite ones keep their sign.
    planes: a column of zeros is three planes of zeros; the split of +inf is inf + NaN + NaN (hi = inf, mid = inf - inf), which
    DESIGN.md allows: the column's planes sum to a non-finite number."""
    N = bias.shape[0]
    total = (lambda y: (y[0].float() + y[1].float()) + y[2].float()) if planes else (lambda y: y.float())   # noqa: E731
    cols = lambda y, j: y[..., j]   # noqa: E731
    clean = run(w, bias)
    assert bool(torch.isfinite(total(clean)).all()) and bool((total(clean) > 0).any()) and bool((total(clean) == 0).any())
    b2 = bias.clone()
    b2[J_NAN], b2[J_PINF], b2[J_NINF] = NAN, INF, -INF
    out = run(w, b2)
    keep = torch.ones(N, dtype=torch.bool, device="cuda")
    keep[[J_NAN, J_PINF, J_NINF]] = False
    assert _all_nan(total(out)[:, J_NAN])
    if planes:
        assert not bool(torch.isfinite(total(out)[:, J_PINF]).any()) and bool((cols(out, J_PINF)[0].float() == INF).all())
    else:
        assert bool((total(out)[:, J_PINF] == INF).all())
    assert bool((_bits(cols(out, J_NINF)) == 0).all())
    assert _same_bits(out[..., keep], clean[..., keep])
    w2 = w.clone()
    w2[J_W, 9] = NAN
    out = run(w2, bias)
    keep = torch.ones(N, dtype=torch.bool, device="cuda")
    keep[J_W] = False
    assert _all_nan(total(out)[:, J_W]) and _same_bits(out[..., keep], clean[..., keep])
    if linear is not None:
        lin_clean, out = linear(w, bias), linear(w, b2)
        keep[[J_NAN, J_PINF, J_NINF, J_W]] = False
        assert bool((total(lin_clean) < 0).any())
        assert _all_nan(total(out)[:, J_NAN]) and _same_bits(out[..., keep], lin_clean[..., keep])
        if planes:
            assert not bool(torch.isfinite(total(out)[:, [J_PINF, J_NINF]]).any())
        else:
            assert bool((total(out)[:, J_PINF] == INF).all()) and bool((total(out)[:, J_NINF] == -INF).all())
        assert _all_nan(total(linear(w2, bias))[:, J_W])


def _operands(M, N, K, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *sh: (torch.rand(sh, device="cuda", generator=g) * 2 - 1)   # noqa: E731
    return r(M, K), r(N, K) / K ** 0.5, r(N) * 0.3


@pytest.mark.parametrize("x3", [False, True])
def test_gemm_bias_relu_epilogue_keeps_nan(x3):
    """brl_mlp_gemm / brl_mlp_gemm_x3, layout NT, epilogue bias + ReLU, M = 200 (ragged: 64- and 128-row tiles), N = 72 (no multiple
    of either column tile, two 64-column tiles), K = 64"""
    from brl_amd import _capi
    L = _capi.lib()
    M, N, K = 200, 72, 64
    x, w, bias = _operands(M, N, K, 1)

    def run(w_, b_):
        y = torch.full((M, N), 7.0, device="cuda")
        if x3:
            _capi.check(L.brl_mlp_gemm_x3(0, 0, 1, x.data_ptr(), K, w_.data_ptr(), K, y.data_ptr(), N, M, N, K, 0, b_.data_ptr(), None, 0, None,
                                          None, 0, _stream()))
        else:
            _capi.check(L.brl_mlp_gemm(0, 0, 1, x.data_ptr(), K, w_.data_ptr(), K, y.data_ptr(), N, M, N, K, 0, b_.data_ptr(), None, 0, None,
                                       None, _stream()))
        torch.cuda.synchronize()
        return y
    _check_bias_and_weight(run, w, bias)


@pytest.mark.parametrize("npx", [3, 1])
def test_linear_x3p_epilogue_keeps_nan(npx):
    """brl_linear_x3p, M = 300 (three row tiles, the last ragged), N = 384, K = 96, x as three planes and as one (a 0/1 input): the fp32
    rows and the plane outputs, with ReLU and with relu = 0"""
    from brl_amd import _capi
    L = _capi.lib()
    M, N, K = 300, 384, 96
    x, w, bias = _operands(M, N, K, 2)
    if npx == 1:
        x = (x > 0.6).float()
        xp = x.to(torch.bfloat16)
    else:
        xp = torch.empty((3, M, K), dtype=torch.bfloat16, device="cuda")
        _capi.check(L.brl_split_planes(0, x.data_ptr(), M * K, xp.data_ptr(), M * K, _stream()))

    def run(w_, b_, relu=1, planes=False):
        wp = torch.empty((3, N, K), dtype=torch.bfloat16, device="cuda")
        _capi.check(L.brl_split_planes(0, w_.data_ptr(), N * K, wp.data_ptr(), N * K, _stream()))
        y = torch.full((M, N), 7.0, device="cuda")
        yp = torch.zeros((3, M, N), dtype=torch.bfloat16, device="cuda")
        _capi.check(L.brl_linear_x3p(0, xp.data_ptr(), npx, K, M * K if npx == 3 else 0, wp.data_ptr(), K, N * K, b_.data_ptr(), relu,
                                     y.data_ptr(), N, yp.data_ptr(), N, M * N, M, N, K, _stream()))
        torch.cuda.synchronize()
        return yp if planes else y
    _check_bias_and_weight(run, w, bias, linear=lambda w_, b_: run(w_, b_, relu=0))
    _check_bias_and_weight(lambda w_, b_: run(w_, b_, planes=True), w, bias, planes=True,
                           linear=lambda w_, b_: run(w_, b_, relu=0, planes=True))


@pytest.mark.parametrize("dt,fmt", [(torch.bfloat16, 1), (torch.float16, 2)])
def test_linear_act_epilogue_keeps_nan(env, dt, fmt):
    """brl_linear_act (16-bit inference layer), M = 300 (two row tiles, the second ragged), N = 256 (two column tiles), K = 64, with ReLU
    and with relu = 0"""
    from brl_amd import _capi
    M, N, K = 300, 256, 64
    x, w, bias = _operands(M, N, K, 3)
    x = x.to(dt)

    def run(w_, b_, relu=1):
        y = torch.full((M, N), 7.0, device="cuda").to(dt)
        w16 = w_.to(dt)
        _capi.check(_capi.lib().brl_linear_act(env._h, x.data_ptr(), K, w16.data_ptr(), K, b_.data_ptr(), y.data_ptr(), N, M, N, K, relu, fmt,
                                               _stream()))
        torch.cuda.synchronize()
        return y
    _check_bias_and_weight(run, w, bias, linear=lambda w_, b_: run(w_, b_, relu=0))


# ---------------------------------------------------------------------------------------------------------------
# b: whole forwards, one NaN in a layer-0 weight
# ---------------------------------------------------------------------------------------------------------------
def _poisoned_net(model="DeepMind"):
    from tests.test_gpu_forward_biases import _net
    net = _net(model)
    with torch.no_grad():
        net.body[0].weight[3, 7] = NAN
    return net


@pytest.mark.parametrize("backend", ["library", "views", "x3", "planes_bool", "planes_bf16", "planes_env"])    # = FP32_BACKENDS
def test_fp32_snapshot_backends_report_a_nan_weight(env, backend, monkeypatch):
    """`heads` of every fp32 InferenceSnapshot backend (the path asserted as tests/test_gpu_forward_biases.py does) on a network with
    body[0].weight[3, 7] = NaN: every output of every row is NaN, as in forward64 — a NaN times a 0 observation bit is NaN, so unit 3
    of layer 0 is NaN in every row and layer 1 spreads it to every unit.  (`library` and `views` run addmm + relu_: with the library's
    fused ReLU epilogue, torch._addmm_activation, 0 of their 300 x 39 outputs were NaN — max(x, 0) returns 0 for a NaN.)"""
    from tests.test_gpu_forward_biases import FP32_BACKENDS, _fp32_snapshot, _obs
    assert list(FP32_BACKENDS) == ["library", "views", "x3", "planes_bool", "planes_bf16", "planes_env"]
    net, n = _poisoned_net(), FP32_BACKENDS[backend]
    obs = _obs(n)
    assert _all_nan(forward64(net, obs))
    snap = _fp32_snapshot(backend, net, env, monkeypatch)
    given = obs.to(torch.bfloat16) if backend == "planes_bf16" else obs
    with torch.no_grad():
        out = snap.heads(given)
    print(f"{backend}: {int(torch.isnan(out).sum())} of {out.numel()} outputs NaN")
    assert out.shape == (n, 39) and _all_nan(out), (backend, int(torch.isnan(out).sum()))


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_16_bit_snapshot_reports_a_nan_weight(env, dt, monkeypatch):
    """the 16-bit InferenceSnapshot on brl_linear_act (`body_nk`), 1000 rows: `heads`, `heads(raw=True)` and the partial head products
    are NaN throughout"""
    from brl_amd.models import InferenceSnapshot
    from tests.test_gpu_forward_biases import _obs
    monkeypatch.delenv("BRL_LINEAR16", raising=False)
    monkeypatch.delenv("BRL_HEAD_PARTS", raising=False)
    net, obs = _poisoned_net(), _obs(1000)
    snap = InferenceSnapshot.make(net, dt, env)
    assert snap.body_nk is not None and snap.lin is None
    with torch.no_grad():
        assert _all_nan(snap.heads(obs)) and _all_nan(snap.heads(obs, raw=True))
        parts = snap.head_parts(obs)
        assert parts is not None and _all_nan(parts[:, :, :39].sum(0))


def test_forward_rows_and_league_forward_report_a_nan_weight():
    """brl_mlp_forward_rows (hidden 200 x 2 ReLU layers, 130 permuted rows of 167) and brl_league_forward (three such networks, six
    groups, group g plays network g % 3) with body[0].weight[3, 7] = NaN in ONE network: that network's rows are NaN in all 39
    columns; the league's other groups are bit for bit the clean run; rows not selected and column 39 keep what they held"""
    from brl_amd import _capi
    from brl_amd.league import _net_record
    from tests.test_gpu_forward_biases import _forward_rows, _raw_arrays
    gen = torch.Generator(device="cuda").manual_seed(17)
    hidden, layers = 200, 2
    nets = [_raw_arrays(hidden, layers, "relu", gen) for _ in range(3)]
    sizes = [0, 1, 63, 64, 65, 7]
    G, R = len(sizes), sum(sizes)
    nboards = R + 50
    obs = torch.rand((nboards, 480), device="cuda", generator=gen) < 0.12
    rows = torch.randperm(nboards, device="cuda", generator=gen)[:R].contiguous()
    first = np.concatenate([[0], np.cumsum(sizes)])
    gf = torch.tensor(first, dtype=torch.int32, device="cuda")
    table = torch.tensor([_net_record(nets[g % 3][1]) for g in range(G)], dtype=torch.int64, device="cuda")

    def league():
        out = torch.full((nboards, 40), 123.0, device="cuda")
        scratch = torch.empty(R * (480 + 2 * hidden), device="cuda")
        _capi.check(_capi.lib().brl_league_forward(0, table.data_ptr(), G, layers, hidden, 0, obs.data_ptr(), rows.data_ptr(), gf.data_ptr(), R,
                                                   scratch.data_ptr(), scratch.numel(), out.data_ptr(), 40, _capi.stream()))
        torch.cuda.synchronize()
        return out
    clean = league()
    assert bool(torch.isfinite(clean).all())
    bad_net, bad_ref = nets[1]
    bad_net.body[0].weight[3, 7] = NAN
    out = league()
    for g in range(G):
        idx = rows[int(first[g]):int(first[g + 1])]
        if g % 3 == 1:
            assert _all_nan(forward64(bad_net, obs[idx])) and _all_nan(out[idx][:, :39]), g
        else:
            assert _same_bits(out[idx], clean[idx]), g
    untouched = torch.ones(nboards, dtype=torch.bool, device="cuda")
    untouched[rows] = False
    assert bool((out[untouched] == 123.0).all()) and bool((out[:, 39] == 123.0).all())
    # brl_mlp_forward_rows on the poisoned network alone
    m = 130
    sel = rows[:m].contiguous()
    one = torch.full((nboards, 40), 123.0, device="cuda")
    _forward_rows(bad_ref, obs, sel, m, one)
    keep = torch.ones(nboards, dtype=torch.bool, device="cuda")
    keep[sel] = False
    assert _all_nan(one[sel][:, :39]) and bool((one[keep] == 123.0).all()) and bool((one[:, 39] == 123.0).all())


def test_fair_forward_reports_nan(monkeypatch):
    """brl_fair_forward (100 rows: seven 16-row workgroups, the last ragged) through ActorCritic._fair_forward — the launch itself, which
    must not decline (None would send the module to torch's layers).  One NaN observation entry: that row's logits and value are
    NaN, every other row is bit for bit the clean launch.  One NaN in a layer-0 weight: everything is NaN, as in the module's float64
    forward on the host."""
    from brl_amd.models import make_forward_pass
    monkeypatch.delenv("BRL_FAIR_FORWARD", raising=False)
    fp = make_forward_pass("relu", "FAIR")
    net = fp.init(3, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(4)

    def launch(x_):
        out = net._fair_forward(x_)
        assert out is not None, "brl_fair_forward declined: the module would run torch's layers"
        torch.cuda.synchronize()
        return out
    with torch.no_grad():
        for q in net.parameters():
            q.add_(torch.randn(q.shape, device="cuda", generator=gen) * 0.05)
        x = (torch.rand((100, 480), device="cuda", generator=gen) < 0.12).float()
        lg0, v0 = launch(x)
        assert lg0.shape == (100, 38) and bool(torch.isfinite(lg0).all()) and bool(torch.isfinite(v0).all())
        x2 = x.clone()
        x2[37, 11] = NAN
        lg, v = launch(x2)
        others = torch.arange(100, device="cuda") != 37
        assert _all_nan(lg[37]) and _all_nan(v[37]) and _same_bits(lg[others], lg0[others]) and _same_bits(v[others], v0[others])
        net.l[0].weight[3, 7] = NAN
        lg, v = launch(x)
        ref = fp.init(3, device="cpu").double()
        ref.load_state_dict({k: t.double().cpu() for k, t in net.state_dict().items()})
        lg64, v64 = ref(x.double().cpu())
    assert _all_nan(lg64) and _all_nan(v64) and _all_nan(lg) and _all_nan(v)


# ---------------------------------------------------------------------------------------------------------------
# c: the policy rollout
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["fp32_eager", "fp32_planes", "bf16"])
def test_rollout_with_a_nan_actor_records_nan(env, case, monkeypatch):
    """make_roll_out, T = 2, with body[0].weight[3, 7] = NaN in the actor (the opponent is clean): the run completes, `traj.value` and
    `traj.log_prob` are NaN throughout, and every recorded action is 0 (Pass, always legal) — the sampler's convention for a row
    without a finite candidate logit (csrc/policy_common.hpp).  (512 tables: the hidden layers on the library's GEMM, addmm + relu_.)"""
    import brl_amd
    from brl_amd.models import make_forward_pass
    from tests.test_gpu_forward_biases import ROLLOUTS, _net
    dt, n, graph, over, envvars = ROLLOUTS[case]
    for k in ("BRL_HEAD_PARTS", "BRL_LINEAR16", "BRL_INFERENCE_PLANES", "BRL_TABLES_PER_WAVE", "BRL_INFERENCE_GEMM"):
        monkeypatch.delenv(k, raising=False)
    T = 2
    fp = make_forward_pass("relu", "DeepMind")
    actor, opp = _poisoned_net(), _net("DeepMind", seed=31, init=12)
    cfg = dict(reward_scale=7600, game_mode="competitive", actor_illegal_action_mask=True, num_steps=T, graph_rollout=graph,
               inference_dtype=dt, **over)
    roll = brl_amd.make_roll_out(cfg, env, fp, fp)
    st = env.init(77, num_envs=n)
    rs, traj = roll((actor, None, st, st.observation, 0, 0), opp)
    torch.cuda.synchronize()
    eng = roll.engine
    assert bool(eng.static) == graph and (not graph or eng.graphs), getattr(eng, "graph_error", None)
    if dt is None:
        assert eng.snap_actor.planes_for(n) == (n >= 4096)
    else:
        assert eng.snap_actor.body_nk is not None
    assert traj.value.shape == (T, n) and _all_nan(traj.value) and _all_nan(traj.log_prob)
    assert bool((traj.action == 0).all()) and bool(traj.legal_action_mask[..., 0].all())
    assert bool(torch.isfinite(traj.reward).all())


# ---------------------------------------------------------------------------------------------------------------
# d: the loss kernels, one poisoned sample
# ---------------------------------------------------------------------------------------------------------------
def _dev(b):
    """the batch on the device, in the kernels' types"""
    t = {k: torch.from_numpy(v).cuda() for k, v in b.items()}
    t["mask"] = t["mask"].to(torch.uint8)
    return t


def _check_loss(kind, i, B, ref, got, clean, mask):
    """got / clean = (stats [7], dlogits [B, 38], dvalue [B]) of the poisoned / clean launch; ref = tests/ppo_numpy's on the poisoned batch"""
    nc.assert_same_nonfinite(got[0].cpu().numpy(), ref[0], f"{kind}: statistics")
    nc.assert_same_nonfinite(got[1][i].cpu().numpy(), ref[1][i], f"{kind}: dlogits of the sample")
    nc.assert_same_nonfinite(got[2][i].cpu().numpy(), ref[2][i], f"{kind}: dvalue of the sample")
    bad_stats, bad_d = nc.EXPECTED[kind]
    assert {nc.STATS[k] for k in range(7) if not np.isfinite(ref[0][k])} == bad_stats
    assert bool(np.isfinite(ref[1][i][mask[i]]).all()) == ("legal" not in bad_d) and bool(np.isfinite(ref[2][i])) == ("v" not in bad_d)
    others = torch.arange(B, device="cuda") != i
    assert _same_bits(got[1][others], clean[1][others]) and _same_bits(got[2][others], clean[2][others]), kind


@pytest.mark.parametrize("B", [17, 256])
def test_ppo_loss_kernel_reports_a_poisoned_sample(B):
    """brl_ppo_loss + brl_ppo_stats (masked policy, value clipping, no reward scaling) with one sample poisoned in each of the six
    ways: the seven statistics are NaN (+inf) exactly where tests/ppo_numpy.head_loss's are, the sample's dlogits / dvalue are NaN
    (+inf) where the reference's are, every other sample's derivatives are bit for bit the clean batch's"""
    from brl_amd import _capi
    L = _capi.lib()
    i = B // 3
    clean = nc.settle(nc.loss_batch(B, seed=B), i)

    def run(b):
        t = _dev(b)
        dl, dv = torch.empty(B, 38, device="cuda"), torch.empty(B, device="cuda")
        partials, illp, out = torch.empty((B + 3) // 4, 8, device="cuda"), torch.empty(B, 38, device="cuda"), torch.zeros(8, device="cuda")
        cfg = nc.LOSS_CFG
        _capi.check(L.brl_ppo_loss(0, t["logits"].data_ptr(), 38, t["value"].data_ptr(), t["mask"].data_ptr(), t["action"].data_ptr(),
                                   t["old_value"].data_ptr(), t["old_log_prob"].data_ptr(), t["gae"].data_ptr(), t["tgt"].data_ptr(), B,
                                   cfg["clip_eps"], cfg["vf_coef"], cfg["ent_coef"], 1, 1, dl.data_ptr(), dv.data_ptr(), partials.data_ptr(),
                                   illp.data_ptr(), _stream()))
        gram = (illp.t() @ illp).contiguous()
        _capi.check(L.brl_ppo_stats(0, partials.data_ptr(), B, gram.data_ptr(), cfg["vf_coef"], cfg["ent_coef"], out.data_ptr(), _stream()))
        torch.cuda.synchronize()
        return out[:7], dl, dv
    base = run(clean)
    assert all(bool(torch.isfinite(x).all()) for x in base)
    for kind in nc.POISONS:
        b = nc.poisoned(clean, kind, i)
        _check_loss(kind, i, B, nc.loss_reference(nc.LOSS_CFG, b), run(b), base, b["mask"])


HX = 16      # (the hidden width stays a multiple of 16)


def _heads_inputs(B, H, i, seed):
    """h [B, 16 + H + 16] >= 0, Wh [39, 16 + H + 16], bh [39] for brl_ppo_heads_loss_split.  The sixteen hidden units at either end are
    0 in every sample and zero-weighted: `_overflow` uses the first and the last to make ONE head of ONE sample infinite or NaN from
    finite inputs — 3e38 x 3e38 = +inf in sample i only, 0 x 3e38 = 0 elsewhere; and 3e38 x -3e38 = -inf in the OTHER half of the K
    range, which the launch sums on its own (two K splits): inf - inf = NaN.  (Inside one fma chain the second product would be added
    exactly, unrounded, and leave +inf.)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    h = torch.zeros(B, H + 2 * HX, device="cuda")
    h[:, HX:HX + H] = torch.randn(B, H, device="cuda", generator=g).relu_()
    Wh = torch.zeros(39, H + 2 * HX, device="cuda")
    Wh[:, HX:HX + H] = torch.randn(39, H, device="cuda", generator=g) / H ** 0.5
    return h, Wh, torch.randn(39, device="cuda", generator=g) * 0.1


def _overflow(h, Wh, i, head, nan):
    h, Wh = h.clone(), Wh.clone()
    h[i, -1], Wh[head, -1] = 3e38, 3e38
    if nan:
        h[i, 0], Wh[head, 0] = 3e38, -3e38
    return h, Wh


@pytest.mark.parametrize("B", [17, 256])
def test_heads_loss_split_reports_a_poisoned_sample(B):
    """brl_ppo_heads_loss_split (the heads product + `_loss_fn` of FusedMinibatch's step) + brl_ppo_stats_gram, K = 16 + 256 + 16 in two splits.  The launch
    forms logits and value itself, so the four poisons on network outputs are made inside it from finite inputs (_heads_inputs): the
    poisoned sample's value is +inf / NaN, one of its legal / illegal logits NaN, every other head of every sample is unchanged (the
    stored heads asserted).  The reference is tests/ppo_numpy.head_loss on the stored heads' float64 counterpart."""
    from brl_amd import _capi
    L = _capi.lib()
    H, i = 256, B // 3
    HT = H + 2 * HX
    batch = nc.loss_batch(B, seed=B + 1)
    h0, Wh0, bh = _heads_inputs(B, H, i, B)
    heads64 = (h0.double() @ Wh0.double().t() + bh.double()).cpu().numpy()
    batch["logits"], batch["value"] = heads64[:, :38].astype(np.float32), heads64[:, 38].astype(np.float32)
    nc.settle(batch, i)
    lgroups = (B + 3) // 4
    cfg = nc.LOSS_CFG

    def run(b, h, Wh):
        t = _dev(b)
        heads, dheads = torch.empty(B, 39, device="cuda"), torch.empty(B, 39, device="cuda")
        partials, gram_p = torch.empty(lgroups, 8, device="cuda"), torch.empty(lgroups, 1444, device="cuda")
        hparts, out, vec = torch.empty(2, B, 39, device="cuda"), torch.zeros(8, device="cuda"), torch.zeros(40, device="cuda")
        _capi.check(L.brl_ppo_heads_loss_split(0, h.data_ptr(), HT, Wh.data_ptr(), bh.data_ptr(), HT, t["mask"].data_ptr(),
                                               t["action"].data_ptr(), t["old_value"].data_ptr(), t["old_log_prob"].data_ptr(),
                                               t["gae"].data_ptr(), t["tgt"].data_ptr(), B, cfg["clip_eps"], cfg["vf_coef"], cfg["ent_coef"],
                                               1, 1, 0, heads.data_ptr(), dheads.data_ptr(), partials.data_ptr(), gram_p.data_ptr(),
                                               hparts.data_ptr(), 2, _stream()))
        _capi.check(L.brl_ppo_stats_gram(0, partials.data_ptr(), lgroups, B, gram_p.data_ptr(), lgroups, cfg["vf_coef"], cfg["ent_coef"], 0.0,
                                         out.data_ptr(), None, vec.data_ptr(), _stream()))
        torch.cuda.synchronize()
        return (out[:7], dheads[:, :38].contiguous(), dheads[:, 38].contiguous()), heads
    base, heads0 = run(batch, h0, Wh0)
    assert all(bool(torch.isfinite(x).all()) for x in base)
    for kind in nc.POISONS:
        b = nc.poisoned(batch, kind, i)          # (the reference's inputs; the launch gets logits / value from h and Wh)
        made = kind in ("nan_value", "inf_value", "nan_legal_logit", "nan_illegal_logit")
        if made:                                 # the head nc.poisoned chose: the value, or the logit it set to NaN
            head = 38 if kind.endswith("value") else int(np.flatnonzero(np.isnan(b["logits"][i]))[0])
        h, Wh = _overflow(h0, Wh0, i, head, kind != "inf_value") if made else (h0, Wh0)
        got, heads = run(b, h, Wh)
        if made:
            want = torch.from_numpy(np.concatenate([b["logits"], b["value"][:, None]], 1))
            nc.assert_same_nonfinite(heads.cpu().numpy(), want.numpy(), f"{kind}: heads")
            ok = torch.isfinite(want).cuda()
            assert int((~ok).sum()) == 1 and _same_bits(heads[ok], heads0[ok])
        _check_loss(kind, i, B, nc.loss_reference(cfg, b), got, base, b["mask"])


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("B", [16, 256])
def test_fair_chain_reports_a_poisoned_sample(B, act):
    """brl_fair_chain (forward + `_loss_fn` + backward chain of the FAIR network, ReLU and tanh) + brl_ppo_stats_gram at 16 and 256
    samples — the entry point takes multiples of 16 only: 17 is refused, asserted.  A NaN `old_log_prob` and a NaN advantage of one
    sample: the statistics and that sample's d(heads) are NaN where tests/ppo_numpy.head_loss's are (on the launch's own last hidden
    layer times the head weights in float64), every other sample's d(heads) and every other sample's rows of the backward chain's
    dz are bit for bit the clean launch.  One NaN in the sample's observation row: its 39 heads are NaN together and the same holds.
    The chain forms its heads inside the launch, so ONE non-finite head of ONE sample is made there from finite inputs: hidden unit
    U is an indicator of sample i — layer 6 reads the observation columns directly, so x0[i, CI] = 3e38 reaches the last hidden
    layer through the two pre-activation shortcuts (z6 -> x3 -> x4) with every weight that touches unit U or column CI zeroed, and
    head_w[head, U] = 3e38 overflows in sample i alone (asserted on the stored x4).  That gives a +inf value, a +inf legal logit
    and a +inf illegal logit, each alone: the statistics and derivatives against tests/ppo_numpy.head_loss on those heads (the
    softmax turns the infinite logit into the same NaNs as a NaN logit: inf - inf), every other sample bit for bit the launch
    without the observation entry.  A lone NaN head cannot be made this way: the heads are ONE fma chain over k, inside which a
    second product of -9e76 is added unrounded to the +inf already there and leaves +inf (brl_ppo_heads_loss_split sums two K
    splits, which is where its NaN heads come from).  A NaN value or NaN logit alone therefore reaches ppo_loss_sample — the code
    the chain shares — through brl_ppo_loss and brl_ppo_heads_loss_split only."""
    from brl_amd import _capi
    L = _capi.lib()
    H, i = 200, B // 3
    g = torch.Generator(device="cuda").manual_seed(B + act)
    f = lambda *s: torch.randn(s, device="cuda", generator=g) * 0.05   # noqa: E731
    net, wk, keep = _capi.FairNet(), _capi.FairWork(), []
    for l in range(11):
        w, b_ = f(H, 480 if l == 0 else 680 if l == 6 else H), f(H)
        keep += [w, b_]
        net.w[l], net.b[l] = w.data_ptr(), b_.data_ptr()
    wh, bh = f(39, H), f(39)
    net.head_w, net.head_b = wh.data_ptr(), bh.data_ptr()
    U, CI, V = 77, 5, 3e38                        # the indicator unit, its observation column, its value in sample i
    W, bs = keep[0::2], keep[1::2]
    W[0][:, CI] = 0
    W[6][:, H + CI] = 0
    W[6][U, :] = 0
    W[6][U, H + CI] = 1
    W[7][:, U] = 0
    W[8][U, :] = 0
    W[9][:, U] = 0
    W[10][U, :] = 0
    bs[6][U], bs[8][U], bs[10][U] = 0, 0, 0
    wh[:, U] = 0
    nwg = B // 16
    shapes = dict(inp=(9, B, H), dzs=(9, B, H), gates=(4, B, H), cat6=(B, 680), x4=(B, H), dz0=(B, H), dz6=(B, H), dheads=(B, 40),
                  tiles=(11 * nwg * H + nwg * 39,), partials=(nwg, 8), gram_partials=(nwg, 1444))
    bufs = {k: torch.zeros(s, device="cuda") for k, s in shapes.items()}
    for k, t in bufs.items():
        setattr(wk, k, t.data_ptr())
    x0 = (torch.rand((B, 480), device="cuda", generator=g) < 0.1).float()
    x0[:, CI] = 0
    cfg = nc.LOSS_CFG

    def run(b, x):
        t = _dev(b)
        rc = L.brl_fair_chain(0, net, x.data_ptr(), t["mask"].data_ptr(), t["action"].data_ptr(), t["old_value"].data_ptr(),
                              t["old_log_prob"].data_ptr(), t["gae"].data_ptr(), t["tgt"].data_ptr(), x.shape[0], cfg["clip_eps"], cfg["vf_coef"],
                              cfg["ent_coef"], 1, 1, 0, act, wk, _stream())
        if x.shape[0] % 16:
            return rc
        _capi.check(rc)
        out, vec = torch.zeros(8, device="cuda"), torch.zeros(40, device="cuda")
        _capi.check(L.brl_ppo_stats_gram(0, bufs["partials"].data_ptr(), nwg, B, bufs["gram_partials"].data_ptr(), nwg, cfg["vf_coef"],
                                         cfg["ent_coef"], 0.0, out.data_ptr(), None, vec.data_ptr(), _stream()))
        torch.cuda.synchronize()
        dh = bufs["dheads"]
        return ((out[:7], dh[:, :38].clone(), dh[:, 38].clone()), bufs["x4"].clone(), bufs["dzs"].clone(), bufs["dz0"].clone())
    batch = nc.loss_batch(B, seed=B + 2)
    _, x4, _, _ = run(batch, x0)
    heads64 = (x4.double() @ wh.double().t() + bh.double()).cpu().numpy()
    batch["logits"], batch["value"] = heads64[:, :38].astype(np.float32), heads64[:, 38].astype(np.float32)
    nc.settle(batch, i)
    base, x4, dzs0, dz00 = run(batch, x0)
    assert all(bool(torch.isfinite(x).all()) for x in base) and float(dzs0.abs().max()) > 0
    others = torch.arange(B, device="cuda") != i
    for kind in ("nan_old_logp", "nan_adv", "nan_observation"):
        x = x0
        if kind == "nan_observation":
            b = {k: v.copy() for k, v in batch.items()}
            b["logits"][i], b["value"][i] = np.nan, np.nan
            x = x0.clone()
            x[i, 11] = NAN
        else:
            b = nc.poisoned(batch, kind, i)
        got, _, dzs, dz0 = run(b, x)
        ref = nc.loss_reference(cfg, b)
        nc.assert_same_nonfinite(got[0].cpu().numpy(), ref[0], f"{kind}: statistics")
        nc.assert_same_nonfinite(got[1][i].cpu().numpy(), ref[1][i], f"{kind}: dlogits of the sample")
        nc.assert_same_nonfinite(got[2][i].cpu().numpy(), ref[2][i], f"{kind}: dvalue of the sample")
        assert np.isnan(ref[0][0]) and np.isnan(ref[1][i]).any()
        assert _same_bits(got[1][others], base[1][others]) and _same_bits(got[2][others], base[2][others]), kind
        assert _same_bits(dzs[:, others], dzs0[:, others]) and _same_bits(dz0[others], dz00[others]), kind
    # ---- one infinite head of sample i, made inside the launch
    legal = np.flatnonzero(batch["mask"][i])
    heads_of = {"inf_value": 38, "inf_legal_logit": int(legal[legal != batch["action"][i]][-1]), "inf_illegal_logit": 37}
    like = {"inf_value": "inf_value", "inf_legal_logit": "nan_legal_logit", "inf_illegal_logit": "nan_illegal_logit"}
    xi = x0.clone()
    xi[i, CI] = V
    for kind, head in heads_of.items():
        wh[head, U] = V
        torch.cuda.synchronize()
        base_k, x4_0, dzs0, dz00 = run(batch, x0)                # (unit U is 0 in every sample: the launch on the clean batch)
        assert all(_same_bits(a, b_) for a, b_ in zip(base_k, base)) and _same_bits(x4_0, x4)
        got, x4_k, dzs, dz0 = run(batch, xi)
        wh[head, U] = 0
        want_x4 = x4.clone()
        want_x4[i, U] = V
        assert _same_bits(x4_k, want_x4)                         # the indicator: x4[i, U] = 3e38, nothing else moved
        with np.errstate(all="ignore"):
            heads = (x4_k.double() @ wh.double().t() + bh.double()).cpu().numpy().astype(np.float32)
        heads[i, head] = np.inf                                  # (3e38 x 3e38 in float32)
        b = {k: v.copy() for k, v in batch.items()}
        b["logits"], b["value"] = heads[:, :38].copy(), heads[:, 38].copy()
        ref = nc.loss_reference(cfg, b)
        bad_stats, bad_d = nc.EXPECTED[like[kind]]
        assert {nc.STATS[k] for k in range(7) if not np.isfinite(ref[0][k])} == bad_stats, kind
        assert bool(np.isfinite(ref[1][i][b["mask"][i]]).all()) == ("legal" not in bad_d) and bool(np.isfinite(ref[2][i])) == ("v" not in bad_d)
        nc.assert_same_nonfinite(got[0].cpu().numpy(), ref[0], f"{kind}: statistics")
        nc.assert_same_nonfinite(got[1][i].cpu().numpy(), ref[1][i], f"{kind}: dlogits of the sample")
        nc.assert_same_nonfinite(got[2][i].cpu().numpy(), ref[2][i], f"{kind}: dvalue of the sample")
        assert _same_bits(got[1][others], base_k[1][others]) and _same_bits(got[2][others], base_k[2][others]), kind
        assert _same_bits(dzs[:, others], dzs0[:, others]) and _same_bits(dz0[others], dz00[others]), kind
    if B == 16:
        b17 = nc.loss_batch(17, seed=1)
        assert run(b17, torch.zeros(17, 480, device="cuda")) == -1


def test_sl_loss_reports_a_nan_logit():
    """brl_sl_loss (sl.sl_loss, 300 rows: more than one workgroup's share, entropy coefficient 0.01) with a NaN on a legal logit of one
    row: total, target_loss and entropy (out[0..2]) are NaN as in tests/sl_teacher.loss64, that row's dlogits are NaN where the
    reference's are, the other rows' dlogits are bit for bit the clean launch's"""
    from brl_amd import sl
    from tests.sl_teacher import loss64
    rng = np.random.default_rng(3)
    B, row = 300, 121
    z = rng.normal(0, 4, (B, 38)).astype(np.float32)
    mask = rng.random((B, 38)) < 0.4
    mask[:, 0] = True
    label = np.array([rng.choice(np.nonzero(m)[0]) for m in mask], np.int32)
    lt, mt = torch.from_numpy(label).cuda(), torch.from_numpy(mask.astype(np.uint8)).cuda()

    def run(zz):
        out, d = torch.zeros(5, device="cuda"), torch.zeros((B, 38), device="cuda")
        sl.sl_loss(torch.from_numpy(zz).cuda(), lt, mt, 0.01, d, out)
        torch.cuda.synchronize()
        return out, d
    out0, d0 = run(z)
    assert bool(torch.isfinite(out0).all()) and bool(torch.isfinite(d0).all())
    z2 = z.copy()
    z2[row, 0] = np.nan
    out, d = run(z2)
    with np.errstate(all="ignore"):
        want, dwant = loss64(z2.astype(np.float64), label, mask, 0.01)
    assert np.isnan(want[:3]).all()
    nc.assert_same_nonfinite(out.cpu().numpy()[[0, 1, 2, 4]], want[[0, 1, 2, 4]], "statistics")
    nc.assert_same_nonfinite(d[row].cpu().numpy(), dwant[row], "dlogits of the row")
    others = torch.arange(B, device="cuda") != row
    assert _same_bits(d[others], d0[others])


# ---------------------------------------------------------------------------------------------------------------
# e: clip + Adam
# ---------------------------------------------------------------------------------------------------------------
N_ADAM, TAIL, TILES = 4096 + 8, 8, 3          # the sizes of tests/test_gpu_parity.py::test_fused_update_helpers_match_torch


def _adam_inputs(bad, where):
    g = torch.Generator(device="cuda").manual_seed(1)
    p0 = torch.randn(N_ADAM, device="cuda", generator=g)
    grad = torch.randn(N_ADAM, device="cuda", generator=g)
    parts = torch.randn(TILES, TAIL, device="cuda", generator=g)
    grad[N_ADAM - TAIL:] = parts.sum(0)
    grad[where] = bad
    return p0, grad, parts


def _torch_step(p0, grad):
    ref = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([ref], lr=1e-3, eps=1e-5)
    ref.grad = grad.clone()
    norm = torch.nn.utils.clip_grad_norm_([ref], 0.5)
    opt.step()
    return ref.detach(), opt.state[ref]["exp_avg"], opt.state[ref]["exp_avg_sq"], norm


def _check_adam(got, want, bad):
    """got / want = (p, m, v, norm): the NaN / inf pattern of torch's, all NaN for a NaN gradient; finite parameters within the
    existing atol 2e-6"""
    for x, y, name in zip(got, want, ("p", "m", "v", "norm")):
        nc.assert_same_nonfinite(x.cpu().numpy(), y.cpu().numpy(), name)
    if bad != bad:
        assert all(_all_nan(x) for x in got)
    else:
        assert int(torch.isnan(want[0]).sum()) == 1 and float(want[3]) == INF
    ok = torch.isfinite(want[0])
    assert torch.allclose(got[0][ok], want[0][ok], atol=2e-6)


@pytest.mark.parametrize("bad,where", [(NAN, 100), (NAN, N_ADAM - 3), (INF, 100)])
def test_adam_clip_fin_gather_goes_nan_like_torch(bad, where):
    """brl_adam_clip_fin_gather, one step from fresh moments, against torch.optim.Adam + clip_grad_norm_.  One NaN gradient element (in
    the body of the buffer, or in the tail the launch sums from tiles): p, m, v and norm_out are all NaN.  One +inf element: the norm is
    +inf, the clip factor 0, that element's p / m / v NaN (0 x inf) and every other parameter finite and within 2e-6 of torch's."""
    from brl_amd import _capi
    L = _capi.lib()
    p0, grad, parts = _adam_inputs(bad, where)
    if where >= N_ADAM - TAIL:
        parts[1, where - (N_ADAM - TAIL)] = bad
    want = _torch_step(p0, grad)
    p, m, v = p0.clone(), torch.zeros(N_ADAM, device="cuda"), torch.zeros(N_ADAM, device="cuda")
    step, scratch, norm = torch.zeros((), device="cuda"), torch.empty(2048, device="cuda"), torch.zeros(1, device="cuda")
    idx = torch.zeros(1, dtype=torch.int32, device="cuda")
    g2 = grad.clone()
    g2[N_ADAM - TAIL:] = 0.0                        # (written by the launch from `parts`)
    _capi.check(L.brl_adam_clip_fin_gather(0, p.data_ptr(), g2.data_ptr(), m.data_ptr(), v.data_ptr(), N_ADAM, step.data_ptr(), 1e-3, None,
                                           0.9, 0.999, 1e-5, 0.5, scratch.data_ptr(), scratch.numel(), idx.data_ptr(), norm.data_ptr(), None,
                                           0, 1, (C.c_void_p * 1)(parts.data_ptr()), (C.c_int64 * 1)(TAIL), (C.c_int64 * 1)(TILES),
                                           (C.c_void_p * 1)(g2[N_ADAM - TAIL:].data_ptr()), _stream()))
    torch.cuda.synchronize()
    _check_adam((p, m, v, norm[0]), want, bad)


@pytest.mark.parametrize("bad", [NAN, INF])
def test_adam_shard_sweeps_go_nan_like_torch(bad):
    """brl_adam_shard_norm / _apply on one bucket cut into two slices: the replicated sweep (ranks 0..2 in one call) against torch as
    above, and the two per-rank sweeps together equal to it — NaN positions equal, everything else bit for bit.  The poisoned element
    lies in rank 0's slice: rank 1's sweep sees it only through the all-gathered norm partials."""
    from brl_amd import _capi
    L = _capi.lib()
    p0, grad, _ = _adam_inputs(bad, 100)
    want = _torch_step(p0, grad)
    geom = _capi.ShardGeom()
    geom.nbuckets, geom.world, geom.nsub = 1, 2, 4
    geom.off[0], geom.len[0] = 0, N_ADAM // 2

    def sweep(per_rank):
        p, m, v = p0.clone(), torch.zeros(N_ADAM, device="cuda"), torch.zeros(N_ADAM, device="cuda")
        step, norm, part = torch.zeros((), device="cuda"), torch.zeros(1, device="cuda"), torch.zeros(8, device="cuda")
        spans = [(0, 1), (1, 2)] if per_rank else [(0, 2)]
        for lo, hi in spans:
            step.zero_()
            _capi.check(L.brl_adam_shard_norm(0, grad.data_ptr(), C.byref(geom), lo, hi, 1.0, part.data_ptr(), step.data_ptr(), None, _stream()))
        for lo, hi in spans:
            _capi.check(L.brl_adam_shard_apply(0, p.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), C.byref(geom), lo, hi,
                                               part.data_ptr(), step.data_ptr(), 1e-3, None, 0.9, 0.999, 1e-5, 0.5, 1.0, norm.data_ptr(), None,
                                               0, _stream()))
        torch.cuda.synchronize()
        assert float(step) == 1.0
        return p, m, v, norm[0]
    whole, ranks = sweep(False), sweep(True)
    _check_adam(whole, want, bad)
    for x, y in zip(whole, ranks):
        assert torch.equal(torch.isnan(x), torch.isnan(y))
        ok = ~torch.isnan(x)
        assert _same_bits(x[ok], y[ok])


# ---------------------------------------------------------------------------------------------------------------
# f: whole update steps
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["fused_minibatch", "fused_fair_chain", "fused_fair_launches", "graphed_eager", "eager"])
def test_update_step_goes_nan_with_the_critic(path):
    """make_update_step, minibatch 256, one epoch of one minibatch, critic.weight[0, 5] = NaN — FusedMinibatch (DeepMind), FusedFair
    with brl_fair_chain and launch by launch, the captured autograd step and the eager one: `total` and `value_loss` are NaN and every
    parameter is NaN afterwards (clip_grad_norm_'s NaN factor reaches all of them), as tests/test_nonfinite_host.py shows for the
    eager step on the CPU"""
    from brl_amd.models import make_forward_pass
    from brl_amd.update import FusedFair, FusedMinibatch, GraphedMinibatch, make_update_step
    from tests.test_update_cpu import CFG, fake_batch
    fair = path.startswith("fused_fair")
    fp = make_forward_pass("relu", "FAIR" if fair else "DeepMind")
    net = fp.init(4, device="cuda")
    with torch.no_grad():
        net.critic.weight[0, 5] = NAN
    tb, adv, tgt = fake_batch(1, 256, seed=6)
    cfg = dict(CFG, minibatch_size=256, update_epochs=1, graph_update=path != "eager", fused_update=path.startswith("fused"),
               fair_chain=path != "fused_fair_launches")
    rs, (total, aux) = make_update_step(cfg, fp)((net, None, None, None, 0, 9), type(tb)(*[x.cuda() for x in tb]), adv.cuda(), tgt.cuda())
    torch.cuda.synchronize()
    step = rs[1].get("graphed")
    if path != "eager":
        want = {"fused_minibatch": FusedMinibatch, "graphed_eager": GraphedMinibatch}.get(path, FusedFair)
        assert isinstance(step, want), rs[1].get("graph_error")
        assert not fair or step.chain == (path == "fused_fair_chain")
    assert total.shape == (1, 1) and _all_nan(total) and _all_nan(aux[0])
    for name, q in net.named_parameters():
        assert _all_nan(q), (name, int(torch.isnan(q).sum()), q.numel())


# ---------------------------------------------------------------------------------------------------------------
# g: GAE
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,N", [(7, 130), (33, 64)])
def test_gae_scans_on_non_finite_inputs(env, oracle, dds, T, N):
    """gae_scan on values, rewards and a last value holding NaN, +inf and -inf, and brl_rollout_random_gae's in-launch scan with such a
    `last_val`, against oracle.gae (pinned against src/gae.py:28-29, 39 by tests/test_nonfinite_host.py), NaN for NaN"""
    from brl_amd import _capi
    from brl_amd.gae import gae_scan
    from brl_amd.roll_out import alloc_transition
    from tests.gpu_util import make_env, to_np
    done, value, reward, last = nc.gae_inputs(T, N, seed=T)
    adv, tgt = gae_scan(env, torch.from_numpy(done).cuda(), torch.from_numpy(value).cuda(), torch.from_numpy(reward).cuda(),
                        torch.from_numpy(last).cuda(), 0.99, 0.95)
    wa, wt = oracle.gae(done.astype(np.uint8), value, reward, last, 0.99, 0.95)
    assert np.isnan(wa).any() and np.isinf(wa).any()
    assert np.array_equal(to_np(adv), wa, equal_nan=True) and np.array_equal(to_np(tgt), wt, equal_nan=True)
    # the scan inside the rollout launch
    e = make_env(dds, 4)
    st = e.init(77, num_envs=N)
    traj = alloc_transition(T, N, e.device)
    p = _capi.TransitionPtrs()
    for f in _capi.TransitionPtrs._names:
        setattr(p, f, getattr(traj, f).data_ptr())
    lo, lm = torch.empty((N, 480), dtype=torch.bool, device="cuda"), torch.empty((N, 38), dtype=torch.bool, device="cuda")
    tc = torch.zeros(1, dtype=torch.int64, device="cuda")
    lv = torch.from_numpy(last).cuda()
    adv, tgt = torch.empty((T, N), device="cuda"), torch.empty((T, N), device="cuda")
    gl = float(torch.tensor(0.99 * 0.95, dtype=torch.float32))
    _capi.check(_capi.lib().brl_rollout_random_gae(e._h, st.packed.data_ptr(), N, T, 5, 7600.0, C.byref(p), lo.data_ptr(), lm.data_ptr(),
                                                   tc.data_ptr(), lv.data_ptr(), 0.99, gl, adv.data_ptr(), tgt.data_ptr(), _stream()))
    torch.cuda.synchronize()
    wa, wt = oracle.gae(to_np(traj.done).astype(np.uint8), to_np(traj.value), to_np(traj.reward), last, 0.99, 0.95)
    assert np.isnan(wa).any() and np.isfinite(wa).any()
    assert np.array_equal(to_np(adv), wa, equal_nan=True) and np.array_equal(to_np(tgt), wt, equal_nan=True)
