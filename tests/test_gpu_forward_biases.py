"""-m gpu: every inference forward of the DeepMind MLPs on networks whose biases are NOT hk.Linear's zeros (tests/nets.py).

On a zero-bias network a forward that drops a bias, or adds another layer's, another network's or the other head's, gives the same
numbers.  Here every network is `perturbed`, every reference is a plain float64 forward computed with torch on the GPU (`forward64`;
`forward16_ref` for the 16-bit paths: float64 on the rounded parameters and activations), and every test first asserts — in float64
— that each bias mix-up of `bias_slots` moves the outputs by at least 8 x the tolerance it is about to use.

  a / b  InferenceSnapshot: every backend, and `refresh` into the same tensors;
  c      the policy rollout's recorded `value` / `log_prob` columns and its opponent snapshot, on every route;
  d      brl_mlp_forward_rows from raw arrays (no module) at widths and depths the suite never checked values at;
  e      brl_league_forward from raw arrays: every network's biases distinct, empty groups first, in the middle and last.

Bounds.  fp32-grade paths: the project's 2e-4 max(1, max|ref|).  16-bit paths: against forward16_ref, 2 x the error torch's own chain
in that dtype (addmm per layer: fp32 accumulation, one rounding per layer; the heads in fp32 on the rounded parameters) has against
the same reference on the same inputs — both chains accumulate in fp32 and round once per layer, they differ in summation order only,
which flips single roundings that then propagate; outputs that went through a 16-bit store (InferenceSnapshot.heads, whose matrix
is the 16-bit GEMM's in either form; the rollout with fuse_heads=False) get one unit in the last place of `dtype` at the value on top.
Measured on the MI355X (printed by each test): see DESIGN section 5.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.nets import assert_sees_bias_slots, copy64, forward16_ref, forward64, perturbed, raw_net

pytestmark = pytest.mark.gpu

NET_SEED, PERTURB_SEED, REFRESH_SEED, OBS_SEED = 11, 21, 29, 5
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}


@pytest.fixture(scope="module")
def env(dds):
    import brl_amd
    return brl_amd.BridgeBidding(lut=(dds["keys"], dds["values"]))


def _net(model, seed=PERTURB_SEED, init=NET_SEED):
    from brl_amd.models import make_forward_pass
    return perturbed(make_forward_pass("relu", model).init(init, device="cuda"), seed)


def _obs(n, seed=OBS_SEED):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.rand((n, 480), device="cuda", generator=g) < 0.12


def _err(out, ref):
    return float((out.double() - ref).abs().max())


def _tol32(ref):
    return 2e-4 * max(1.0, float(ref.abs().max()))


def _chain16(net, obs, dt):
    """torch's own 16-bit forward: addmm + ReLU per layer in `dt`, the heads in fp32 on the rounded head parameters"""
    with torch.no_grad():
        h = obs.to(dt)
        for lin in net.body:
            h = torch.addmm(lin.bias.to(dt), h, lin.weight.to(dt).t()).relu_()
        hw = torch.cat([net.actor.weight, net.critic.weight]).to(dt).float()
        hb = torch.cat([net.actor.bias, net.critic.bias]).to(dt).float()
        return torch.addmm(hb, h.float(), hw.t())


def _ulp(ref, dt):
    """one unit in the last place of `dt` at each |ref| (0 at 0)"""
    p = 7 if dt == torch.bfloat16 else 10
    _, e = torch.frexp(ref.abs())            # |ref| = m 2^e, m in [0.5, 1)
    return torch.where(ref == 0, torch.zeros_like(ref), torch.ldexp(torch.ones_like(ref), e - 1 - p))


def _bound16(net, obs, dt, ref16):
    """-> (the library chain's error against ref16, the bound of a kernel path = 2 x that, one ulp of `dt` at max|ref16|)"""
    e_lib = _err(_chain16(net, obs, dt), ref16)
    return e_lib, 2 * e_lib, float(_ulp(ref16.abs().max(), dt))


def _head_h_form(snap, given):
    """what a step kernel forms from the stored last layer (brl_macro_ext.head_h): hidden x head_wt^T + head_bf, here in float64"""
    with torch.no_grad():
        return snap.hidden(given).double() @ snap.head_wt.double().t() + snap.head_bf.double()


def _excess(out, ref, allowance):
    """max of |out - ref| - allowance (elementwise)"""
    return float(((out.double() - ref).abs() - allowance).max())


# ---------------------------------------------------------------------------------------------------------------
# a / b: InferenceSnapshot, fp32-grade backends
# ---------------------------------------------------------------------------------------------------------------
FP32_BACKENDS = {"library": 300, "views": 300, "x3": 4096, "planes_bool": 4096, "planes_bf16": 4096, "planes_env": 4096}


def _fp32_snapshot(backend, net, env, monkeypatch):
    from brl_amd.models import InferenceSnapshot
    monkeypatch.setenv("BRL_INFERENCE_PLANES", "0" if backend == "x3" else "1")
    if backend == "library":
        snap = InferenceSnapshot.make(net, gemm="library")
        assert snap.lin is None and snap.wp is None and not snap.views
    elif backend == "views":
        snap = InferenceSnapshot.make(net, views=True, gemm="library")
        assert snap.views and snap.body[0][1].data_ptr() == net.body[0].bias.data_ptr()
    elif backend == "x3":
        snap = InferenceSnapshot.make(net, gemm="bf16x3")
        assert snap.gemm_x3 and snap.lin is not None and snap.wp is None
    else:
        snap = InferenceSnapshot.make(net, env=env if backend == "planes_env" else None, own_cast=True, gemm="bf16x3")
        assert snap.wp is not None and snap.planes_for(4096)
    assert snap.body_nk is None
    return snap


def _addresses(snap):
    t = []
    if not snap.views:
        t += [x for pair in snap.body for x in pair]
    for group in (snap.lin if not snap.views else None, snap.body_nk):
        if group is not None:
            t += [x for pair in group for x in pair]
    t += list(snap.wp or []) + [snap.head_w, snap.head_wt, snap.head_b, snap.head_bf]
    return [x.data_ptr() for x in t]


@pytest.mark.parametrize("backend", list(FP32_BACKENDS))
@pytest.mark.parametrize("model", ["DeepMind", "DeepMind_6"])
def test_fp32_snapshot_backends_add_every_bias(env, model, backend, monkeypatch):
    """`heads` of an fp32 InferenceSnapshot against forward64 within 2e-4 max(1, max|ref|), at the smallest row count that still takes
    the backend's path (asserted): torch's addmm + relu_ on copies (300 rows) and on views of the module's own parameters,
    brl_mlp_gemm_x3 (4096 rows, BRL_INFERENCE_PLANES=0), brl_linear_x3p with the observation given as bool, as bf16, and cast by the
    library (`env` + own_cast); the two bf16x3 paths also within 1.05 e_lib + 1e-7 scale of the library path's own error; the same
    bound for `hidden` times `head_wt` plus `head_bf`, what a step kernel would form from the stored last layer.  Then the
    network is perturbed again in place and `refresh` re-reads it: the same addresses, the new reference within the same bound, the
    old reference at least 8 bounds away."""
    n = FP32_BACKENDS[backend]
    net, obs = _net(model), _obs(n)
    ref = forward64(net, obs)
    tol = _tol32(ref)
    sens = assert_sees_bias_slots(net, obs, tol)
    snap = _fp32_snapshot(backend, net, env, monkeypatch)
    given = obs.to(torch.bfloat16) if backend == "planes_bf16" else obs
    x = snap._input(given)
    assert x.dtype == (torch.bfloat16 if backend.startswith("planes") else torch.float32)
    assert snap.route(x) == {"library": "library", "views": "library", "x3": "x3"}.get(backend, "planes")
    with torch.no_grad():
        out = snap.heads(given)
    assert out.dtype == torch.float32 and out.shape == (n, 39)
    e = _err(out, ref)
    print(f"{model} {backend}: error {e:.2e} of {tol:.2e}; smallest bias-slot effect {sens:.3f}")
    assert e < tol and _err(_head_h_form(snap, given), ref) < tol
    e_lib = None
    if backend in ("x3", "planes_bool", "planes_bf16", "planes_env"):
        from brl_amd.models import InferenceSnapshot
        with torch.no_grad():
            e_lib = _err(InferenceSnapshot.make(net, gemm="library").heads(obs), ref)
        print(f"{model} {backend}: library path {e_lib:.2e}")
        assert e_lib < tol and e <= 1.05 * e_lib + 1e-7 * max(1.0, float(ref.abs().max())), (e, e_lib)
    # ---- refresh
    before = _addresses(snap)
    perturbed(net, REFRESH_SEED)
    snap.refresh(net)
    assert _addresses(snap) == before
    ref2 = forward64(net, obs)
    tol2 = _tol32(ref2)
    assert_sees_bias_slots(net, obs, tol2)
    with torch.no_grad():
        out2 = snap.heads(given)
    assert _err(out2, ref2) < tol2 and _err(out2, ref) >= 8 * tol2, (_err(out2, ref2), _err(out2, ref))
    assert _err(_head_h_form(snap, given), ref2) < tol2          # (head_wt and head_bf follow too)


# ---------------------------------------------------------------------------------------------------------------
# a / b: InferenceSnapshot, 16-bit
# ---------------------------------------------------------------------------------------------------------------
def _four_forms(snap, obs):
    """the four ways a 16-bit snapshot's outputs are consumed -> {name: ([n, 39] float64, stored in 16 bits?)}"""
    with torch.no_grad():
        raw = snap.heads(obs, raw=True)
        full = snap.heads(obs)
        assert raw.dtype == snap.dtype and full.dtype == torch.float32 and torch.equal(full, raw.float())
        parts = snap.head_parts(obs)
        assert parts is not None and parts.shape == (snap.head_wt.shape[1] // 128, obs.shape[0], snap.HEAD_PART_LD)
        lg = snap.head_bf.clone().expand(obs.shape[0], 39).contiguous()
        for p_ in range(parts.shape[0]):
            lg = lg + parts[p_, :, :39]                      # brl_policy_step_ex's order (brl_macro_ext.head_part)
        h = snap.hidden(obs)
        assert h.dtype == snap.dtype
        prod = h.double() @ snap.head_wt.double().t() + snap.head_bf.double()      # brl_macro_ext.head_h's product
    return {"heads": (full.double(), True), "heads(raw)": (raw.double(), True), "head_parts": (lg.double(), False),
            "hidden + head_h": (prod, False)}


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("model", ["DeepMind", "DeepMind_6"])
def test_16_bit_snapshot_adds_every_bias(env, model, dt, monkeypatch):
    """A 16-bit InferenceSnapshot with a library handle (hidden layers on brl_linear_act, `body_nk`) at 1000 rows, consumed in its four
    forms — `heads`, `heads(raw=True)`, `head_parts` summed in the step kernel's order plus `head_bf`, and `hidden` times `head_wt`
    plus `head_bf` — against forward16_ref within 2 x the library chain's error (+ one ulp of the dtype for the two forms that were
    stored in 16 bits: `heads` is `heads(raw=True).float()`, asserted).  Then `refresh` (`_refresh16`) after a second perturbation:
    the same addresses, the new reference within the bound, the old one 8 bounds away — in all four forms and through the torch
    fallback that rebuilds the transposed weights on demand (`_body_stale`, reached with a strided input).
    Measured on the MI355X, 4- / 6-layer network, as built -> after the refresh.  Library chain against forward16_ref: bf16 6.2e-4 /
    7.1e-4 -> 1.0e-3 / 9.2e-4, fp16 7.3e-5 / 1.0e-4 -> 1.2e-4 / 1.7e-4; the bounds are twice that (bf16 1.2e-3 .. 2.0e-3, fp16 1.5e-4
    .. 3.4e-4), one ulp at the largest output is 2.0e-3 (bf16) and 2.4e-4 (fp16).  `head_parts` and `hidden` x `head_wt` have exactly
    the library chain's error (brl_linear_act rounds every activation as the library does; what is left is the fp32 head product);
    the stored forms are 4.2e-4 .. 7.5e-4 (bf16) and 5.8e-5 .. 1.5e-4 (fp16) beyond their rounding.  The smallest bias-slot effect
    is 0.069 / 0.030 as built (0.115 / 0.066 refreshed) against 8 x (bound + ulp) of at most 0.032 / 0.027."""
    from brl_amd.models import InferenceSnapshot
    monkeypatch.delenv("BRL_LINEAR16", raising=False)
    monkeypatch.delenv("BRL_HEAD_PARTS", raising=False)
    dtype = DT[dt]
    n = 1000
    net, obs = _net(model), _obs(n)
    snap = InferenceSnapshot.make(net, dtype, env)
    assert snap.body_nk is not None and snap.lin is None and snap._input(obs).dtype == dtype
    for step in ("built", "refreshed"):
        ref16 = forward16_ref(net, obs, dtype)
        e_lib, bound, ulp = _bound16(net, obs, dtype, ref16)
        sens = assert_sees_bias_slots(net, obs, bound + ulp)
        print(f"{model} {dt} {step}: library chain {e_lib:.2e} -> bound {bound:.2e} (+ ulp {ulp:.2e} where stored); smallest "
              f"bias-slot effect {sens:.3f}")
        forms = _four_forms(snap, obs)
        if step == "refreshed":      # ... and torch's chain on the transposed copies, rebuilt from body_nk on demand
            assert snap._body_stale
            wide = torch.zeros((n, 512), dtype=dtype, device="cuda")
            wide[:, :480] = obs.to(dtype)
            with torch.no_grad():
                forms["torch fallback"] = (snap.heads(None, x=wide[:, :480]).double(), True)
            assert not snap._body_stale
        for name, (out, stored) in forms.items():
            ex = _excess(out, ref16, _ulp(ref16, dtype) if stored else 0.0)
            print(f"    {name}: error {_err(out, ref16):.2e}, beyond its rounding {ex:.2e}")
            assert ex < bound, (name, ex, bound)
            if step == "refreshed":
                assert _err(out, old) >= 8 * (bound + ulp), name
        if step == "built":
            old, before = ref16, _addresses(snap)
            perturbed(net, REFRESH_SEED)
            snap.refresh(net)
            assert _addresses(snap) == before


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_16_bit_snapshot_on_the_library_gemm_adds_every_bias(env, dt, monkeypatch):
    """BRL_LINEAR16=0: the 16-bit snapshot's hidden layers on torch's addmm + relu_ (no `body_nk`): `heads`, `hidden` times
    `head_wt` plus `head_bf`, and the plain `refresh` of a 16-bit snapshot, as above"""
    from brl_amd.models import InferenceSnapshot
    monkeypatch.setenv("BRL_LINEAR16", "0")
    dtype = DT[dt]
    net, obs = _net("DeepMind"), _obs(1000)
    snap = InferenceSnapshot.make(net, dtype, env)
    assert snap.body_nk is None and snap.head_parts(obs) is None
    old = None
    for step in ("built", "refreshed"):
        ref16 = forward16_ref(net, obs, dtype)
        e_lib, bound, ulp = _bound16(net, obs, dtype, ref16)
        assert_sees_bias_slots(net, obs, bound + ulp)
        with torch.no_grad():
            out = snap.heads(obs)
        ex = _excess(out, ref16, _ulp(ref16, dtype))
        eh = _err(_head_h_form(snap, obs), ref16)         # (head_bf: read by the step kernel only, brl_macro_ext.head_h)
        print(f"{dt} {step}: library chain {e_lib:.2e}, snapshot {_err(out, ref16):.2e}, beyond its rounding {ex:.2e} of {bound:.2e}; "
              f"hidden + head_h {eh:.2e}")
        assert ex < bound and eh < bound
        if old is not None:
            assert _err(out, old) >= 8 * (bound + ulp)
        else:
            old, before = ref16, _addresses(snap)
            perturbed(net, REFRESH_SEED)
            snap.refresh(net)
            assert _addresses(snap) == before


# ---------------------------------------------------------------------------------------------------------------
# c: the policy rollout's recorded columns
# ---------------------------------------------------------------------------------------------------------------
ROLLOUTS = {
    "fp32_eager": (None, 512, False, {}, {}),
    "fp32_graph": (None, 512, True, {}, {}),
    "fp32_graph_6": (None, 512, True, {}, {}),                   # DeepMind_6
    "fp32_planes": (None, 4096, True, {}, {}),
    "fp32_peaked": (None, 512, True, {}, {}),                    # actor head weights x 8
    "bf16": ("bf16", 1024, True, {}, {}),
    "bf16_no_fused_heads": ("bf16", 1024, True, {"fuse_heads": False}, {}),
    "bf16_head_h": ("bf16", 1024, True, {}, {"BRL_HEAD_PARTS": "0"}),
    "bf16_library_gemm": ("bf16", 1024, True, {}, {"BRL_LINEAR16": "0"}),   # no body_nk: heads from the stored layer, plain refresh
    "fp16": ("fp16", 1024, True, {}, {}),
}


def _log_prob64(logits, mask, action):
    lg = torch.where(mask, logits, torch.full_like(logits, float("-inf")))
    lsm = lg - torch.logsumexp(lg, 1, keepdim=True)
    return lsm.gather(1, action.long()[:, None])[:, 0]


@pytest.mark.parametrize("case", list(ROLLOUTS))
def test_rollout_records_value_and_log_prob_of_the_current_networks(env, case, monkeypatch):
    """make_roll_out, T = 3, two calls; between them the actor is perturbed again in place and ANOTHER opponent module is passed.
    After each call: traj.value against the value column of the actor's reference on traj.obs, traj.log_prob against the masked
    log-softmax of the reference logits at the recorded action, and — white box, the opponent's outputs are otherwise seen only
    through sampled calls — roll.engine.snap_opp.heads(traj.obs[0]) against the CURRENT opponent's reference (and 8 bounds away
    from the previous opponent's).  Bounds: the logits bound of the snapshot tests for value (fp32: 2e-4 max(1, max|ref|); 16-bit:
    2 x the library chain's error on these observations, + one ulp where the step kernel is handed 16-bit outputs), twice that for
    log_prob — a log-sum-exp moves by at most the largest logit error, the selected logit by as much again.  Each route is asserted:
    eager / captured, bf16 observations on the planes path, heads from partial products, from the stored layer (BRL_HEAD_PARTS=0),
    from the raw 16-bit matrix (fuse_heads=False), the hidden layers on the library's GEMM (BRL_LINEAR16=0).
    Measured on the MI355X, first -> second call.  fp32: value within 1.2e-7 .. 2.5e-7 and log_prob within 5.1e-7 .. 2.3e-6 of bounds of
    2e-4 .. 1.7e-3.  bf16: library chain 4.2e-4 -> 9.7e-4 on the recorded observations, so value bounds of 8.4e-4 -> 1.9e-3 (errors
    3.3e-4 -> 4.2e-4) and log_prob bounds of 1.7e-3 -> 3.9e-3 (errors 1.3e-4 -> 4.6e-4; with fuse_heads=False 5.6e-3 -> 7.8e-3 and
    8.7e-4 -> 9.9e-4).  fp16: library chain 7.0e-5 -> 1.1e-4, value errors 6.2e-5 -> 7.9e-5, log_prob 5.2e-5 -> 5.3e-5.  The smallest
    bias-slot effect on the recorded observations is 0.069 -> 0.113 (six layers: 0.029 -> 0.058)."""
    import brl_amd
    from brl_amd.models import make_forward_pass
    dt, n, graph, over, envvars = ROLLOUTS[case]
    for k in ("BRL_HEAD_PARTS", "BRL_LINEAR16", "BRL_INFERENCE_PLANES", "BRL_TABLES_PER_WAVE", "BRL_INFERENCE_GEMM"):
        monkeypatch.delenv(k, raising=False)
    for k, v in envvars.items():
        monkeypatch.setenv(k, v)
    dtype = DT.get(dt)
    model = "DeepMind_6" if case == "fp32_graph_6" else "DeepMind"
    T = 3
    fp = make_forward_pass("relu", model)
    actor = _net(model)
    if case == "fp32_peaked":
        with torch.no_grad():
            actor.actor.weight.mul_(8.0)
    opps = [_net(model, seed=31, init=12), _net(model, seed=34, init=13)]
    cfg = dict(reward_scale=7600, game_mode="competitive", actor_illegal_action_mask=True, num_steps=T, graph_rollout=graph,
               inference_dtype=dt, **over)
    roll = brl_amd.make_roll_out(cfg, env, fp, fp)
    st = env.init(77, num_envs=n)
    rs = (actor, None, st, st.observation, 0, 0)

    def reference(net, obs):
        """-> (reference [rows, 39], logits / value bound, the ulp allowance of 16-bit stored outputs at max|ref|, its elementwise form)"""
        if dtype is None:
            ref = forward64(net, obs)
            return ref, _tol32(ref), 0.0, 0.0
        ref = forward16_ref(net, obs, dtype)
        e_lib, bound, ulp = _bound16(net, obs, dtype, ref)
        print(f"{case}: library chain {e_lib:.2e} -> bound {bound:.2e}, ulp {ulp:.2e}")
        return ref, bound, ulp, _ulp(ref, dtype)

    prev_opp_ref = None
    for call in range(2):
        if call == 1:
            perturbed(actor, REFRESH_SEED)
        rs, traj = roll(rs, opps[call])
        torch.cuda.synchronize()
        eng = roll.engine
        # ---- the route
        assert bool(eng.static) == graph and (not graph or eng.graphs), getattr(eng, "graph_error", None)
        if dtype is None:
            assert eng.xin.dtype == (torch.bfloat16 if n >= 4096 else torch.float32)
            assert (eng.snap_actor.wp is not None) and eng.snap_actor.planes_for(n) == (n >= 4096)
        else:
            own16 = case != "bf16_library_gemm"
            assert (eng.snap_actor.body_nk is not None) == own16 and (eng.snap_opp.body_nk is not None) == own16
            fused = eng._fused_heads(False)
            assert (fused is None) == (case == "bf16_no_fused_heads")
            if fused is not None:
                assert (fused.head_parts(traj.obs[0]) is None) == (case in ("bf16_head_h", "bf16_library_gemm"))
        stored16 = case == "bf16_no_fused_heads"           # the step kernel reads the GEMM's 16-bit logits and value (in_fmt)
        # ---- the recorded columns
        obs = traj.obs.reshape(T * n, 480)
        ref, bound, ulp, ulp_el = reference(actor, obs)
        scalar = bound + (ulp if stored16 else 0.0)
        sens = assert_sees_bias_slots(actor, obs, 2 * scalar)
        value, logp = traj.value.reshape(-1).double(), traj.log_prob.reshape(-1).double()
        mask, action = traj.legal_action_mask.reshape(T * n, 38), traj.action.reshape(-1)
        assert bool(mask.gather(1, action.long()[:, None]).all())
        want_lp = _log_prob64(ref[:, :38], mask, action)
        ev = _excess(value, ref[:, 38], ulp_el[:, 38] if stored16 else 0.0)
        elp = float((logp - want_lp).abs().max())
        print(f"{case} call {call}: max|ref| {float(ref.abs().max()):.3f}, value beyond its rounding {ev:.2e} of {bound:.2e}, log_prob "
              f"{elp:.2e} of {2 * scalar:.2e}; smallest bias-slot effect {sens:.3f}")
        assert ev < bound and elp < 2 * scalar
        # ---- the opponent's snapshot
        o0 = traj.obs[0]
        oref, obound, oulp, oulp_el = reference(opps[call], o0)
        assert_sees_bias_slots(opps[call], o0, obound + oulp)
        with torch.no_grad():
            oout = eng.snap_opp.heads(o0)
        eo = _excess(oout, oref, oulp_el)                 # (a 16-bit snapshot's `heads` is the 16-bit GEMM's matrix)
        print(f"{case} call {call}: opponent snapshot beyond its rounding {eo:.2e} of {obound:.2e}")
        assert eo < obound
        if prev_opp_ref is not None:
            assert _err(oout, forward64(prev_opp_ref, o0)) >= 8 * (obound + oulp)
        prev_opp_ref = copy64(opps[call])


# ---------------------------------------------------------------------------------------------------------------
# d / e: brl_mlp_forward_rows and brl_league_forward from raw arrays
# ---------------------------------------------------------------------------------------------------------------
HE = 6 ** 0.5


def _raw_arrays(hidden, layers, act, gen, gain=1.0):
    """a network as plain fp32 tensors: weights U(-1, 1) / sqrt(k) (the hidden layers' x `gain`), every bias its own N(0, 0.3) draw;
    critic_b 4 bytes off a 16-byte boundary, everything else 16-byte aligned -> (tests/nets network over the tensors, its
    brl_mlp_ref).  gain: U(-1, 1) / sqrt(k) has variance 1 / 3k — behind a ReLU every layer shrinks what enters it to 0.41 of it,
    and through eight layers a dropped layer-0 bias moves the outputs by 7e-4, 3.5 x the bound: invisible by the 8 x rule.  The
    eight-layer networks therefore draw their hidden weights from U(-1, 1) sqrt(6 / k) (variance 2 / k: a ReLU layer keeps the
    scale), where the smallest effect of a slot is 0.05 or more."""
    from brl_amd import _capi
    u = lambda o, k, g=1.0: ((torch.rand((o, k), device="cuda", generator=gen) * 2 - 1) * (g / k ** 0.5)).contiguous()   # noqa: E731
    nb = lambda o: (torch.randn(o, device="cuda", generator=gen) * 0.3).contiguous()                                       # noqa: E731
    body = [(u(hidden, 480 if i == 0 else hidden, gain), nb(hidden)) for i in range(layers)]
    actor = (u(38, hidden), nb(38))
    pad = torch.zeros(8, device="cuda")
    pad[1:2] = nb(1)
    critic = (u(1, hidden), pad[1:2])
    assert critic[1].data_ptr() % 16 == 4 and actor[0].data_ptr() % 16 == 0 and critic[0].data_ptr() % 16 == 0
    assert all(w.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0 for w, b in body)
    net = raw_net(body, actor, critic, torch.relu if act == "relu" else torch.tanh)
    r = _capi.MlpRef()
    r.nlayers, r.act, r.in_features, r.hidden = layers, 0 if act == "relu" else 1, 480, hidden
    for i, (w, b) in enumerate(body):
        r.w[i], r.b[i] = w.data_ptr(), b.data_ptr()
    r.actor_w, r.actor_b, r.critic_w, r.critic_b = actor[0].data_ptr(), actor[1].data_ptr(), critic[0].data_ptr(), critic[1].data_ptr()
    return net, r


def _forward_rows(r, obs, rows, m, out):
    from brl_amd import _capi
    hidden = int(r.hidden)
    scratch = torch.empty(m * (480 + 2 * hidden), device="cuda")
    _capi.check(_capi.lib().brl_mlp_forward_rows(0, C.byref(r), obs.data_ptr(), None if rows is None else rows.data_ptr(), m,
                                                 scratch.data_ptr(), scratch.numel(), out.data_ptr(), out.stride(0), _capi.stream()))
    torch.cuda.synchronize()


@pytest.mark.parametrize("ldo", [39, 40])
@pytest.mark.parametrize("permuted", [False, True])
@pytest.mark.parametrize("hidden,layers,act,m,gain", [(64, 1, "relu", 1, 1.0), (260, 3, "tanh", 5, 1.0), (200, 2, "relu", 130, 1.0),
                                                      (1024, 8, "relu", 63, HE)])
def test_forward_rows_from_raw_arrays(hidden, layers, act, m, gain, permuted, ldo):
    """brl_mlp_forward_rows on a brl_mlp_ref filled from plain tensors — the narrowest network and a single row, a width that is no
    multiple of the 32- and 64-column tiles, more rows than one 64-row tile, and the widest and deepest network the entry point takes —
    with rows = NULL (the first m boards) and with a permutation, row stride 39 and 40: against float64 within 2e-4 max(1,
    max|ref|); unselected rows and column 39 keep what they held."""
    gen = torch.Generator(device="cuda").manual_seed(1000 * hidden + 10 * layers + m)
    net, r = _raw_arrays(hidden, layers, act, gen, gain)
    n = m + 37
    obs = torch.rand((n, 480), device="cuda", generator=gen) < 0.12
    rows = torch.randperm(n, device="cuda", generator=gen)[:m].contiguous() if permuted else None
    sel = rows if permuted else torch.arange(m, device="cuda")
    ref = forward64(net, obs[sel])
    tol = _tol32(ref)
    sens = assert_sees_bias_slots(net, obs[sel], tol)
    out = torch.full((n, ldo), 123.0, device="cuda")
    _forward_rows(r, obs, rows, m, out)
    e = _err(out[sel][:, :39], ref)
    print(f"hidden {hidden} x {layers} {act} m={m}: error {e:.2e} of {tol:.2e}; smallest bias-slot effect {sens:.3f}")
    assert e < tol
    untouched = torch.ones(n, dtype=torch.bool, device="cuda")
    untouched[sel] = False
    assert bool((out[untouched] == 123.0).all()) and (ldo == 39 or bool((out[:, 39] == 123.0).all()))


@pytest.mark.parametrize("model", ["DeepMind", "DeepMind_6"])
def test_forward_rows_by_reference_of_a_module(model):
    """evaluation._Forward._by_reference — the brl_mlp_ref the evaluators and the league fill from a module — names every layer's own
    weight and bias and both heads, and brl_mlp_forward_rows on it equals the module's float64 forward on a perturbed network"""
    from brl_amd.evaluation import _Forward
    net = _net(model)
    r = _Forward._by_reference(net)
    assert r is not None and int(r.nlayers) == len(net.body) and int(r.hidden) == 1024 and int(r.act) == 0
    for i, lin in enumerate(net.body):
        assert (r.w[i], r.b[i]) == (lin.weight.data_ptr(), lin.bias.data_ptr()), i
    assert all(r.w[i] is None and r.b[i] is None for i in range(len(net.body), 8))
    assert (r.actor_w, r.actor_b, r.critic_w, r.critic_b) == (net.actor.weight.data_ptr(), net.actor.bias.data_ptr(),
                                                             net.critic.weight.data_ptr(), net.critic.bias.data_ptr())
    n, m = 200, 130
    obs = _obs(n)
    rows = torch.randperm(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))[:m].contiguous()
    ref = forward64(net, obs[rows])
    tol = _tol32(ref)
    assert_sees_bias_slots(net, obs[rows], tol)
    out = torch.full((n, 40), 123.0, device="cuda")
    _forward_rows(r, obs, rows, m, out)
    assert _err(out[rows][:, :39], ref) < tol


@pytest.mark.parametrize("sizes", [[0, 1, 63, 64, 65, 7], [64, 7, 0, 65, 1, 63], [65, 63, 1, 7, 64, 0]])
@pytest.mark.parametrize("hidden,layers,act,gain", [(260, 3, "tanh", 1.0), (1024, 8, "relu", HE)])
def test_league_forward_from_raw_arrays(hidden, layers, act, gain, sizes):
    """brl_league_forward on three networks given as plain tensors, every bias of every network its own draw, six groups (group g
    plays network g % 3) with an empty group first, in the middle or last: each group's rows bit for bit what brl_mlp_forward_rows
    writes for that group's network, and within 2e-4 max(1, max|ref|) of that network's float64 forward; rows that are not routed
    and column 39 untouched."""
    from brl_amd import _capi
    from brl_amd.league import _net_record
    gen = torch.Generator(device="cuda").manual_seed(hidden + sizes[0])
    nets = [_raw_arrays(hidden, layers, act, gen, gain) for _ in range(3)]
    G, R = len(sizes), sum(sizes)
    nboards = R + 50
    obs = torch.rand((nboards, 480), device="cuda", generator=gen) < 0.12
    rows = torch.randperm(nboards, device="cuda", generator=gen)[:R].contiguous()
    first = np.concatenate([[0], np.cumsum(sizes)])
    gf = torch.tensor(first, dtype=torch.int32, device="cuda")
    table = torch.tensor([_net_record(nets[g % 3][1]) for g in range(G)], dtype=torch.int64, device="cuda")
    out = torch.full((nboards, 40), 123.0, device="cuda")
    scratch = torch.empty(R * (480 + 2 * hidden), device="cuda")
    _capi.check(_capi.lib().brl_league_forward(0, table.data_ptr(), G, layers, hidden, 0 if act == "relu" else 1, obs.data_ptr(),
                                               rows.data_ptr(), gf.data_ptr(), R, scratch.data_ptr(), scratch.numel(), out.data_ptr(), 40,
                                               _capi.stream()))
    torch.cuda.synchronize()
    want = torch.full((nboards, 40), 123.0, device="cuda")
    for g in range(G):
        if sizes[g] == 0:
            continue
        net, r = nets[g % 3]
        idx = rows[int(first[g]):int(first[g + 1])].contiguous()
        _forward_rows(r, obs, idx, sizes[g], want)
        ref = forward64(net, obs[idx])
        tol = _tol32(ref)
        assert_sees_bias_slots(net, obs[idx], tol)
        other = forward64(nets[(g + 1) % 3][0], obs[idx])            # (another network's parameters are far away)
        assert _err(out[idx][:, :39], ref) < tol and float((other - ref).abs().max()) >= 8 * tol, (g, sizes[g])
    assert torch.equal(out, want)
    untouched = torch.ones(nboards, dtype=torch.bool, device="cuda")
    untouched[rows] = False
    assert bool((out[untouched] == 123.0).all()) and bool((out[:, 39] == 123.0).all())
