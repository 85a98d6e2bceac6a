"""Helpers shared by the -m gpu parity tests: GPU State <-> oracle state comparison."""
import os

import numpy as np
import torch

# oracle field -> brl_amd State attribute
FIELD_MAP = {
    "current_player": "current_player", "terminated": "terminated", "step_count": "_step_count", "turn": "_turn",
    "dealer": "_dealer", "vul_ns": "_vul_NS", "vul_ew": "_vul_EW", "last_bid": "_last_bid",
    "last_bidder": "_last_bidder", "call_x": "_call_x", "call_xx": "_call_xx", "pass_num": "_pass_num",
    "illegal": "_illegal", "lut_idx": "_lut_idx", "board_ctr": "_board_count",
    "shuffled_players": "_shuffled_players", "first_denomination_ns": "_first_denomination_NS",
    "first_denomination_ew": "_first_denomination_EW", "rewards": "rewards", "hand": "_hand", "tricks": "_dds_tricks",
    "legal_action_mask": "legal_action_mask", "observation": "observation",
}


def to_np(t):
    a = t.detach().cpu().numpy()
    return a.astype(np.uint8) if a.dtype == np.bool_ else a


def assert_state_equal(gpu_state, orc_state, fields=None, where=""):
    got = gpu_state.all_fields()
    torch.cuda.synchronize()
    for of, gf in FIELD_MAP.items():
        if fields is not None and of not in fields:
            continue
        g = to_np(got[gf])
        o = orc_state[of]
        g = g.astype(np.int64) if g.dtype.kind in "iub" else g
        o = o.astype(np.int64) if o.dtype.kind in "iub" else o
        if not np.array_equal(g, o):
            bad = np.nonzero((g != o).reshape(g.shape[0], -1).any(1))[0]
            e = int(bad[0])
            raise AssertionError(f"{where}: field {of} differs on {len(bad)} tables, first table {e}:\n gpu={g[e]}\n orc={o[e]}")


def _assert_log_info(got, want, names=None):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        g, w = to_np(g).astype(np.float64), np.asarray(w, np.float64)
        # counts / n in fp32 on both sides, sums of <= 8192 terms: 1e-6 absolute + 1e-5 relative
        assert g.shape == w.shape and np.allclose(g, w, rtol=1e-5, atol=1e-6), f"log_info[{i}]: {g} != {w}"


def random_legal_actions(rng, mask):
    """one uniformly random legal action per row of a [N,38] 0/1 mask"""
    m = mask.astype(np.float64)
    r = rng.random(m.shape) * m
    return r.argmax(axis=1).astype(np.int32)


def make_env(dds, k, ws=None, lut=None, **kwargs):
    """k: tables per wave of the per-step kernels; ws: "0" for the K-tables-per-wave fused rollout
    (k_rollout_random<K>), "ws" for the barrier-synchronised wave-specialised kernel (k_rollout_ws) on every shape,
    None for the library default (the flag-synchronised k_rollout_fs where it applies: substeps 1, T <= 40, n % 32 == 0;
    k_rollout_ws otherwise); kwargs: further arguments of BridgeBidding (env_offset)."""
    import brl_amd
    new = {"BRL_TABLES_PER_WAVE": str(k), "BRL_ROLLOUT_WS": "0" if ws == "0" else None,
           "BRL_ROLLOUT_FS": "0" if ws == "ws" else None}
    old = {key: os.environ.get(key) for key in new}
    for key, v in new.items():
        if v is None:
            os.environ.pop(key, None)
        else:
            os.environ[key] = v
    try:
        return brl_amd.BridgeBidding(lut=lut if lut is not None else (dds["keys"], dds["values"]), **kwargs)
    finally:
        for key, v in old.items():
            if v is None:
                os.environ.pop(key, None)
            else:
                os.environ[key] = v


def gemm_operands(layout, M, N, K, seed, device="cuda"):
    """the operands of one brl_mlp_gemm product, uniform in [-1, 1): A ([M, K], or [K, M] for BRL_GEMM_TN), B ([N, K] for
    BRL_GEMM_NT, else [K, N]), bias [N], gate [M, N] — drawn on `device` in that order from a generator seeded with `seed`"""
    g = torch.Generator(device=device).manual_seed(seed)
    r = lambda *sh: (torch.rand(sh, device=device, generator=g) * 2 - 1)  # noqa: E731
    akc, bkc = layout != 2, layout == 0
    A = r(M, K) if akc else r(K, M)
    Bm = r(N, K) if bkc else r(K, N)
    bias, gate = r(N), r(M, N)
    return A, Bm, bias, gate


def gemm_ref64(layout, epi, act, A, Bm, bias, gate):
    """the float64 product of those operands with brl_mlp_gemm's epilogue `epi` (1: bias + ReLU / tanh, 2: the activation
    derivative from `gate`; 0 and 3 leave the product as it is)"""
    a64 = A.double() if layout != 2 else A.double().t()
    b64 = Bm.double().t() if layout == 0 else Bm.double()
    ref = a64 @ b64
    if epi == 1:
        ref = ref + bias.double()
        ref = ref.clamp_min(0) if act == 0 else ref.tanh()
    if epi == 2:
        ref = ref * ((gate > 0).double() if act == 0 else (1 - gate.double() ** 2))
    return ref


def gemm_bound(ref, K):
    """max |brl_mlp_gemm - float64| allowed: fp32 k-ordered fma chains, 2e-4 * max|ref| at K = 1024"""
    return 2e-4 * max(1.0, float(ref.abs().max())) * (K / 1024 + 1) ** 0.5


def replay_policy_rollout(oracle, ref, traj, sub_actions, seed, reward_scale=7600.0, env_offset=0, detail=None):
    """Replays the recorded actions of a policy-in-the-loop rollout (sub-step 1: traj.action, sub-steps 2-4:
    sub_actions) through the oracle's auto_reset(step) and returns the Transition columns the reference's _env_step
    would have stored (src/roll_out.py:63-103, src/utils.py:69-128): pre-step obs / mask of the acting player (G4),
    done = OR of the four terminated flags (G2), reward = (r1+r2+r3+r4)[actor] / reward_scale (G1), boards replaced
    mid-macro-step (G3).  `ref` ends as the post-rollout state (rewards / terminated of the last macro-step).
    `detail`: a dict that receives, for every sub-step, the pre-step observation and mask of the player to act ("sub_obs"
    [T, 4, n, 480], "sub_mask" [T, 4, n, 38]) and, appended to detail["events"], the boards that sub-step finished, read off a copy
    stepped without the re-deal (tests/bidder_net.py: step_with_events, census); detail["t0"] numbers the macro-steps of a later call."""
    act0, sub = to_np(traj.action), to_np(sub_actions)
    T, n = act0.shape
    want = {"obs": np.zeros((T, n, 480), np.uint8), "legal_action_mask": np.zeros((T, n, 38), np.uint8),
            "done": np.zeros((T, n), np.uint8), "reward": np.zeros((T, n), np.float32)}
    if detail is not None:
        from tests.bidder_net import step_with_events
        detail["sub_obs"], detail["sub_mask"] = np.zeros((T, 4, n, 480), np.uint8), np.zeros((T, 4, n, 38), np.uint8)
        events, t0 = detail.setdefault("events", []), detail.get("t0", 0)
    count = 0
    for t in range(T):
        want["obs"][t] = ref["observation"]
        want["legal_action_mask"][t] = ref["legal_action_mask"]
        actor = ref["current_player"].copy()
        racc = np.zeros((n, 4), np.float32)
        term = np.zeros(n, np.int32)
        for k in range(4):
            a = act0[t] if k == 0 else sub[t, k - 1]
            if detail is None:
                oracle.step(ref, a, autoreset=True, seed=seed, env_offset=env_offset)
            else:
                detail["sub_obs"][t, k], detail["sub_mask"][t, k] = ref["observation"], ref["legal_action_mask"]
                step_with_events(oracle, ref, a, seed, env_offset, t0 + t, k, actor, events)
            racc += ref["rewards"]
            term |= ref["terminated"]
        want["done"][t] = term
        want["reward"][t] = racc[np.arange(n), actor] / np.float32(reward_scale)
        count += int(term.sum())
    ref["rewards"] = racc          # src/utils.py:126-128
    ref["terminated"] = term
    want["terminated_count"] = count
    return want
