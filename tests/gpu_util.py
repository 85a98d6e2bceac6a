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
