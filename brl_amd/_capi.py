"""ctypes binding of include/brl_hip.h.  No torch types cross this boundary: raw device
pointers (tensor.data_ptr()) and the current HIP stream handle only."""
from __future__ import annotations

import ctypes as C
import os

import torch

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "lib", "libbrl_hip.so")

STATE_WORDS = 16
OBS_SIZE = 480
NUM_ACTIONS = 38

_vp = C.c_void_p


class Fields(C.Structure):
    _names = ["current_player", "terminated", "rewards", "step_count", "turn", "dealer", "vul_ns", "vul_ew",
              "shuffled_players", "last_bid", "last_bidder", "call_x", "call_xx", "pass_num",
              "first_denomination_ns", "first_denomination_ew", "hand", "tricks", "lut_idx", "board_ctr", "illegal"]
    _fields_ = [(n, _vp) for n in _names]


class TransitionPtrs(C.Structure):
    _names = ["done", "action", "value", "reward", "log_prob", "obs", "legal_action_mask"]
    _fields_ = [(n, _vp) for n in _names]


class TableInfoPtrs(C.Structure):
    _names = ["terminated", "rewards", "last_bid", "last_bidder", "call_x", "call_xx"]
    _fields_ = [(n, _vp) for n in _names]


class MacroExt(C.Structure):
    _fields_ = [("first", C.c_int32), ("last", C.c_int32), ("value_in", _vp), ("value_stride", C.c_int64), ("value_out", _vp),
                ("done_out", _vp), ("reward_out", _vp), ("actor", _vp), ("reward_scale", C.c_float), ("obs_fmt", C.c_int32),
                ("terminated_count", _vp), ("obs_cast", _vp), ("in_fmt", C.c_int32), ("reserved", C.c_int32),
                ("head_h", _vp), ("head_ldh", C.c_int64), ("head_w", _vp), ("head_b", _vp), ("head_hidden", C.c_int32),
                ("head_fmt", C.c_int32), ("head_part", _vp), ("head_part_stride", C.c_int64), ("head_part_ld", C.c_int32),
                ("head_nparts", C.c_int32)]


class EvalStatsPtrs(C.Structure):
    _names = ["illegal_prob_sum", "step_count", "pass_count", "bid_count"]
    _fields_ = [(n, _vp) for n in _names]


class MlpRef(C.Structure):
    """brl_mlp_ref: a "DeepMind" network by reference (pointers into the module's own parameters)"""
    _fields_ = [("nlayers", C.c_int32), ("act", C.c_int32), ("in_features", C.c_int64), ("hidden", C.c_int64),
                ("w", _vp * 8), ("b", _vp * 8), ("actor_w", _vp), ("actor_b", _vp), ("critic_w", _vp), ("critic_b", _vp)]


class ShardGeom(C.Structure):
    """brl_shard_geom: the bucketed flat buffers of the multi-rank PPO step (offsets / slice lengths in floats)"""
    _fields_ = [("nbuckets", C.c_int32), ("world", C.c_int32), ("nsub", C.c_int32), ("reserved", C.c_int32),
                ("off", C.c_int64 * 12), ("len", C.c_int64 * 12)]


class FairNet(C.Structure):
    """brl_fair_net: the FAIR network's parameters (nn.Linear layout), device pointers"""
    _fields_ = [("w", _vp * 11), ("b", _vp * 11), ("head_w", _vp), ("head_b", _vp)]


class FairWork(C.Structure):
    """brl_fair_work: what brl_fair_chain leaves for the weight-gradient products and brl_bias_finalize_rows"""
    _names = ("inp", "dzs", "gates", "cat6", "x4", "dz0", "dz6", "dheads", "tiles", "partials", "gram_partials")
    _fields_ = [(n, _vp) for n in _names]


class LeagueNet(C.Structure):
    """brl_league_net (include/brl_league.h): one "DeepMind" fp32 network by reference, 20 device pointers"""
    _fields_ = [("w", _vp * 8), ("b", _vp * 8), ("actor_w", _vp), ("actor_b", _vp), ("critic_w", _vp), ("critic_b", _vp)]


EVAL_COUNTS = 231  # BRL_EVAL_COUNTS


class BrlError(RuntimeError):
    pass


def _signatures() -> dict:
    """the argtypes of every `int brl_*(` entry point, keyed by the header of include/ that declares it (tests/test_capi_cpu.py holds
    every prototype of every header against this table)"""
    i64, i32, u32, u64, f32 = C.c_int64, C.c_int, C.c_uint32, C.c_uint64, C.c_float
    return {
        "brl_hip.h": {
            "brl_version": [],
            "brl_create": [i32, _vp, _vp, i64, C.POINTER(_vp)],
            "brl_set_lut": [_vp, _vp, _vp, i64],
            "brl_destroy": [_vp],
            "brl_set_rng": [_vp, u64, u64],
            "brl_init_random": [_vp, _vp, i64, u32, _vp],
            "brl_init_from_deals": [_vp, _vp, i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
            "brl_step": [_vp, _vp, _vp, i64, _vp, i32, _vp, _vp, _vp, _vp, _vp, _vp],
            "brl_observe": [_vp, _vp, i64, _vp, _vp, _vp, _vp],
            "brl_get_fields": [_vp, _vp, i64, C.POINTER(Fields), _vp],
            "brl_rollout_random": [_vp, _vp, i64, i32, i32, u32, f32, C.POINTER(TransitionPtrs), _vp, _vp, _vp, _vp],
            "brl_rollout_random_gae": [_vp, _vp, i64, i32, u32, f32, C.POINTER(TransitionPtrs), _vp, _vp, _vp, _vp, f32, f32, _vp, _vp,
                                       _vp],
            "brl_policy_step": [_vp, _vp, _vp, i64, _vp, i32, u32, i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
            "brl_policy_step_at": [_vp, _vp, _vp, i64, _vp, i64, i32, _vp, u32, i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
            "brl_policy_step_ex": [_vp, _vp, _vp, i64, _vp, i64, i32, _vp, u32, i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                   C.POINTER(MacroExt), _vp],
            "brl_obs_cast": [_vp, _vp, i64, _vp, i32, _vp],
            "brl_obs_cast_rows": [_vp, _vp, _vp, i64, _vp, i32, _vp],
            "brl_live_index": [_vp, _vp, i64, _vp, _vp, i64, _vp],
            "brl_linear_act_heads": [_vp, _vp, i64, _vp, i64, _vp, _vp, i64, i64, i32, i32, i32, i32, _vp, i64, i32, _vp, i64, i64, _vp],
            "brl_linear_act": [_vp, _vp, i64, _vp, i64, _vp, _vp, i64, i64, i32, i32, i32, i32, _vp],
            "brl_gae": [_vp, _vp, _vp, _vp, _vp, f32, f32, i32, i64, _vp, _vp, _vp],
            "brl_imp_reward": [_vp, _vp, _vp, _vp, i64, _vp],
            "brl_duplicate_step": [_vp, _vp, _vp, i64, _vp, C.POINTER(TableInfoPtrs), C.POINTER(TableInfoPtrs),
                                   _vp, _vp, _vp, _vp, _vp, _vp],
            "brl_eval_step": [_vp, _vp, _vp, i64, _vp, i64, _vp, i64, C.POINTER(TableInfoPtrs), C.POINTER(TableInfoPtrs),
                              C.POINTER(EvalStatsPtrs), i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
            "brl_eval_step_team": [_vp, _vp, _vp, i64, _vp, i64, i32, C.POINTER(TableInfoPtrs), C.POINTER(TableInfoPtrs),
                                   C.POINTER(EvalStatsPtrs), i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
            "brl_eval_reduce": [_vp, i64, C.POINTER(TableInfoPtrs), C.POINTER(TableInfoPtrs), _vp, _vp, _vp, _vp],
            "brl_ppo_loss": [i32, _vp, i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, i64, f32, f32, f32, i32, i32, _vp, _vp, _vp, _vp, _vp],
            "brl_ppo_stats": [i32, _vp, i64, _vp, f32, f32, _vp, _vp],
            "brl_ppo_heads_loss_split": [i32, _vp, i64, _vp, _vp, i64, _vp, _vp, _vp, _vp, _vp, _vp, i64, f32, f32, f32, i32, i32, i32, _vp, _vp, _vp, _vp, _vp, i32, _vp],
            "brl_ppo_heads_bwd": [i32, _vp, _vp, i64, _vp, i64, i64, i32, i32, _vp, _vp, _vp, _vp, _vp, _vp, i64, _vp, _vp, _vp, _vp],
            "brl_ppo_stats_rows": [i32, _vp, _vp, i64, i64, f32, f32, f32, _vp, _vp],
            "brl_mb_gather_bind": [i32, C.POINTER(TransitionPtrs), _vp, _vp, _vp, _vp, i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, i64, _vp, _vp],
            "brl_adam_clip_fin_gather": [i32, _vp, _vp, _vp, _vp, i64, _vp, f32, _vp, f32, f32, f32, f32, _vp, i64, _vp, _vp, _vp, i64,
                                         i32, _vp, _vp, _vp, _vp, _vp],
            "brl_mb_gather_dev": [i32, _vp, i64, _vp],
            "brl_ppo_stats_gram": [i32, _vp, i64, i64, _vp, i64, f32, f32, f32, _vp, _vp, _vp, _vp],
            "brl_ppo_illegal_grad": [i32, _vp, _vp, _vp, f32, i64, _vp, _vp],
            "brl_act_bwd_colsum": [i32, _vp, _vp, i64, i64, i64, i32, _vp, _vp],
            "brl_act_bwd_colsum_heads_dw": [i32, _vp, _vp, i64, i64, i64, i32, _vp, _vp, _vp, i64, i64, i64, i32, _vp, _vp, _vp, _vp, i64,
                                            _vp, _vp, _vp, _vp],
            "brl_bias_finalize_ex": [i32, i32, _vp, _vp, _vp, _vp, _vp],
            "brl_bias_finalize_rows": [i32, i32, _vp, _vp, _vp, _vp, i32, _vp, _vp],
            "brl_fair_forward": [i32, C.POINTER(FairNet), _vp, i64, i32, _vp, _vp, _vp],
            "brl_mlp_gemm_group": [i32, i32, i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
            "brl_fair_chain": [i32, C.POINTER(FairNet), _vp, _vp, _vp, _vp, _vp, _vp, _vp, i64, f32, f32, f32, i32, i32, i32, i32,
                               C.POINTER(FairWork), _vp],
            "brl_mlp_gemm": [i32, i32, i32, _vp, i64, _vp, i64, _vp, i64, i64, i64, i64, i32, _vp, _vp, i64, _vp, _vp, _vp],
            "brl_mlp_gemm_x3_workspace": [i64, i64, i64, _vp],
            "brl_mlp_gemm_x3_group": [i32, i32, i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
            "brl_split_planes": [i32, _vp, i64, _vp, i64, _vp],
            "brl_linear_x3p": [i32, _vp, i32, i64, i64, _vp, i64, i64, _vp, i32, _vp, i64, _vp, i64, i64, i64, i64, i64, _vp],
            "brl_mlp_gemm_x3": [i32, i32, i32, _vp, i64, _vp, i64, _vp, i64, i64, i64, i64, i32, _vp, _vp, i64, _vp, _vp, i64, _vp],
            "brl_mlp_forward_rows": [i32, C.POINTER(MlpRef), _vp, _vp, i64, _vp, i64, _vp, i64, _vp],
            "brl_adam_shard_norm": [i32, _vp, C.POINTER(ShardGeom), i32, i32, f32, _vp, _vp, _vp, _vp],
            "brl_adam_shard_apply": [i32, _vp, _vp, _vp, _vp, C.POINTER(ShardGeom), i32, i32, _vp, _vp, f32, _vp, f32, f32, f32, f32, f32, _vp,
                                     _vp, i64, _vp],
            "brl_mlp_gemm_dh_heads_dw": [i32, _vp, i64, _vp, i64, _vp, i64, i64, i64, i64, i32, _vp, i64, _vp, _vp, _vp, i64, i64, i64, i32,
                                         _vp, _vp, _vp, _vp, i64, _vp, _vp, _vp, _vp],
        },
        "brl_sl.h": {   # the supervised pre-trainer's entry points
            "brl_sl_sample": [i32, _vp, _vp, i64, u64, i64, _vp, _vp, _vp],
            "brl_sl_replay": [i32, _vp, _vp, _vp, i64, _vp, _vp, i64, _vp, _vp, _vp, _vp],
            "brl_sl_loss": [i32, _vp, i64, _vp, _vp, i64, f32, _vp, _vp, _vp, i64, _vp],
        },
        "brl_league.h": {   # the batched league evaluation
            "brl_league_route": [i32, _vp, _vp, i32, i64, _vp, _vp, i64, i64, _vp, _vp, _vp, _vp],
            "brl_league_forward": [i32, _vp, i64, i32, i64, i32, _vp, _vp, _vp, i64, _vp, i64, _vp, i64, _vp],
        },
        "brl_boards.h": {   # the board records
            "brl_board_records": [i32, _vp, i64, _vp, _vp],
            "brl_board_imp": [i32, _vp, _vp, i64, _vp, _vp],
            "brl_board_keep_a": [i32, _vp, _vp, _vp, _vp, _vp, _vp, i64, _vp],
        },
        "brl_book.h": {   # the bidding-system book
            "brl_book_samples": [i32, _vp, i64, _vp, i32, i32, _vp, _vp, _vp],
            "brl_book_reduce": [i32, _vp, _vp, i64, _vp, i64, _vp, _vp],
        },
        "brl_par.h": {   # the double-dummy par
            "brl_par": [i32, _vp, _vp, _vp, i64, _vp, _vp],
            "brl_par_imp": [i32, _vp, _vp, i64, i32, _vp, _vp],
        },
        "brl_review.h": {   # the call review
            "brl_review_expand": [i32, _vp, _vp, i64, i32, _vp, i64, i64, _vp, _vp, _vp],
            "brl_review_reduce": [i32, _vp, _vp, i64, _vp, i64, _vp, _vp, _vp],
        },
        "brl_belief.h": {   # the hand beliefs
            "brl_belief_deal": [i32, _vp, i64, i64, u64, i64, _vp, _vp, _vp],
            "brl_belief_logp": [i32, _vp, i64, _vp, i64, _vp, i64, _vp, _vp, i64, _vp, _vp, _vp],
            "brl_belief_reduce": [i32, _vp, i64, i64, _vp, _vp, _vp, _vp, _vp],
        },
        "brl_belief_smc.h": {   # the beliefs' resample-move stages
            "brl_belief_resample": [i32, _vp, i64, _vp, i64, i64, u64, i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
            "brl_belief_propose": [i32, _vp, _vp, i64, _vp, i64, i64, u64, i64, i64, _vp, _vp, _vp, _vp],
            "brl_belief_accept": [i32, _vp, i64, _vp, i64, i64, u64, i64, i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
        },
        "brl_compare.h": {   # the system diff
            "brl_compare_tables": [i32, _vp, i64, _vp, i64, _vp, _vp, _vp],
            "brl_compare_rows": [i32, _vp, i64, _vp, i64, i32, i32, _vp, i64, _vp, i64, _vp, _vp, _vp],
            "brl_compare_reduce": [i32, _vp, i64, _vp, i64, _vp, _vp, _vp],
        },
        "brl_crossplay.h": {   # cross-play's route
            "brl_xplay_route": [i32, _vp, _vp, i32, i64, _vp, _vp, i64, i64, _vp, _vp, _vp, _vp],
        },
        "brl_distill.h": {   # policy distillation's targets and loss head
            "brl_distill_targets": [i32, _vp, i64, i64, _vp, i64, i64, _vp, _vp, i64, i32, f32, _vp, _vp, _vp, _vp],
            "brl_distill_loss": [i32, _vp, i64, _vp, i64, _vp, _vp, _vp, _vp, i64, f32, f32, f32, _vp, _vp, _vp, _vp, _vp],
        },
        "brl_lines.h": {   # the auction lines' beam search
            "brl_lines_init": [i32, _vp, i64, i32, i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
            "brl_lines_expand": [i32, _vp, _vp, _vp, _vp, i64, i32, i32, _vp, i64, _vp, i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
            "brl_lines_finish": [i32, _vp, _vp, i64, _vp, _vp],
            "brl_lines_imp": [i32, _vp, _vp, _vp, _vp, _vp, _vp, i64, i32, _vp, _vp],
        },
        "brl_positions.h": {   # the position queries
            "brl_position_rows": [i32, _vp, i64, _vp, _vp, _vp, _vp, _vp, _vp],
            "brl_position_answers": [i32, _vp, i64, _vp, i64, _vp, _vp, i64, i32, _vp, _vp, _vp],
        },
    }


SIGNATURES = _signatures()
EXPORTS = ["brl_last_error", *SIGNATURES["brl_hip.h"]]   # every symbol of include/brl_hip.h (brl_last_error returns a string)

_lib = None


def lib() -> C.CDLL:
    """Loads libbrl_hip.so.  Fails loudly — there is no fallback path."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise BrlError(
            f"{LIB_PATH} is missing: the HIP extension has not been built. "
            "Run `python -m brl_amd.build` (needs hipcc, gfx950). brl_amd has no CPU fallback."
        )
    L = C.CDLL(LIB_PATH)
    L.brl_last_error.restype = C.c_char_p
    for sigs in SIGNATURES.values():
        for name, args in sigs.items():
            fn = getattr(L, name)
            fn.argtypes = args
            fn.restype = C.c_int
    _lib = L
    return L


def check(rc: int) -> None:
    if rc != 0:
        raise BrlError(f"libbrl_hip error {rc}: {lib().brl_last_error().decode()}")


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def device_index(t) -> int:
    """the device ordinal of a tensor (the current device for a device without an index)"""
    i = t.device.index
    return i if i is not None else torch.cuda.current_device()


def stream(index=None) -> int:
    """the current HIP stream's handle on device ``index`` (default: the current device), what every C-ABI call takes.
    torch.cuda.current_stream() costs ~9 us per call (device lookups, a Stream object): ~30 us of an evaluator's 75 us host
    iteration; the raw accessor is the same handle in ~0.3 us."""
    if index is None:
        index = torch.cuda.current_device()
    if _raw_stream is not None:
        return _raw_stream(index)
    return torch.cuda.current_stream(index).cuda_stream


def ptr(t):
    """Device pointer of a torch tensor (or None)."""
    if t is None:
        return None
    assert t.is_contiguous(), "brl_amd passes raw pointers: tensors must be contiguous"
    return t.data_ptr()
