"""k_rollout_fs's first slots: slot 0's rows come straight from the incoming table image (whose scalars the launch must
leave alone until its write-back), every later slot from the prep wave's commands.  One and two workgroups, launches of
1, 2 and 3 steps (where the logic wave is done while the first rows are still being stored), 9 and 40, each through
brl_rollout_random and brl_rollout_random_gae, two calls in a row so that the second starts from mid-auction tables — and,
where the launch is long enough, with a board ending (a deal) in each of its first three steps.  Byte for byte against the CPU oracle and against k_rollout_ws on the same input."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests.gpu_util import assert_state_equal, make_env, to_np

pytestmark = pytest.mark.gpu

GAMMA, LAM = 0.99, 0.9
COLUMNS = ("obs", "legal_action_mask", "action", "done", "value", "reward", "log_prob")
BIG_OFFSET = 2**32 + 5
SHAPES = [(n, T, 0) for n in (32, 64) for T in (1, 2, 3, 9, 40)] + [(64, 9, BIG_OFFSET)]


def _last_val(n, T):
    return np.random.default_rng(1000 * n + T).standard_normal(n).astype(np.float32)


def oracle_calls(oracle, n, T, env_offset, seed):
    """the oracle's two back-to-back rollouts: per call its columns, the state after it, advantages / targets"""
    ref = oracle.init_random(n, seed=seed, env_offset=env_offset)
    calls = []
    for call in range(2):
        want = oracle.rollout_random(ref, T, seed=seed, env_offset=env_offset, draw_base=call * T)
        want["adv"], want["tgt"] = oracle.gae(want["done"], want["value"], want["reward"], _last_val(n, T), GAMMA, LAM)
        want["state"] = ref.copy()
        calls.append(want)
    return calls


def deals_in_first_slots(calls):
    """a board ends (so the next slot starts with a deal) at step 0, at step 1 and at step 2 of the second call"""
    done = calls[1]["done"]
    return done.shape[0] >= 3 and all(done[t].any() for t in range(3))


@functools.lru_cache(maxsize=None)
def _reference(oracle, n, T, env_offset):
    """(seed, the oracle's two calls), computed once per shape.  T >= 3: the first seed in range(16) whose second call
    deals in each of its first three steps."""
    if T < 3:
        return 0, oracle_calls(oracle, n, T, env_offset, 0)
    for seed in range(16):
        calls = oracle_calls(oracle, n, T, env_offset, seed)
        if deals_in_first_slots(calls):
            return seed, calls
    return None, None


def _run(e, n, T, seed, gae):
    """two launches on one table set through the C API; per call every buffer the launch writes, as torch tensors"""
    from brl_amd import _capi
    from brl_amd.bridge_bidding import State
    from brl_amd.roll_out import alloc_transition
    dev = e.device
    st = e.init(seed, num_envs=n)
    lv = torch.from_numpy(_last_val(n, T)).to(dev)
    gl = float(torch.tensor(GAMMA * LAM, dtype=torch.float32))
    s = torch.cuda.current_stream().cuda_stream
    outs = []
    for call in range(2):
        traj = alloc_transition(T, n, dev)
        p = _capi.TransitionPtrs()
        for f in _capi.TransitionPtrs._names:
            getattr(traj, f).view(torch.uint8).fill_(0xA5)
            setattr(p, f, getattr(traj, f).data_ptr())
        lo = torch.full((n, 480), 0xA5, dtype=torch.uint8, device=dev)
        lm = torch.full((n, 38), 0xA5, dtype=torch.uint8, device=dev)
        tc = torch.zeros(1, dtype=torch.int64, device=dev)
        out = {name: getattr(traj, name) for name in COLUMNS}
        if gae:
            out["adv"], out["tgt"] = torch.empty((T, n), device=dev), torch.empty((T, n), device=dev)
            _capi.check(_capi.lib().brl_rollout_random_gae(e._h, st.packed.data_ptr(), n, T, call * T, 7600.0, C.byref(p), lo.data_ptr(),
                                                           lm.data_ptr(), tc.data_ptr(), lv.data_ptr(), GAMMA, gl,
                                                           out["adv"].data_ptr(), out["tgt"].data_ptr(), s))
        else:
            _capi.check(_capi.lib().brl_rollout_random(e._h, st.packed.data_ptr(), n, T, 1, call * T, 7600.0, C.byref(p), lo.data_ptr(),
                                                       lm.data_ptr(), tc.data_ptr(), s))
        torch.cuda.synchronize()
        out.update(last_obs=lo, last_mask=lm, count=tc, packed=st.packed.clone())
        outs.append(out)
    return outs, State(e, st.packed)


@pytest.mark.parametrize("gae", [False, True], ids=["rollout", "rollout_gae"])
@pytest.mark.parametrize("n,T,env_offset", SHAPES)
def test_first_slots_match_oracle_and_ws(dds, oracle, n, T, env_offset, gae):
    seed, want = _reference(oracle, n, T, env_offset)
    assert seed is not None, f"no seed in range(16) deals in each of the first three steps of the second call (n={n} T={T})"
    kw = {"env_offset": env_offset} if env_offset else {}
    got, final = _run(make_env(dds, 4, **kw), n, T, seed, gae)
    for call in range(2):
        g, w = got[call], want[call]
        where = f"n={n} T={T} seed={seed} call {call}"
        for name in COLUMNS + (("adv", "tgt") if gae else ()):
            a = to_np(g[name])
            assert a.shape == w[name].shape and a.tobytes() == w[name].tobytes(), f"{where}: {name}"
        assert np.array_equal(to_np(g["last_obs"]), w["state"]["observation"]), f"{where}: last_obs"
        assert np.array_equal(to_np(g["last_mask"]), w["state"]["legal_action_mask"]), f"{where}: last_mask"
        assert int(g["count"].item()) == w["terminated_count"], f"{where}: terminated count"
    assert_state_equal(final, want[1]["state"], where=f"n={n} T={T} seed={seed} final state")
    # the same input through k_rollout_ws
    other, _ = _run(make_env(dds, 4, "ws", **kw), n, T, seed, gae)
    for call in range(2):
        for name, x in got[call].items():
            assert torch.equal(x, other[call][name]), f"n={n} T={T} seed={seed} call {call}: {name} differs from k_rollout_ws"
