"""-m gpu: the policy sampler (categorical<K>, brl_amd/csrc/policy_common.hpp) and the evaluators' illegal_mass<K> against
the float64 reference of tests/categorical_ref.py — every lane layout, every input format, peaked / tied / underflowing
/ poisoned rows, ragged batches and the two ends of the draw range.  One launch of brl_amd.utils.policy_step each."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests.categorical_cases import family_of_rows, make_rows, stepped_states
from tests.categorical_ref import BAND, U24, accept_matrix, log_softmax64, mode64
from tests.conftest import GOLDEN
from tests.gpu_util import assert_state_equal, make_env, to_np

pytestmark = pytest.mark.gpu

SEED, DRAWS = 19, 16
DTYPE = {0: torch.float32, 1: torch.bfloat16, 2: torch.float16}
STRIDE = {0: 38, 1: 40, 2: 38}          # (bf16: rows 40 apart, the two columns behind the logits hold NaN)
# every K sees 67 (a ragged last wave at every K) and 1 or 3 (invalid lanes inside the first wave); 1000 once per K
SIZES = {(1, 0): (67, 1), (1, 1): (67, 3), (1, 2): (67, 3, 1000), (2, 0): (67, 3, 1000), (2, 1): (67, 1), (2, 2): (67, 3),
         (4, 0): (67, 1, 1000), (4, 1): (67, 3), (4, 2): (67, 1), (8, 0): (67, 3), (8, 1): (67, 1, 1000), (8, 2): (67, 3)}
ALL = np.ones(38, np.uint8)


def on_device(rows, fmt):
    """the rows in the kernel's input format on the device ([n, 38] view of a [n, STRIDE] buffer) and, as float32 numpy,
    what they round to: the reference's input"""
    t = torch.from_numpy(rows).to(DTYPE[fmt])
    buf = torch.full((rows.shape[0], STRIDE[fmt]), float("nan"), dtype=DTYPE[fmt], device="cuda")
    buf[:, :38] = t.cuda()
    return buf[:, :38], t.float().numpy()


class Launcher:
    """policy_step on one batch of states, autoreset off; returns (action, log_prob) as numpy, the next state in .out"""

    def __init__(self, env, st, fmt):
        from brl_amd import _capi
        self.env, self.st, n = env, st, st.packed.shape[0]
        self.ext = _capi.MacroExt(in_fmt=fmt) if fmt else None
        self.out = torch.empty_like(st.packed)
        self.action = torch.empty(n, dtype=torch.int32, device="cuda")
        self.logp = torch.empty(n, dtype=torch.float32, device="cuda")

    def launch(self, lg, mode, draw, action, logp):
        from brl_amd.utils import policy_step
        policy_step(self.env, self.st.packed, self.out, lg, mode, draw, False, action=action, log_prob=logp, ext=self.ext)

    def __call__(self, lg, mode, draw=0):
        self.action.fill_(-7)
        self.logp.fill_(float("nan"))
        self.launch(lg, mode, draw, self.action, self.logp)
        return to_np(self.action).copy(), to_np(self.logp).copy()

    def next_state(self):
        from brl_amd.bridge_bidding import State
        return State(self.env, self.out)


def stepped_env(dds, oracle, k, n, env_offset=0, steps=3, rng=None, forced=True):
    """a K-tables-per-wave environment `steps` calls past the deal, with the oracle's copy of its states"""
    ref, calls = stepped_states(oracle, n, SEED, env_offset, steps, rng, forced)
    env = make_env(dds, k, env_offset=env_offset)
    st = env.init(SEED, num_envs=n)
    for act in calls:
        st = env.step(st, torch.from_numpy(act))
    return env, st, ref


def assert_log_prob(lp, lsm, a, where):
    want = lsm[np.arange(len(a)), a]
    # atol: the suite's fp32 log-softmax tolerance; rtol: (la - mx) is ONE fp32 subtraction, half an ulp = 6e-8 relative
    # of a difference that reaches 80 for the peaked rows, plus logf(total) with total good to ~11 * 2**-24
    bad = ~(np.abs(lp - want) <= 1e-5 + 1e-6 * np.abs(want))
    assert not bad.any(), f"{where}: log_prob off on rows {np.nonzero(bad)[0][:8]}: {lp[bad][:8]} vs {want[bad][:8]}"


def oracle_next(oracle, ref, a):
    nxt = ref.copy()
    oracle.step(nxt, a.astype(np.int32))
    return nxt


@pytest.mark.parametrize("fmt", [0, 1, 2])
@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_sampler_matrix_against_float64(dds, oracle, k, fmt):
    from brl_amd.utils import MODE, SAMPLE, UNMASKED
    rng = np.random.default_rng(100 * k + fmt)
    pairs = multi = 0
    for n in SIZES[(k, fmt)]:
        env, st, ref = stepped_env(dds, oracle, k, n)
        assert_state_equal(st, ref, where=f"K={k} n={n} stepped")
        mask = ref["legal_action_mask"].astype(np.uint8)
        if n >= 67:
            assert (mask.sum(1) == 1).any() and (mask.sum(1) > 5).any()   # real single-call masks and wide ones
        u24 = np.array([[oracle.action_draw(SEED, e, d) >> 8 for e in range(n)] for d in range(DRAWS)])
        run = Launcher(env, st, fmt)
        rows_i = np.arange(n)
        for masked in (True, False):
            where = f"K={k} fmt={fmt} n={n} {'masked' if masked else 'unmasked'}"
            flag = 0 if masked else UNMASKED
            cand = mask if masked else np.broadcast_to(ALL, mask.shape)
            fams = np.array(family_of_rows(n, shift=k + 3 * fmt + n))
            lg, rows = on_device(make_rows(rng, fams, mask, masked, fp16=fmt == 2), fmt)
            lsm = log_softmax64(rows, cand)
            assert np.isfinite(lsm.max(1)).all()        # every row has a finite candidate logit (others have no reference)
            finite_cands = (np.isfinite(np.where(cand.astype(bool), rows, -np.inf))).sum(1)
            single = finite_cands == 1
            assert single[fams == "single"].all()
            # 1. MODE: the first maximum, exactly
            a, lp = run(lg, MODE | flag)
            assert np.array_equal(a, mode64(rows, cand)), where
            assert_log_prob(lp, lsm, a, where + " mode")
            assert (lp[single] == 0.0).all() and np.isfinite(rows[rows_i, a][single]).all(), where
            assert_state_equal(run.next_state(), oracle_next(oracle, ref, a), where=where + " mode, next state")
            results = {("mode", 0): (a, lp)}
            # 2. / 3. SAMPLE: the float64 inverse CDF within BAND of the draw, a candidate, never a -inf call
            for d in range(DRAWS):
                a, lp = run(lg, SAMPLE | flag, d)
                results[("sample", d)] = (a, lp)
                acc = accept_matrix(rows, cand, u24[d])
                bad = ~acc[rows_i, a]
                assert not bad.any(), (f"{where} draw {d}: rows {np.nonzero(bad)[0][:8]} ({fams[bad][:8]}) took {a[bad][:8]}, "
                                       f"u24 {u24[d][bad][:8]}, acceptable {[np.nonzero(r)[0].tolist() for r in acc[bad][:8]]}")
                assert cand[rows_i, a].all() and np.isfinite(rows[rows_i, a]).all(), where
                assert (lp[single] == 0.0).all(), where
                assert_log_prob(lp, lsm, a, f"{where} draw {d}")
                pairs += n
                multi += int((acc.sum(1) > 1).sum())
                if d == 0:
                    assert_state_equal(run.next_state(), oracle_next(oracle, ref, a), where=where + " sample, next state")
            # 4. what illegal entries hold never matters: bit-identical to the same rows with 0.0 there, nothing NaN
            pois = fams == "poisoned"
            if masked:
                clean = rows.copy()
                clean[pois] = np.where(mask[pois].astype(bool), rows[pois], 0.0)
                assert not np.isfinite(rows[pois]).all() or not pois.any() or mask[pois].all(axis=1).any()
                lg2, _ = on_device(clean, fmt)
                for (kind, d), (a, lp) in list(results.items())[:5]:
                    a2, lp2 = run(lg2, (MODE if kind == "mode" else SAMPLE) | flag, d)
                    assert np.array_equal(a2[pois], a[pois]) and np.array_equal(lp2[pois].view(np.int32), lp[pois].view(np.int32)), where
                    assert not np.isnan(lp).any() and not np.isnan(lp2).any(), where
            # 5. no leakage between the tables of a wave: every third row among flat neighbours gives the same bits
            keep = (rows_i % 3) == (k % 3)
            alone = make_rows(rng, ["flat"] * n, mask, masked)
            alone[keep] = rows[keep]
            lg3, _ = on_device(alone, fmt)
            for (kind, d), (a, lp) in list(results.items())[:5]:
                a3, lp3 = run(lg3, (MODE if kind == "mode" else SAMPLE) | flag, d)
                assert np.array_equal(a3[keep], a[keep]) and np.array_equal(lp3[keep].view(np.int32), lp[keep].view(np.int32)), where
    # 6. the reference left the sampler a choice on at most 1 % of the (row, draw) pairs actually met
    assert pairs >= 2 * DRAWS * 68 and multi <= 0.01 * pairs, (multi, pairs)


with open(os.path.join(GOLDEN, "extreme_draws.json")) as _f:
    EXTREME = json.load(_f)


@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_sampler_at_the_ends_of_the_draw_range(dds, oracle, k):
    """The draws 2**24 - 1, 2**24 - 2, 1 and 0 (tests/golden/extreme_draws.json) on 64 peaked / one-hot rows each, the
    table that gets the draw on lane-slot 0 of a wave, on a wave's last table and in the ragged last wave of 67.
    Before the drawable-cell rule of categorical<K> the card failed this on 347 of 2048 rows at K = 1 and 468 / 456 / 434 of
    3072 at K = 2 / 4 / 8: 24-37 rows per K at each of the two top draws (the fall-through to the highest-numbered candidate,
    calls of probability down to 1e-44) and 294-398 at the draw 0 (a first candidate of probability below 2**-42)."""
    from brl_amd.utils import SAMPLE, UNMASKED
    n, R = 67, 64
    fams = ["peaked8", "peaked20", "onehot"] * 21 + ["peaked8"]
    rng = np.random.default_rng(k)
    failures, checked = {}, 0
    for name, triples in EXTREME.items():
        for ti, t in enumerate(triples):
            assert t["seed"] == SEED
            masked = ti % 2 == 0
            for j in sorted({k, 2 * k - 1, 66}):
                env, st, ref = stepped_env(dds, oracle, k, n, env_offset=t["env_id"] - j, steps=1 + ti % 3,
                                           rng=np.random.default_rng(t["env_id"] + j), forced=False)
                mask = ref["legal_action_mask"].astype(np.uint8)
                cand = np.broadcast_to(mask[j] if masked else ALL, (R, 38))
                rows = make_rows(rng, fams, np.broadcast_to(mask[j], (R, 38)), masked)
                batch = np.broadcast_to(make_rows(rng, ["flat"] * n, mask, masked), (R, n, 38)).copy()
                batch[:, j] = rows
                lg = torch.from_numpy(batch).cuda()
                action = torch.full((R, n), -7, dtype=torch.int32, device="cuda")
                logp = torch.full((R, n), float("nan"), dtype=torch.float32, device="cuda")
                run = Launcher(env, st, 0)
                for r in range(R):    # no read-back between the launches: each writes its own row of action / logp
                    run.launch(lg[r], SAMPLE | (0 if masked else UNMASKED), t["draw"], action[r], logp[r])
                a, lp = to_np(action)[:, j], to_np(logp)[:, j]
                lsm = log_softmax64(rows, cand)
                p = np.exp(lsm)
                acc = accept_matrix(rows, cand, np.full(R, t["u24"]))
                bad = ~acc[np.arange(R), a]                                   # assertion 2
                bad |= ~cand[np.arange(R), a].astype(bool)
                pa = p[np.arange(R), a]
                if t["u24"] == 0:                                             # assertion 7
                    bad |= a != np.argmax(p > U24 * BAND, axis=1)
                if t["u24"] >= (1 << 24) - 2:
                    bad |= ~(pa >= 2.0 ** -25)
                checked += R
                if bad.any():
                    failures[(name, t["env_id"], j)] = (int(bad.sum()), a[bad][:4].tolist(), pa[bad][:4].tolist())
                else:
                    assert_log_prob(lp, lsm, a, f"K={k} {name} env {t['env_id']} j={j}")   # assertion 3
    print(f"K={k}: {sum(v[0] for v in failures.values())} of {checked} rows outside the reference: {failures}")
    assert not failures


@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_illegal_mass_against_float64(dds, oracle, k):
    """One evaluator step with statistics on peaked / one-hot rows: illegal_prob_sum = softmax(logits) . ~mask in float64,
    the greedy call = mode64, finished boards and boards waiting for the other team log nothing."""
    from brl_amd import _capi
    from brl_amd._capi import check, ptr, stream
    from brl_amd.evaluation import EvalStats
    n = 67
    rng = np.random.default_rng(7 + k)
    ref = oracle.init_random(n, seed=SEED)
    env = make_env(dds, k)
    st = env.init(SEED, num_envs=n)
    for s in range(4):                     # every seventh table passes out (finished), the others make four legal calls
        act = np.where(np.arange(n) % 7 == 0, 0, 3 + s + np.arange(n) % 5 * (s + 1)).astype(np.int32)
        st = env.step(st, torch.from_numpy(act))
        oracle.step(ref, act)
    assert_state_equal(st, ref, where="stepped")
    mask, done, team = ref["legal_action_mask"].astype(bool), ref["terminated"].astype(bool), ref["current_player"] >> 1
    assert done.any() and not done.all() and (team[~done] == 0).any() and (team[~done] == 1).any()
    fams = family_of_rows(n, shift=k)
    fams = [{"flat": "peaked8", "ties": "peaked20", "single": "onehot", "poisoned": "peaked40", "neg_inf_legal": "onehot"}.get(f, f)
            for f in fams]                 # peaked8/20/40, onehot, max_on_illegal (mass near 1)
    rows = make_rows(rng, fams, mask.astype(np.uint8), True)
    lg = torch.from_numpy(rows).cuda()
    p = np.exp(log_softmax64(rows, np.broadcast_to(ALL, rows.shape)))
    want_mass = (p * ~mask).sum(1)
    for acting_team in (-1, 0, 1):
        stats = EvalStats(n, "cuda")
        ps = stats.ptrs()
        action = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        out = torch.empty_like(st.packed)
        if acting_team < 0:
            check(_capi.lib().brl_eval_step(env._h, ptr(st.packed), ptr(out), n, lg.data_ptr(), 38, lg.data_ptr(), 38, None, None,
                                            C.byref(ps), 0, None, None, ptr(action), None, None, None, None, None, stream()))
        else:
            check(_capi.lib().brl_eval_step_team(env._h, ptr(st.packed), ptr(out), n, lg.data_ptr(), 38, acting_team, None, None,
                                                 C.byref(ps), 0, None, None, ptr(action), None, None, None, None, None, None,
                                                 stream()))
        logs = ~done & ((acting_team < 0) | (team == acting_team))
        got, steps, a = to_np(stats.illegal_prob_sum), to_np(stats.step_count), to_np(action)
        want = np.zeros((n, 2))
        want[np.arange(n), team] = np.where(logs, want_mass, 0.0)
        # a quotient of two fp32 sums of <= 38 terms in [0, 1]: each good to (7 additions + 2 ulp of expf) ~ 11 * 2**-24, the
        # quotient to ~1.4e-6 relative — 1e-5; the absolute term for masses that are sums of underflowing terms
        assert np.all(np.abs(got - want) <= 1e-6 + 1e-5 * np.abs(want)), (k, acting_team, np.abs(got - want).max())
        assert np.array_equal(steps[np.arange(n), team], logs.astype(np.int32)) and steps.sum() == logs.sum()
        assert (got[~logs] == 0.0).all()
        assert np.array_equal(a[logs], mode64(rows, mask)[logs])
    assert want_mass[~done].max() > 0.9 and want_mass[~done].min() < 1e-6
