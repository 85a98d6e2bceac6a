"""-m gpu: the policy rollout (make_roll_out -> _PolicyRollout: four brl_policy_step_ex sub-steps per macro-step, rewards summed and
`terminated` OR-ed on the device, boards replaced inside a macro-step, heads formed in the launch on the 16-bit paths, eager and as
hipGraphs) on a network that BIDS (tests/bidder_net.py), on every inference route.  Freshly initialised networks play at random: no
board is passed out, 1 % of the contracts make, 99.8 % of the auctions end at the 7 level (tests/test_bidder_host.py).  Here boards end
by four passes, in made part-scores and games and in failed contracts, at each of the four sub-step positions, with the actor
declaring and defending, and the rollout goes on with the freshly dealt board inside the same macro-step.

Per case:
  (a) what test_policy_rollout_replays_through_oracle asserts: obs, legal_action_mask, done, reward and the final packed state
      bit-exact against the oracle's replay of the recorded calls; last_obs, terminated_count, the draw counter + 4 T;
  (b) the census of the replay (the boards the ORACLE finished on the recorded calls) as a condition on the input: the first case
      meets the whole list of test_bidder_host.py, every other case has a pass-out, made and failed contracts and boards ending at
      every sub-step position (free-run: at sub-steps 1 and 3 only and never doubled — see test_bidder_host.py for why);
  (c) fp32 routes: EVERY recorded call — sub-step k of macro-step t of table i — lies in the float64 sampler's accept set
      (tests/categorical_ref.py) for the draw Oracle.action_draw(seed, env_offset + i, rng0 + 4 t + k) >> 8, the float64 logits of the
      network whose turn it is on the oracle's pre-step observation, and the oracle's pre-step mask (all 38 calls for the unmasked
      actor), with band = BAND + 2 tol, tol = 2e-4 max(1, max|ref|): a logit error d moves no CDF value by more than 2 d.  The first
      case first shows, on the reference side, that the draws of index + 1 would put at least a quarter of the rows outside;
      free-run: the opponents' calls are passes and the partner's is a maximum of the masked float64 logits within 2 tol;
  (d) traj.value / traj.log_prob within the bounds of test_rollout_records_value_and_log_prob_of_the_current_networks (imported);
  (e) first case: gae_scan on done / value / reward bit-identical to Oracle.gae, with `done` at zero (pass-out), positive and
      negative reward in those columns.
"""
import numpy as np
import pytest
import torch

from tests import bidder_net as bn
from tests import categorical_ref as cref
from tests.gpu_util import assert_state_equal, replay_policy_rollout, to_np
from tests.nets import forward16_ref, forward64
from tests.test_gpu_forward_biases import DT, _bound16, _excess, _log_prob64, _tol32

pytestmark = pytest.mark.gpu

CASES = {   # the smallest shapes at which each route can still go wrong
    "fp32_eager": dict(n=1000, T=16, calls=2, seed=4242),                     # ragged (no multiple of 64), the library route; the second
    "fp32_graph": dict(n=1000, T=16, calls=2, seed=4242, graph=True),         # call continues draw_base, terminated_count and the state
    "fp32_planes": dict(n=4096, T=8, graph=True),                            # brl_linear_x3p: the smallest n that takes it
    "fp32_x3": dict(n=4096, T=8, gemm="bf16x3", planes="0"),                 # brl_mlp_gemm_x3
    "bf16_graph": dict(n=1000, T=16, graph=True, dt="bf16"),                 # heads formed in the step launch
    "fp16_eager": dict(n=1000, T=16, dt="fp16"),
    "unmasked": dict(n=700, T=12, masked=False),                             # the actor may draw an illegal call: board over, offender -1
    "shard": dict(n=1000, T=8, graph=True, offset=3 * 8192, rng0=1000),      # draws and deals of the global tables
    "free_run": dict(n=700, T=12, mode="free-run"),                          # (last: it compares its made share with every other case)
}
FULL = ("fp32_eager", "fp32_graph")
CENSUS = {}      # case -> census of its replay, for the free-run comparison


@pytest.fixture(scope="module")
def nets():
    return bn.pair("cuda")


def _case(name):
    return dict(dict(n=0, T=0, calls=1, seed=99, graph=False, dt=None, gemm=None, planes=None, mode="competitive", masked=True, offset=0,
                     rng0=0), **CASES[name])


def check_calls(oracle, actor, opp, detail, act0, sub, seed, offset, rng0, mode="competitive", masked=True, shifted=False, device="cuda"):
    """(c) for one call of the rollout.  -> (rows checked, rows outside their accept set, with `shifted` the share of rows whose
    REFERENCE call for the right draw lies outside the accept set of the draw of index + 1)"""
    T, n = act0.shape
    rows = outside = wrong = 0
    for t in range(T):
        for k in range(4):
            a = act0[t] if k == 0 else sub[t, k - 1]
            if mode != "competitive" and k in (1, 3):
                assert (a == 0).all()                     # the opponents pass
                continue
            obs, mask = detail["sub_obs"][t, k], detail["sub_mask"][t, k]
            ref = forward64(opp if k in (1, 3) else actor, torch.from_numpy(obs).to(device)).cpu().numpy()
            tol = 2e-4 * max(1.0, float(np.abs(ref).max()))
            logits = ref[:, :38]
            cand = np.ones_like(mask) if (k == 0 and not masked) else mask
            if mode != "competitive" and k == 2:          # the partner takes the mode
                best = np.where(cand.astype(bool), logits, -np.inf).max(1)
                assert (cand[np.arange(n), a] == 1).all() and (logits[np.arange(n), a] >= best - 2 * tol).all(), (t, k)
                continue
            u24 = bn.draws24(oracle, seed, offset, n, rng0 + 4 * t + k)
            ok = cref.accept_matrix(logits, cand, u24, cref.BAND + 2 * tol)[np.arange(n), a]
            rows, outside = rows + n, outside + int((~ok).sum())
            if shifted:
                a_ref = bn.sample64(logits, cand, u24)
                off = cref.accept_matrix(logits, cand, bn.draws24(oracle, seed, offset, n, rng0 + 4 * t + k + 1), cref.BAND + 2 * tol)
                wrong += int((~off[np.arange(n), a_ref]).sum())
    return rows, outside, wrong


@pytest.mark.parametrize("case", list(CASES))
def test_bidder_rollout(dds, oracle, nets, case, monkeypatch):
    """Measured on the MI355X (printed by each case).  No case found a defect; all nine take 6 s together.
    Census of the replay — boards, pass-outs, made, failed; final contracts at levels 1..7; undoubled / doubled / redoubled; boards
    by ending sub-step 0..3; the smallest of the twelve cells; distinct outcomes:
      fp32_eager = fp32_graph (two calls)  17017, 790, 6994, 9233; 3691 3391 3772 2842 1592 667 272; 14137 / 1470 / 620;
                                           5451 2965 5548 3053; 99; 1696 (741 pass-outs four calls after the table's previous board)
      fp32_planes = fp32_x3                16229, 807, 6782, 8640; 3757 3399 3573 2538 1353 585 217; 13779 / 1212 / 431;
                                           5036 2612 5479 3102; 96; 1568
      bf16_graph                           8352, 384, 3487, 4481; 1832 1768 1889 1358 703 308 110; 7076 / 645 / 247; 2660 1429 2809 1454
      fp16_eager                           8345, 387, 3474, 4484; 1827 1764 1879 1367 700 309 112; 7070 / 643 / 245; 2654 1427 2811 1453
      unmasked                             4404 (681 ended by an illegal call), 192, 1595, 1936; 3194 / 261 / 76; 1494 718 1467 725
      shard                                3966, 202, 1681, 2083; 3356 / 305 / 103; 1246 639 1297 784
      free_run                             7110, 3697, 2638, 775; 2750 405 212 41 5 0 0; never doubled; 0 2681 0 4429
    (the same pair of freshly initialised networks at 1000 x 16: 5711 boards, no pass-out, 68 made, 5698 at the 7 level, 224 distinct
    outcomes against the bidder's 1324 — tests/test_bidder_host.py).  Made share of the contracts: free-run 0.773, the others
    0.431 .. 0.452; per finished board free-run has 0.371 against 0.362 .. 0.424, because two passes of one side pass a free-run board
    out (52 % of its boards) — the share is therefore taken over the contracts.
    (c) 0 of 64000 + 64000 (first case), 131072 (4096 x 8), 33600 (unmasked), 32000 (shard), 8400 (free-run) recorded calls outside
    their accept set; the draws of index + 1 put 0.371 of the first case's reference calls outside.
    (d) max|ref| 13.9 .. 16.5, logits from -16.5 to 12.5, smallest recorded log_prob -9.1 .. -12.0.  fp32 routes: value error 3.5e-6 ..
    6.0e-6 of bounds of 2.8e-3 .. 3.3e-3, log_prob error 3.3e-5 .. 5.7e-5 of 5.6e-3 .. 6.6e-3.  bf16: library chain 3.9e-2 (one
    rounding of a count near 10 that fell the other way), so value 2.0e-3 of 7.8e-2 and log_prob 9.5e-3 of 1.6e-1; fp16: library chain
    7.8e-3, value 9.8e-4 of 1.6e-2, log_prob 7.0e-3 of 3.1e-2.
    A deliberately wrong reference fails the first case: the draw index shifted by one at (c) (23759 of 64000 calls outside), sub-step
    2's reward left out of the replay's sum at (a) `reward`, a pass-out taken as not done at (a) `done`."""
    import brl_amd
    from brl_amd.gae import gae_scan
    from brl_amd.models import make_forward_pass
    c = _case(case)
    n, T, seed, offset, rng0, dt, mode, masked = c["n"], c["T"], c["seed"], c["offset"], c["rng0"], c["dt"], c["mode"], c["masked"]
    for key in ("BRL_HEAD_PARTS", "BRL_LINEAR16", "BRL_INFERENCE_PLANES", "BRL_TABLES_PER_WAVE", "BRL_INFERENCE_GEMM"):
        monkeypatch.delenv(key, raising=False)
    if c["planes"] is not None:
        monkeypatch.setenv("BRL_INFERENCE_PLANES", c["planes"])
    dtype = DT.get(dt)
    actor, opp = nets
    env = brl_amd.BridgeBidding(lut=(dds["keys"], dds["values"]), env_offset=offset)
    cfg = dict(reward_scale=7600, game_mode=mode, actor_illegal_action_mask=masked, actor_illegal_action_penalty=not masked, gamma=1.0,
               gae_lambda=0.95, num_steps=T, graph_rollout=c["graph"], inference_dtype=dt, inference_gemm=c["gemm"])
    fp = make_forward_pass("relu", "DeepMind")
    roll = brl_amd.make_roll_out(cfg, env, fp, fp)
    st = env.init(seed, num_envs=n)
    ref = oracle.init_random(n, seed=seed, env_offset=offset)
    rs = (actor, None, st, st.observation, 0, rng0)
    detail, total = {"events": []}, 0
    for call in range(c["calls"]):
        draw0 = rs[5]
        rs, traj = roll(rs, opp)
        torch.cuda.synchronize()
        eng = roll.engine
        where = f"{case} call {call}"
        # ---- the route
        assert bool(eng.static) == c["graph"] and (not c["graph"] or eng.graphs), getattr(eng, "graph_error", None)
        if dtype is None:
            planes = n >= 4096 and c["planes"] != "0"
            assert eng.xin.dtype == (torch.bfloat16 if planes else torch.float32), where
            assert (eng.snap_actor.wp is not None) == (c["planes"] != "0") and bool(eng.snap_actor.planes_for(n)) == planes, where
            assert eng.snap_actor.gemm_x3 and eng.snap_opp.gemm_x3, where       # (what n >= 4096 rows run on; fewer: the library's GEMM)
        else:
            assert eng._fused_heads(False) is not None and eng._fused_heads(True) is not None, where
        # ---- (a) the replay
        detail["t0"] = call * T
        want = replay_policy_rollout(oracle, ref, traj, roll.sub_actions, seed, env_offset=offset, detail=detail)
        for name in ("obs", "legal_action_mask", "done", "reward"):
            assert np.array_equal(to_np(getattr(traj, name)), want[name]), f"{where}: {name}"
        assert_state_equal(rs[2], ref, where=f"{where}: final state")
        assert np.array_equal(to_np(rs[3]), ref["observation"]), f"{where}: last_obs"
        total += want["terminated_count"]
        assert int(rs[4].item()) == total and rs[5] == draw0 + 4 * T, where
        act0, sub, mask = to_np(traj.action), to_np(roll.sub_actions), want["legal_action_mask"]
        legal = np.take_along_axis(mask, act0[..., None].astype(np.int64), 2)[..., 0]
        if masked:
            assert legal.all(), f"{where}: sampled action illegal"
        else:           # the bidder does not put -inf on illegal calls: some are drawn; board over, the offender's -1 scaled
            bad = legal == 0
            assert bad.any() and (want["done"][bad] == 1).all()
            assert (to_np(traj.reward)[bad] == np.float32(-1.0) / np.float32(7600.0)).all()
        # ---- (c) every recorded call against the float64 sampler at the rollout's own draw
        if dtype is None:
            rows, outside, wrong = check_calls(oracle, actor, opp, detail, act0, sub, seed, offset, draw0, mode, masked,
                                               shifted=case in FULL and call == 0)
            if case in FULL and call == 0:
                print(f"{where}: the draws of index + 1 put {wrong / rows:.3f} of the reference's calls outside their accept set")
                assert wrong >= 0.25 * rows
            print(f"{where}: {outside} of {rows} recorded calls outside their accept set")
            assert outside == 0, where
        # ---- (d) the recorded value and log_prob
        obs = traj.obs.reshape(T * n, 480)
        if dtype is None:
            refv = forward64(actor, obs)
            bound = _tol32(refv)
        else:
            refv = forward16_ref(actor, obs, dtype)
            e_lib, bound, ulp = _bound16(actor, obs, dtype, refv)      # (heads formed in the launch: nothing was stored in 16 bits)
            print(f"{where}: library chain {e_lib:.2e} -> bound {bound:.2e} (one ulp at the largest output: {ulp:.2e})")
        cand = traj.legal_action_mask.reshape(T * n, 38) if masked else torch.ones((T * n, 38), dtype=torch.bool, device="cuda")
        want_lp = _log_prob64(refv[:, :38], cand, traj.action.reshape(-1))
        ev = _excess(traj.value.reshape(-1), refv[:, 38], 0.0)
        elp = float((traj.log_prob.reshape(-1).double() - want_lp).abs().max())
        print(f"{where}: max|ref| {float(refv.abs().max()):.2f}, logits span {float(refv[:, :38].min()):.1f} .. {float(refv[:, :38].max()):.1f}, "
              f"value error {ev:.2e} of {bound:.2e}, log_prob error {elp:.2e} of {2 * bound:.2e}, smallest log_prob {float(want_lp.min()):.1f}")
        assert ev < bound and elp < 2 * bound, where
        assert float(refv[:, 38].std()) > 0.1          # the stored value is not ~0
        # ---- (e) GAE on these columns
        if case in FULL:
            g = torch.Generator().manual_seed(5 + call)
            last_val = torch.randn(n, generator=g).cuda()
            adv, tgt = gae_scan(env, traj.done, traj.value, traj.reward, last_val, 1.0, 0.95)
            wa, wt = oracle.gae(want["done"], to_np(traj.value), want["reward"], to_np(last_val), 1.0, 0.95)
            assert np.array_equal(to_np(adv), wa) and np.array_equal(to_np(tgt), wt), f"{where}: GAE"
            d, r = want["done"] == 1, want["reward"]
            assert (d & (r == 0)).any() and (d & (r > 0)).any() and (d & (r < 0)).any() and (r[~d] == 0).all()
    # ---- (b) the census of the replay: a condition on the input
    cs = CENSUS[case] = bn.census(detail["events"])
    print(f"{case}: census {cs}")
    assert cs["boards"] >= total > 0         # (terminated_count counts macro-steps with `done`; two boards can end in one)
    if case in FULL:
        assert bn.full_conditions(cs) == []
    if mode == "competitive":
        assert bn.basic_conditions(cs) == []
        assert (cs["illegal"] > 0) == (not masked)
    else:
        assert bn.basic_conditions(cs, positions=(1, 3)) == [] and cs["by_k"][0] == 0 and cs["by_k"][2] == 0
        share = lambda x: x["made"] / (x["made"] + x["down"])        # noqa: E731
        for other in CASES:
            if other not in CENSUS:       # (run alone: the same rollout on the host — the census is an input condition)
                o = _case(other)
                CENSUS[other] = bn.census(bn.simulate(oracle, *bn.pair(), o["n"], o["T"] * o["calls"], o["seed"], o["mode"], o["masked"],
                                                      o["offset"], o["rng0"])[0])
            print(f"made share of the contracts, {other}: {share(CENSUS[other]):.3f} ({CENSUS[other]['made'] / CENSUS[other]['boards']:.3f} of the boards)")
        assert all(share(cs) > share(CENSUS[other]) for other in CASES if other != case)
