"""The supervised pre-trainer on the GPU (brl_amd/sl.py, include/brl_sl.h).

The three kernels: the replay against the oracle at every decision point in file order and, row for row, in any order with
duplicates and at small batch sizes; the device sampler against its numpy restatement at n = 1000, at every n around a change of
the Feistel half width, at n = 1 and across 2^32 examples; the loss against float64 on random rows and on the rows and sizes where
it can go wrong (ties, equal logits, one legal call, +-100 logits, an illegal label; 1 .. 513 rows) with a per-row derivative
bound measured in numpy float32.

What is built on them: one ``SLStep`` — the batch it drew, its metrics row, every gradient, Adam's parameters and moments —
against a float64 restatement started from the device's own state, graph and eager, one step per replay and two; graph replays
against one-step replays and the eager composition; ``evaluate_pairs`` over several chunks, ``evaluate_all``, ``EvalStream`` and
``output_samples`` against float64 on the oracle's batches; ``train_sl``'s split of graph replays around evaluations; learning a
synthetic teacher; and ``python -m brl_amd.sl`` end to end."""
import copy
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sl_teacher as T  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _set(n, seed, kind="random"):
    from brl_amd import sl, sl_data
    ts = sl_data.parse_trajectories(T.random_file(n, seed, kind))
    return ts, sl.DeviceSet(ts, DEV)


def _np(t):
    return t.detach().cpu().double().numpy()


def test_replay_matches_the_oracle_at_every_decision_point(oracle):
    from brl_amd import sl, sl_data
    ts, data = _set(2000, seed=11)
    nc = ts.n_calls()
    assert nc.max() == 319 and (nc == 4).sum() >= 10 and (ts.calls == 2).sum() > 0
    traj, pos = sl_data.decision_points(ts)
    b = sl.Batch(traj.size, DEV)
    sl.sl_replay(data, torch.from_numpy(traj).to(DEV), torch.from_numpy(pos).to(DEV), b.obs, b.mask, b.label)
    obs, mask, label = b.obs.cpu().numpy(), b.mask.cpu().numpy(), b.label.cpu().numpy()
    assert np.array_equal(label, ts.calls.astype(np.int32))
    # the oracle: the converted deal, dealer 0, nobody vulnerable, identity seating, every auction stepped to its end (which
    # host_batch asserts to be at the trajectory's last call and nowhere before)
    want_obs, want_mask, want_label = T.host_batch(ts, traj, pos, oracle)
    for k in range(int(nc.max())):
        rows = np.nonzero(pos == k)[0]
        assert np.array_equal(obs[rows], want_obs[rows]), f"obs differs at call {k}"
        assert np.array_equal(mask[rows], want_mask[rows]), f"mask differs at call {k}"
    assert np.array_equal(label, want_label)


def test_replay_in_any_order():
    """The replay of a fixed random permutation of a 300-trajectory set's decision points, about 5 % of them twice, against the
    replay of the same points in file order (which test_replay_matches_the_oracle_at_every_decision_point holds to the oracle):
    every row bit for bit the ordered run's row of its (trajectory, call index).  The first wave of four examples holds the
    319-call auction's last decision (a prefix of 318 calls) twice beside two empty prefixes; batches of 1 .. 5 and 63 .. 65
    from the head of the list leave partial waves and a partial block."""
    from brl_amd import sl, sl_data
    ts, data = _set(300, seed=19)
    nc = ts.n_calls()
    assert nc.max() == 319 and (nc == 4).sum() >= 5
    traj, pos = sl_data.decision_points(ts)
    total = traj.size

    def replay(t, p):
        b = sl.Batch(t.size, DEV)
        sl.sl_replay(data, torch.from_numpy(t).to(DEV), torch.from_numpy(p).to(DEV), b.obs, b.mask, b.label)
        return b.obs.cpu().numpy(), b.mask.cpu().numpy(), b.label.cpu().numpy()

    want = replay(traj, pos)
    rng = np.random.default_rng(20)
    order = np.concatenate([rng.permutation(total), rng.integers(0, total, total // 20)])
    rng.shuffle(order)
    long_last = int(ts.offsets[1] + 318)
    order = np.concatenate([[long_last, int(ts.offsets[7]), long_last, int(ts.offsets[1])], order])
    assert pos[order[:4]].tolist() == [318, 0, 318, 0] and np.unique(order).size == total and order.size > total * 1.04
    got = replay(traj[order], pos[order])
    for g, w, name in zip(got, want, ("obs", "mask", "label")):
        assert np.array_equal(g, w[order]), name
    for n in (1, 2, 3, 4, 5, 63, 64, 65):
        got = replay(traj[order[:n]], pos[order[:n]])
        for g, w, name in zip(got, want, ("obs", "mask", "label")):
            assert np.array_equal(g, w[order[:n]]), (n, name)


def test_device_sampler_equals_the_numpy_restatement():
    from brl_amd import sl
    ts, data = _set(1000, seed=12)
    b = sl.Batch(ts.n + 37, DEV)
    counter = torch.zeros(1, dtype=torch.int64, device=DEV)
    for start in (0, ts.n - 20, 5 * ts.n + 3):
        counter.fill_(start)
        sl.sl_sample(data, counter, 42, b.traj, b.pos)
        t, p = T.sample(ts.offsets, 42, start, ts.n + 37)
        assert np.array_equal(b.traj.cpu().numpy(), t) and np.array_equal(b.pos.cpu().numpy(), p)
    counter.zero_()
    sl.sl_sample(data, counter, 42, b.traj, b.pos)
    assert sorted(b.traj[:ts.n].cpu().tolist()) == list(range(ts.n))    # each trajectory once in the first epoch


SAMPLER_NS = (1, 2, 3, 4, 5, 16, 17, 64, 65, 257)


@functools.lru_cache(maxsize=None)
def _sampler_file():
    from brl_amd import sl_data
    lines = T.random_file(1000, seed=21).strip().split("\n")
    lines = [lines[7], lines[1], lines[0]] + lines[2:7] + lines[8:]
    ts = sl_data.parse_trajectories("\n".join(lines) + "\n")
    assert ts.n_calls()[:2].tolist() == [4, 319]
    return ts


def sampler_set(n):
    """the first n trajectories of a 1000-trajectory random set whose file starts with a pass-out (4 calls) and the 319-call auction"""
    from brl_amd import sl_data
    ts = _sampler_file()
    return sl_data.TrajectorySet(ts.hands[:n].copy(), ts.offsets[:n + 1].copy(), ts.calls[:ts.offsets[n]].copy())


def check_stream_blocks(n, traj, pos, n_calls):
    """what every sampler owes at the head of its stream: the first three blocks of n are permutations of range(n), not all the
    same one from n = 5 on, and every call index lies inside its trajectory"""
    for e in range(3):
        assert sorted(traj[e * n:(e + 1) * n].tolist()) == list(range(n)), (n, e)
    if n >= 5:
        assert not (np.array_equal(traj[:n], traj[n:2 * n]) and np.array_equal(traj[:n], traj[2 * n:3 * n])), n
    assert (pos >= 0).all() and (pos < n_calls[traj]).all(), n


def test_device_sampler_small_and_wrapping():
    """brl_sl_sample at every n where the Feistel half width changes — 4, 16 and 64 fill their domain (no cycle walk), 5, 17 and 65
    are one past it (the longest walks) — at n = 1, 2, 3 and at 257: 3 n + 2 examples from counter 0 equal tests/sl_teacher.sample,
    whole epochs are permutations, call indices stay inside trajectories of 4 and of 319 calls.  Then counters on both sides of
    2^32 and at 3 x 2^32 + 1, at n = 3 and n = 1000: the example index's high word enters the call-index draw, and the epoch
    number and the index inside the epoch come from 64-bit arithmetic."""
    from brl_amd import sl
    counter = torch.zeros(1, dtype=torch.int64, device=DEV)
    for n in SAMPLER_NS:
        ts = sampler_set(n)
        data = sl.DeviceSet(ts, DEV)
        batch = 3 * n + 2
        traj = torch.zeros(batch, dtype=torch.int64, device=DEV)
        pos = torch.zeros(batch, dtype=torch.int32, device=DEV)
        counter.zero_()
        sl.sl_sample(data, counter, 42, traj, pos)
        t, p = T.sample(ts.offsets, 42, 0, batch)
        got_t, got_p = traj.cpu().numpy(), pos.cpu().numpy()
        assert np.array_equal(got_t, t) and np.array_equal(got_p, p), n
        check_stream_blocks(n, got_t, got_p, ts.n_calls())
    for n in (3, 1000):
        ts = sampler_set(n)
        data = sl.DeviceSet(ts, DEV)
        traj = torch.zeros(64, dtype=torch.int64, device=DEV)
        pos = torch.zeros(64, dtype=torch.int32, device=DEV)
        for start in (2 ** 32 - 10, 3 * 2 ** 32 + 1):
            counter.fill_(start)
            sl.sl_sample(data, counter, 42, traj, pos)
            t, p = T.sample(ts.offsets, 42, start, 64)
            got_t, got_p = traj.cpu().numpy(), pos.cpu().numpy()
            assert np.array_equal(got_t, t) and np.array_equal(got_p, p), (n, start)
            assert (got_p >= 0).all() and (got_p < ts.n_calls()[got_t]).all()


@pytest.mark.parametrize("ent_coef", [0.0, 0.01])
def test_loss_matches_float64(ent_coef):
    from brl_amd import sl
    rng = np.random.default_rng(3)
    B = 777
    z = rng.normal(0, 4, (B, 38)).astype(np.float32)
    z[:32] = rng.choice([-60.0, 60.0], (32, 38)) * rng.random((32, 38))
    mask = rng.random((B, 38)) < 0.4
    mask[:, 0] = True
    mask[40:50] = False
    mask[40:50, 0] = True
    label = np.array([rng.choice(np.nonzero(m)[0]) if i % 7 else rng.integers(0, 38) for i, m in enumerate(mask)], np.int32)
    want, dwant = T.loss64(z.astype(np.float64), label, mask, ent_coef)
    zs = torch.zeros((B, 40), device=DEV)            # a row stride larger than 38
    zs[:, :38] = torch.from_numpy(z)
    lt, mt = torch.from_numpy(label).to(DEV), torch.from_numpy(mask.astype(np.uint8)).to(DEV)
    out, out2 = torch.zeros(5, device=DEV), torch.zeros(5, device=DEV)
    d = torch.zeros((B, 38), device=DEV)
    sl.sl_loss(zs[:, :38], lt, mt, ent_coef, d, out)
    sl.sl_loss(zs[:, :38], lt, mt, ent_coef, None, out2)
    got, dgot = out.cpu().double().numpy(), d.cpu().double().numpy()
    assert np.allclose(got, want, rtol=1e-6, atol=1e-7), (got, want)
    assert np.abs(dgot - dwant).max() <= 1e-6 * np.abs(dwant).max()
    assert torch.equal(out, out2)


# ---- the loss kernel at the rows and sizes where it can go wrong ----------------------------------------------------------------
def edge_rows(rng):
    """[(kind, logits float32 [38], legal bool [38], label)]: one row of every kind test_loss_edges_match_float64 names"""
    f = np.float32
    rows = []

    def base():
        z = rng.normal(0, 2, 38).astype(f)
        m = rng.random(38) < 0.4
        m[0] = True
        return z, m

    for k in (2, 3):
        for where in ("first", "later", "neither"):
            z, m = base()
            idx = np.sort(rng.choice(38, k, replace=False))
            z[idx] = f(z.max() + f(1.5))                 # k equal largest logits, bit for bit
            m[idx] = True
            other = int(rng.choice([j for j in np.nonzero(m)[0] if j not in idx] or [j for j in range(38) if j not in idx]))
            rows.append((f"tie{k}_{where}", z, m, {"first": int(idx[0]), "later": int(idx[-1]), "neither": other}[where]))
    for label in (0, 5):
        z, m = base()
        z[:] = f(0.37)
        m[5] = True
        rows.append((f"all_equal_label{label}", z, m, label))
    z, m = base()
    m[:] = False
    m[7] = True
    rows.append(("single_legal", z, m, 7))
    z, m = base()
    m[11] = False
    z[11] = f(z.max() + f(100.0))
    rows.append(("illegal_100_above", z, m, int(rng.choice(np.nonzero(m)[0]))))
    z, m = base()
    m[[3, 9]] = True
    z[9] = f(z.max() + f(100.0))
    rows.append(("legal_100_above", z, m, 3))
    z, m = base()
    m[13] = False
    rows.append(("illegal_label", z, m, 13))
    z, m = base()
    z = (rng.choice([-60.0, 60.0], 38) * rng.random(38)).astype(f)
    rows.append(("magnitude_60", z, m, int(rng.choice(np.nonzero(m)[0]))))
    return rows


def edge_batch(B, rng):
    """(logits [B, 38] float32, mask bool, label int32, {kind: row indices}): test_loss_matches_float64's random rows with the
    rows of `edge_rows` at the head and, from 2 x their number on, again at the tail (the last staging round's rows)"""
    z = rng.normal(0, 4, (B, 38)).astype(np.float32)
    mask = rng.random((B, 38)) < 0.4
    mask[:, 0] = True
    label = np.array([rng.choice(np.nonzero(m)[0]) if i % 7 else rng.integers(0, 38) for i, m in enumerate(mask)], np.int32)
    kinds = {}
    edges = edge_rows(rng)
    starts = [0] + ([B - len(edges)] if B >= 2 * len(edges) else [])
    for s in starts:
        for i, (kind, zr, mr, lab) in enumerate(edges):
            z[s + i], mask[s + i], label[s + i] = zr, mr, lab
            kinds.setdefault(kind, []).append(s + i)
    return z, mask, label, kinds


def _run_loss(z, mask, label, ent_coef, grad=True):
    from brl_amd import sl
    B = z.shape[0]
    zs = torch.zeros((B, 40), device=DEV)            # a row stride larger than 38
    zs[:, :38] = torch.from_numpy(z)
    lt, mt = torch.from_numpy(label).to(DEV), torch.from_numpy(mask.astype(np.uint8)).to(DEV)
    out = torch.zeros(5, device=DEV)
    d = torch.full((B, 38), float("nan"), device=DEV) if grad else None
    sl.sl_loss(zs[:, :38], lt, mt, ent_coef, d, out)
    return out.cpu(), (d.cpu() if grad else None)


def check_loss_edges(z, mask, label, ent_coef, single_rows):
    """one batch of test_loss_edges_match_float64: every check but the derivative's bounds -> (per row: the kernel's derivative
    error over its yardstick max(loss32's error on that row, eps32 x the row's largest |d64|); the batch's worst row over loss32's
    worst row or that row's eps32 floor)"""
    eps32 = float(np.finfo(np.float32).eps)
    want, d64 = T.loss64(z.astype(np.float64), label, mask, ent_coef)
    _, d32 = T.loss32(z, label, mask, ent_coef)
    out, d = _run_loss(z, mask, label, ent_coef)
    out2, _ = _run_loss(z, mask, label, ent_coef, grad=False)
    got, dgot = out.double().numpy(), d.double().numpy()
    assert np.isfinite(dgot).all()
    assert np.allclose(got, want, rtol=1e-6, atol=1e-7), (got, want)
    assert np.float32(got[3]) == np.float32(want[3]), (got[3], want[3])            # accuracy: numpy's first-maximum rule, exactly
    assert torch.equal(out, out2)                                                  # the metrics-only call, bit for bit
    if len(single_rows):
        # a single legal call: its masked policy is one certain call — no entropy, no entropy term in the derivative
        _, d0 = _run_loss(z, mask, label, 0.0)
        assert torch.equal(d[single_rows], d0[single_rows])
        if z.shape[0] == 1:
            assert float(out[2]) == 0.0 and float(out[0]) == float(out[1])
    err = np.abs(dgot - d64).max(1)
    err32 = np.abs(d32.astype(np.float64) - d64).max(1)
    floor = eps32 * np.abs(d64).max(1)
    ratio = err / np.maximum(err32, floor)
    worst = int(np.argmax(err))
    return ratio, float(err[worst] / max(err32.max(), floor[worst]))


@pytest.mark.parametrize("ent_coef", [0.0, 0.01, 1.0])
@pytest.mark.parametrize("B", [1, 255, 256, 257, 512, 513])
def test_loss_edges_match_float64(B, ent_coef):
    """brl_sl_loss on 1, 255, 256, 257, 512 and 513 rows (the kernel stages 256 rows per round: last rounds of 255, 256 and 1 rows,
    one to three rounds) with, among random rows, at the head and at the tail of the batch: two and three tied largest logits with
    the label on the first, a later one and neither; 38 equal logits; a single legal call; an illegal logit 100 above every legal
    one; a legal logit 100 above the rest; an illegal label; +-60 logits.  B = 1 runs each kind alone.
      * the five outputs within rtol 1e-6 / atol 1e-7 of tests/sl_teacher.loss64; the accuracy exactly float64's (the ties are exact:
        numpy's first-maximum rule decides); the metrics-only call bit for bit the same five floats;
      * a single legal call: the derivative at any ent_coef is bit for bit the one at ent_coef = 0; alone in a batch, entropy 0;
      * the derivative PER ROW (asserted last, behind everything above): max_j |d - d64| <= 4 x max(max_j |d32 - d64|, eps32 max_j
        |d64|) with d32 = tests/sl_teacher.loss32, the same formulas in numpy float32 — a row of small derivatives is held to its own
        scale, not to the batch's largest; and the batch's worst row <= 4 x loss32's worst row (or that row's eps32 floor).
    Measured on the MI355X: the largest per-row ratio over the eighteen cases is 0.48 (a random row, B = 513, ent_coef 1), the
    batch's worst row at most 0.14 x loss32's worst row: the kernel takes the derivative in float64 and rounds once at the store.
    With the derivative in float32 — the formulas of loss32, device expf / logf, sums in column order — the bound was missed in
    twelve of the cases: 21.1 on the rows of 38 equal logits at ent_coef 1 (p (log p + H) is 0 in float64 and a few eps32 log(n) / n
    in float32, weighted 1 / B beside a target term of 1 / (38 B)), 8.4 on random rows at ent_coef 0 (the common error of log sum exp
    against a row whose largest |softmax - onehot| is well under 1), while the batch's worst row stayed within 1.93 x loss32's."""
    rng = np.random.default_rng(100 + B)
    if B == 1:
        edges = edge_rows(rng)
        results = [check_loss_edges(zr[None], mr[None], np.array([lab], np.int32), ent_coef, [0] if kind == "single_legal" else [])
                   for kind, zr, mr, lab in edges]
        per_row = {kind: round(float(r[0][0]), 3) for (kind, _, _, _), r in zip(edges, results)}
        print(f"B=1 ent_coef={ent_coef}: per-row ratios {per_row}")
        assert max(per_row.values()) <= 4, per_row
        return
    z, mask, label, kinds = edge_batch(B, rng)
    ratio, batch = check_loss_edges(z, mask, label, ent_coef, kinds["single_legal"])
    kind_of = {r: k for k, rows in kinds.items() for r in rows}
    over = {f"row {r} ({kind_of.get(r, 'random')})": round(float(ratio[r]), 3) for r in np.nonzero(ratio > 4)[0]}
    print(f"B={B} ent_coef={ent_coef}: worst per-row ratio {ratio.max():.3f} at row {int(np.argmax(ratio))} "
          f"({kind_of.get(int(np.argmax(ratio)), 'random')}), {len(over)} rows over 4: {over}; worst row over loss32's worst row {batch:.3f}")
    assert batch <= 4, batch
    assert not over, over


# ---- one SLStep against float64 ---------------------------------------------------------------------------------------------------
SL_STEP_CASES = [("DeepMind", "relu", 128), ("DeepMind", "tanh", 37), ("FAIR", "relu", 128), ("FAIR", "tanh", 37)]
SL_INIT_SEED, SL_PERTURB_SEED = 1, 22
SL_DATA_SEED = 18                # the 500-trajectory random set of every case
SL_STREAM_SEEDS = {}             # a case's stream seed: 5 unless that misses a cap of the input conditions
SL_ENT, SL_LR = 0.01, 1e-3
NEAR_TIE = 1e-5                  # a float64 top-two logit gap below this: fp32 may pick the other call
NEAR_TIE_CAP = 1                 # such rows per batch
SL_AMBIGUOUS_CAP = 1e-4          # of all ReLU gate entries of a step
SMALL_GRADIENT = 1e-4            # of the largest weight gradient: below it Adam's eps = 1e-8 is not negligible against |g|
SMALL_GRADIENT_CAP = 0.2         # the share of entries that may be so small


def sl_stream_seed(case):
    return SL_STREAM_SEEDS.get(tuple(case), 5)


def sl_step_net(model, activation, device):
    """`init(1)` with N(0, 0.01) added to every weight and N(0, 0.1) to every bias (drawn on the host: the CPU check of the cases'
    inputs sees the same network)"""
    from brl_amd.models import make_forward_pass
    from tests.nets import perturbed
    return perturbed(make_forward_pass(activation, model).init(SL_INIT_SEED), SL_PERTURB_SEED).to(device)


def sl_params_of(net, model):
    from tests.ppo_numpy import fair_params_of, params_of
    return fair_params_of(net) if model == "FAIR" else params_of(net)


def sl_lins(net, model):
    return (list(net.l) if model == "FAIR" else list(net.body)) + [net.actor, net.critic]


def sl_gate_entries(model, P, B):
    """ReLU gate entries of one step: B x 4 x 1024 (DeepMind), B x 12 x 200 (FAIR)"""
    return B * P[0][0].shape[0] * (12 if model == "FAIR" else len(P) - 2)


def sl_gate_fn(model, activation, P, stored, ambiguous):
    """the gate_fn of tests/test_gpu_update_float64.py for `model` (None under tanh): z > 0 except inside the fp32 rounding band of
    the pre-activation, where the gate is stored[...] (None: z > 0 all the same) and ambiguous[0] counts the entry"""
    from tests.test_gpu_update_float64 import deepmind_gate_fn, fair_gate_fn
    if activation != "relu":
        return None
    return (fair_gate_fn if model == "FAIR" else deepmind_gate_fn)(P, stored, ambiguous)


def sl_state_of(net, opt, model):
    """(P, M, V) float64 host copies of the parameters and Adam's moments (zeros where the optimizer holds none yet)"""
    lins = sl_lins(net, model)
    st = opt.state
    M = [tuple(_np(st[q]["exp_avg"]) if q in st else np.zeros(tuple(q.shape)) for q in (l.weight, l.bias)) for l in lins]
    V = [tuple(_np(st[q]["exp_avg_sq"]) if q in st else np.zeros(tuple(q.shape)) for q in (l.weight, l.bias)) for l in lins]
    return sl_params_of(net, model), M, V


def sl_stored_gates(net, obs, model):
    """the ReLU gates of a fp32 forward of `net` on obs, layer by layer as the step's own training forward runs it: one bool array
    per hidden layer (DeepMind) or per site of tests/ppo_numpy.fair_forward (FAIR)"""
    a = net.act
    outs = []

    def keep(v):
        outs.append(v)
        return v
    with torch.no_grad():
        x = obs
        if model != "FAIR":
            for lin in net.body:
                x = keep(a(lin(x)))
        else:
            L, inp = net.l, obs
            x = L[0](x); s1 = x
            x = keep(a(x)); x = keep(a(L[1](x))); x = keep(a(L[2](x))); x = x + s1; s2 = x
            x = keep(a(x)); x = keep(a(L[3](x))); x = keep(a(L[4](x))); x = x + s2
            x = torch.cat([L[5](x), inp], dim=-1)
            x = L[6](x); s3 = x
            x = keep(a(x)); x = keep(a(L[7](x))); x = keep(a(L[8](x))); x = x + s3; s4 = x
            x = keep(a(x)); x = keep(a(L[9](x))); x = keep(a(L[10](x)))
            assert len(outs) == 12
    return [(v > 0).cpu().numpy() for v in outs]


def small_gradient_share(G):
    """(per-entry masks like G of the entries Adam's tight parameter bound applies to, the share of the others).  The bound's
    derivation needs eps << |g|: it applies where |g64| >= SMALL_GRADIENT x the largest weight gradient — and where g64 is exactly 0
    (a never-set observation column, a unit ReLU switched off in every row, the value head: the step's gradient is the same exact
    zero, so the update depends on the moments alone and no division by |g| + eps amplifies anything)."""
    gmax = max(np.abs(gw).max() for gw, _ in G)
    big = [tuple((np.abs(g) >= SMALL_GRADIENT * gmax) | (g == 0) for g in pair) for pair in G]
    n = sum(b.size for pair in big for b in pair)
    return big, 1.0 - sum(int(b.sum()) for pair in big for b in pair) / n


def sl_reference_step(model, activation, P, M, V, t, obs, mask, label, stored):
    """the float64 reference of step t from state (P, M, V) on a batch -> (metrics row, G, P1, M1, V1, ambiguous gate entries)"""
    from tests.ppo_numpy import adam_step
    ambiguous = [0]
    gate_fn = sl_gate_fn(model, activation, P, stored, ambiguous)
    row, G = T.sl_step64(P, obs, mask, label, SL_ENT, activation, model, gate_fn)
    P1, M1, V1, _ = adam_step(None, t, P, M, V, G, lr=SL_LR, eps=1e-8, clip=False)
    return row, G, P1, M1, V1, ambiguous[0]


def accuracy_interval(P, obs, label, activation, model):
    """the float32 values the accuracy of float64 parameters P on a batch may take: rows whose top-two logit gap is below NEAR_TIE
    may fall either way -> (set of np.float32, number of such rows)"""
    logits, _ = T.logits64(P, obs, activation, model)
    tie = T.top_two_gap(logits) < NEAR_TIE
    sure = int(((np.argmax(logits, 1) == label) & ~tie).sum())
    B = logits.shape[0]
    return {np.float32(k / B) for k in range(sure, sure + int(tie.sum()) + 1)}, int(tie.sum())


def check_sl_step(tag, model, activation, net, opt, t, row, P, ref, batch, P_post):
    """the checks of test_sl_step_matches_float64 behind step t: row = the returned metrics row, P the parameters before the
    step, ref = sl_reference_step's result on `batch` = (obs, mask, label), P_post the float64 parameters the post-update
    accuracy is taken on"""
    want_row, G, P1, M1, V1, n_amb = ref
    obs, mask, label = batch
    B = obs.shape[0]
    lins = sl_lins(net, model)
    assert n_amb <= SL_AMBIGUOUS_CAP * sl_gate_entries(model, P, B), (tag, n_amb)
    for k in range(3):
        assert abs(float(row[k]) - want_row[k]) < 2e-5, (tag, k, float(row[k]), want_row[k])
    allowed, n_tie = accuracy_interval(P_post, obs, label, activation, model)
    assert n_tie <= NEAR_TIE_CAP and np.float32(row[3]) in allowed, (tag, float(row[3]), sorted(allowed), n_tie)
    # the gradients opt.step() left in place; the value head takes no part in the loss
    gmax = max(np.abs(gw).max() for gw, _ in G)
    errs = [(np.abs(_np(lin.weight.grad) - gw).max(), np.abs(_np(lin.bias.grad) - gb).max()) for lin, (gw, gb) in zip(lins[:-1], G[:-1])]
    for k, (ew, eb) in enumerate(errs):
        assert ew < 2e-5 * gmax + 1e-9 and eb < 2e-5 * gmax + 1e-9, (tag, k, ew, eb, gmax)
    for q in (net.critic.weight, net.critic.bias):
        assert q.grad is None or not bool(q.grad.any()), tag
    assert not G[-1][0].any() and not G[-1][1].any()
    # Adam (b1 0.9, b2 0.999, eps 1e-8, no clipping)
    gc = max(max(np.abs(gw).max(), np.abs(gb).max()) for gw, gb in G)
    vmax = max(np.abs(v_).max() for pair in V1 for v_ in pair)
    big, share = small_gradient_share(G)
    got = sl_params_of(net, model)
    st = opt.state
    worst_p = worst_small = worst_m = worst_v = moved = 0.0
    for lin, p1, m1, v1, p0, p_, bg in zip(lins, P1, M1, V1, P, got, big):
        for q, a, mm, vv, a0, b_, bb in zip((lin.weight, lin.bias), p1, m1, v1, p0, p_, bg):
            e = np.abs(b_ - a)
            worst_p = max(worst_p, e[bb].max(initial=0.0))
            worst_small = max(worst_small, e[~bb].max(initial=0.0))
            worst_m = max(worst_m, np.abs((_np(st[q]["exp_avg"]) if q in st else 0.0) - mm).max())
            worst_v = max(worst_v, np.abs((_np(st[q]["exp_avg_sq"]) if q in st else 0.0) - vv).max())
            moved = max(moved, np.abs(a - a0).max())
    print(f"{tag}: {n_amb} ambiguous gates, {n_tie} near ties, losses off by {max(abs(float(row[k]) - want_row[k]) for k in range(3)):.2e}, "
          f"worst gradient error {max(max(e) for e in errs):.2e} of {2e-5 * gmax + 1e-9:.2e}; parameters off by {worst_p / SL_LR:.4f} lr "
          f"(moved {moved / SL_LR:.2f} lr), {100 * share:.1f} % of entries under {SMALL_GRADIENT} gmax off by {worst_small / SL_LR:.3f} lr; "
          f"exp_avg by {worst_m:.2e} of {2e-5 * gc + 1e-12:.2e}, exp_avg_sq by {worst_v:.2e} of {4e-8 * gc * gc + 1e-6 * vmax:.2e}")
    assert share < SMALL_GRADIENT_CAP, (tag, share)
    assert worst_p < 0.02 * SL_LR and worst_small <= SL_LR and moved > 0.3 * SL_LR, (tag, worst_p, worst_small, moved)
    assert worst_m < 2e-5 * gc + 1e-12, (tag, worst_m, gc)
    assert worst_v < 4e-8 * gc * gc + 1e-6 * vmax, (tag, worst_v, gc, vmax)
    assert {int(s_["step"]) for s_ in st.values()} == {t}, tag


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("model, activation, B", SL_STEP_CASES)
def test_sl_step_matches_float64(model, activation, B, graph, oracle):
    """Five steps of ``SLStep`` (entropy_coef 0.01, lr 1e-3, steps_per_graph 2) on a 500-trajectory random set, from a network whose
    every parameter is perturbed (no bias is hk.Linear's zero) — through the graphs (``run``) and without them (``eager``).  Steps
    1, 2, 3 run one at a time; the float64 reference of step t (tests/sl_teacher.sl_step64 + tests/ppo_numpy.adam_step with eps
    1e-8 and no clipping) starts from the device's own parameters and moments, copied to the host before the step, so errors do not
    build up.  Steps 4 and 5 are ONE ``run(2)`` (one replay of the 2-step graph) / ``eager(2)``: row 0 against the reference from
    the device's state before it, row 1 against the reference continued from row 0's float64 update, on the batches
    tests/sl_teacher.sample + host_batch say the stream holds there — a row taken from another step, or from behind the update,
    is seen here.  After each step:
      * the batch: ``st.b.traj / pos`` are examples (t - 1) B .. t B - 1 of the stream's numpy restatement, ``obs / mask / label``
        the oracle's rows of them (host_batch), the counter is t B;
      * the metrics row: total, target and entropy within 2e-5 of float64 on the PRE-update parameters; the accuracy is float64's
        on the POST-update parameters (FAIR: the no-grad forward is brl_fair_forward on parameters a replayed graph just wrote).
        A row whose float64 top-two logit gap is under 1e-5 may fall either way: at most 1 per batch, and the accuracy must be one
        of the values they allow;
      * every ``p.grad`` left behind ``opt.step()`` within 2e-5 max|gW| + 1e-9 of float64 (test_gpu_update_float64's bound); the
        value head's are None or exactly zero;
      * parameters, exp_avg and exp_avg_sq against ``adam_step(t)`` on the float64 gradients with test_gpu_update_float64's bounds
        (its docstring derives them): 0.02 lr (and moved > 0.3 lr), 2e-5 gc + 1e-12, 4e-8 gc^2 + 1e-6 max|v|.  The parameter bound's
        derivation takes eps as negligible against |g|, which eps = 1e-8 is not on gradients near zero: it is applied where |g64|
        >= 1e-4 max|gW| and where g64 is exactly 0 (structural zeros — a quarter of a ReLU net's entries: the step's own gradient
        is the same exact zero, nothing is divided by it); the other entries are within lr, and they are fewer than 20 % of all.
    ReLU gates: where a float64 pre-activation is within its fp32 rounding band of 0 (deepmind_gate_fn / fair_gate_fn of
    tests/test_gpu_update_float64.py) the gate is that of a fp32 layer-by-layer forward of the pre-update parameters on the step's
    batch; such entries are fewer than 1e-4 of all.  The caps on ambiguous gates, near ties and small gradients are conditions on
    the inputs: tests/test_sl_host.py evaluates them for step 1 of every case without a GPU.
    Measured on the MI355X over all cases and steps (graph and eager agree to the digit): at most 19 of 524288 (DeepMind) and 6 of
    307200 (FAIR) ambiguous gates, none under tanh; no near tie; losses off by <= 3.8e-7; gradients by <= 3 % of their bound;
    parameters by <= 0.0005 lr where the tight bound applies; between 0.8 % (FAIR tanh) and 17.8 % (DeepMind ReLU, step 3) of the
    entries under 1e-4 max|gW|, off by <= 0.014 lr; exp_avg by <= 0.8 %, exp_avg_sq by <= 15 % of their bounds.  No float32 rounding
    of the reference came near a bound, so none is raised."""
    from brl_amd import sl
    ts, data = _set(500, seed=SL_DATA_SEED)
    seed = sl_stream_seed((model, activation, B))
    net = sl_step_net(model, activation, DEV)
    opt = sl.make_optimizer(net, SL_LR)
    st = sl.SLStep(net, opt, data, B, seed, SL_ENT, steps_per_graph=2, graph=graph)
    assert int(st.counter.item()) == 0
    steps = st.run if graph else st.eager

    def device_batch(t):
        traj, pos = T.sample(ts.offsets, seed, (t - 1) * B, B)
        assert np.array_equal(st.b.traj.cpu().numpy(), traj) and np.array_equal(st.b.pos.cpu().numpy(), pos), t
        obs, mask, label = T.host_batch(ts, traj, pos, oracle)
        assert np.array_equal(st.b.obs.cpu().numpy(), obs) and np.array_equal(st.b.mask.cpu().numpy(), mask), t
        assert np.array_equal(st.b.label.cpu().numpy(), label), t
        assert int(st.counter.item()) == t * B
        return obs, mask, label

    for t in (1, 2, 3):
        P, M, V = sl_state_of(net, opt, model)
        before = copy.deepcopy(net)
        row = steps(1).cpu().numpy()[0]
        batch = device_batch(t)
        stored = sl_stored_gates(before, st.b.obs, model) if activation == "relu" else None
        ref = sl_reference_step(model, activation, P, M, V, t, *batch, stored)
        check_sl_step(f"{model} {activation} B={B} {'graph' if graph else 'eager'} t={t}", model, activation, net, opt, t, row, P, ref,
                      batch, sl_params_of(net, model))
    # steps 4 and 5 in one call
    P, M, V = sl_state_of(net, opt, model)
    before = copy.deepcopy(net)
    rows = steps(2).cpu().numpy()
    assert rows.shape == (2, 4)
    traj4, pos4 = T.sample(ts.offsets, seed, 3 * B, B)
    batch4 = T.host_batch(ts, traj4, pos4, oracle)
    obs4 = torch.from_numpy(batch4[0]).to(DEV)
    ref4 = sl_reference_step(model, activation, P, M, V, 4, *batch4, sl_stored_gates(before, obs4, model) if activation == "relu" else None)
    want4, _, P4, M4, V4, amb4 = ref4
    assert amb4 <= SL_AMBIGUOUS_CAP * sl_gate_entries(model, P, B)
    for k in range(3):
        assert abs(float(rows[0, k]) - want4[k]) < 2e-5, ("row 0", k, float(rows[0, k]), want4[k])
    allowed, n_tie = accuracy_interval(P4, batch4[0], batch4[2], activation, model)
    assert n_tie <= NEAR_TIE_CAP and np.float32(rows[0, 3]) in allowed, ("row 0", float(rows[0, 3]), sorted(allowed))
    batch5 = device_batch(5)
    with torch.no_grad():   # the fp32 network the float64 state behind row 0 rounds to: its gates stand for the device's
        for lin, (W, b) in zip(sl_lins(before, model), P4):
            lin.weight.copy_(torch.from_numpy(W)); lin.bias.copy_(torch.from_numpy(b))
    stored = sl_stored_gates(before, st.b.obs, model) if activation == "relu" else None
    ref5 = sl_reference_step(model, activation, P4, M4, V4, 5, *batch5, stored)
    check_sl_step(f"{model} {activation} B={B} {'graph' if graph else 'eager'} t=5 (row 1 of 2)", model, activation, net, opt, 5, rows[1],
                  P4, ref5, batch5, sl_params_of(net, model))


def _make(model, seed, data, S, graph, lr=1e-3, B=128):
    from brl_amd import sl
    from brl_amd.models import make_forward_pass
    net = make_forward_pass("relu", model).init(seed, device=DEV)
    opt = sl.make_optimizer(net, lr)
    return net, sl.SLStep(net, opt, data, B, seed, 0.01, steps_per_graph=S, graph=graph)


@pytest.mark.parametrize("model", ["DeepMind", "FAIR"])
def test_graph_replay_equals_one_step_replays_and_eager(model):
    _, data = _set(500, seed=13, kind="teacher")
    net0, _ = _make(model, 1, data, 8, graph=False)
    nets, rows = [], []
    for mode in ("graph8", "graph1", "eager"):
        net, st = _make(model, 1, data, 8, graph=(mode != "eager"))
        if mode == "graph8":
            r = torch.cat([st.run(8).clone() for _ in range(2)])
        elif mode == "graph1":
            r = torch.cat([st.run(1).clone() for _ in range(16)])
        else:
            r = st.eager(16)
        torch.cuda.synchronize()
        nets.append(net)
        rows.append(r.cpu())
        assert int(st.counter.item()) == 16 * 128
    for net, r in zip(nets[1:], rows[1:]):
        assert torch.equal(r, rows[0])
        for a, b in zip(nets[0].parameters(), net.parameters()):
            assert torch.equal(a, b)
    for net in nets:   # the value head gets no gradient
        assert torch.equal(net.critic.weight, net0.critic.weight) and torch.equal(net.critic.bias, net0.critic.bias)
        assert not torch.equal(net.actor.weight, net0.actor.weight)


@pytest.mark.parametrize("model, steps, floor", [("DeepMind", 500, 0.9), ("FAIR", 300, 0.85)])
def test_it_learns_a_synthetic_teacher(model, steps, floor):
    from brl_amd import sl
    _, train = _set(2000, seed=14, kind="teacher")
    _, test = _set(500, seed=15, kind="teacher")
    net, st = _make(model, 0, train, 8, graph=True)
    before = sl.evaluate_all(net, test)["accuracy"]
    for _ in range(steps // 8):
        st.run(8)
    after = sl.evaluate_all(net, test)
    assert before < 0.2 and after["accuracy"] >= floor, (before, after)


# ---- the evaluators -----------------------------------------------------------------------------------------------------------------
METRIC_KEYS = ("total_loss", "target_loss", "entropy", "accuracy", "illegal_actions_prob")


def check_metrics(got, P, batch, ent_coef, activation, model, what):
    """five metrics (total, target, entropy, accuracy, illegal mass) within 2e-5 of sl_step64's row on the batch; rows with a top-two
    gap under NEAR_TIE (at most one) may count either way in the accuracy"""
    obs, mask, label = batch
    want, _ = T.sl_step64(P, obs, mask, label, ent_coef, activation, model)
    logits, _ = T.logits64(P, obs, activation, model)
    n_tie = int((T.top_two_gap(logits) < NEAR_TIE).sum())
    assert n_tie <= NEAR_TIE_CAP, (what, n_tie)
    for k in (0, 1, 2, 4):
        assert abs(got[k] - want[k]) < 2e-5, (what, k, got[k], want[k])
    assert abs(got[3] - want[3]) < 2e-5 + n_tie / obs.shape[0], (what, got[3], want[3])


@pytest.mark.parametrize("model, activation", [("FAIR", "tanh"), ("DeepMind", "relu")])
def test_evaluate_pairs_is_the_examples_mean_over_chunks(model, activation, oracle):
    """``evaluate_pairs`` on 257 examples that are not in file order, in chunks of 100 (100 + 100 + 57: the chunk means weighted by
    their sizes): all five metrics within 2e-5 of float64 (tests/sl_teacher.sl_step64 on the oracle's rows of the same examples)
    and within 1e-6 of the one-chunk call; ``evaluate_all`` is ``evaluate_pairs`` on ``decision_points``."""
    from brl_amd import sl, sl_data
    ts, data = _set(60, seed=23)
    rng = np.random.default_rng(24)
    traj = rng.integers(0, ts.n, 257)
    pos = (rng.random(257) * ts.n_calls()[traj]).astype(np.int32)
    assert (np.diff(traj) < 0).any()
    net = sl_step_net(model, activation, DEV)
    P = sl_params_of(net, model)
    tt, pp = torch.from_numpy(traj).to(DEV), torch.from_numpy(pos).to(DEV)
    chunked = sl.evaluate_pairs(net, data, tt, pp, 0.01, chunk=100)
    whole = sl.evaluate_pairs(net, data, tt, pp, 0.01, chunk=65536)
    assert tuple(chunked) == tuple(whole) == METRIC_KEYS
    check_metrics([chunked[k] for k in METRIC_KEYS], P, T.host_batch(ts, traj, pos, oracle), 0.01, activation, model, "chunk=100")
    for k in METRIC_KEYS:
        assert abs(chunked[k] - whole[k]) < 1e-6, (k, chunked[k], whole[k])
    every = sl_data.decision_points(ts)
    assert sl.evaluate_all(net, data, 0.01) == sl.evaluate_pairs(net, data, torch.from_numpy(every[0]).to(DEV),
                                                                  torch.from_numpy(every[1]).to(DEV), 0.01)


@pytest.mark.parametrize("model, activation", [("FAIR", "tanh"), ("DeepMind", "relu")])
def test_eval_stream_draws_its_own_examples(model, activation, oracle):
    """``EvalStream`` with batch 100 on a 60-trajectory set (the second call crosses an epoch): each ``next`` leaves examples
    100 k .. 100 k + 99 of the numpy stream of ITS seed in its buffers, the oracle's rows of them, the counter at 100 (k + 1), and
    returns the five ``test/...`` metrics within 2e-5 of float64."""
    from brl_amd import sl
    ts, data = _set(60, seed=25)
    net = sl_step_net(model, activation, DEV)
    P = sl_params_of(net, model)
    ev = sl.EvalStream(data, 100, seed=9)
    for k in range(2):
        m = ev.next(net, 0.01)
        assert list(m) == ["test/total_loss", "test/target_loss", "test/entropy", "test/test_accuracy", "test/illegal_actions_prob"]
        assert int(ev.counter.item()) == 100 * (k + 1)
        traj, pos = T.sample(ts.offsets, 9, 100 * k, 100)
        assert np.array_equal(ev.b.traj.cpu().numpy(), traj) and np.array_equal(ev.b.pos.cpu().numpy(), pos), k
        batch = T.host_batch(ts, traj, pos, oracle)
        for got, want in zip((ev.b.obs, ev.b.mask, ev.b.label), batch):
            assert np.array_equal(got.cpu().numpy(), want), k
        check_metrics(list(m.values()), P, batch, 0.01, activation, model, f"next {k}")
    assert (99 // ts.n, 100 // ts.n, 199 // ts.n) == (1, 1, 3)     # (both calls cross an epoch of the 60 trajectories)


@pytest.mark.parametrize("max_samples", [3, 1000])
def test_output_samples_show_the_first_differing_call(max_samples, oracle):
    """``output_samples`` of an untrained (perturbed) DeepMind net on a 40-trajectory set, trajectories in a fixed RandomState's
    order: it returns min(max_samples, trajectories with a differing call); every block's auction and "Ground truth" are the calls
    before, and the recorded call at, the first position where the float64 argmax differs from the record; its five listed calls
    are the float64 top five in order.  Condition on the inputs: no position of the set has a top-two gap under 1e-5 (an argmax
    fp32 may decide otherwise); a top-five order is compared only where the six largest logits are 1e-5 apart."""
    from brl_amd import sl, sl_data
    from brl_amd.sl_data import CALL_NAMES
    ts, data = _set(40, seed=26)
    net = sl_step_net("DeepMind", "relu", DEV)
    P = sl_params_of(net, "DeepMind")
    blocks = []
    count = sl.output_samples(net, data, max_samples, np.random.RandomState(7), out=blocks.append)
    traj, pos = sl_data.decision_points(ts)
    obs, _, label = T.host_batch(ts, traj, pos, oracle)
    logits, _ = T.logits64(P, obs, "relu", "DeepMind")
    assert not (T.top_two_gap(logits) < NEAR_TIE).any()
    want = []
    for t in np.random.RandomState(7).permutation(ts.n):
        lo, hi = int(ts.offsets[t]), int(ts.offsets[t + 1])
        differs = np.nonzero(np.argmax(logits[lo:hi], 1) != label[lo:hi])[0]
        if differs.size:
            want.append((int(t), int(differs[0])))
    assert len(want) > 3 and count == len(blocks) == min(max_samples, len(want))
    for (t, k), block in zip(want, blocks):
        lines = block.split("\n")
        calls = ts.calls[ts.offsets[t]:ts.offsets[t + 1]]
        assert lines[0].startswith(f"Seat {'NESW'[k % 4]} to call")
        assert lines[1] == f"  hand: {sl_data.hand_string(ts.hands[t, k % 4])}"
        assert lines[2] == "  auction: " + (" ".join(CALL_NAMES[c] for c in calls[:k]) or "(none)")
        assert lines[8] == f"Ground truth {CALL_NAMES[calls[k]]}" and len(lines) == 10
        z = logits[ts.offsets[t] + k]
        top = np.argsort(-z, kind="stable")
        if (np.diff(-z[top[:6]]) >= NEAR_TIE).all():
            assert [ln.split()[0] for ln in lines[3:8]] == [CALL_NAMES[a] for a in top[:5]], (t, k)
        p = np.exp(z - z.max()) / np.exp(z - z.max()).sum()
        assert all(abs(float(ln.split()[1]) - p[a]) < 0.006 for ln, a in zip(lines[3:8], top[:5]))


def test_train_sl_splits_graph_replays_around_evaluations(tmp_path, monkeypatch):
    """``train_sl`` in-process, 20 iterations, an evaluation every 8, 8 steps per graph: the replays are 8 + 8 + 4 one-step ones
    (k = min(S, iterations - i, eval_every - i % eval_every)); steps 0 .. 19 are each logged once, in order; evaluations are
    logged at steps 7 and 15 only, each before its step's own row; params-8.pkl and params-16.pkl are written; the train stream
    ends at 20 x 32 examples."""
    from brl_amd import sl
    data_dir, save = tmp_path / "data", tmp_path / "save"
    data_dir.mkdir()
    (data_dir / "train.txt").write_text(T.random_file(100, seed=27, kind="teacher"))
    (data_dir / "test.txt").write_text(T.random_file(40, seed=28, kind="teacher"))
    made, ks = [], []

    class Recorded(sl.SLStep):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)

        def run(self, k):
            ks.append(k)
            return super().run(k)
    monkeypatch.setattr(sl, "SLStep", Recorded)
    logs = []
    cfg = dict(data_path=str(data_dir), save_path=str(save), iterations=20, eval_every=8, train_batch=32, eval_batch=64, num_examples=1)
    sl.train_sl(cfg, log=logs.append, steps_per_graph=8)
    assert ks == [8, 8, 4] and len(made) == 1 and made[0].S == 8 and made[0].B == 32
    assert int(made[0].counter.item()) == 20 * 32
    dicts = [m for m in logs if isinstance(m, dict)]
    train = [m for m in dicts if "train/total_loss" in m]
    evals = [m for m in dicts if "test/test_accuracy" in m]
    assert [m["step"] for m in train] == list(range(20))
    assert all(set(m) == {"step", "train/total_loss", "train/target_loss", "train/entropy", "train/train_accuracy"} for m in train)
    assert [m["step"] for m in evals] == [7, 15]
    assert all(set(m) == {"step", "test/total_loss", "test/target_loss", "test/entropy", "test/test_accuracy",
                          "test/illegal_actions_prob"} for m in evals)
    order = [("eval" if "test/test_accuracy" in m else "train", m["step"]) for m in dicts if "step" in m]
    assert order.index(("eval", 7)) == order.index(("train", 7)) - 1 and order.index(("eval", 15)) == order.index(("train", 15)) - 1
    assert dicts[-1]["steps"] == 20 and len(dicts) == 23
    assert sorted(os.listdir(save)) == ["params-16.pkl", "params-8.pkl"]


def test_cli_end_to_end(tmp_path):
    from brl_amd import checkpoint, sl
    data_dir, save = tmp_path / "data", tmp_path / "save"
    data_dir.mkdir()
    (data_dir / "train.txt").write_text(T.random_file(300, seed=16, kind="teacher"))
    (data_dir / "test.txt").write_text(T.random_file(100, seed=17, kind="teacher"))
    args = [f"data_path={data_dir}", f"save_path={save}", "iterations=40", "eval_every=20", "train_batch=64", "eval_batch=256",
            "num_examples=1"]
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "brl_amd.sl"] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(os.listdir(save)) == ["params-20.pkl", "params-40.pkl"]
    for key in ("train/total_loss", "train/target_loss", "train/entropy", "train/train_accuracy", "test/test_accuracy",
                "test/total_loss", "test/target_loss", "test/entropy", "test/illegal_actions_prob", "Ground truth"):
        assert key in r.stdout, key
    from brl_amd.train import parse_cli
    cfg = parse_cli(args, defaults=sl.SL_DEFAULTS)
    net = sl.train_sl(cfg, log=lambda m: None)
    loaded = checkpoint.load_params(str(save / "params-40.pkl"), "relu", "DeepMind", DEV)
    x = (torch.rand((64, 480), device=DEV) < 0.1).float()
    with torch.no_grad():
        assert torch.allclose(loaded(x)[0], net(x)[0], rtol=1e-6, atol=1e-6)
