"""Policy distillation: a student fitted to the masked policy and the value of an ensemble of K teachers, on the positions a
behaviour policy reaches at the table (include/brl_distill.h holds the definition).

``python -m brl_amd.distill teacher_model_path=a.pt,b.pkl save_path=DIR [key=value ...]`` (``DISTILL_DEFAULTS``).  It changes a
trained network's architecture (a 4 x 1024 DeepMind bidder as the 200-wide FAIR net, or back), merges a population into the one
network that bids like the mixture, and pre-trains without recorded auctions.  Every ``eval_every`` iterations it writes
``save_path/params-{iteration}.pkl`` (``sl.save_pickle``), which ``brl_amd.train`` (``initial_model_path``), ``eval``, ``league``
and ``crossplay`` read.

One iteration: ``make_roll_out`` (competitive, masked) collects ``num_steps x num_envs`` positions — the actor is the behaviour
network, the opponent a teacher, cycling through the ensemble by iteration; only ``obs`` and ``legal_action_mask`` are used —,
``teacher_heads`` runs every teacher on them, ``brl_distill_targets`` forms q, v* and the teachers' entropy once for all rows, and
``DistillStep`` runs ``update_epochs`` passes of minibatches: S steps (gather, forward, ``brl_distill_loss`` with the gradient,
backward through the layers, Adam) per hipGraph; torch differentiates the network's layers only.
"""
from __future__ import annotations

import os
import sys
import time

import numpy as np
import torch

from . import _capi
from ._capi import NUM_ACTIONS, OBS_SIZE, device_index, stream
from ._capture import capture_each, preserved, warm_up
from .models import InferenceSnapshot, make_forward_pass
from .sl import make_optimizer, save_pickle

MAX_TEACHERS = 8     # BRL_DISTILL_MAX_TEACHERS
BLOCK = 64           # BRL_DISTILL_BLOCK
METRICS = ("total", "policy_loss", "value_loss", "teacher_entropy", "student_entropy", "agreement", "illegal_actions_prob")

DISTILL_DEFAULTS = dict(
    teacher_model_path=None, teacher_weights=None, teacher_model_type="DeepMind", teacher_activation="relu",
    type_of_model="FAIR", activation="relu", initial_model_path=None,
    dds_path="dds_results/train_000.npy", num_envs=8192, num_steps=32, iterations=100, update_epochs=2, minibatch_size=1024,
    learning_rate=1e-4, tau=1.0, policy_coef=1.0, value_coef=0.5, behaviour="teacher", teacher_iterations=10,
    eval_every=10, num_eval_envs=1000, save_path=None, rng_seed=42,
)


def mixture_weights(weights, k: int) -> np.ndarray:
    """the K mixture weights as the kernels take them: positive, normalised in float64 to sum 1, then float32.  ``weights``: None
    (uniform), a sequence, or a comma list"""
    if weights is None:
        w = np.ones(k, np.float64)
    else:
        w = np.asarray([float(x) for x in weights.split(",")] if isinstance(weights, str) else weights, np.float64).reshape(-1)
    if w.shape[0] != k or not 1 <= k <= MAX_TEACHERS:
        raise ValueError(f"{w.shape[0]} weights for {k} teachers (1 .. {MAX_TEACHERS})")
    if not (np.isfinite(w).all() and (w > 0).all()):
        raise ValueError("mixture weights are finite and > 0")
    return (w / w.sum()).astype(np.float32)


def work_doubles(batch: int) -> int:
    """doubles of ``brl_distill_loss``'s workspace for a batch: 8 per block of 64 rows"""
    return 8 * ((int(batch) + BLOCK - 1) // BLOCK)


def _u8(mask):
    return mask.view(torch.uint8) if mask.dtype == torch.bool else mask


# ---- the two entry points -----------------------------------------------------------------------------------------------------
def distill_targets(t_logits, t_values, weights, mask, tau: float, q, vstar, hq) -> None:
    """one ``brl_distill_targets`` launch.  t_logits float32 [K, n, 38] and t_values float32 [K, n], views of any strides with
    unit stride along the calls (``heads[:, :, :38]``, ``heads[:, :, 38]`` of ``teacher_heads``); weights float32 [K]
    (``mixture_weights``); mask bool / uint8 [n, 38]; q [n, 38], vstar [n], hq [n] float32"""
    k, n = t_logits.shape[0], t_logits.shape[1]
    assert t_logits.dtype == torch.float32 and t_values.dtype == torch.float32 and t_logits.stride(2) == 1
    assert t_values.shape == (k, n) and weights.shape == (k,) and weights.dtype == torch.float32 and mask.shape == (n, NUM_ACTIONS)
    assert q.shape == (n, NUM_ACTIONS) and vstar.shape == (n,) and hq.shape == (n,)
    di = device_index(q)
    _capi.check(_capi.lib().brl_distill_targets(di, t_logits.data_ptr(), t_logits.stride(0), t_logits.stride(1), t_values.data_ptr(),
                                                 t_values.stride(0), t_values.stride(1), _capi.ptr(weights), _capi.ptr(_u8(mask)), n, k,
                                                 float(tau), _capi.ptr(q), _capi.ptr(vstar), _capi.ptr(hq), stream(di)))


def distill_loss(z, u, q, vstar, hq, mask, tau: float, c_pol: float, c_val: float, dz, du, out, work=None) -> None:
    """``brl_distill_loss``: z float32 [B, 38] (any row stride) and u float32 [B] (any stride) of the student, q / vstar / hq of
    ``distill_targets``, mask bool / uint8 [B, 38]; dz [B, 38] and du [B] (both None: metrics only); out float32 [8]; work
    float64 [``work_doubles(B)``] (allocated here when None)"""
    b = z.shape[0]
    assert z.dtype == torch.float32 and u.dtype == torch.float32 and z.stride(1) == 1 and u.shape == (b,) and mask.shape == (b, NUM_ACTIONS)
    assert q.shape == (b, NUM_ACTIONS) and vstar.shape == (b,) and hq.shape == (b,) and out.shape == (8,)
    if work is None:
        work = torch.empty(work_doubles(b), dtype=torch.float64, device=z.device)
    assert work.dtype == torch.float64 and work.numel() >= work_doubles(b)
    di = device_index(z)
    _capi.check(_capi.lib().brl_distill_loss(di, z.data_ptr(), z.stride(0), u.data_ptr(), u.stride(0), _capi.ptr(q), _capi.ptr(vstar),
                                              _capi.ptr(hq), _capi.ptr(_u8(mask)), b, float(tau), float(c_pol), float(c_val), _capi.ptr(dz),
                                              _capi.ptr(du), _capi.ptr(out), _capi.ptr(work), stream(di)))


# ---- forwards -----------------------------------------------------------------------------------------------------------------
def _heads_into(net, snap, obs_bool, out, chunk):
    for i in range(0, obs_bool.shape[0], chunk):
        o = obs_bool[i:i + chunk]
        if snap is not None:
            out[i:i + chunk].copy_(snap.heads(o))
        else:
            logits, value = net(o.float())
            out[i:i + chunk, :NUM_ACTIONS].copy_(logits)
            out[i:i + chunk, NUM_ACTIONS].copy_(value)


def teacher_heads(teachers, obs_bool, out=None, chunk: int = 65536):
    """each teacher's heads of obs_bool bool [n, 480] -> out float32 [K, n, 39] (38 logits, then the value), in chunks, without
    autograd: ``InferenceSnapshot.heads`` — whichever inference route the row count selects, as in the evaluators — where a
    snapshot covers the teacher, else the module.  Teachers that are the same object share one forward."""
    k, n = len(teachers), obs_bool.shape[0]
    if out is None:
        out = torch.empty((k, n, NUM_ACTIONS + 1), dtype=torch.float32, device=obs_bool.device)
    assert out.shape == (k, n, NUM_ACTIONS + 1) and out.dtype == torch.float32
    first = {}
    with torch.no_grad():
        for i, t in enumerate(teachers):
            if id(t) in first:
                out[i].copy_(out[first[id(t)]])
                continue
            first[id(t)] = i
            _heads_into(t, InferenceSnapshot.make(t, views=True), obs_bool, out[i], chunk)
    return out


def ensemble_targets(teachers, weights, obs_bool, mask, tau: float, q, vstar, hq, heads=None, chunk: int = 65536):
    """``teacher_heads``, then one ``brl_distill_targets`` over all rows, into q / vstar / hq; returns the heads"""
    heads = teacher_heads(teachers, obs_bool, heads, chunk)
    distill_targets(heads[:, :, :NUM_ACTIONS], heads[:, :, NUM_ACTIONS], weights, mask, tau, q, vstar, hq)
    return heads


def distill_evaluate(student, teachers, obs, mask, weights=None, tau: float = 1.0, policy_coef: float = 1.0, value_coef: float = 0.5,
                     chunk: int = 65536) -> dict:
    """the metrics row of explicit positions as a dict (``METRICS``): obs bool [n, 480], mask bool / uint8 [n, 38]"""
    dev, n = obs.device, obs.shape[0]
    w = torch.from_numpy(mixture_weights(weights, len(teachers))).to(dev)
    f = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)     # noqa: E731
    q, vstar, hq, own, out = f(n, NUM_ACTIONS), f(n), f(n), f(n, NUM_ACTIONS + 1), f(8)
    ensemble_targets(teachers, w, obs, mask, tau, q, vstar, hq, chunk=chunk)
    with torch.no_grad():
        _heads_into(student, None, obs, own, chunk)
    distill_loss(own[:, :NUM_ACTIONS], own[:, NUM_ACTIONS], q, vstar, hq, mask, tau, policy_coef, value_coef, None, None, out)
    return dict(zip(METRICS, out.cpu().numpy().tolist()))


# ---- the step -----------------------------------------------------------------------------------------------------------------
class DistillStep:
    """S minibatch steps per hipGraph replay over a collected set of at most ``capacity`` rows, held in this object's own
    buffers (a captured graph keeps their addresses): ``data_obs`` bool [capacity, 480], ``data_mask`` uint8 [capacity, 38],
    ``data_q`` / ``data_vstar`` / ``data_hq`` — written by the caller (``ensemble_targets`` straight into them) — and ``perm``, the
    epoch's device permutation with its ``cursor``.  One step: gather rows perm[cursor .. cursor + B) into the static [B, 480]
    observation, forward, ``brl_distill_loss`` with the gradient (metrics row ``rows[s]``, before the update),
    ``torch.autograd.backward([logits, value], [dz, du])``, fused capturable Adam, cursor += B.  Both heads learn.  A run of
    k < S steps replays a 1-step graph k times."""

    def __init__(self, net, opt, batch: int, capacity: int, tau: float = 1.0, policy_coef: float = 1.0, value_coef: float = 0.5,
                 steps_per_graph: int = 8, graph: bool = True):
        self.net, self.opt = net, opt
        self.B, self.cap, self.S = int(batch), int(capacity), int(steps_per_graph)
        self.tau, self.c_pol, self.c_val = float(tau), float(policy_coef), float(value_coef)
        assert 1 <= self.B <= self.cap
        dev = next(net.parameters()).device
        f = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)     # noqa: E731
        self.data_obs = torch.zeros((self.cap, OBS_SIZE), dtype=torch.bool, device=dev)
        self.data_mask = torch.zeros((self.cap, NUM_ACTIONS), dtype=torch.uint8, device=dev)
        self.data_q, self.data_vstar, self.data_hq = f(self.cap, NUM_ACTIONS), f(self.cap), f(self.cap)
        self.data_mask[:, 0] = 1     # (warm-up and capture read the buffers as they are: a finite loss on Pass alone)
        self.data_q[:, 0] = 1.0
        self.perm = torch.zeros(self.cap, dtype=torch.int64, device=dev)
        self.cursor = torch.zeros(1, dtype=torch.int64, device=dev)
        self.lane = torch.arange(self.B, dtype=torch.int64, device=dev)
        self.obs = f(self.B, OBS_SIZE)
        self.dz, self.du = f(self.B, NUM_ACTIONS), f(self.B)
        self.work = torch.zeros(work_doubles(self.B), dtype=torch.float64, device=dev)
        self.rows = f(self.S, 8)
        self.graphs = {}
        if graph:
            self._capture()

    def _step(self, s: int):
        idx = self.perm.index_select(0, self.cursor + self.lane)
        self.obs.copy_(self.data_obs.index_select(0, idx))
        mask, q = self.data_mask.index_select(0, idx), self.data_q.index_select(0, idx)
        vstar, hq = self.data_vstar.index_select(0, idx), self.data_hq.index_select(0, idx)
        logits, value = self.net(self.obs)
        distill_loss(logits, value, q, vstar, hq, mask, self.tau, self.c_pol, self.c_val, self.dz, self.du, self.rows[s], self.work)
        self.opt.zero_grad(set_to_none=False)
        torch.autograd.backward([logits, value], [self.dz, self.du])
        self.opt.step()
        self.cursor.add_(self.B)

    def _steps(self, k: int):
        for s in range(k):
            self._step(s)

    def _capture(self):
        # warm-up and capture run the real step: parameters, optimizer state and the cursor are put back afterwards
        ks = sorted({1, self.S})
        with preserved(self.net.parameters(), self.opt, tensors=(self.cursor,)):
            warm_up(lambda: (self.cursor.zero_(), self._step(0)), 3)
            self.cursor.zero_()
            self.graphs = dict(zip(ks, capture_each([lambda k=k: self._steps(k) for k in ks])))

    def load(self, obs_bool, mask, q, vstar, hq) -> int:
        """copies a collected set into the buffers (a caller may instead write ``data_*[:n]`` itself); -> its rows"""
        n = obs_bool.shape[0]
        assert n <= self.cap
        self.data_obs[:n].copy_(obs_bool)
        self.data_mask[:n].copy_(_u8(mask))
        self.data_q[:n].copy_(q)
        self.data_vstar[:n].copy_(vstar)
        self.data_hq[:n].copy_(hq)
        return n

    def shuffle(self, n: int, generator) -> int:
        """a new epoch over rows 0 .. n - 1: ``perm[:n]`` from ``generator`` (a seeded device generator), cursor 0; -> the
        epoch's steps, n // B (the permutation's tail is left out)"""
        assert self.B <= n <= self.cap
        self.perm[:n].copy_(torch.randperm(n, generator=generator, device=self.perm.device))
        self.cursor.zero_()
        return n // self.B

    def run(self, k: int):
        """k <= S steps: one S-step replay when k == S, else k 1-step replays.  Returns the device metrics rows [k, 8] (before each
        update); reading them is the caller's choice."""
        assert 1 <= k <= self.S
        if k == self.S:
            self.graphs[self.S].replay()
            return self.rows
        rows = []
        for _ in range(k):
            self.graphs[1].replay()
            rows.append(self.rows[:1].clone())
        return torch.cat(rows)

    def eager(self, k: int):
        """the same k steps without graphs (the composition the graphs are checked against)"""
        rows = []
        for _ in range(k):
            self._step(0)
            rows.append(self.rows[:1].clone())
        return torch.cat(rows)

    def epoch(self, n: int, generator):
        """one pass over rows 0 .. n - 1 in a fresh permutation; -> the metrics rows [n // B, 8] on the device"""
        steps, rows, i = self.shuffle(n, generator), [], 0
        while i < steps:
            k = min(self.S, steps - i) if self.graphs else 1
            rows.append((self.run(k) if self.graphs else self.eager(k)).clone())
            i += k
        return torch.cat(rows)


# ---- the loop -----------------------------------------------------------------------------------------------------------------
def _paths(text):
    return [p for p in str(text).split(",") if p]


def train_distill(config, log=print, teachers=None, lut=None, steps_per_graph: int = 8, device=None):
    """the loop of the module docstring; returns the trained student.  ``log`` receives one metric dict per iteration and one per
    evaluation.  ``teachers``: modules to use instead of loading ``teacher_model_path``; ``lut``: (keys, values) instead of
    ``dds_path``."""
    import brl_amd
    from .checkpoint import load_params
    from .evaluation import make_simple_duplicate_evaluate
    cfg = dict(DISTILL_DEFAULTS)
    cfg.update(config)
    if cfg["behaviour"] not in ("teacher", "student"):
        raise ValueError(f"behaviour={cfg['behaviour']!r}: 'teacher' or 'student'")
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    t_act, t_type = cfg["teacher_activation"], cfg["teacher_model_type"]
    if teachers is None:
        if not cfg["teacher_model_path"]:
            raise SystemExit("teacher_model_path= is required (a comma list of params files)")
        teachers = [load_params(p, t_act, t_type, dev) for p in _paths(cfg["teacher_model_path"])]
    teachers = list(teachers)
    K = len(teachers)
    weights = torch.from_numpy(mixture_weights(cfg["teacher_weights"], K)).to(dev)
    seed = int(cfg["rng_seed"])
    student_fp, teacher_fp = make_forward_pass(cfg["activation"], cfg["type_of_model"]), make_forward_pass(t_act, t_type)
    if cfg["initial_model_path"]:
        student = load_params(cfg["initial_model_path"], cfg["activation"], cfg["type_of_model"], dev)
    else:
        student = student_fp.init(seed, device=dev)
    opt = make_optimizer(student, float(cfg["learning_rate"]))
    tau, c_pol, c_val = float(cfg["tau"]), float(cfg["policy_coef"]), float(cfg["value_coef"])
    N, T, B = int(cfg["num_envs"]), int(cfg["num_steps"]), int(cfg["minibatch_size"])
    n = N * T
    if B > n:
        raise ValueError(f"minibatch_size={B} exceeds the {n} positions of one iteration")
    make_env = (lambda: brl_amd.BridgeBidding(lut=lut, device=dev)) if lut is not None else (lambda: brl_amd.BridgeBidding(cfg["dds_path"], device=dev))
    env, eval_env = make_env(), make_env()     # evaluation has its own handle: env.init re-keys a handle's generator
    roll_cfg = dict(num_steps=T, reward_scale=7600.0, game_mode="competitive", actor_illegal_action_mask=True)
    rolls = {"teacher": brl_amd.make_roll_out(roll_cfg, env, teacher_fp, teacher_fp),
             "student": brl_amd.make_roll_out(roll_cfg, env, student_fp, teacher_fp)}
    held_roll = brl_amd.make_roll_out(roll_cfg, eval_env, teacher_fp, teacher_fp)     # (re-deals from eval_env's own key)
    duplicate = make_simple_duplicate_evaluate(eval_env, cfg["activation"], cfg["type_of_model"], t_act, t_type, int(cfg["num_eval_envs"]))
    step = DistillStep(student, opt, B, n, tau, c_pol, c_val, steps_per_graph)
    heads = torch.empty((K, n, NUM_ACTIONS + 1), dtype=torch.float32, device=dev)
    gen = torch.Generator(device=dev).manual_seed(seed)
    state = env.init(seed, num_envs=N)
    rs = (None, None, state, state.observation, 0, 0)
    iters, every = int(cfg["iterations"]), int(cfg["eval_every"])
    t0 = time.perf_counter()
    for it in range(iters):
        by_student = cfg["behaviour"] == "student" and it >= int(cfg["teacher_iterations"])
        actor = student if by_student else teachers[it % K]
        rs, traj = rolls["student" if by_student else "teacher"]((actor,) + tuple(rs[1:]), teachers[it % K])
        step.data_obs.copy_(traj.obs.reshape(n, OBS_SIZE))
        step.data_mask.copy_(traj.legal_action_mask.reshape(n, NUM_ACTIONS))
        ensemble_targets(teachers, weights, step.data_obs, step.data_mask, tau, step.data_q, step.data_vstar, step.data_hq, heads)
        rows = torch.cat([step.epoch(n, gen) for _ in range(int(cfg["update_epochs"]))])
        m = rows.double().mean(0).cpu().numpy().tolist()
        log({"iteration": it, "behaviour": "student" if by_student else "teacher", "steps": rows.shape[0],
             **{"train/" + k: v for k, v in zip(METRICS, m)}})
        if every > 0 and (it + 1) % every == 0:
            held = eval_env.init(seed + 1 + it, num_envs=N)
            _, ht = held_roll((teachers[0], None, held, held.observation, 0, 0), teachers[it % K])
            ev = distill_evaluate(student, teachers, ht.obs.reshape(n, OBS_SIZE), ht.legal_action_mask.reshape(n, NUM_ACTIONS),
                                  weights.cpu().numpy(), tau, c_pol, c_val)
            (imp, se, _), _, _ = duplicate(student, teachers[0], 0)
            print(f"After {it + 1} iterations, held-out agreement: {ev['agreement']:.4f}, policy loss: {ev['policy_loss']:.5f}, "
                  f"IMP vs teacher 0: {float(imp):.3f} ± {float(se):.3f}")
            if cfg["save_path"] is not None:
                os.makedirs(cfg["save_path"], exist_ok=True)
                save_pickle(student, os.path.join(cfg["save_path"], f"params-{it + 1}.pkl"))
            log({"iteration": it, **{"test/" + k: v for k, v in ev.items()}, "test/imp": float(imp), "test/imp_se": float(se)})
    torch.cuda.synchronize(dev)
    log({"iterations": iters, "seconds": time.perf_counter() - t0})
    return student


def main(argv=None):
    from .train import parse_cli
    cfg = parse_cli(sys.argv[1:] if argv is None else argv, defaults=DISTILL_DEFAULTS)
    print(cfg)
    train_distill(cfg)


if __name__ == "__main__":
    main()
