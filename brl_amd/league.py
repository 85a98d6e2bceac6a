"""League evaluation: many network pairs in ONE batched duplicate match — the reference's ``workspace/eval_selfplay_league.py``
(every pair of a run's checkpoints, the IMP matrices its figures are drawn from) and PFSP's ``league_imps`` (ppo.py:399-421: the
learner against every pool checkpoint).

    python -m brl_amd.league models_directory=rl_log exp_name=exp_0000/rl_params skip_interval=100 [dds_path=...] [max_boards=65536]

A league of P matches of n boards is one batch of P * n boards (match-major: board b belongs to match b // n) in which every
board's call comes from one of M networks of ONE architecture.  Per iteration (the teams alternate, as in ``_eval_loop``):

1. ``brl_league_route``: the boards whose team acts, grouped by the network that plays that team in their match;
2. ``brl_league_forward``: the cast, every hidden layer and the heads as one launch each over all groups;
3. ``brl_eval_step_team`` on the whole batch (unchanged: one logits row per board);
4. ``_DoneWatch.post`` / ``poll`` — the only host synchronisation.

Every match plays the SAME n boards (those of ``eval_env.init(rng_key, num_envs=n)``, dealt once and tiled), so match p gives the
numbers of ``make_simple_duplicate_evaluate(...)(params_list[i], params_list[j], rng_key)``.  ``method="loop"`` plays the pairs
one by one through the existing evaluator's loop: FAIR networks, mixed architectures and the timing baseline.
"""
from __future__ import annotations

import ctypes as C
import itertools
import os
import sys

import numpy as np
import torch

from . import _capi
from ._capi import OBS_SIZE, check, device_index, ptr, stream

LEAGUE_DEFAULTS = dict(  # workspace/eval_selfplay_league.py: SelfplayLeagueConfig, same names and defaults
    models_directory="models", exp_name="pretrained-rl-with-sp", num_eval_envs=100, skip_interval=100, max_step=10000,
    save_fig_directory_path="", activation="relu", model_type="DeepMind",
    # build-side (not in the reference, which reads dds_results/test_000.npy)
    dds_path="dds_results/test_000.npy", max_boards=65536,
)

LDO = 40   # row stride of the logits buffer: 38 logits + the value, padded to whole 16 bytes


# ---------------------------------------------------------------------------------------------------------------
# host logic (no GPU: unit-tested on the CPU)
# ---------------------------------------------------------------------------------------------------------------
def parse(argv, defaults=None):
    """``key=value`` arguments; an unknown key is an error (train.parse_cli's rules for the types)"""
    from .train import parse_cli
    return parse_cli(argv, defaults=LEAGUE_DEFAULTS if defaults is None else defaults)


def checkpoint_step(name: str) -> int:
    return int(name.split("-")[1].split(".")[0])


def select_checkpoints(names, skip_interval: int, max_step: int):
    """the reference's filter (eval_selfplay_league.py:57-70): the name contains "params", its step is a multiple of
    ``skip_interval`` and at most ``max_step``; sorted by name.  torch state_dicts (.pt) and Haiku pickles (.pkl)."""
    return sorted(p for p in names
                  if "params" in p and p.endswith((".pt", ".pkl"))
                  and checkpoint_step(p) % skip_interval == 0 and checkpoint_step(p) <= max_step)


def batch_plan(num_pairs: int, n: int, max_boards: int):
    """[(first, last + 1)] match ranges of at most ``max_boards // n`` matches: every pair exactly once, memory bounded"""
    per = int(max_boards) // int(n)
    if per < 1:
        raise ValueError(f"max_boards={max_boards} is below one match of {n} boards")
    return [(s, min(s + per, num_pairs)) for s in range(0, num_pairs, per)]


def team_order(pairs, team: int):
    """The static visiting order of a batch's matches for ``team``: ``order`` (a permutation of the batch's matches, stable-sorted
    by the network that plays ``team``), ``group_of`` (slot k's group = index into ``nets``, non-decreasing) and ``nets`` (the
    distinct networks that can act for this team, ascending)."""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    order = np.argsort(pairs[:, team], kind="stable")
    nets, inverse = np.unique(pairs[:, team], return_inverse=True)
    return order.astype(np.int32), inverse.reshape(-1)[order].astype(np.int32), nets.astype(np.int64)


def league_matrices(imp, pairs, num_models: int):
    """eval_selfplay_league.py:112-121: ``win_lose[i][j] = -imp``, ``win_lose[j][i] = imp`` for match (i, j); the same with imp
    clipped to [-1, 1]; the sign only.  Zero diagonal."""
    win_lose = np.zeros((num_models, num_models))
    clip = np.zeros_like(win_lose)
    dis = np.zeros_like(win_lose)
    for v, (i, j) in zip(np.asarray(imp, np.float64), np.asarray(pairs).reshape(-1, 2)):
        win_lose[i][j], win_lose[j][i] = -v, v
        c = np.clip(v, -1, 1)
        clip[i][j], clip[j][i] = -c, c
        s = float(np.sign(v))
        dis[i][j], dis[j][i] = -s, s
    return win_lose, clip, dis


def all_pairs(num_models: int):
    return np.array(list(itertools.combinations(range(num_models), 2)), np.int64).reshape(-1, 2)


# ---------------------------------------------------------------------------------------------------------------
# the evaluation
# ---------------------------------------------------------------------------------------------------------------
def _net_record(ref) -> list:
    """brl_league_net of a brl_mlp_ref: its 20 pointers"""
    return [ref.w[i] or 0 for i in range(8)] + [ref.b[i] or 0 for i in range(8)] + [ref.actor_w, ref.actor_b, ref.critic_w, ref.critic_b]


def _not_batchable(model_type, refs):
    """why this league cannot run as one batch (then it runs as a loop), or None"""
    if not str(model_type).startswith("DeepMind"):
        return f"model_type {model_type}"
    if any(r is None for r in refs):
        return "a network is not an fp32 DeepMind MLP on the GPU (<= 8 layers, hidden % 4 == 0 and <= 1024, ReLU / tanh)"
    shapes = {(int(r.nlayers), int(r.hidden), int(r.act)) for r in refs}
    if len(shapes) != 1:
        return f"mixed architectures {sorted(shapes)}"
    return None


def make_league_evaluate(eval_env, activation, model_type, num_eval_envs, max_boards=65536, method="batched", record=None,
                         shard=None):
    """-> ``league_evaluate(params_list, pairs, rng_key) -> (imp[P], se[P], win_rate[P], cum_return[P, n])``: match p is
    ``params_list[pairs[p][0]]`` (team 1) against ``params_list[pairs[p][1]]`` (team 2) on the n = ``num_eval_envs`` boards of
    ``eval_env.init(rng_key, num_envs=n)``; mean IMP, ``std(ddof=1) / sqrt(n)`` and ``mean(cum_return > 0)`` of its own row of
    ``cum_return`` (src/evaluation.py:199-201).

    ``method``: "batched" (matches in batches of ``max_boards // n``, so that memory is bounded: at hidden 1024 an
    acting row holds 8 KB of activations; "DeepMind" fp32 networks of one shape — anything else runs
    as "loop", and ``league_evaluate.last_method`` says which ran) or "loop" (one evaluation per pair, the existing loop).
    ``record``: an optional dict; batched runs append to ``record["batches"]`` one dict per batch with ``matches`` (first, last +
    1), ``table_a`` / ``table_b`` (the batch's Table_info) and per iteration ``action``, ``rows``, ``group_first`` (and ``logits``
    when ``record["logits"]`` is true).  ``shard`` (evaluation._Shard): the n boards are split over the ranks; the three statistics
    are those of all boards on every rank, ``cum_return`` holds this rank's."""
    from .duplicate import Table_info
    from .evaluation import _DoneWatch, _eval_loop, _Forward, _Shard
    from .models import make_forward_pass
    if method not in ("batched", "loop"):
        raise ValueError(f"method {method!r}: 'batched' or 'loop'")
    forward_pass = make_forward_pass(activation, model_type)
    n_global = int(num_eval_envs)
    batch_plan(1, n_global, max_boards)   # (max_boards below one match: an error now, not at the first league)
    dev = eval_env.device
    lib = _capi.lib()

    def play_loop(params_list, pairs, rng_key, sh, cum):
        fwds = {}
        for p, (i, j) in enumerate(pairs):
            for k in (i, j):
                if k not in fwds:
                    fwds[k] = _Forward(forward_pass, params_list[k])
            state = sh.init(eval_env, rng_key)
            tables = (Table_info.from_state(state), Table_info.from_state(state))
            _eval_loop(eval_env, state, fwds[i], fwds[j], tables, None, 0, cum[p], None)

    def play_batched(refs, pairs, rng_key, sh, cum):
        n = sh.n
        nlayers, hidden, act = int(refs[0].nlayers), int(refs[0].hidden), int(refs[0].act)
        records = np.array([_net_record(r) for r in refs], np.int64).reshape(len(refs), 20)
        state0 = sh.init(eval_env, rng_key)                      # the n boards, dealt once
        table0 = Table_info.from_state(state0)
        obs0, term0, cur0 = state0.observation, state0.terminated, state0.current_player
        di = device_index(state0.packed)
        for first, last in batch_plan(len(pairs), n_global, max_boards):
            nb = last - first
            B = nb * n
            packed = state0.packed.repeat(nb, 1)
            tables = tuple(Table_info(*(t.repeat((nb,) + (1,) * (t.dim() - 1)) for t in table0)) for _ in range(2))
            pa, pb = tables[0]._ptrs(), tables[1]._ptrs()
            obs = [obs0.repeat(nb, 1), torch.empty((B, OBS_SIZE), dtype=torch.bool, device=dev)]
            term, cur = term0.repeat(nb), cur0.repeat(nb)
            cumb = cum[first:last].view(-1)
            out = torch.zeros((B, LDO), dtype=torch.float32, device=dev)
            action = torch.empty(B, dtype=torch.int32, device=dev)
            rows = torch.zeros(B, dtype=torch.int64, device=dev)
            work = torch.empty(2 * nb, dtype=torch.int32, device=dev)
            scratch = torch.empty(B * (OBS_SIZE + 2 * hidden), dtype=torch.float32, device=dev)
            teams = []
            for t in (0, 1):   # the static part of a team's iterations: its order of the matches and its table of networks
                order, group_of, nets = team_order(pairs[first:last], t)
                teams.append((torch.from_numpy(order).to(dev), torch.from_numpy(group_of).to(dev),
                              torch.from_numpy(records[nets].copy()).to(dev), len(nets),
                              torch.zeros(len(nets) + 1, dtype=torch.int32, device=dev)))
            rec = None
            if record is not None:
                rec = {"matches": (first, last), "table_a": tables[0], "table_b": tables[1], "action": [], "rows": [],
                       "group_first": [], "logits": []}
                record.setdefault("batches", []).append(rec)
            watch = _DoneWatch.take(eval_env, B, False)
            i, rmax = 0, B
            while True:
                polled = watch.poll(i)
                if polled is not None:
                    if polled[0] >= B:
                        watch.release()
                        break
                    rmax = min(rmax, B - polled[0])   # boards finish and never restart: a bound of the rows that can act
                t = i & 1
                order, group_of, nets, G, gf = teams[t]
                check(lib.brl_league_route(di, ptr(term), ptr(cur), t, n, ptr(order), ptr(group_of), nb, G, ptr(work), ptr(rows),
                                           ptr(gf), stream()))
                check(lib.brl_league_forward(di, ptr(nets), G, nlayers, hidden, act, ptr(obs[i & 1]), ptr(rows), ptr(gf), rmax,
                                             ptr(scratch), scratch.numel(), ptr(out), LDO, stream()))
                if rec is not None and record.get("logits"):
                    rec["logits"].append(out.clone())
                check(lib.brl_eval_step_team(eval_env._h, ptr(packed), ptr(packed), B, ptr(out), LDO, t, C.byref(pa), C.byref(pb),
                                             None, 0, ptr(cumb), None, ptr(action), ptr(obs[(i & 1) ^ 1]), None, None, ptr(term),
                                             ptr(cur), None, stream()))
                if rec is not None:
                    rec["action"].append(action.clone())
                    rec["rows"].append(rows.clone())
                    rec["group_first"].append(gf.clone())
                watch.post(i, term)
                i += 1

    def league_evaluate(params_list, pairs, rng_key):
        pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
        if len(pairs) and (pairs.min() < 0 or pairs.max() >= len(params_list)):
            raise ValueError("pairs name a network outside params_list")
        sh = _Shard(n_global, shard)
        use = method
        with torch.no_grad():
            cum = torch.zeros((len(pairs), sh.n), dtype=torch.float32, device=dev)
            refs = None
            if use == "batched":
                refs = [_Forward._by_reference(m) for m in params_list]
                if _not_batchable(model_type, refs) is not None:
                    use = "loop"
            league_evaluate.last_method = use
            if len(pairs):
                if use == "batched":
                    play_batched(refs, pairs, rng_key, sh, cum)
                else:
                    play_loop(params_list, pairs, rng_key, sh, cum)
            nf = float(n_global)
            if sh.active:   # sums over every rank's boards (IMPs are integers: exact in float64)
                x = cum.to(torch.float64)
                s = sh.allsum(torch.stack([x.sum(1), (x * x).sum(1), (x > 0).sum(1).to(torch.float64)]))
                mean = s[0] / nf
                var = ((s[1] - nf * mean * mean) / (nf - 1.0)).clamp_min(0.0)
                return mean.to(torch.float32), (var.sqrt() / nf ** 0.5).to(torch.float32), (s[2] / nf).to(torch.float32), cum
            imp = cum.mean(dim=1)
            se = cum.std(dim=1, unbiased=True) / nf ** 0.5          # src/evaluation.py:199
            win_rate = (cum > 0).sum(dim=1) / nf                    # :200
            return imp, se, win_rate, cum

    league_evaluate.last_method = None
    return league_evaluate


def round_robin(params_list, eval_env, activation, model_type, num_eval_envs, rng_key=0, **kw):
    """every pair i < j of ``params_list`` -> the three matrices of the reference's league script (``league_matrices``)"""
    pairs = all_pairs(len(params_list))
    ev = make_league_evaluate(eval_env, activation, model_type, num_eval_envs, **kw)
    imp = ev(params_list, pairs, rng_key)[0]
    return league_matrices(imp.cpu().numpy(), pairs, len(params_list))


def one_vs_many(params, others, eval_env, activation, model_type, num_eval_envs, rng_key=0, **kw):
    """``imp[K]`` of ``params`` as team 1 against each of ``others`` (ppo.py:399-421: what PFSP ranks its pool by)"""
    pairs = [(0, k + 1) for k in range(len(others))]
    ev = make_league_evaluate(eval_env, activation, model_type, num_eval_envs, **kw)
    return ev([params] + list(others), pairs, rng_key)[0]


# ---------------------------------------------------------------------------------------------------------------
def save_heatmaps(matrices, directory, exp_name, log=print):
    """the three figures of the reference script, drawn with matplotlib alone (``imshow(cmap="bwr_r")``; the reference uses
    seaborn's heatmap); a missing matplotlib is reported, never an error"""
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except Exception as e:   # (ImportError, or a broken backend)
        log(f"no figures: matplotlib is not usable ({e})")
        return []
    paths = []
    for m, suffix in zip(matrices, ("league", "league_clip", "league_dis")):
        plt.figure()
        plt.imshow(m, cmap="bwr_r")
        plt.colorbar()
        plt.xlabel(r"Step ($\times {10}^2$)")
        path = os.path.join(directory, f"{exp_name.replace(os.sep, '_')}_{suffix}.png")
        plt.savefig(path)
        plt.close()
        paths.append(path)
    return paths


def main(argv, log=print):
    import brl_amd
    from .checkpoint import load_params
    cfg = parse(argv)
    directory = os.path.join(cfg["models_directory"], cfg["exp_name"])
    names = select_checkpoints(os.listdir(directory), cfg["skip_interval"], cfg["max_step"])
    log(names)
    env = brl_amd.BridgeBidding(cfg["dds_path"])
    params_list = [load_params(os.path.join(directory, p), cfg["activation"], cfg["model_type"], env.device) for p in names]
    log("league match start")
    matrices = round_robin(params_list, env, cfg["activation"], cfg["model_type"], cfg["num_eval_envs"], rng_key=0,
                           max_boards=cfg["max_boards"])
    tag = cfg["exp_name"].replace(os.sep, "_")
    for m, suffix in zip(matrices, ("", "_clip", "_dis")):
        np.save(f"win_lose{suffix}_{tag}.npy", m)
    save_heatmaps(matrices, cfg["save_fig_directory_path"], cfg["exp_name"], log)
    return matrices


if __name__ == "__main__":
    main(sys.argv[1:])
