"""League evaluation: many network pairs in ONE batched duplicate match — the reference's ``workspace/eval_selfplay_league.py``
(every pair of a run's checkpoints, the IMP matrices its figures are drawn from) and PFSP's ``league_imps`` (ppo.py:399-421: the
learner against every pool checkpoint).

    python -m brl_amd.league models_directory=rl_log exp_name=exp_0000/rl_params skip_interval=100 [dds_path=...] [max_boards=65536]

A league of P matches of n boards is one batch of P * n boards (match-major: board b belongs to match b // n) in which every
board's call comes from one of M networks of ONE architecture, played by ``_match_batch.play_batches`` with ``brl_league_route``:
the boards whose team acts are grouped by the network that plays that team in their match.

Every match plays the SAME n boards (those of ``eval_env.init(rng_key, num_envs=n)``, dealt once and tiled), so match p gives the
numbers of ``make_simple_duplicate_evaluate(...)(params_list[i], params_list[j], rng_key)``.  ``method="loop"`` plays the pairs
one by one through the existing evaluator's loop: FAIR networks, mixed architectures and the timing baseline.
"""
from __future__ import annotations

import itertools
import os
import sys

import numpy as np
import torch

from ._match_batch import LDO, Route, _net_record, per_match_stats, play_batches  # noqa: F401  (LDO, _net_record: imported from here)

LEAGUE_DEFAULTS = dict(  # workspace/eval_selfplay_league.py: SelfplayLeagueConfig, same names and defaults
    models_directory="models", exp_name="pretrained-rl-with-sp", num_eval_envs=100, skip_interval=100, max_step=10000,
    save_fig_directory_path="", activation="relu", model_type="DeepMind",
    # build-side (not in the reference, which reads dds_results/test_000.npy)
    dds_path="dds_results/test_000.npy", max_boards=65536,
)


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
LEAGUE_ROUTE = Route("brl_league_route", 1, team_order)   # a slot is a match: the acting boards by their team's network


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
    from .evaluation import _eval_loop, _Forward, _Shard
    from .models import make_forward_pass
    if method not in ("batched", "loop"):
        raise ValueError(f"method {method!r}: 'batched' or 'loop'")
    forward_pass = make_forward_pass(activation, model_type)
    n_global = int(num_eval_envs)
    batch_plan(1, n_global, max_boards)   # (max_boards below one match: an error now, not at the first league)
    dev = eval_env.device

    def play_loop(params_list, pairs, rng_key, sh, cum):
        fwds = {}
        for p, (i, j) in enumerate(pairs):
            for k in (i, j):
                if k not in fwds:
                    fwds[k] = _Forward(forward_pass, params_list[k])
            state = sh.init(eval_env, rng_key)
            tables = (Table_info.from_state(state), Table_info.from_state(state))
            _eval_loop(eval_env, state, fwds[i], fwds[j], tables, None, 0, cum[p], None)

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
                if use == "batched":   # (the plan is made from the global n; a rank tiles its own sh.n boards)
                    play_batches(eval_env, refs, pairs, LEAGUE_ROUTE, sh.init(eval_env, rng_key),
                                 batch_plan(len(pairs), n_global, max_boards), cum, record)
                else:
                    play_loop(params_list, pairs, rng_key, sh, cum)
            return (*per_match_stats(cum, n_global, sh), cum)

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
