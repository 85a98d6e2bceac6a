"""Cross-play: duplicate matches with a network per PLAYER, batched (include/brl_crossplay.h holds the definition).

    python -m brl_amd.crossplay models_directory=rl_log exp_name=exp_0000/rl_params opp_model_path=opp.pt [skip_interval=100
        max_step=10000 num_eval_envs=100 dds_path=... max_boards=65536 save_path=cross_play.json]

Everything else in the project gives both players of a team ONE network.  A line-up ``(p0, p1, p2, p3)`` gives player id k the
network ``params_list[pk]``: every call of player k is that network's masked arg-max.  Players {0, 1} are team 1, players {2, 3}
team 2; the league's match (i, j) is the line-up (i, i, j, j), bit for bit.  ``cross_play`` plays the M x M line-ups (x, y, o, o)
against one opponent o on the same boards and reports what a pair loses by not sharing a system (``CrossPlay.gap``).

A batch of P line-ups of n boards is the league's batch (match-major, every match on the SAME n boards), played by the league's
driver (``_match_batch.play_batches``) with ``brl_xplay_route``: the boards whose team acts are grouped by the network of the
PLAYER to call (slot = (match, half), half = ``current_player & 1``).

``method="loop"`` plays one line-up at a time: the acting team's logits are ``where(half == 0, f_a(obs), f_b(obs))`` of its two
players' networks (one forward when they share one): FAIR networks, mixed architectures and the timing baseline.
"""
from __future__ import annotations

import ctypes as C
import json
import os
import sys

import numpy as np
import torch

from . import _capi
from ._capi import NUM_ACTIONS, OBS_SIZE, check, ptr, stream
from ._match_batch import Route, new_record, per_match_stats, play_batches
from .league import LEAGUE_DEFAULTS, _not_batchable, batch_plan, select_checkpoints

CROSSPLAY_DEFAULTS = dict(   # the league's names and defaults where the names coincide
    models_directory=LEAGUE_DEFAULTS["models_directory"], exp_name=LEAGUE_DEFAULTS["exp_name"], opp_model_path="",
    num_eval_envs=LEAGUE_DEFAULTS["num_eval_envs"], skip_interval=LEAGUE_DEFAULTS["skip_interval"],
    max_step=LEAGUE_DEFAULTS["max_step"], activation=LEAGUE_DEFAULTS["activation"], model_type=LEAGUE_DEFAULTS["model_type"],
    dds_path=LEAGUE_DEFAULTS["dds_path"], max_boards=LEAGUE_DEFAULTS["max_boards"], save_path="",
)


# ---------------------------------------------------------------------------------------------------------------
# host logic (no GPU: unit-tested on the CPU)
# ---------------------------------------------------------------------------------------------------------------
def parse(argv):
    """``key=value`` arguments; an unknown key is an error (train.parse_cli's rules for the types)"""
    from .train import parse_cli
    return parse_cli(argv, defaults=CROSSPLAY_DEFAULTS)


def _lineups(lineups):
    return np.asarray(lineups, np.int64).reshape(-1, 4)


def lineup_order(lineups, team: int):
    """The static visiting order of a batch's slots for ``team``.  Slot ``2 * match + half`` belongs to the network
    ``lineups[match][2 * team + half]``; ``order`` is the stable sort of the slots by that network (a permutation of
    0 .. 2 nmatch - 1), ``group_of`` position k's group = index into ``nets`` (non-decreasing) and ``nets`` the distinct networks
    that can act for this team, ascending.  Where both players of a team share a network the slots (2m, 2m + 1) stay adjacent
    and in one group: the league's ``team_order`` with every match split in two."""
    keys = _lineups(lineups)[:, 2 * team:2 * team + 2].reshape(-1)
    order = np.argsort(keys, kind="stable")
    nets, inverse = np.unique(keys, return_inverse=True)
    return order.astype(np.int32), inverse.reshape(-1)[order].astype(np.int32), nets.astype(np.int64)


XPLAY_ROUTE = Route("brl_xplay_route", 2, lineup_order)   # a slot is (match, half): the acting boards by their player's network


def cross_lineups(num_models: int):
    """the M x M line-ups (x, y, o, o), x-major, with o = ``num_models`` (the opponent appended to the list)"""
    M = int(num_models)
    return np.array([(x, y, M, M) for x in range(M) for y in range(M)], np.int64).reshape(-1, 4)


class CrossPlay:
    """The M x M partnerships (x, y) of M networks against one opponent, on the same n boards (numpy float64 arrays):

    ``imp[x, y]`` ± ``se[x, y]``: mean IMP of line-up (x, y, o, o); the diagonal is each network's self-play result against o.
    ``sym = (imp + imp.T) / 2``.  ``gap[x, y]`` ± ``gap_se[x, y]``: paired per board, because every line-up plays the same
    boards — ``g_b = (c_xy,b + c_yx,b) / 2 - (c_xx,b + c_yy,b) / 2``, ``gap = mean(g)``, ``gap_se = std(g, ddof=1) / sqrt(n)``.
    A negative gap is the IMPs per board the pair loses by not sharing a system; the diagonal is exactly 0."""

    def __init__(self, cum_return, imp=None, se=None, names=None):
        c = np.asarray(cum_return, np.float64)
        M = int(round(c.shape[0] ** 0.5))
        if c.ndim != 2 or M * M != c.shape[0]:
            raise ValueError(f"cum_return {c.shape}: [M * M, n], line-up (x, y) in row x * M + y")
        n = c.shape[1]
        c = c.reshape(M, M, n)
        self.n, self.names = n, (list(names) if names is not None else [str(k) for k in range(M)])
        self.cum_return = c
        self.imp = c.mean(axis=2) if imp is None else np.asarray(imp, np.float64).reshape(M, M)
        self.se = (c.std(axis=2, ddof=1) / np.sqrt(n) if n > 1 else np.zeros((M, M))) if se is None \
            else np.asarray(se, np.float64).reshape(M, M)
        self.sym = (self.imp + self.imp.T) / 2
        d = np.arange(M)
        own = c[d, d]                                                    # [M, n]: c_xx
        g = (c + c.transpose(1, 0, 2)) / 2 - (own[:, None, :] + own[None, :, :]) / 2
        self.gap = g.mean(axis=2)
        self.gap_se = g.std(axis=2, ddof=1) / np.sqrt(n) if n > 1 else np.zeros((M, M))

    def __len__(self):
        return self.imp.shape[0]

    def worst(self, k: int = 5):
        """the k pairs x < y with the most negative gap: [(x, y, gap, gap_se)], the pairs to hand to ``make_policy_diff``"""
        M = len(self)
        pairs = [(x, y) for x in range(M) for y in range(x + 1, M)]
        pairs.sort(key=lambda p: (self.gap[p], p))
        return [(x, y, float(self.gap[x, y]), float(self.gap_se[x, y])) for x, y in pairs[:max(0, int(k))]]

    def stacked(self):
        """[4, M, M]: imp, se, gap, gap_se"""
        return np.stack([self.imp, self.se, self.gap, self.gap_se])

    def to_text(self) -> str:
        M, w = len(self), max(5, max(len(s) for s in self.names))
        cell = lambda v, e: f"{v:+7.3f} ± {e:5.3f}"   # noqa: E731
        lines = [f"cross-play of {M} networks as partners, {self.n} boards per line-up (x, y, o, o): IMP of the pair (row x = player 0, "
                 f"column y = player 1)"]
        head = " " * w + "  " + "  ".join(f"{s:>15}" for s in self.names)
        for title, a, e in (("IMP", self.imp, self.se), ("gap (paired per board; negative: lost by not sharing a system)", self.gap, self.gap_se)):
            lines += [title, head]
            lines += [f"{self.names[x]:>{w}}  " + "  ".join(cell(a[x, y], e[x, y]) for y in range(M)) for x in range(M)]
        return "\n".join(lines)

    def to_dict(self):
        return {"names": self.names, "boards": self.n, "imp": self.imp.tolist(), "se": self.se.tolist(), "sym": self.sym.tolist(),
                "gap": self.gap.tolist(), "gap_se": self.gap_se.tolist(),
                "worst": [{"x": x, "y": y, "gap": g, "gap_se": e} for x, y, g, e in self.worst(len(self) * len(self))]}

    def to_json(self, path):
        with open(path, "w") as f:
            json.dump(self.to_dict(), f, indent=1)


# ---------------------------------------------------------------------------------------------------------------
# the evaluation
# ---------------------------------------------------------------------------------------------------------------
def make_lineup_evaluate(eval_env, activation, model_type, num_eval_envs, max_boards=65536, method="batched", record=None,
                         boards=False):
    """-> ``lineup_evaluate(params_list, lineups, rng_key) -> (imp[P], se[P], win_rate[P], cum_return[P, n])``: match p seats
    ``params_list[lineups[p][k]]`` as player k on the n = ``num_eval_envs`` boards of ``eval_env.init(rng_key, num_envs=n)``;
    the statistics are ``league_evaluate``'s (mean IMP, ``std(ddof=1) / sqrt(n)``, ``mean(cum_return > 0)``, player 0's side).

    ``method``: "batched" (line-ups in batches of ``max_boards // n``; "DeepMind" fp32 networks of one shape — anything else runs
    as "loop", and ``lineup_evaluate.last_method`` says which ran) or "loop" (one line-up at a time).  ``record``: the league's
    debugging dict: ``record["batches"]`` receives one dict per batch (per line-up for the loop) with ``matches``, ``table_a`` /
    ``table_b`` and per iteration ``action``, ``rows``, ``group_first`` (batched only) and ``logits`` when ``record["logits"]``
    is true.  ``boards=True``: additionally returns one ``BoardRecords`` per line-up (both tables, IMP, ``dda``) — what
    ``system_book(records)`` reads to show what a call means in THAT partnership.  Runs on one rank."""
    from .boards import _KeepA
    from .dist import one_rank_only
    from .duplicate import Table_info
    from .evaluation import _DoneWatch, _Forward
    from .models import make_forward_pass
    if method not in ("batched", "loop"):
        raise ValueError(f"method {method!r}: 'batched' or 'loop'")
    forward_pass = make_forward_pass(activation, model_type)
    n = int(num_eval_envs)
    batch_plan(1, n, max_boards)   # (max_boards below one match: an error now, not at the first call)
    dev = eval_env.device
    lib = _capi.lib()

    def play_loop(params_list, lineups, rng_key, cum, out_records):
        fwds = {}
        for p, lu in enumerate(lineups):
            for k in lu:
                if int(k) not in fwds:
                    fwds[int(k)] = _Forward(forward_pass, params_list[int(k)])
            state = eval_env.init(rng_key, num_envs=n)
            tables = (Table_info.from_state(state), Table_info.from_state(state))
            pa, pb = tables[0]._ptrs(), tables[1]._ptrs()
            packed, obs = state.packed, state.observation
            term, cur = state.terminated.clone(), state.current_player.clone()
            dda = state._dds_tricks
            action = torch.empty(n, dtype=torch.int32, device=dev)
            keep = _KeepA(packed, tables[0]) if boards else None
            rec = new_record(record, p, p + 1, tables)
            watch = _DoneWatch.take(eval_env, n, False)
            i = 0
            while True:
                polled = watch.poll(i)
                if polled is not None and polled[0] >= n:
                    watch.release()
                    break
                t = i & 1
                fa, fb = fwds[int(lu[2 * t])], fwds[int(lu[2 * t + 1])]
                lg, lb = _Forward.whole_pair(fa, fb, obs)
                if fb is not fa:   # the half decides whose logits a board takes
                    lg = torch.where((cur & 1)[:, None] == 0, lg[:, :NUM_ACTIONS], lb[:, :NUM_ACTIONS])
                lg = lg.contiguous()
                if rec is not None and record.get("logits"):
                    rec["logits"].append(lg[:, :NUM_ACTIONS].clone())
                nobs = torch.empty((n, OBS_SIZE), dtype=torch.bool, device=dev)
                check(lib.brl_eval_step_team(eval_env._h, ptr(packed), ptr(packed), n, lg.data_ptr(), lg.stride(0), t, C.byref(pa),
                                             C.byref(pb), None, 0, ptr(cum[p]), None, ptr(action), ptr(nobs), None, None, ptr(term),
                                             ptr(cur), None, stream()))
                obs = nobs
                if keep is not None:
                    keep.after_step(action)
                if rec is not None:
                    rec["action"].append(action.clone())
                watch.post(i, term)
                i += 1
            if keep is not None:
                out_records.extend(keep.records("lineup_evaluate", dda, cum[p:p + 1], n))

    def lineup_evaluate(params_list, lineups, rng_key):
        one_rank_only("lineup_evaluate")
        lineups = _lineups(lineups)
        if len(lineups) and (lineups.min() < 0 or lineups.max() >= len(params_list)):
            raise ValueError("lineups name a network outside params_list")
        use = method
        with torch.no_grad():
            cum = torch.zeros((len(lineups), n), dtype=torch.float32, device=dev)
            refs, out_records = None, []
            if use == "batched":
                refs = [_Forward._by_reference(m) for m in params_list]
                if _not_batchable(model_type, refs) is not None:
                    use = "loop"
            lineup_evaluate.last_method = use
            if len(lineups):
                if use == "batched":
                    out_records = play_batches(eval_env, refs, lineups, XPLAY_ROUTE, eval_env.init(rng_key, num_envs=n),
                                               batch_plan(len(lineups), n, max_boards), cum, record, boards, "lineup_evaluate")
                else:
                    play_loop(params_list, lineups, rng_key, cum, out_records)
            stats = per_match_stats(cum, n) if len(lineups) else (cum.new_zeros(0),) * 3
            return (*stats, cum, out_records) if boards else (*stats, cum)

    lineup_evaluate.last_method = None
    return lineup_evaluate


def cross_play(params_list, opponent_params, eval_env, activation, model_type, num_eval_envs, rng_key=0, names=None, **kw):
    """the M x M line-ups (x, y, o, o) of ``params_list`` as partners against ``opponent_params`` -> ``CrossPlay``"""
    M = len(params_list)
    ev = make_lineup_evaluate(eval_env, activation, model_type, num_eval_envs, **kw)
    out = ev(list(params_list) + [opponent_params], cross_lineups(M), rng_key)
    imp, se, cum = out[0], out[1], out[3]
    cp = CrossPlay(cum.cpu().numpy(), imp.cpu().numpy(), se.cpu().numpy(), names)
    cp.last_method = ev.last_method
    return cp


# ---------------------------------------------------------------------------------------------------------------
def main(argv, log=print):
    import brl_amd
    from .checkpoint import load_params
    cfg = parse(argv)
    if not cfg["opp_model_path"]:
        raise SystemExit("opp_model_path= is required: the opponent every partnership plays")
    directory = os.path.join(cfg["models_directory"], cfg["exp_name"])
    names = select_checkpoints(os.listdir(directory), cfg["skip_interval"], cfg["max_step"])
    log(names)
    env = brl_amd.BridgeBidding(cfg["dds_path"])
    params_list = [load_params(os.path.join(directory, p), cfg["activation"], cfg["model_type"], env.device) for p in names]
    opponent = load_params(cfg["opp_model_path"], cfg["activation"], cfg["model_type"], env.device)
    cp = cross_play(params_list, opponent, env, cfg["activation"], cfg["model_type"], cfg["num_eval_envs"], rng_key=0,
                    names=[os.path.splitext(p)[0].replace("params-", "") for p in names], max_boards=cfg["max_boards"])
    log(cp.to_text())
    np.save(f"cross_play_{cfg['exp_name'].replace(os.sep, '_')}.npy", cp.stacked())
    if cfg["save_path"]:
        cp.to_json(cfg["save_path"])
    return cp


if __name__ == "__main__":
    main(sys.argv[1:])
