"""The batched duplicate-match driver under the league (league.py) and cross-play (crossplay.py); DESIGN §10.

A batch is nb matches of n boards, match-major (board b belongs to match b // n), every match on the SAME n boards (dealt once by
the caller and tiled), in which every board's call comes from one of M networks of ONE architecture.  Per iteration (the teams
alternate, as in ``_eval_loop``):

1. the route's export (``brl_league_route`` / ``brl_xplay_route``): the boards whose team acts, grouped by network;
2. ``brl_league_forward``: the cast, every hidden layer and the heads as one launch each over all groups;
3. ``brl_eval_step_team`` on the whole batch (unchanged: one logits row per board);
4. ``_DoneWatch.post`` / ``poll`` — the only host synchronisation.

What the two callers differ in is a ``Route``; the statistics of the finished matches are ``per_match_stats``.
"""
from __future__ import annotations

import ctypes as C
from typing import Callable, NamedTuple

import numpy as np
import torch

from . import _capi
from ._capi import OBS_SIZE, check, device_index, ptr, stream

LDO = 40   # row stride of the logits buffer: 38 logits + the value, padded to whole 16 bytes


class Route(NamedTuple):
    """how a batch's acting boards are grouped by network"""
    export: str        # the C export: (device, terminated, current_player, team, n, order, group_of, nmatch, ngroups, work, rows, group_first, stream)
    slots: int         # slots of the visiting order per match; ``work`` holds twice as many ints
    order: Callable    # (matchups of the batch, team) -> (order, group_of, nets): league.team_order / crossplay.lineup_order


def _net_record(ref) -> list:
    """brl_league_net of a brl_mlp_ref: its 20 pointers"""
    return [ref.w[i] or 0 for i in range(8)] + [ref.b[i] or 0 for i in range(8)] + [ref.actor_w, ref.actor_b, ref.critic_w, ref.critic_b]


def new_record(record, first, last, tables):
    """the entry of the matches [first, last) in the debugging dict ``record`` (appended to ``record["batches"]``), or None"""
    if record is None:
        return None
    rec = {"matches": (first, last), "table_a": tables[0], "table_b": tables[1], "action": [], "rows": [], "group_first": [],
           "logits": []}
    record.setdefault("batches", []).append(rec)
    return rec


def play_batches(eval_env, refs, matchups, route, state0, plan, cum, record=None, boards=False, who=""):
    """Plays the matches ``matchups`` ([P, 2] pairs or [P, 4] line-ups of indices into ``refs``, the networks' brl_mlp_refs) on the
    boards of ``state0``, in the batches ``plan`` ([(first, last + 1)] match ranges), adding every board's IMP into its match's row
    of ``cum`` [P, n].  ``record``: the debugging dict (``new_record``).  ``boards``: keep table A's final states too and return one
    ``BoardRecords`` per match (else the list is empty); ``who`` names the caller in their error."""
    from .boards import _KeepA
    from .duplicate import Table_info
    from .evaluation import _DoneWatch
    lib, dev, n = _capi.lib(), eval_env.device, state0.num_envs
    route_export = getattr(lib, route.export)
    nlayers, hidden, act = int(refs[0].nlayers), int(refs[0].hidden), int(refs[0].act)
    net_records = np.array([_net_record(r) for r in refs], np.int64).reshape(len(refs), 20)
    table0 = Table_info.from_state(state0)
    obs0, term0, cur0 = state0.observation, state0.terminated, state0.current_player
    dda = state0._dds_tricks if boards else None   # (a launch of its own: only where the records need it)
    di = device_index(state0.packed)
    out_records = []
    for first, last in plan:
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
        work = torch.empty(2 * route.slots * nb, dtype=torch.int32, device=dev)
        scratch = torch.empty(B * (OBS_SIZE + 2 * hidden), dtype=torch.float32, device=dev)
        teams = []
        for t in (0, 1):   # the static part of a team's iterations: its order of the slots and its table of networks
            order, group_of, nets = route.order(matchups[first:last], t)
            teams.append((torch.from_numpy(order).to(dev), torch.from_numpy(group_of).to(dev),
                          torch.from_numpy(net_records[nets].copy()).to(dev), len(nets),
                          torch.zeros(len(nets) + 1, dtype=torch.int32, device=dev)))
        keep = _KeepA(packed, tables[0]) if boards else None
        rec = new_record(record, first, last, tables)
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
            check(route_export(di, ptr(term), ptr(cur), t, n, ptr(order), ptr(group_of), nb, G, ptr(work), ptr(rows), ptr(gf), stream()))
            check(lib.brl_league_forward(di, ptr(nets), G, nlayers, hidden, act, ptr(obs[i & 1]), ptr(rows), ptr(gf), rmax,
                                         ptr(scratch), scratch.numel(), ptr(out), LDO, stream()))
            if rec is not None and record.get("logits"):
                rec["logits"].append(out.clone())
            check(lib.brl_eval_step_team(eval_env._h, ptr(packed), ptr(packed), B, ptr(out), LDO, t, C.byref(pa), C.byref(pb),
                                         None, 0, ptr(cumb), None, ptr(action), ptr(obs[(i & 1) ^ 1]), None, None, ptr(term),
                                         ptr(cur), None, stream()))
            if keep is not None:
                keep.after_step(action)
            if rec is not None:
                rec["action"].append(action.clone())
                rec["rows"].append(rows.clone())
                rec["group_first"].append(gf.clone())
            watch.post(i, term)
            i += 1
        if keep is not None:
            out_records.extend(keep.records(who, dda, cum[first:last], n))
    return out_records


def per_match_stats(cum, n_global, shard=None):
    """-> (imp, se, win_rate) of every row of ``cum`` [P, n]: mean, ``std(ddof=1) / sqrt(n)`` and ``mean(cum > 0)``
    (src/evaluation.py:199-201).  With an active ``shard`` (evaluation._Shard) the rows hold this rank's boards of ``n_global`` and
    the statistics are those of all boards, the same on every rank: sums in float64 (IMPs are integers: exact), reduced once."""
    nf = float(n_global)
    if shard is not None and shard.active:
        x = cum.to(torch.float64)
        s = shard.allsum(torch.stack([x.sum(1), (x * x).sum(1), (x > 0).sum(1).to(torch.float64)]))
        mean = s[0] / nf
        var = ((s[1] - nf * mean * mean) / (nf - 1.0)).clamp_min(0.0)
        return mean.to(torch.float32), (var.sqrt() / nf ** 0.5).to(torch.float32), (s[2] / nf).to(torch.float32)
    return cum.mean(dim=1), cum.std(dim=1, unbiased=True) / nf ** 0.5, (cum > 0).sum(dim=1) / nf
