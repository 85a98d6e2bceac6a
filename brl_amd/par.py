"""Double-dummy par: par score, par contracts and IMPs against par (include/brl_par.h holds the definition).

* ``par_of(dda, dealer, vul_ns, vul_ew)`` — one ``brl_par`` launch: a par record per board, on the device.
* ``par_imp(rec, par, sign=1)`` — one ``brl_par_imp`` launch: the IMP of each board record against its par.
* ``PAR_DTYPE`` — the record as a numpy structured dtype; ``par_contracts(row, dda)`` names its contracts.
* ``par_stats(records)`` — how far from par each team bid, per table and pooled (numpy on the host, like ``board_stats``).
"""
from __future__ import annotations

import numpy as np

from .boards import ILLEGAL, STRAINS, TERMINATED

PASSED_OUT, DEALER_DEPENDENT = 1, 2     # BRL_PAR_* flags
NO_RESULT = -2 ** 31                    # BRL_PAR_NO_RESULT

PAR_DTYPE = np.dtype([("score_ns", "<i4"), ("score_ns_alt", "<i4"), ("flags", "<u4"), ("zero", "<u4"),
                      ("contracts_ns", "<u8"), ("contracts_ew", "<u8")])
assert PAR_DTYPE.itemsize == 32

# the IMP scale: a difference of at least IMP_STEPS[k] is worth k + 1 IMPs
IMP_STEPS = np.array([20, 50, 90, 130, 170, 220, 270, 320, 370, 430, 500, 600, 750, 900, 1100, 1300, 1500, 1750, 2000, 2250,
                      2500, 3000, 3500, 4000], np.int64)


# ---- the device path ---------------------------------------------------------------------------------------------------------
def _on_device(x, dtype, dev):
    import torch
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x))
    return x.to(device=dev, dtype=dtype).contiguous()


def par_of(dda, dealer, vul_ns, vul_ew):
    """uint8 [n,32] on the device: ``brl_par`` of the boards — ``dda`` [n,20] (or [n,4,5]) double-dummy tricks
    [seat][strain], ``dealer`` [n] seats 0..3, ``vul_ns`` / ``vul_ew`` [n] 0 or 1; torch tensors or numpy arrays of any integer
    type (numpy arrays go to the device of a tensor among them, or to the current one).  One launch on the current stream, no
    synchronisation."""
    import torch

    from . import _capi
    dev = next((x.device for x in (dda, dealer, vul_ns, vul_ew) if isinstance(x, torch.Tensor) and x.is_cuda), None)
    if dev is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    dda = _on_device(dda, torch.uint8, dev).reshape(-1, 20)
    n = dda.shape[0]
    if dda.data_ptr() % 16:
        dda = dda.clone()
    dealer = _on_device(dealer, torch.uint8, dev).reshape(-1)
    vul = (_on_device(vul_ns, torch.uint8, dev).reshape(-1) & 1) | ((_on_device(vul_ew, torch.uint8, dev).reshape(-1) & 1) << 1)
    if dealer.shape[0] != n or vul.shape[0] != n:
        raise ValueError("dda, dealer, vul_ns and vul_ew hold different numbers of boards")
    out = torch.empty((n, PAR_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    if n:
        di = _capi.device_index(out)
        _capi.check(_capi.lib().brl_par(di, _capi.ptr(dda), _capi.ptr(dealer), _capi.ptr(vul), n, _capi.ptr(out), _capi.stream(di)))
    return out


def par_imp(rec, par, sign: int = 1):
    """int32 [n] on the device: ``brl_par_imp`` — ``sign`` x the IMP of ``rec``'s North-South score (uint8 [n,368] device
    records) against ``par`` (uint8 [n,32], ``par_of``); ``NO_RESULT`` where the record holds no result"""
    import torch

    from . import _capi
    n = rec.shape[0]
    if par.shape[0] != n:
        raise ValueError("one par record per board record")
    out = torch.empty(n, dtype=torch.int32, device=rec.device)
    if n:
        di = _capi.device_index(rec)
        _capi.check(_capi.lib().brl_par_imp(di, _capi.ptr(rec), _capi.ptr(par), n, int(sign), _capi.ptr(out), _capi.stream(di)))
    return out


# ---- the host side -------------------------------------------------------------------------------------------------------------
def par_array(x) -> np.ndarray:
    """``PAR_DTYPE`` [n] of par records: a structured array, their bytes as uint8 [n,32], or the device tensor"""
    if not isinstance(x, np.ndarray):
        x = x.detach().cpu().contiguous().numpy()
    return x if x.dtype == PAR_DTYPE else np.ascontiguousarray(x).view(PAR_DTYPE).reshape(-1)


def imp_of(diff) -> np.ndarray:
    """the IMPs of score differences (int64 array), signed"""
    diff = np.asarray(diff, np.int64)
    return np.sign(diff) * np.searchsorted(IMP_STEPS, np.abs(diff), side="right")


def imp_vs_par(rec: np.ndarray, par: np.ndarray) -> np.ndarray:
    """int32 [n], what ``par_imp`` computes with sign +1, from host arrays (``RECORD_DTYPE``, ``PAR_DTYPE``)"""
    imp = imp_of(rec["score_ns"].astype(np.int64) - par["score_ns"].astype(np.int64))
    result = ((rec["flags"] & TERMINATED) != 0) & ((rec["flags"] & ILLEGAL) == 0)
    return np.where(result, imp, NO_RESULT).astype(np.int32)


def par_contracts(par_row, dda=None):
    """the par contracts of one record, ascending: ``["4S by NS"]``, ``["5HX by EW"]``; a passed-out par has none.  ``X``: the
    contract fails — its side has fewer than level + 6 tricks in ``dda`` (the board's 20 counts).  Without ``dda`` the same is
    read from the par score: a side whose par contract costs it points has failed."""
    out = []
    r = int(par_row["score_ns"])
    t = None if dda is None else np.asarray(dda).reshape(4, 5).astype(np.int64) & 15
    for side, name in ((0, "NS"), (1, "EW")):
        mask = int(par_row["contracts_" + name.lower()])
        for b in range(35):
            if (mask >> b) & 1:
                level, strain = b // 5 + 1, b % 5
                fails = (r < 0) == (side == 0) if t is None else max(t[side, strain], t[side + 2, strain]) < level + 6
                out.append(f"{level}{STRAINS[strain]}{'X' if fails else ''} by {name}")
    return out


def _mean_se(x):
    nan = float("nan")
    x = np.asarray(x, np.float64)
    return {"count": int(x.size), "mean": float(x.mean()) if x.size else nan,
            "se": float(x.std(ddof=1) / np.sqrt(x.size)) if x.size > 1 else nan}


def _team_stats(imp, at_par, holder):
    """one team's results: ``imp`` from its side, ``at_par`` per result, ``holder`` 0 own side holds the par contracts / 1 the
    other side / 2 nobody"""
    out = {"imp": _mean_se(imp), "at_par": float(at_par.mean()) if at_par.size else float("nan")}
    for k, name in enumerate(("own_par", "their_par", "passed_par")):
        s = _mean_se(imp[holder == k])
        out[name] = {"count": s["count"], "mean": s["mean"]}
    return out


def par_stats(records) -> dict:
    """How far from par the two teams bid.  ``records``: a ``BoardRecords`` with the deals' ``dda`` (its ``par()`` is used).

      {"boards", "tables": {"a": T, "b": T}, "teams": {"team1": S, "team2": S}}
      T = {"skipped", "abs_imp", "team1": S, "team2": S};   S = {"imp": {"count", "mean", "se"}, "at_par",
           "own_par": {"count", "mean"}, "their_par": {...}, "passed_par": {...}}

    A result is one finished table of one board, seen by one team: its IMP against par is that of the table's North-South
    score for the team sitting North-South there and its negative for the other team.  The team sitting North-South is read
    from the record's ``seating``: the player at seat 0, ``>> 1`` (0 is team 1).  ``imp``: mean ± standard error over the
    team's results; ``at_par``: the share of results whose score equals the par score; ``own_par`` / ``their_par`` /
    ``passed_par``: the same results split by who holds the board's par contracts — the team's own side at that table, the
    other side, or nobody (par is a pass-out); ``abs_imp``: per table the mean |IMP vs par|.  ``tables`` holds each table on its
    own, ``teams`` a team's results of both tables pooled.  Records without a result (``NO_RESULT``: unfinished, or ended by an
    illegal call) are left out and counted as ``skipped``.

    At one table the two teams' values are negatives of each other (and ``at_par`` is the same number): the splits and
    ``abs_imp`` carry the information there, not the grand mean.  Pooled over both tables of a duplicate match a team's mean
    says how its bidding in both directions compares with par."""
    par = records.par()
    n = len(par)
    out = {"boards": n, "tables": {}, "teams": {}}
    pooled = {0: [], 1: []}
    tables = ["a"] + (["b"] if records.table_b is not None else [])
    for table in tables:
        rec = records.cpu(table)
        imp = records.imp_vs_par(table).astype(np.int64)
        keep = imp != NO_RESULT
        ns_team = ((rec["seating"] & 3) >> 1).astype(np.int64)          # the team index of the player at seat 0
        # who holds the par contracts, from North-South's side: 0 North-South, 1 East-West, 2 nobody
        holder_ns = np.where(par["contracts_ns"] != 0, 0, np.where(par["contracts_ew"] != 0, 1, 2))
        at_par = rec["score_ns"] == par["score_ns"]
        t = {"skipped": int((~keep).sum()), "abs_imp": float(np.abs(imp[keep]).mean()) if keep.any() else float("nan")}
        for team in (0, 1):
            sits_ns = ns_team == team
            mine = np.where(sits_ns, imp, -imp)
            holder = np.where(sits_ns | (holder_ns == 2), holder_ns, 1 - holder_ns)
            t[f"team{team + 1}"] = _team_stats(mine[keep], at_par[keep], holder[keep])
            pooled[team].append((mine[keep], at_par[keep], holder[keep]))
        out["tables"][table] = t
    for team in (0, 1):
        out["teams"][f"team{team + 1}"] = _team_stats(*(np.concatenate([p[k] for p in pooled[team]]) for k in range(3)))
    return out


def stats_lines(stats: dict):
    """one line per team of ``par_stats``' pooled results, as ``python -m brl_amd.eval ... par=1`` prints them"""
    lines = []
    for name, s in stats["teams"].items():
        split = ", ".join(f"{k.split('_')[0]} {s[k]['mean']:+.2f} (n={s[k]['count']})" for k in ("own_par", "their_par", "passed_par"))
        lines.append(f"par {name}: {s['imp']['mean']:+.3f} ± {s['imp']['se']:.3f} IMP vs par over {s['imp']['count']} results, "
                     f"at par {100 * s['at_par']:.1f}%; by par holder: {split}")
    return lines
