"""Bidding statistics read from board records (numpy only): ``board_stats(BoardRecords.cpu(), imp)``.

High-card points and suit lengths are counted from the card NAMES (``boards.hand_names``: the one card mapping), not from any
packed form."""
from __future__ import annotations

import numpy as np

from .boards import ILLEGAL, PASSED_OUT, STRAINS, TERMINATED, hand_names

HCP = {"A": 4, "K": 3, "Q": 2, "J": 1}


def side_counts(hands, declarer):
    """(high-card points, {suit: length}) of the declaring side (declarer and partner) from the four hand words"""
    names = hand_names(hands[declarer]) + hand_names(hands[declarer ^ 2])
    return sum(HCP.get(c[1], 0) for c in names), {s: sum(1 for c in names if c[0] == s) for s in "CDHS"}


def board_stats(rec: np.ndarray, imp=None) -> dict:
    """``rec``: records of finished tables (``RECORD_DTYPE``).  Ratios are over all records, except where said.
      pass_out_ratio, doubled_ratio (contracts doubled or redoubled / contracts), made_ratio (contracts made / contracts),
      mean_level (over contracts), strain_agreement (suit contracts in the declaring side's longest combined suit — any of
      them on a tie — / suit contracts), level_hcp_corr (Pearson, over contracts), imp_mean / imp_se (when ``imp`` is given)"""
    n = int(rec.shape[0])
    flags = rec["flags"]
    has = ((flags & TERMINATED) != 0) & ((flags & (PASSED_OUT | ILLEGAL)) == 0)
    idx = np.nonzero(has)[0]
    level = rec["level"][idx].astype(np.float64)
    made = rec["tricks"][idx].astype(np.int64) >= rec["level"][idx].astype(np.int64) + 6
    hcp, agree, suit = [], 0, 0
    for i in idx:
        r = rec[i]
        pts, length = side_counts(r["hands"], int(r["declarer"]))
        hcp.append(pts)
        if r["strain"] < 4:
            suit += 1
            agree += length[STRAINS[r["strain"]]] == max(length.values())
    hcp = np.array(hcp, np.float64)
    nan = float("nan")
    corr = nan
    if idx.size >= 2 and level.std() > 0 and hcp.std() > 0:
        corr = float(((level - level.mean()) * (hcp - hcp.mean())).mean() / (level.std() * hcp.std()))
    out = {"boards": n, "contracts": int(idx.size),
           "pass_out_ratio": float(((flags & PASSED_OUT) != 0).sum() / n) if n else nan,
           "made_ratio": float(made.mean()) if idx.size else nan,
           "mean_level": float(level.mean()) if idx.size else nan,
           "doubled_ratio": float((rec["doubled"][idx] > 0).mean()) if idx.size else nan,
           "strain_agreement": agree / suit if suit else nan,
           "level_hcp_corr": corr}
    if imp is not None:
        x = np.asarray(imp, np.float64)
        out["imp_mean"] = float(x.mean())
        out["imp_se"] = float(x.std(ddof=1) / np.sqrt(x.size)) if x.size > 1 else nan
    return out
