"""Trajectory files of the supervised pre-trainer (sl.py:88-117) as a packed set for the device.

A line holds space-separated OpenSpiel action ids: 52 chance actions (the deal), the calls (52..89), then 52 play actions,
except for a pass-out (exactly 52 + 4 tokens), which has no play.  The play is dropped (``_no_play_trajectory``, sl.py:88-97).

* Deal: chance action k (k = 0..51) gives card c to seat k % 4 counted from the dealer (seat 0).  The OpenSpiel card id c is
  the observation's hand-bit index rank * 4 + suit (suits C,D,H,S; ranks 2..A).  [RECALL, unpinned: the OpenSpiel side of this
  is evidenced by workspace/test_bridge_with_openspiel.py:80-88,186,196 only; there is no pyspiel here to check it against.]
* Calls: OpenSpiel action a in 52..89 is pgx action a - 52 (test_bridge_with_openspiel.py:108,117).

``load_trajectories`` checks every line and rejects the first malformed one with its line number; the checks are numpy passes
over the whole file (the auction check steps all trajectories together, one call position at a time).
"""
from __future__ import annotations

import os
import time
from typing import NamedTuple

import numpy as np

NUM_CARDS = 52
MIN_ACTION = 52      # OpenSpiel id of the first call (Pass)
NUM_CALLS = 38
MAX_AUCTION = 319    # 3 passes + 34 x (bid P P X P P XX P P) + 7NT P P X P P XX P P P


class TrajectorySet(NamedTuple):
    """hands uint64 [N,4]: seat s's cards as observation hand bits; offsets int64 [N+1]; calls uint8 [total]: pgx call ids."""
    hands: np.ndarray
    offsets: np.ndarray
    calls: np.ndarray

    @property
    def n(self) -> int:
        return int(self.hands.shape[0])

    def n_calls(self) -> np.ndarray:
        return np.diff(self.offsets)


class MalformedTrajectory(ValueError):
    pass


def _reject(line_no, what):
    raise MalformedTrajectory(f"line {int(line_no)}: {what}")


def openspiel_to_pgx_card(c):
    """the pgx / oracle card id (suit * 13 + rank, suits S,H,D,C, ranks A,2..K) of OpenSpiel card c = rank * 4 + suit"""
    c = np.asarray(c)
    return (3 - c % 4) * 13 + (c // 4 + 1) % 13


def pack_hands(deal: np.ndarray) -> np.ndarray:
    """deal int [N,52] (OpenSpiel chance actions) -> uint64 [N,4]: bit c of seat k % 4 for chance action k"""
    deal = np.asarray(deal, np.int64).reshape(-1, 13, 4)
    bits = np.left_shift(np.uint64(1), deal.astype(np.uint64))
    return np.bitwise_or.reduce(bits, axis=1)


def auction_errors(calls: np.ndarray, offsets: np.ndarray) -> np.ndarray:
    """per trajectory: 0 = a legal auction that ends exactly at its last call, 1 = an illegal call, 2 = it ends early or not at
    all.  pgx rules (dealer seat 0): Pass always; a bid above the last bid; X of the opponents' undoubled bid; XX of one's own
    side's doubled bid; over after four opening passes or three passes after a bid."""
    n = offsets.shape[0] - 1
    lens = np.diff(offsets)
    err = np.zeros(n, np.int8)
    lb1 = np.zeros(n, np.int64)       # last bid + 1 (0: none)
    lbseat = np.zeros(n, np.int64)
    x = np.zeros(n, bool)
    xx = np.zeros(n, bool)
    npass = np.zeros(n, np.int64)
    over = np.zeros(n, bool)
    err[lens > MAX_AUCTION] = 2
    for k in range(int(min(lens.max(initial=0), MAX_AUCTION))):
        live = (k < lens) & (err == 0)
        if not live.any():
            break
        idx = np.nonzero(live)[0]
        a = calls[offsets[idx] + k].astype(np.int64)
        seat = k % 4
        early = over[idx]
        own = (lbseat[idx] % 2) == (seat % 2)
        has = lb1[idx] > 0
        ok = (a == 0) | ((a == 1) & has & ~own & ~x[idx] & ~xx[idx]) | ((a == 2) & has & own & x[idx] & ~xx[idx]) \
            | ((a >= 3) & (a - 2 > lb1[idx]))
        err[idx[early]] = 2
        err[idx[~early & ~ok]] = 1
        bid = a >= 3
        lb1[idx[bid]] = a[bid] - 2
        lbseat[idx[bid]] = seat
        x[idx[bid]] = False
        xx[idx[bid]] = False
        x[idx[a == 1]] = True
        xx[idx[a == 2]] = True
        npass[idx] = np.where(a == 0, npass[idx] + 1, 0)
        over[idx] = npass[idx] == np.where(lb1[idx] > 0, 3, 4)
    err[(err == 0) & ~over] = 2
    return err


def parse_trajectories(text: str, first_line: int = 1) -> TrajectorySet:
    """the lines of a trajectory file -> TrajectorySet; MalformedTrajectory names the first bad line (1-based).  Lines of
    whitespace only are skipped."""
    lines = text.split("\n")
    ntok = np.fromiter((len(l.split()) for l in lines), np.int64, count=len(lines))
    keep = np.nonzero(ntok > 0)[0]
    ntok = ntok[keep]
    line_no = keep + first_line
    try:
        tokens = np.array(" ".join(lines[i] for i in keep).split(), dtype=np.int64)
    except ValueError:
        bad = next(i for i in keep if not all(t.lstrip("-").isdigit() for t in lines[i].split()))
        _reject(bad + first_line, "not a list of integers")
    if keep.size == 0:
        raise MalformedTrajectory("no trajectories")
    starts = np.concatenate([[0], np.cumsum(ntok)[:-1]])
    passout = ntok == NUM_CARDS + 4
    ncalls = np.where(passout, 4, ntok - 2 * NUM_CARDS)
    bad = np.nonzero(~passout & (ncalls < 4))[0]
    if bad.size:
        _reject(line_no[bad[0]], f"{ntok[bad[0]]} tokens: not 52 + 4 (a pass-out) nor 52 + calls + 52 play actions")
    deal = tokens[starts[:, None] + np.arange(NUM_CARDS)]
    bad = np.nonzero((np.sort(deal, axis=1) != np.arange(NUM_CARDS)).any(axis=1))[0]
    if bad.size:
        _reject(line_no[bad[0]], "the first 52 actions are not a permutation of the 52 cards")
    offsets = np.concatenate([[0], np.cumsum(ncalls)]).astype(np.int64)
    rel = np.arange(offsets[-1]) - np.repeat(offsets[:-1], ncalls)
    raw = tokens[np.repeat(starts + NUM_CARDS, ncalls) + rel]
    bad_call = (raw < MIN_ACTION) | (raw >= MIN_ACTION + NUM_CALLS)
    if bad_call.any():
        t = int(np.searchsorted(offsets, np.nonzero(bad_call)[0][0], side="right") - 1)
        _reject(line_no[t], f"call {int(raw[np.nonzero(bad_call)[0][0]])} outside 52..89")
    calls = (raw - MIN_ACTION).astype(np.uint8)
    err = auction_errors(calls, offsets)
    bad = np.nonzero(err)[0]
    if bad.size:
        t = bad[0]
        _reject(line_no[t], "the auction has an illegal call" if err[t] == 1 else "the auction does not end exactly at its last call")
    return TrajectorySet(pack_hands(deal), offsets, calls)


def load_trajectories(path: str, log=print) -> TrajectorySet:
    t0 = time.perf_counter()
    with open(path) as f:
        text = f.read()
    ts = parse_trajectories(text)
    if log is not None:
        log(f"{os.path.basename(path)}: {ts.n} trajectories, {ts.calls.size} calls, loaded and checked in "
            f"{time.perf_counter() - t0:.2f} s")
    return ts


def decision_points(ts: TrajectorySet):
    """(trajectory, call index) of every call of the set, in file order: int64 [total], int32 [total]"""
    nc = ts.n_calls()
    traj = np.repeat(np.arange(ts.n, dtype=np.int64), nc)
    pos = (np.arange(ts.calls.size) - np.repeat(ts.offsets[:-1], nc)).astype(np.int32)
    return traj, pos


CALL_NAMES = ["Pass", "X", "XX"] + [f"{lv}{s}" for lv in range(1, 8) for s in ("C", "D", "H", "S", "N")]


def hand_string(bits: int) -> str:
    """one seat's cards from its observation hand bits: 'S AK3 H ... D ... C ...'"""
    ranks = "23456789TJQKA"
    out = []
    for suit, name in ((3, "S"), (2, "H"), (1, "D"), (0, "C")):
        cards = "".join(ranks[r] for r in range(12, -1, -1) if (int(bits) >> (r * 4 + suit)) & 1)
        out.append(f"{name} {cards or '-'}")
    return " ".join(out)
