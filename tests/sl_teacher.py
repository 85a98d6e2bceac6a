"""Synthetic trajectory files for the supervised pre-trainer's tests (brl_amd/sl.py) and the host restatements they check it
against.  No dataset is needed: deals are random, auctions are random legal ones or follow a simple teacher.

* ``sample``: the example stream (brl_sl_sample, include/brl_sl.h) in numpy.
* ``host_batch``: the observation rows, legal masks and labels of given (trajectory, call index) pairs through the oracle.
* ``loss64``: sl.py's loss, its metrics and d total / d logits in float64; ``loss32``: the same formulas in numpy float32, the
  reference's own precision — the yardstick of the loss kernel's per-row derivative bound.
* ``logits64`` / ``sl_step64``: one supervised step in float64 — the forward of tests/ppo_numpy.py, ``loss64``, the written-out
  backward with no value gradient -> the metrics row and the gradients (checked against torch autograd in float64 by
  tests/test_sl_host.py); ``top_two_gap`` for the rows whose argmax fp32 may decide otherwise.
"""
import numpy as np

PASS, X, XX = 0, 1, 2


def legal_calls(lb1, lbseat, x, xx, seat):
    out = [PASS]
    if lb1 > 0:
        own = (lbseat % 2) == (seat % 2)
        if not own and not x and not xx:
            out.append(X)
        if own and x and not xx:
            out.append(XX)
    out += list(range(3 + lb1, 38))
    return out


def random_auction(rng, p_pass=0.55, p_double=0.3):
    """a random legal auction (pgx call ids), doubles and redoubles included, ended by the rules"""
    calls, lb1, lbseat, x, xx, npass = [], 0, 0, False, False, 0
    while True:
        seat = len(calls) % 4
        legal = legal_calls(lb1, lbseat, x, xx, seat)
        dbl = [a for a in legal if a in (X, XX)]
        bids = [a for a in legal if a >= 3]
        u = rng.random()
        if dbl and u < p_double:
            a = dbl[0]
        elif u < p_pass or not bids:
            a = PASS
        else:
            a = bids[min(int(rng.integers(0, 4)), len(bids) - 1)]
        calls.append(a)
        if a >= 3:
            lb1, lbseat, x, xx = a - 2, seat, False, False
        elif a == X:
            x = True
        elif a == XX:
            xx = True
        npass = npass + 1 if a == PASS else 0
        if npass == (3 if lb1 else 4):
            return calls


def maximal_auction():
    """the longest legal auction: 3 passes, then every bid doubled and redoubled with passes between (319 calls)"""
    calls = [PASS] * 3
    for b in range(35):
        calls += [3 + b, PASS, PASS, X, PASS, PASS, XX, PASS, PASS]
    calls.append(PASS)
    assert len(calls) == 319
    return calls


def teacher_auction(deal):
    """the first seat with a 5+ card suit bids 1 of its longest (lowest on ties); everyone else passes"""
    deal = np.asarray(deal)
    calls = []
    for seat in range(4):
        cards = deal[seat::4]                    # chance action k goes to seat k % 4
        lengths = np.bincount(cards % 4, minlength=4)   # OpenSpiel card c = rank * 4 + suit (C,D,H,S)
        if lengths.max() >= 5:
            suit = int(np.argmax(lengths))       # first maximum = the lowest suit
            return calls + [3 + suit, PASS, PASS, PASS]
        calls.append(PASS)
    return calls


def line(deal, calls, rng=None):
    """one trajectory line: the deal, the calls (OpenSpiel ids), the play (52 actions) unless it is a pass-out"""
    toks = list(map(int, deal)) + [c + 52 for c in calls]
    if calls != [PASS] * 4:
        play = rng.permutation(52) if rng is not None else np.arange(52)
        toks += list(map(int, play))
    return " ".join(map(str, toks))


def random_file(n, seed, kind="random"):
    """n lines; kind 'random': random legal auctions (a few pass-outs and one maximal auction among them); 'teacher'"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        deal = rng.permutation(52)
        if kind == "teacher":
            calls = teacher_auction(deal)
        elif i == 1:
            calls = maximal_auction()
        elif i % 50 == 7:
            calls = [PASS] * 4
        else:
            calls = random_auction(rng)
        out.append(line(deal, calls, rng))
    return "\n".join(out) + "\n"


# ---- numpy restatement of brl_sl_sample ---------------------------------------------------------------------------------------
STREAM_SL_PERM = 0x42534C50
STREAM_SL_POS = 0x42534C43
M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    c = [np.asarray(v, np.uint64) & M32 for v in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = np.uint64(k0) & M32, np.uint64(k1) & M32
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        h0, l0 = p0 >> np.uint64(32), p0 & M32
        h1, l1 = p1 >> np.uint64(32), p1 & M32
        c = [h1 ^ c[1] ^ k0, l1, h0 ^ c[3] ^ k1, l0]
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return c


def feistel(x, half, e, seed):
    m = np.uint64((1 << half) - 1)
    x = np.asarray(x, np.uint64)
    L, R = x >> np.uint64(half), x & m
    for r in range(4):
        o = philox4x32_10(R, r, e, STREAM_SL_PERM, seed & 0xFFFFFFFF, seed >> 32)
        L, R = R, L ^ (o[0] & m)
    return (L << np.uint64(half)) | R


def half_bits(n):
    h = 1
    while (1 << (2 * h)) < n:
        h += 1
    return h


def sample(offsets, seed, counter, batch):
    """(traj int64 [batch], pos int32 [batch]) of examples counter .. counter + batch - 1"""
    offsets = np.asarray(offsets, np.int64)
    n = offsets.shape[0] - 1
    g = counter + np.arange(batch, dtype=np.int64)
    e = (g // n).astype(np.uint64)
    x = (g % n).astype(np.uint64)
    half = half_bits(n)
    x = feistel(x, half, e, seed)
    while (x >= n).any():
        bad = x >= n
        x[bad] = feistel(x[bad], half, e[bad], seed)
    o = philox4x32_10(g.astype(np.uint64) & M32, g.astype(np.uint64) >> np.uint64(32), 0, STREAM_SL_POS, seed & 0xFFFFFFFF,
                      seed >> 32)
    t = x.astype(np.int64)
    nc = (offsets[t + 1] - offsets[t]).astype(np.uint64)
    pos = ((o[0] * nc) >> np.uint64(32)).astype(np.int32)
    return t, pos


# ---- float64 restatement of sl.py's loss and its gradient ---------------------------------------------------------------------
def loss64(logits, label, mask, ent_coef):
    """(out[5], dlogits) in float64: total, target_loss, entropy, accuracy, illegal_prob; d total / d logits"""
    z = np.asarray(logits, np.float64)
    B = z.shape[0]
    m = np.asarray(mask, bool)
    onehot = np.zeros_like(z)
    onehot[np.arange(B), label] = 1.0
    ls2 = z - z.max(1, keepdims=True)
    ls2 = ls2 - np.log(np.exp(ls2).sum(1, keepdims=True))
    p2 = np.exp(ls2)
    zm = np.where(m, z, -np.inf)
    lsm = zm - zm.max(1, keepdims=True)
    lsm = lsm - np.log(np.exp(lsm).sum(1, keepdims=True))
    p = np.where(m, np.exp(lsm), 0.0)
    plogp = np.where(p == 0, 0.0, p * np.where(m, lsm, 0.0))      # 0 log 0 = 0; a NaN probability stays NaN (distrax)
    H = -plogp.sum(1)
    tgt = -(onehot * ls2).mean()
    out = np.array([tgt - ent_coef * H.mean(), tgt, H.mean(), (np.argmax(z, 1) == label).mean(), (p2 * ~m).sum(1).mean()])
    d = (p2 - onehot) / (38 * B) + ent_coef * np.where(m, p * (np.where(m, lsm, 0.0) + H[:, None]), 0.0) / B
    return out, d


def loss32(logits, label, mask, ent_coef):
    """`loss64`'s formulas evaluated in numpy float32 throughout (the reference computes in float32) -> (out[5], dlogits), float32"""
    f = np.float32
    z = np.asarray(logits, f)
    B = z.shape[0]
    m = np.asarray(mask, bool)
    onehot = np.zeros_like(z)
    onehot[np.arange(B), label] = f(1.0)
    ls2 = z - z.max(1, keepdims=True)
    ls2 = ls2 - np.log(np.exp(ls2).sum(1, keepdims=True, dtype=f))
    p2 = np.exp(ls2)
    zm = np.where(m, z, f(-np.inf))
    lsm = zm - zm.max(1, keepdims=True)
    lsm = lsm - np.log(np.exp(lsm).sum(1, keepdims=True, dtype=f))
    p = np.where(m, np.exp(lsm), f(0.0))
    lsm0 = np.where(m, lsm, f(0.0))
    plogp = np.where(p == 0, f(0.0), p * lsm0)
    H = -plogp.sum(1, dtype=f)
    tgt = -(onehot * ls2).mean(dtype=f)
    Hm = H.mean(dtype=f)
    out = np.array([tgt - f(ent_coef) * Hm, tgt, Hm, (np.argmax(z, 1) == label).mean(dtype=f), (p2 * ~m).sum(1, dtype=f).mean(dtype=f)], f)
    d = (p2 - onehot) / f(38 * B) + f(ent_coef) * np.where(m, p * (lsm0 + H[:, None]), f(0.0)) / f(B)
    assert out.dtype == f and d.dtype == f
    return out, d


# ---- the examples of given (trajectory, call index) pairs through the oracle ---------------------------------------------------
def host_batch(ts, traj, pos, oracle):
    """(obs float32 [B, 480], mask uint8 [B, 38], label int32 [B]) of examples (traj[i], pos[i]) of the TrajectorySet `ts`: the
    converted deal (seat s holds the cards of its hand bits), dealer 0, nobody vulnerable, identity seating; the oracle steps each
    trajectory's calls and is observed for the seat to act before call pos[i].  Every trajectory is stepped through its largest
    requested call: the auction is over behind that call exactly where it is the trajectory's last."""
    from brl_amd import sl_data
    traj, pos = np.asarray(traj, np.int64), np.asarray(pos, np.int64)
    B = traj.shape[0]
    obs, mask = np.zeros((B, 480), np.float32), np.zeros((B, 38), np.uint8)
    nc_all = ts.n_calls()
    assert B > 0 and (traj >= 0).all() and (traj < ts.n).all() and (pos >= 0).all() and (pos < nc_all[traj]).all()
    uniq, inv = np.unique(traj, return_inverse=True)
    last = np.zeros(uniq.size, np.int64)
    np.maximum.at(last, inv, pos)
    cards = np.arange(52)
    hand = np.stack([np.concatenate([sl_data.openspiel_to_pgx_card(cards[((int(ts.hands[t, s]) >> cards) & 1) == 1]) for s in range(4)])
                     for t in uniq])
    st = oracle.init_explicit(hand, 0, 0, 0, [0, 1, 2, 3], np.zeros((uniq.size, 20), np.uint8))
    nc, start = nc_all[uniq], ts.offsets[uniq]
    for k in range(int(last.max()) + 1):
        want = np.nonzero(pos == k)[0]
        if want.size:
            sub = st[inv[want]]
            assert not sub["terminated"].any()
            obs[want] = oracle.observe(sub, sub["current_player"]).astype(np.float32)
            mask[want] = sub["legal_action_mask"]
        live = np.nonzero(k <= last)[0]
        sub = st[live]
        oracle.step(sub, ts.calls[start[live] + k].astype(np.int32))
        assert np.array_equal(sub["terminated"].astype(bool), k == nc[live] - 1), f"the auction's end is not at its last call (call {k})"
        st[live] = sub
    label = ts.calls[ts.offsets[traj] + pos].astype(np.int32)
    return obs, mask, label


# ---- one supervised step in float64 ---------------------------------------------------------------------------------------------
def logits64(params, obs, activation, model, gate_fn=None):
    """(logits, tape for `_backward`) of tests/ppo_numpy.forward (model "DeepMind...") or fair_forward ("FAIR") in float64"""
    from tests import ppo_numpy as N
    x = np.asarray(obs, np.float64)
    if model == "FAIR":
        logits, _, h, tape = N.fair_forward(params, x, activation, gate_fn)
        return logits, (h, tape)
    logits, _, hs, _, dacts = N.forward(params, x, activation, gate_fn)
    return logits, (hs, dacts)


def top_two_gap(logits):
    """per row: the largest logit minus the second largest (0 at a tie)"""
    s = np.sort(np.asarray(logits, np.float64), axis=1)
    return s[:, -1] - s[:, -2]


def sl_step64(params, obs, mask, label, ent_coef, activation, model, gate_fn=None):
    """One step of brl_amd.sl.SLStep in float64 -> (metrics row [total, target, entropy, accuracy, illegal] of the forward on
    `params`, grads like params): the forward, `loss64`, the factored backward of tests/ppo_numpy.py with d loss / d value = 0
    (the value head takes no part in the supervised loss: its gradients are zeros)."""
    from tests import ppo_numpy as N
    logits, tape = logits64(params, obs, activation, model, gate_fn)
    row, d = loss64(logits, np.asarray(label, np.int64), mask, ent_coef)
    dv = np.zeros(logits.shape[0])
    grads = N.fair_backward(params, d, dv, *tape, activation) if model == "FAIR" else N.backward(params, d, dv, *tape)
    return row, grads
