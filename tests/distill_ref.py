"""A numpy restatement of include/brl_distill.h: the ensemble's soft targets, the distillation loss, its gradients and its metrics
row.  No tests in here.  ``restate(..., dtype=np.float64)`` is the reference; ``dtype=np.float32`` runs the same formulas, every
operation in float32 and the sums over the calls in the header's order, which is what the GPU tests take their tolerance from
(``tolerance``).  The rows' terms are added as float64 in both.

The one liberty: log q is formed with the maximum over the teachers taken first (the header's kernel keeps a running maximum and
rescales); in exact arithmetic the two are the same number."""
import numpy as np

NA = 38
METRICS = ("total", "policy_loss", "value_loss", "teacher_entropy", "student_entropy", "agreement", "illegal_actions_prob")


def _lsm(x, mask, tau, dt):
    """lsm_j of the masked softmax of x / tau, [B, 38] (junk on illegal calls)"""
    y = (x.astype(dt) / dt(tau)).astype(dt)
    mx = np.max(np.where(mask, y, dt(-np.inf)), axis=1)     # (np.max keeps a NaN)
    s = np.zeros(x.shape[0], dt)
    for j in range(NA):
        s = (s + np.where(mask[:, j], np.exp(y[:, j] - mx), dt(0))).astype(dt)
    return ((y - mx[:, None]) - np.log(s)[:, None]).astype(dt)


def _cross(q, logv, mask, dt):
    """sum over the legal calls with q_j > 0 of q_j * logv_j (0 log 0 = 0; a NaN q stays)"""
    acc = np.zeros(q.shape[0], dt)
    for j in range(NA):
        acc = (acc + np.where(mask[:, j] & ~(q[:, j] <= 0), q[:, j] * logv[:, j], dt(0))).astype(dt)
    return acc


def _first_max(x, mask):
    """the first maximum over the legal calls; a NaN is never a maximum; 0 where nothing is above -inf"""
    best = np.full(x.shape[0], -np.inf, x.dtype)
    arg = np.zeros(x.shape[0], np.int64)
    for j in range(NA):
        c = mask[:, j] & (x[:, j] > best)
        arg = np.where(c, j, arg)
        best = np.where(c, x[:, j], best)
    return arg


def targets(t, v, w, mask, tau, dtype=np.float64):
    """t [K, B, 38], v [K, B], w [K] (normalised), mask bool [B, 38] -> q [B, 38], vstar [B], hq [B]"""
    dt = dtype
    mask = np.asarray(mask, bool)
    K, B = t.shape[0], t.shape[1]
    w = np.asarray(w).astype(dt)
    with np.errstate(all="ignore"):
        q = np.zeros((B, NA), dt)
        vstar = np.zeros(B, dt)
        a = []
        for k in range(K):
            l = _lsm(t[k], mask, tau, dt)
            q = (q + np.where(mask, w[k] * np.exp(l), dt(0))).astype(dt)
            a.append((np.log(w[k]) + l).astype(dt))
            vstar = (vstar + w[k] * v[k].astype(dt)).astype(dt)
        a = np.stack(a)
        M = np.max(a, axis=0)
        s = np.zeros((B, NA), dt)
        for k in range(K):
            s = (s + np.where(a[k] == -np.inf, dt(0), np.exp(a[k] - M))).astype(dt)
        logq = (M + np.log(s)).astype(dt)
        hq = -_cross(q, logq, mask, dt)
    return q, vstar, hq


def loss(z, u, q, vstar, hq, mask, tau, c_pol=1.0, c_val=0.5, dtype=np.float64):
    """-> dict: dz [B, 38], du [B], per-row policy_loss / value_loss, metrics float64 [8]"""
    dt = dtype
    mask = np.asarray(mask, bool)
    B = z.shape[0]
    z, u, q, vstar, hq = (np.asarray(x).astype(dt) for x in (z, u, q, vstar, hq))
    tau_, cp, cv, nb = dt(tau), dt(c_pol), dt(c_val), dt(B)
    with np.errstate(all="ignore"):
        l = _lsm(z, mask, tau, dt)
        p = np.where(mask, np.exp(l), dt(0)).astype(dt)
        H = -_cross(p, l, mask, dt)
        ce = -_cross(q, l, mask, dt)
        lpol = ((tau_ * tau_) * (ce - hq)).astype(dt)
        d = (u - vstar).astype(dt)
        lval = (d * d).astype(dt)
        dz = np.where(mask, ((cp * tau_) / nb) * (p - q), dt(0)).astype(dt)
        du = (((dt(2) * cv) / nb) * d).astype(dt)
        mx2 = np.max(z, axis=1)
        s2 = np.zeros(B, dt)
        for j in range(NA):
            s2 = (s2 + np.exp(z[:, j] - mx2)).astype(dt)
        lse2 = np.log(s2)
        ill = np.zeros(B, dt)
        for j in range(NA):
            ill = (ill + np.where(mask[:, j], dt(0), np.exp((z[:, j] - mx2) - lse2))).astype(dt)
        agree = _first_max(z, mask) == _first_max(q, mask)
        mean = lambda x: np.sum(np.asarray(x, np.float64)) / float(B)     # noqa: E731
        pol, val = mean(lpol), mean(lval)
        metrics = np.array([float(c_pol) * pol + float(c_val) * val, pol, val, mean(hq), mean(H), mean(agree), mean(ill), 0.0])
    return {"dz": dz, "du": du, "policy_loss": lpol, "value_loss": lval, "metrics": metrics}


def restate(z, u, t, v, w, mask, tau, c_pol=1.0, c_val=0.5, dtype=np.float64):
    """targets and loss in one: dict with q, vstar, hq, dz, du, policy_loss, value_loss, metrics"""
    q, vstar, hq = targets(np.asarray(t), np.asarray(v), w, mask, tau, dtype)
    out = loss(z, u, q, vstar, hq, mask, tau, c_pol, c_val, dtype)
    out.update(q=q, vstar=vstar, hq=hq)
    return out


def total(z, u, t, v, w, mask, tau, c_pol=1.0, c_val=0.5):
    """the float64 total alone (what the finite differences differentiate)"""
    return float(restate(z, u, t, v, w, mask, tau, c_pol, c_val)["metrics"][0])


def tolerance(want64, got32):
    """the GPU tests' bound on max |device - want64| for one quantity (an array, or one metric): 4 x the largest error of the
    float32 restatement on the same inputs, never less than 4 * 2^-24 * max |want64|"""
    want64, got32 = np.asarray(want64, np.float64), np.asarray(got32, np.float64)
    err32 = float(np.max(np.abs(got32 - want64))) if want64.size else 0.0
    return max(4.0 * err32, 4.0 * 2.0 ** -24 * float(np.max(np.abs(want64))))


def inputs(B, K, seed):
    """the GPU tests' rows: N(0, 4) logits, 32 rows of +-60 logits, rows with only Pass legal, an all-legal row, unequal weights"""
    rng = np.random.default_rng(seed)
    z = rng.normal(0, 4, (B, NA)).astype(np.float32)
    t = rng.normal(0, 4, (K, B, NA)).astype(np.float32)
    big = min(32, B)
    z[:big] = (rng.choice([-60.0, 60.0], (big, NA)) * rng.random((big, NA))).astype(np.float32)
    t[:, :big] = (rng.choice([-60.0, 60.0], (K, big, NA)) * rng.random((K, big, NA))).astype(np.float32)
    mask = rng.random((B, NA)) < 0.4
    mask[:, 0] = True
    mask[40:50] = False         # only Pass legal (the +-60 rows' first when B is small)
    mask[min(3, B - 1)] = False
    mask[:, 0] = True
    mask[B - 1] = True          # all legal
    u = rng.normal(0, 1, B).astype(np.float32)
    v = rng.normal(0, 1, (K, B)).astype(np.float32)
    w = np.arange(1, K + 1, dtype=np.float64) ** 2
    w = (w / w.sum()).astype(np.float32)
    return z, u, t, v, w, mask
