"""A DeepMind-architecture ActorCritic (480 -> 4 x 1024 ReLU -> 38 + 1) that bids like a bridge player, a host simulation of the
macro-step rollout on it, and the census of the boards it finishes.  No tests in here.

``ForwardPass.init`` networks have nearly flat logits: a rollout on them is random play (99.8 % of auctions end at the 7 level, down;
no pass-out).  A hand-written part of this network's weights computes a point-count bidder from the observation instead:

  layer 0   reads the 480 bits (layout: bridge_oracle.c A3): high-card points of the own hand (4/3/2/1 on the A/K/Q/J bits at
            428 + rank * 4 + suit), the four suit lengths, "how many bids at level >= L were made" for L = 1..7 (sums of the bid bits),
            the bids of the own side and of the other side, partner's bids by strain, the doubled bits, both vulnerability bits;
  layer 1-2 carry the counts (identity rows: counts are >= 0, a ReLU leaves them alone) and form 0 / 1 indicators from them as
            relu(c) - relu(c - 1): "a bid at level >= L was made", "own side / other side has bid", "a double was made", "12+ points";
  layer 3   carries everything to the heads;
  heads     pass falls with points; a bid rises with points, with length in its strain and with partner's bids in it, falls by 2 per
            level, or per level already reached, and by 4 more once its own level was reached (so insufficient bids are unlikely, not impossible: the unmasked policy does draw
            some); double and redouble get small logits; value = (points - 10) / 16 +- 1/8 for who has bid.

Every constructed weight and bias is a multiple of 1/16 that bf16 holds exactly (asserted), every constructed bias is non-zero: a unit
holds its count PLUS an offset (0.25 more per layer it is carried through) that the next layer's bias takes off again, so a dropped
bias shows.  Logits stay within +-30 (test_bidder_host.py).  Every other weight and bias gets `tests.nets.perturbed`-style noise, small against the constructed
part: no hidden unit is idle, no bias is zero.  `temperature` divides the policy head; powers of two keep it exact.
"""
import numpy as np
import torch

from tests import categorical_ref as cref

PASS, DBL, RDBL, BID0 = 0, 1, 2, 3
CARD0, HIST0 = 428, 8            # own cards at 428 + rank * 4 + suit; bid b's twelve bits at 8 + b * 12 (made / doubled / redoubled x seat)
STYLE = {"pass": 12.5, "own": 2.5, "opp": 1.0, "double": -3.0, "redouble": -3.0}     # the constants of the rule that were tuned (test_bidder_host.py)
STEP = 0.25                      # a carried unit's offset grows by this per layer, so that every constructed bias is non-zero


class _Circuit:
    """Named units in the four hidden layers of a 480 -> 4 x 1024 -> 39 network.  A unit holds relu(value + offset); `unit` writes
    the weights and the bias that make it so from the named units of the layer before (whose offsets the bias takes off)."""

    def __init__(self, hidden=1024, layers=4):
        ins = [480] + [hidden] * (layers - 1)
        self.W = [torch.zeros(hidden, k, dtype=torch.float64) for k in ins] + [torch.zeros(39, hidden, dtype=torch.float64)]
        self.B = [torch.zeros(hidden, dtype=torch.float64) for _ in ins] + [torch.zeros(39, dtype=torch.float64)]
        self.Wset = [torch.zeros_like(w, dtype=torch.bool) for w in self.W]
        self.Bset = [torch.zeros_like(b, dtype=torch.bool) for b in self.B]
        self.names = [{} for _ in ins]     # per hidden layer: name -> (unit, offset)

    def _row(self, layer, row, terms, const):
        for src, coef in terms.items():
            col, off = (src, 0.0) if layer == 0 else self.names[layer - 1][src]
            self.W[layer][row, col] += coef
            self.Wset[layer][row, col] = True
            const -= coef * off
        self.B[layer][row] = const
        self.Bset[layer][row] = True
        assert const != 0.0, (layer, row)

    def unit(self, layer, name, terms, const=0.0, off=STEP):
        assert name not in self.names[layer]
        row = len(self.names[layer])
        self.names[layer][name] = (row, off)
        self._row(layer, row, terms, const + off)

    def carry(self, layer, *names, to=None):
        for name in names:
            self.unit(layer, to.format(name) if to else name, {name: 1.0}, off=self.names[layer - 1][name][1] + STEP)

    def head(self, row, terms, const, scale=1.0):
        self._row(len(self.names), row, {k: v * scale for k, v in terms.items()}, const * scale)


def _circuit(temperature):
    c = _Circuit()
    card = lambda rank, suit: CARD0 + rank * 4 + suit            # noqa: E731  rank 0..12 = 2..A, suit 0..3 = C, D, H, S
    bit = lambda b, kind, rel: HIST0 + b * 12 + kind * 4 + rel   # noqa: E731  kind 0 made / 1 doubled / 2 redoubled; rel 0 me, 2 partner
    bids = range(35)                                             # b = (level - 1) * 5 + strain, strain C, D, H, S, NT
    # ---- layer 0: counts read from the observation
    c.unit(0, "hcp", {card(8 + p, s): float(p) for p in (1, 2, 3, 4) for s in range(4)})
    for s in range(4):
        c.unit(0, f"len{s}", {card(r, s): 1.0 for r in range(13)})
    for L in range(1, 8):
        c.unit(0, f"lvl{L}", {bit(b, 0, rel): 1.0 for b in bids if b // 5 + 1 >= L for rel in range(4)})
    c.unit(0, "own", {bit(b, 0, rel): 1.0 for b in bids for rel in (0, 2)})
    c.unit(0, "opp", {bit(b, 0, rel): 1.0 for b in bids for rel in (1, 3)})
    for d in range(5):
        c.unit(0, f"p{d}", {bit(b, 0, 2): 1.0 for b in bids if b % 5 == d})
    c.unit(0, "dbl", {bit(b, 1, rel): 1.0 for b in bids for rel in range(4)})
    c.unit(0, "vul_we", {1: 1.0})
    c.unit(0, "vul_they", {3: 1.0})
    kept = ["hcp", "vul_we", "vul_they"] + [f"len{s}" for s in range(4)] + [f"p{d}" for d in range(5)]
    counts = [f"lvl{L}" for L in range(1, 8)] + ["own", "opp", "dbl"]
    # ---- layer 1: the two halves of every indicator, min(1, c) = relu(c) - relu(c - 1)
    c.carry(1, *kept)
    c.carry(1, *counts, to="{}_a")
    for name in counts:
        c.unit(1, name + "_b", {name: 1.0}, const=-1.0, off=0.0)
    c.unit(1, "h12_a", {"hcp": 1.0}, const=-11.0, off=0.0)
    c.unit(1, "h12_b", {"hcp": 1.0}, const=-12.0, off=0.0)
    # ---- layer 2: the indicators
    c.carry(2, *kept)
    for name in counts:
        c.unit(2, "i" + name, {name + "_a": 1.0, name + "_b": -1.0})
    c.unit(2, "open", {"h12_a": 1.0, "h12_b": -1.0})
    # ---- layer 3
    ind = ["i" + name for name in counts] + ["open"]
    c.carry(3, *kept, *ind)
    # ---- heads
    s = 1.0 / temperature
    reach = {f"ilvl{L}": 0.5 for L in range(1, 8)}
    c.head(PASS, {"hcp": -0.375, "open": -1.0}, STYLE["pass"], s)
    c.head(DBL, dict(reach, hcp=0.25, iopp=3.0, vul_they=0.25), STYLE["double"], s)
    c.head(RDBL, {"hcp": 0.25, "idbl": 5.0}, STYLE["redouble"], s)
    for b in bids:
        level, d = b // 5 + 1, b % 5
        terms = {"hcp": 0.375, f"ilvl{level}": -4.0, "iown": STYLE["own"], "iopp": STYLE["opp"], f"p{d}": 1.0, "vul_we": -0.25}
        terms.update({f"ilvl{L}": -2.0 for L in range(level + 1, 8)})      # (a bid below the level reached gains nothing by being low)
        if d < 4:
            terms[f"len{d}"] = 0.75
        c.head(BID0 + b, terms, -2.0 * level + (3.0 if d == 4 else 0.0), s)
    c.head(38, {"hcp": 0.0625, "iown": 0.125, "iopp": -0.125}, -0.625)     # value = (points - 10) / 16 +- 1/8
    return c


def bidder(seed, device="cpu", temperature=1.0, w=0.044, b=0.03):
    """-> ActorCritic("relu", "DeepMind") on `device` holding the constructed bidder; every parameter that is not part of it gets noise
    from a host generator seeded with `seed`: N(0, b) on the biases, N(0, w) on the weights between two units that hold only noise
    (sqrt(2 / 1024): a ReLU layer then keeps the scale; each such row shifted to sum to zero, or the common mean of the positive
    units before it would decide the unit's sign and leave a few idle by the last layer), N(0, w / 32) on the other weights of a constructed unit's row (what it reads besides its
    rule) and column (who else reads it), N(0, w / 128) where both are constructed.  The counts are always positive and up to a
    hundred times a noise unit's output: read at full scale they would decide a noise unit's sign for every input and leave one in
    fourteen idle, and would move each other by +-0.1 per layer, the logits by up to 3.  A pure function of its arguments."""
    from brl_amd.models import ActorCritic
    c = _circuit(temperature)
    net = ActorCritic(38, "relu", "DeepMind")
    gen = torch.Generator().manual_seed(seed)
    layers = list(net.body) + [None]
    with torch.no_grad():
        for i, lin in enumerate(layers):
            W, B, Ws, Bs = c.W[i].float(), c.B[i].float(), c.Wset[i], c.Bset[i]
            assert torch.equal(W.double(), c.W[i]) and torch.equal(B.double(), c.B[i])
            assert torch.equal(W.bfloat16().float(), W) and torch.equal(B.bfloat16().float(), B), f"layer {i}: not exact in bf16"
            rows, cols = Bs[:, None], c.Bset[i - 1][None, :] if i else torch.zeros(1, 480, dtype=torch.bool)
            std = torch.where(rows & cols, w / 128, torch.where(rows | cols, w / 32, w)).float()
            params = [(net.actor.weight, W[:38], Ws[:38], std[:38]), (net.actor.bias, B[:38], Bs[:38], b),
                      (net.critic.weight, W[38:], Ws[38:], std[38:]), (net.critic.bias, B[38:], Bs[38:], b)] if lin is None \
                else [(lin.weight, W, Ws, std), (lin.bias, B, Bs, b)]
            for q, val, isset, scale in params:
                noise = torch.randn(q.shape, generator=gen, dtype=q.dtype) * scale
                if q.dim() == 2 and i and lin is not None:      # a noise unit's weights on the noise units before it: zero sum
                    free = (~rows & ~cols).float()
                    noise = noise - free * (noise * free).sum(1, keepdim=True) / free.sum(1, keepdim=True).clamp(min=1.0)
                q.copy_(torch.where(isset, val, noise))
    return net.to(device)


ACTOR, OPPONENT = {"seed": 1, "temperature": 1.0}, {"seed": 2, "temperature": 2.0}


def pair(device="cpu"):
    """the two parameter sets the rollout tests play: the actor, and an opponent with other noise and a flatter policy"""
    return bidder(device=device, **ACTOR), bidder(device=device, **OPPONENT)


def rule(obs, temperature=1.0):
    """The constructed part alone, in float64, on [n, 480] observations -> ({name: what the unit of that name holds in the last hidden
    layer, offset taken off}, [n, 39] logits and value of the rule)."""
    c = _circuit(temperature)
    h = torch.from_numpy(np.ascontiguousarray(obs)).double()
    for W, B in zip(c.W[:-1], c.B[:-1]):
        h = torch.relu(h @ W.t() + B)
    named = {name: (h[:, unit] - off).numpy() for name, (unit, off) in c.names[-1].items()}
    return named, (h @ c.W[-1].t() + c.B[-1]).numpy()


# -------------------------------------------------------------------------------------------------------------------------------
# host simulation of the macro-step rollout (src/utils.py:69-128, src/roll_out.py:63-103)
# -------------------------------------------------------------------------------------------------------------------------------
EVENT_FIELDS = ("last_bid", "last_bidder", "call_x", "call_xx", "first_denomination_ns", "first_denomination_ew", "vul_ns", "vul_ew",
                "tricks", "rewards", "shuffled_players", "illegal", "turn")


def host_forward(net, obs):
    """fp32 forward of the module on the host -> [n, 38] float64 logits"""
    with torch.no_grad():
        logits, _ = net(torch.from_numpy(np.ascontiguousarray(obs)).float())
    return logits.double().numpy()


def step_with_events(oracle, ref, action, seed, env_offset, t, k, actor, events):
    """`Oracle.step(..., autoreset=True)` on `ref`; the boards that this call finished are first read off a copy stepped WITHOUT the
    re-deal (contract, doubling, declarer, vulnerability, tricks and rewards are still there) and appended to `events`."""
    pre = ref.copy()
    pre["terminated"] = 0          # what auto_reset clears before it steps (src/utils.py:34-43)
    pre["truncated"] = 0
    pre["step_count"] = 0
    oracle.step(pre, action)
    idx = np.nonzero(pre["terminated"])[0]
    if len(idx):
        ev = {f: pre[f][idx].copy() for f in EVENT_FIELDS}
        ev.update(table=idx, t=np.full(len(idx), t), k=np.full(len(idx), k), actor=actor[idx].copy())
        events.append(ev)
    oracle.step(ref, action, autoreset=True, seed=seed, env_offset=env_offset)
    assert np.array_equal(ref["terminated"], pre["terminated"]) and np.array_equal(ref["rewards"], pre["rewards"])


def draws24(oracle, seed, env_offset, n, index):
    """the 24-bit action draws of tables env_offset .. env_offset + n at draw index `index` (mod 2^32)"""
    return np.array([oracle.action_draw(seed, env_offset + i, index & 0xFFFFFFFF) >> 8 for i in range(n)], dtype=np.int64)


def sample64(logits, cand, u24):
    """`categorical_ref.inverse_cdf64`, row by row: the first action whose float64 CDF exceeds u24 / 2^24"""
    return np.argmax(cref.cdf64(logits, cand) > (u24.astype(np.float64) * cref.U24)[:, None], axis=1).astype(np.int32)


def simulate(oracle, net, opp, n, T, seed, game_mode="competitive", masked=True, env_offset=0, rng0=0, observations=None):
    """The macro-step loop on the host: per macro-step the actor network calls (sampled; from all 38 calls if not `masked`), then
    opponent, actor network (the partner's seat), opponent; competitive: all sampled under the mask; free-run: the opponents pass and
    the partner takes the mode.  The draw of sub-step k of macro-step t is Oracle.action_draw(seed, env_offset + i, rng0 + 4 t + k).
    `observations`: a list that receives every observation a network was given.
    -> (events of the finished boards for `census`, the largest |logit| either network produced)"""
    ref = oracle.init_random(n, seed=seed, env_offset=env_offset)
    events, top = [], 0.0
    for t in range(T):
        actor = ref["current_player"].copy()
        for k in range(4):
            mask = ref["legal_action_mask"].copy()
            if game_mode != "competitive" and k in (1, 3):
                a = np.zeros(n, np.int32)
            else:
                logits = host_forward(opp if k in (1, 3) else net, ref["observation"])
                top = max(top, float(np.abs(logits).max()))
                if observations is not None:
                    observations.append(ref["observation"].copy())
                if game_mode != "competitive" and k == 2:
                    a = cref.mode64(logits, mask).astype(np.int32)
                else:
                    cand = np.ones_like(mask) if (k == 0 and not masked) else mask
                    a = sample64(logits, cand, draws24(oracle, seed, env_offset, n, rng0 + 4 * t + k))
            step_with_events(oracle, ref, a, seed, env_offset, t, k, actor, events)
    return events, top


# -------------------------------------------------------------------------------------------------------------------------------
# census of finished boards
# -------------------------------------------------------------------------------------------------------------------------------
ROLES = ("declaring", "defending", "pass-out")


def census(events):
    """A list of finished-board chunks (`step_with_events`) -> counts: boards, pass-outs, boards ended by an illegal call, made and
    failed contracts, contracts by level and by doubling, boards by ending sub-step k, the 4 x 3 cells k x (actor on the declaring
    side, on the defending side, pass-out), distinct (contract, doubling, vulnerability, tricks) outcomes, auction lengths, and
    `chained`: pass-outs that follow the end of the table's previous board by exactly four calls."""
    if not events:
        ev = {f: np.zeros((0,), np.int64) for f in ("table", "t", "k", "actor", "last_bid", "illegal", "turn")}
    else:
        ev = {f: np.concatenate([e[f] for e in events]) for f in events[0]}
    nb = len(ev["table"])
    out = {"boards": nb, "illegal": int(ev["illegal"].sum()) if nb else 0}
    cells = np.zeros((4, 3), np.int64)
    levels, doubling, outcomes = np.zeros(8, np.int64), np.zeros(3, np.int64), set()
    made = down = passout = 0
    for j in range(nb):
        k = int(ev["k"][j])
        if ev["illegal"][j]:
            continue
        lb = int(ev["last_bid"][j])
        if lb < 0:
            passout += 1
            cells[k, 2] += 1
            assert not ev["rewards"][j].any()
            continue
        seats = ev["shuffled_players"][j]
        seat = lambda p: int(np.nonzero(seats == p)[0][0])      # noqa: E731
        ns = seat(int(ev["last_bidder"][j])) % 2 == 0
        d, level = lb % 5, lb // 5 + 1
        declarer = int((ev["first_denomination_ns"] if ns else ev["first_denomination_ew"])[j][d])
        vul = int((ev["vul_ns"] if ns else ev["vul_ew"])[j])
        tricks = int(ev["tricks"][j][declarer * 5 + d])
        dbl = 2 if ev["call_xx"][j] else (1 if ev["call_x"][j] else 0)
        ok = tricks >= level + 6
        made, down = made + ok, down + (not ok)
        levels[level] += 1
        doubling[dbl] += 1
        outcomes.add((lb, dbl, vul, tricks))
        declaring = (seat(int(ev["actor"][j])) % 2 == 0) == ns
        cells[k, 0 if declaring else 1] += 1
        r = float(ev["rewards"][j][int(ev["actor"][j])])
        assert (r > 0) == (ok == declaring) and r != 0, (r, ok, declaring)     # the score's sign, from the contract alone
    out.update(passout=passout, made=int(made), down=int(down), levels=levels[1:].tolist(), doubling=doubling.tolist(),
               by_k=np.bincount(ev["k"], minlength=4).tolist() if nb else [0] * 4, cells=cells.tolist(), outcomes=len(outcomes))
    if nb:
        calls = ev["turn"] + 1
        out["auction"] = (int(calls.min()), float(calls.mean()), int(calls.max()))
        when = 4 * ev["t"] + ev["k"]
        chained = 0
        for tb in np.unique(ev["table"]):
            sel = np.nonzero(ev["table"] == tb)[0]
            sel = sel[np.argsort(when[sel], kind="stable")]
            for a, b in zip(sel[:-1], sel[1:]):
                chained += int(ev["last_bid"][b] < 0 and not ev["illegal"][b] and when[b] - when[a] == 4)
        out["chained"] = chained
    else:
        out["auction"], out["chained"] = (0, 0.0, 0), 0
    return out


def full_conditions(c):
    """the coverage conditions of a rollout that is to exercise every ending of a board; -> the list of those NOT met"""
    nb, miss = max(1, c["boards"]), []
    if c["passout"] < 0.02 * nb:
        miss.append(f"pass-outs {c['passout']} < 2 % of {nb}")
    if c["made"] < 0.20 * nb:
        miss.append(f"made contracts {c['made']} < 20 % of {nb}")
    if c["down"] < 0.20 * nb:
        miss.append(f"failed contracts {c['down']} < 20 % of {nb}")
    if min(c["levels"][:5]) == 0:
        miss.append(f"a level of 1..5 without a final contract: {c['levels']}")
    if min(c["doubling"]) == 0:
        miss.append(f"undoubled / doubled / redoubled: {c['doubling']}")
    if min(min(row) for row in c["cells"]) < 16:
        miss.append(f"a cell of (ending sub-step) x {ROLES} under 16 boards: {c['cells']}")
    if c["chained"] < 1:
        miss.append("no board that ends and is followed by a pass-out four calls later")
    return miss


def basic_conditions(c, passout=True, positions=(0, 1, 2, 3)):
    """the conditions every rollout case must meet; -> the list of those NOT met"""
    miss = []
    if passout and c["passout"] < 1:
        miss.append("no pass-out")
    if c["made"] < 1 or c["down"] < 1:
        miss.append(f"made {c['made']}, failed {c['down']}")
    if any(c["by_k"][k] == 0 for k in positions):
        miss.append(f"boards by ending sub-step: {c['by_k']}")
    return miss
