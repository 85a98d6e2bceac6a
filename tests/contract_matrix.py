"""The full duplicate-score table as scripted auctions (a helper: no tests in here).

``law_score`` is the duplicate score of the declaring side written from the Laws of Duplicate Bridge (Law 77) as tables and
plain loops over tricks — it is NOT derived from ``contract_score`` (brl_amd/csrc/bridge_device.hpp), oracle/bridge_oracle.c or
oracle/pyref.py and uses no closed forms.  ``build_matrix`` turns every outcome cell

    5 strains x 7 levels x 3 doublings x 2 vulnerabilities of the declaring side x 14 trick counts = 2940 cells

into scripted tables: each cell is declared from each of the four seats (11 760 cases) and reached through three auction shapes
that lead to the same contract and the same declarer (35 280 tables), plus the four pass-outs.  Everything a test expects of a
table — the rewards by player id, the final contract, the declarer — is computed here from the case description alone.

Encodings (include/brl_hip.h): strain 0..4 = C, D, H, S, NT; call 0 = pass, 1 = X, 2 = XX, 3 + 5 * (level - 1) + strain = a bid;
seats 0..3 = N, E, S, W; tricks [seat * 5 + strain]; ``shuffled[seat]`` = the player id sitting there; players {0, 1} are partners.
"""
from __future__ import annotations

import numpy as np

from tests.test_oracle_kat import IMP_THRESHOLDS

PASS, X, XX = 0, 1, 2
N_CELLS = 5 * 7 * 3 * 2 * 14
SHAPES = ("direct", "raised", "overcalled")
N_CASES = len(SHAPES) * 4 * N_CELLS
N_TABLES = N_CASES + 4          # + one pass-out per dealer
PAIR_STRIDE = 1471              # table B of case i plays the direct auction of case (i + PAIR_STRIDE) % N_TABLES
REWARD_SCALE = 7600

# ---- Law 77, as tables ---------------------------------------------------------------------------------------------------------
FIRST_TRICK = (20, 20, 30, 30, 40)          # C, D, H, S, NT: the first odd trick
LATER_TRICK = (20, 20, 30, 30, 30)          # every further one
TIMES = (1, 2, 4)                           # undoubled, doubled, redoubled
GAME = (300, 500)                           # by vulnerability
PART_SCORE = 50
SMALL_SLAM = (500, 750)
GRAND_SLAM = (1000, 1500)
INSULT = (0, 50, 100)
OVERTRICK_DOUBLED = (100, 200)              # by vulnerability; redoubled: twice that
UNDERTRICK_UNDOUBLED = (50, 100)
UNDERTRICK_DOUBLED = ((100, 200, 200) + (300,) * 10, (200,) + (300,) * 12)   # the 1st .. 13th, by vulnerability


def law_score(strain: int, level: int, vul: int, doubling: int, tricks: int) -> int:
    """score of the declaring side: ``level`` ``strain`` (un-, re-)doubled, vulnerable or not, ``tricks`` tricks taken"""
    assert 0 <= strain <= 4 and 1 <= level <= 7 and vul in (0, 1) and doubling in (0, 1, 2) and 0 <= tricks <= 13
    need = level + 6
    if tricks < need:
        penalty = 0
        for k in range(need - tricks):
            penalty += UNDERTRICK_UNDOUBLED[vul] if doubling == 0 else UNDERTRICK_DOUBLED[vul][k] * (2 if doubling == 2 else 1)
        return -penalty
    points = 0
    for k in range(level):
        points += (FIRST_TRICK if k == 0 else LATER_TRICK)[strain] * TIMES[doubling]
    score = points + (GAME[vul] if points >= 100 else PART_SCORE)
    if level == 6:
        score += SMALL_SLAM[vul]
    if level == 7:
        score += GRAND_SLAM[vul]
    score += INSULT[doubling]
    for _ in range(tricks - need):
        score += LATER_TRICK[strain] if doubling == 0 else OVERTRICK_DOUBLED[vul] * doubling
    return score


def imp(diff: int) -> int:
    """the IMP scale of the reference's threshold list, signed"""
    n = 0
    for th in IMP_THRESHOLDS:
        if abs(diff) >= th:
            n += 1
    return n if diff >= 0 else -n


def cell_of(index: int):
    """cell index 0..2939 -> (strain, level, doubling, vul, tricks)"""
    tricks = index % 14
    vul = index // 14 % 2
    doubling = index // 28 % 3
    level = index // 84 % 7 + 1
    strain = index // 588
    return strain, level, doubling, vul, tricks


def seatings():
    """the eight seatings that keep the teams {0, 1} and {2, 3} opposite each other (player id at seat N, E, S, W)"""
    out = []
    for ns in ((0, 1), (1, 0), (2, 3), (3, 2)):
        others = (2, 3) if ns[0] < 2 else (0, 1)
        for ew in (others, others[::-1]):
            out.append([ns[0], ew[0], ns[1], ew[1]])
    return out


def direct_auction(level, strain, doubling, passes):
    """opening passes up to the declarer, the bid, X by the left-hand opponent, XX by the declarer's partner, three passes"""
    return [PASS] * passes + [3 + 5 * (level - 1) + strain] + [X, XX][:doubling] + [PASS] * 3


def auction(shape, level, strain, doubling, passes):
    """-> (calls, position of the declarer's first call).  The call at position ``passes`` is the first bid."""
    bid = 3 + 5 * (level - 1) + strain
    if shape == 0 or level == 1:
        return direct_auction(level, strain, doubling, passes), passes
    if shape == 1:   # the declarer names the strain one level lower, the partner raises: the last bidder is not the declarer
        return [PASS] * passes + [bid - 5, PASS, bid] + [X, XX][:doubling] + [PASS] * 3, passes
    # the right-hand opponent names the strain first, one level lower; X by them after two passes, XX by the declarer
    return [PASS] * passes + [bid - 5, bid] + ([PASS, PASS, X] if doubling else []) + ([XX] if doubling == 2 else []) + [PASS] * 3, passes + 1


def filler_tricks(t, seat, strain):
    """what the 19 entries a correct scorer does not read hold: never ``t``"""
    return (t + 1 + (5 * seat + strain) % 13) % 14


class Matrix:
    """Arrays over the n = N_TABLES scripted tables, filled by ``build_matrix`` and ``_pair_tables`` (int32 [n] unless noted).

    the board:        hand [n, 52], dealer, vul_ns, vul_ew, shuffled [n, 4], tricks uint8 [n, 20], row (the fixture's deal)
    the script:       calls [n, max_len] (padded with passes), length, max_len, passes (opening passes before the first bid)
    the description:  cell, shape, declarer, strain, level, doubling, vul (of the declaring side), taken, seating, passout
    the expectation:  score (declaring side), score_ns, rewards float32 [n, 4] by player id, last_bid, last_bidder (player id)
    table B of board i (the direct auction of case b_case[i] from board i's dealer, seats swapped):
                      b_case, b_shuffled [n, 4], b_length, b_declarer, b_strain, b_level, b_doubling, b_taken, b_passout,
                      b_score, b_score_ns, b_rewards float32 [n, 4], b_last_bid
    both tables back to back, as duplicate_step plays them:
                      pair_calls [n, pair_max], pair_length, pair_max
    the IMPs:         imp_ns (of the pair sitting North-South at table A), imp_rewards float32 [n, 4] by player id"""


def build_matrix(hands) -> Matrix:
    """``hands`` int32 [rows, 52]: the deals of the ``dds`` fixture as card ids per seat -> the ``Matrix`` of every table"""
    n = N_TABLES
    seats8 = seatings()
    m = Matrix()
    scripts = []
    ints = {k: np.zeros(n, np.int32) for k in ("dealer", "vul_ns", "vul_ew", "cell", "shape", "declarer", "strain", "level", "doubling",
                                               "vul", "taken", "seating", "passout", "score", "score_ns", "last_bid", "last_bidder",
                                               "row", "passes")}
    shuffled = np.zeros((n, 4), np.int32)
    tricks = np.zeros((n, 20), np.uint8)
    rewards = np.zeros((n, 4), np.float32)
    for i in range(n):
        v = {k: 0 for k in ints}
        v["row"] = i % len(hands)
        v["seating"] = (i // 7 + i // N_CELLS) % 8
        seating = seats8[v["seating"]]
        other_vul = i // 5 % 2
        if i >= N_CASES:      # the pass-outs, one per dealer: tricks that would score if anything were read
            v.update(passout=1, dealer=i - N_CASES, vul_ns=i % 2, vul_ew=other_vul, cell=-1, shape=-1, declarer=-1, last_bid=-1,
                     last_bidder=-1)
            calls = [PASS] * 4
            tricks[i] = [filler_tricks(7, s, d) for s in range(4) for d in range(5)]
        else:
            shape, rot, cell = i // (4 * N_CELLS), i // N_CELLS % 4, i % N_CELLS
            strain, level, doubling, vul, taken = cell_of(cell)
            declarer = (cell + cell // 14 + rot) % 4
            passes = (i // 3 + shape) % 4    # differs between the three shapes of one (cell, declarer): 4 * N_CELLS // 3 % 4 == 0
            calls, at = auction(shape, level, strain, doubling, passes)
            first_bidder = declarer if at == passes else (declarer - 1) % 4
            vuls = [other_vul, other_vul]
            vuls[declarer % 2] = vul
            score = law_score(strain, level, vul, doubling, taken)
            bidder_seat = (declarer + 2) % 4 if (shape == 1 and level > 1) else declarer
            v.update(dealer=(first_bidder - passes) % 4, vul_ns=vuls[0], vul_ew=vuls[1], cell=cell, shape=shape, declarer=declarer,
                     strain=strain, level=level, doubling=doubling, vul=vul, taken=taken, score=score, passes=passes,
                     score_ns=score if declarer % 2 == 0 else -score, last_bid=5 * (level - 1) + strain,
                     last_bidder=seating[bidder_seat])
            for s in range(4):
                for d in range(5):
                    tricks[i, s * 5 + d] = taken if (s, d) == (declarer, strain) else filler_tricks(taken, s, d)
                rewards[i, seating[s]] = score if s % 2 == declarer % 2 else -score
        for k in ints:
            ints[k][i] = v[k]
        shuffled[i] = seating
        scripts.append(calls)
    m.n = n
    m.length = np.array([len(c) for c in scripts], np.int32)
    m.max_len = int(m.length.max())
    m.calls = np.zeros((n, m.max_len), np.int32)
    for i, c in enumerate(scripts):
        m.calls[i, :len(c)] = c
    for k, a in ints.items():
        setattr(m, k, a)
    m.shuffled, m.tricks, m.rewards = shuffled, tricks, rewards
    m.hand = np.ascontiguousarray(hands[m.row], dtype=np.int32)
    _pair_tables(m)
    return m


def _pair_tables(m: Matrix):
    """Table B of board i: the same board, flags and trick table, seats swapped as ``duplicate_init`` swaps them, played with the
    DIRECT auction of case j = (i + PAIR_STRIDE) % n from board i's dealer.  Its score comes from ``law_score`` at whatever the
    trick table holds for B's (declarer, strain)."""
    n = m.n
    m.b_case = (np.arange(n) + PAIR_STRIDE) % n
    m.b_shuffled = m.shuffled[:, [1, 0, 3, 2]].copy()
    scripts = []
    for k in ("b_declarer", "b_strain", "b_level", "b_doubling", "b_taken", "b_score", "b_score_ns", "b_passout", "b_last_bid"):
        setattr(m, k, np.zeros(n, np.int32))
    m.b_rewards = np.zeros((n, 4), np.float32)
    for i in range(n):
        j = int(m.b_case[i])
        if m.passout[j]:
            scripts.append([PASS] * 4)
            m.b_passout[i], m.b_declarer[i], m.b_last_bid[i] = 1, -1, -1
            continue
        strain, level, doubling = int(m.strain[j]), int(m.level[j]), int(m.doubling[j])
        scripts.append(direct_auction(level, strain, doubling, int(m.passes[j])))
        declarer = (int(m.dealer[i]) + int(m.passes[j])) % 4
        vul = int((m.vul_ns[i], m.vul_ew[i])[declarer % 2])
        taken = int(m.tricks[i, declarer * 5 + strain])
        score = law_score(strain, level, vul, doubling, taken)
        m.b_declarer[i], m.b_strain[i], m.b_level[i], m.b_doubling[i], m.b_taken[i] = declarer, strain, level, doubling, taken
        m.b_score[i], m.b_score_ns[i], m.b_last_bid[i] = score, score if declarer % 2 == 0 else -score, 5 * (level - 1) + strain
        for s in range(4):
            m.b_rewards[i, m.b_shuffled[i, s]] = score if s % 2 == declarer % 2 else -score
    m.b_length = np.array([len(c) for c in scripts], np.int32)
    # both tables back to back, as duplicate_step plays them: table A's calls, then table B's (padded with passes)
    m.pair_length = m.length + m.b_length
    m.pair_max = int(m.pair_length.max())
    m.pair_calls = np.zeros((n, m.pair_max), np.int32)
    for i, c in enumerate(scripts):
        m.pair_calls[i, :m.length[i]] = m.calls[i, :m.length[i]]
        m.pair_calls[i, m.length[i]:m.pair_length[i]] = c
    m.imp_ns = np.array([imp(int(a) - int(b)) for a, b in zip(m.score_ns, m.b_score_ns)], np.int32)
    # by player id: the reference adds a player's two table scores (src/duplicate.py:15-70)
    m.imp_rewards = np.array([[imp(int(a) + int(b)) for a, b in zip(ra, rb)] for ra, rb in zip(m.rewards, m.b_rewards)], np.float32)


def expected_step_rewards(m: Matrix, k: int):
    """rewards [n, 4] of lockstep step k (call k of every table; finished tables are stepped on with passes): the table's rewards
    on the step that ends it, zeros before and after"""
    return np.where((m.length - 1 == k)[:, None], m.rewards, np.float32(0)).astype(np.float32)


_CACHE = {}


def matrix(dds, oracle) -> Matrix:
    """the one matrix of a test session"""
    if "m" not in _CACHE:
        hands = np.stack([oracle.key_to_hand(k) for k in dds["keys"]])
        _CACHE["m"] = build_matrix(hands)
    return _CACHE["m"]


def oracle_init(oracle, m: Matrix, rows=None, shuffled=None):
    sl = slice(None) if rows is None else rows
    return oracle.init_explicit(m.hand[sl], m.dealer[sl], m.vul_ns[sl], m.vul_ew[sl], (m.shuffled if shuffled is None else shuffled)[sl],
                                m.tricks[sl])


def oracle_lockstep(dds, oracle):
    """The matrix stepped through the C oracle, every table one call per step for max_len + 1 steps (a finished table is stepped
    on with passes) -> dict: rewards [steps, n, 4], terminated [steps, n], legal [n] (every scripted call was legal when made),
    state (after the last step).  Computed once per session; treat as read-only."""
    if "lockstep" not in _CACHE:
        m = matrix(dds, oracle)
        st = oracle_init(oracle, m)
        steps = m.max_len + 1
        out = {"rewards": np.zeros((steps, m.n, 4), np.float32), "terminated": np.zeros((steps, m.n), np.uint8),
               "legal": np.ones(m.n, bool), "first": st.copy()}
        for k in range(steps):
            act = m.calls[:, k] if k < m.max_len else np.zeros(m.n, np.int32)
            out["legal"] &= st["legal_action_mask"][np.arange(m.n), act] == 1
            oracle.step(st, np.ascontiguousarray(act))
            out["rewards"][k] = st["rewards"]
            out["terminated"][k] = st["terminated"]
        out["state"] = st
        _CACHE["lockstep"] = out
    return _CACHE["lockstep"]


def oracle_pairs(dds, oracle):
    """Both tables of every board through ``oracle.duplicate_step`` in lockstep (pair_max + 1 steps) -> dict: state, A, B (the
    Table_info arrays), returns [n, 4] (the rewards summed over the steps: the IMPs, emitted once).  Once per session."""
    if "pairs" not in _CACHE:
        from oracle import Oracle
        m = matrix(dds, oracle)
        st = oracle_init(oracle, m)
        A, B = Oracle.table_info_from(st), Oracle.table_info_from(st)
        returns = np.zeros((m.n, 4), np.float32)
        for k in range(m.pair_max + 1):
            act = m.pair_calls[:, k] if k < m.pair_max else np.zeros(m.n, np.int32)
            oracle.duplicate_step(st, np.ascontiguousarray(act), A, B)
            returns += st["rewards"]
        _CACHE["pairs"] = {"state": st, "A": A, "B": B, "returns": returns}
    return _CACHE["pairs"]


# ---- states one pass from the end, for the fused random rollouts --------------------------------------------------------------
ROLLOUT_SLOTS = 65536
ROLLOUT_SEED = 4242
ROLLOUT_DRAW_BASE = 5
ROLLOUT_T = 2
PLACEMENT_HINT = ("rollout_placement: some cell found no slot whose first action draw is a pass for its legal set; with another "
                  "ROLLOUT_SEED / ROLLOUT_DRAW_BASE or fewer slots the draws may not suffice: raise ROLLOUT_SLOTS (never drop cells)")


def rollout_placement(dds, oracle):
    """Every cell (the direct shape, the declarer seat rotating with the cell: tables 0 .. N_CELLS - 1) played up to but without
    its final pass, each placed in an env slot whose first action draw is a pass for that table's legal set.  A table with L legal
    calls passes when mulhi(draw, L) == 0, about one slot in L, so a slot that suits a table with many legal calls suits every
    table with fewer: the tables are served largest L first from the slots in ascending order of their draw.
    -> dict: slots [N_CELLS] (slot of table c), state (oracle states of all ROLLOUT_SLOTS slots before the rollout: init_random
    with the placed tables written over their slots), prefix (the N_CELLS oracle states alone), actor_sign [N_CELLS] (+1: the
    player who makes the final pass is on the declaring side), want (oracle.rollout_random of ``state``, which is advanced to
    ``final``).  Once per session; read-only."""
    if "rollout" not in _CACHE:
        m = matrix(dds, oracle)
        cells = np.arange(N_CELLS)
        assert (m.shape[cells] == 0).all() and (m.cell[cells] == cells).all()
        pre = oracle_init(oracle, m, cells)
        for k in range(m.max_len):                    # only the tables that still have a call before their last one are stepped
            live = np.nonzero(m.length[cells] - 1 > k)[0]
            if len(live) == 0:
                break
            sub = pre[live]
            oracle.step(sub, np.ascontiguousarray(m.calls[live, k]))
            pre[live] = sub
        assert (pre["terminated"] == 0).all() and (pre["pass_num"] == 2).all()
        n_legal = np.array([oracle.random_action(pre[c:c + 1], 0)[1] for c in cells])
        draws = np.array([oracle.action_draw(ROLLOUT_SEED, e, ROLLOUT_DRAW_BASE) for e in range(ROLLOUT_SLOTS)], np.uint64)
        by_draw = np.argsort(draws, kind="stable")
        by_legal = np.argsort(-n_legal, kind="stable")
        slots = np.full(N_CELLS, -1, np.int64)
        for rank, c in enumerate(by_legal):
            e = int(by_draw[rank])
            if (int(draws[e]) * int(n_legal[c])) >> 32 == 0:
                slots[c] = e
        state = oracle.init_random(ROLLOUT_SLOTS, seed=ROLLOUT_SEED)
        placed = slots >= 0
        state[slots[placed]] = pre[placed]
        last_seat = (m.dealer[cells] + m.length[cells] - 1) % 4
        out = {"slots": slots, "prefix": pre, "n_legal": n_legal, "draws": draws,
               "actor_sign": np.where(last_seat % 2 == m.declarer[cells] % 2, 1, -1), "state": state.copy()}
        out["want"] = oracle.rollout_random(state, ROLLOUT_T, seed=ROLLOUT_SEED, draw_base=ROLLOUT_DRAW_BASE)
        out["final"] = state
        _CACHE["rollout"] = out
    return _CACHE["rollout"]
