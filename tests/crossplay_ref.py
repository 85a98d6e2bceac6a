"""Restatements for the cross-play tests (include/brl_crossplay.h), in plain numpy: the route, and the replay of one line-up's
recorded calls through the CPU oracle that also says who was to call, and on what observation.  No tests in here."""
import numpy as np


def xroute_numpy(terminated, current_player, team, n, order, group_of, ngroups):
    """(rows, group_first) of brl_xplay_route: the boards b with terminated[b] == 0 and current_player[b] >> 1 == team, by position
    k of ``order`` (slot order[k] = 2 * match + half: the boards of that match whose current_player & 1 is the half), ascending
    inside a slot; group_first = prefix sums of the sizes of the groups ``group_of[k]``"""
    terminated, current_player = np.asarray(terminated), np.asarray(current_player)
    rows, sizes = [], np.zeros(ngroups, np.int64)
    for k, s in enumerate(np.asarray(order).tolist()):
        m, half = s >> 1, s & 1
        b = np.arange(m * n, (m + 1) * n)
        act = b[(terminated[b] == 0) & ((current_player[b] >> 1) == team) & ((current_player[b] & 1) == half)]
        rows.extend(act.tolist())
        sizes[group_of[k]] += len(act)
    return np.array(rows, np.int64), np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def replay_lineup(oracle, n, seed, calls, logits=None):
    """One line-up's recorded calls ([iterations][n], -1 = the board waited) through ``oracle.duplicate_step`` on the boards of
    ``init_random(n, seed)``: who acted and who waited (iteration i belongs to team i & 1), every call legal, waiting boards keep
    their state, finished boards never wait; with ``logits`` ([iterations][n, 38]): each call is the arg-max of the recorded
    logits over the oracle's legal mask.
    -> (cum_return [n], table A's and table B's info, steps): ``steps[i]`` = what the oracle showed BEFORE iteration i's calls:
    ``observation`` [n, 480], ``legal`` [n, 38] bool, ``player`` [n] (current_player) and ``live`` [n] (the boards that called)."""
    from oracle import Oracle
    ref = oracle.init_random(n, seed=seed)
    oA, oB = Oracle.table_info_from(ref), Oracle.table_info_from(ref)
    cum = np.zeros(n, np.float32)
    rows = np.arange(n)
    steps = []
    for i, act in enumerate(calls):
        idle = act < 0
        live = (ref["terminated"] == 0) & ~idle
        team = ref["current_player"] >> 1
        assert (team[live] == (i & 1)).all() and (team[idle & (ref["terminated"] == 0)] != (i & 1)).all()
        assert not (idle & (ref["terminated"] != 0)).any()
        legal = ref["legal_action_mask"].astype(bool)
        assert legal[rows, np.where(idle, 0, act)][live].all()
        if logits is not None:
            masked = np.where(legal, logits[i], -np.inf)
            assert np.array_equal(act[live], masked.argmax(1)[live])
        steps.append({"observation": ref["observation"].copy(), "legal": legal.copy(), "player": ref["current_player"].copy(),
                      "live": live.copy()})
        keep = (ref[idle].copy(), oA[idle].copy(), oB[idle].copy())
        oracle.duplicate_step(ref, np.where(idle, 0, act).astype(np.int32), oA, oB)
        ref[idle], oA[idle], oB[idle] = keep
        cum[~idle] += ref["rewards"][~idle, 0]
    assert ref["terminated"].all() and oA["terminated"].all() and oB["terminated"].all()
    return cum, oA, oB, steps


def decisions_of(steps, calls, player):
    """the decisions of ``player`` in a replay: (iteration index [m], board [m], observation [m, 480] bool, legal [m, 38] bool,
    call [m])"""
    it, bd, obs, legal, call = [], [], [], [], []
    for i, (s, act) in enumerate(zip(steps, calls)):
        b = np.nonzero(s["live"] & (s["player"] == player))[0]
        it.append(np.full(len(b), i))
        bd.append(b)
        obs.append(s["observation"][b].astype(bool))
        legal.append(s["legal"][b])
        call.append(act[b])
    return np.concatenate(it), np.concatenate(bd), np.concatenate(obs), np.concatenate(legal), np.concatenate(call)


def seating_byte(shuffled_players):
    """brl_board_record.seating of a table whose seat s holds player shuffled_players[.., s]"""
    sp = np.asarray(shuffled_players).astype(np.int64)
    return sum(sp[:, s] << (2 * s) for s in range(4)).astype(np.uint8)
