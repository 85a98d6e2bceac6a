/*
 * brl_crossplay.h — C-ABI of cross-play (brl_amd/csrc/brl_crossplay.hip, part of libbrl_hip.so): duplicate matches in which
 * every PLAYER has a network of its own, batched like the league (brl_league.h).  The league gives both players of a team one
 * network; here the two partners may differ — ad-hoc partnership, zero-shot coordination: do two bidders share a system?
 *
 * Kept apart from brl_hip.h like brl_league.h: the entry point has no oracle counterpart; brl_version() does not count it.
 *
 * Conventions are brl_hip.h's: 0 on success, <0 (BRL_E_*) on error with the message in brl_last_error(); every pointer is a
 * device pointer on `device`; `stream` is a hipStream_t passed as void*; nothing synchronises.  No handle.
 *
 * Definition.  A line-up is four network indices (p0, p1, p2, p3).  Every call of player id k (current_player == k, 0..3) is
 * the masked arg-max (the evaluators' masked_mode) of the logits of network pk.  Players {0, 1} are team 1 and players {2, 3}
 * team 2, as everywhere; nothing else about a duplicate match changes (brl_eval_step_team plays it, unchanged: one logits row
 * per board).  The league's match (i, j) is the line-up (i, i, j, j).
 *
 * The half of a board is current_player & 1: which of the acting team's two players is to call.
 *
 * What a line-up is NOT.  Table B is table A with neighbouring seats exchanged (the seat index list 1, 0, 3, 2).  Which player of
 * the other team receives player 0's cards at table B therefore depends on the board's random seating: player 2 when the seats
 * N, E, S, W hold players 0, 2, 1, 3 and player 3 when they hold 0, 3, 1, 2.  So a line-up of four different networks has NO
 * team-swapped counterpart that is its negative board by board.  Antisymmetry holds only where both players of each team share a network — the league's case.  The duplicate compares
 * PARTNERSHIPS on the same cards, not players: (p0, p1, ..) and (p1, p0, ..) differ only through the random seating.
 *
 * Layout: the batch holds nmatch matches (line-ups) of n boards each, match-major: board b belongs to match b / n.  For one
 * team the unit of the visiting order is a slot = (match, half), slot id 2 * match + half; there are 2 * nmatch of them:
 *   order    int32 [2 * nmatch]  position k of the order is slot order[k] (a permutation of 0 .. 2 nmatch - 1)
 *   group_of int32 [2 * nmatch]  the group (= network) of position k, 0 <= group_of[k] < ngroups, non-decreasing in k
 * Both are static for a batch and a team: built once, on the host.
 */
#ifndef BRL_CROSSPLAY_H
#define BRL_CROSSPLAY_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The boards that act for `team` (0: players {0,1}, 1: players {2,3}), grouped by the network of the acting PLAYER: board b
 * acts when terminated[b] == 0 and current_player[b] >> 1 == team (both are outputs of brl_eval_step_team), in slot
 * 2 * (b / n) + (current_player[b] & 1).
 *   rows        int64 [nmatch * n]   rows[0 .. R): the acting boards, by position k of the order and, inside a slot, by ascending
 *                                    board index (so: grouped by network); entries from R on are left as they are
 *   group_first int32 [ngroups + 1]  prefix sums of the groups' sizes: group g owns rows[group_first[g] .. group_first[g + 1]);
 *                                    group_first[ngroups] = R — what brl_league_forward consumes, unchanged
 *   work        int32 [4 * nmatch]   scratch (per slot id: its count, then its first row)
 * Three launches — counts (one wave per MATCH: terminated / current_player read once per 64 boards, two ballots + popcounts,
 * both halves' counts written), an exclusive scan over the positions of the order by one workgroup, a compacting scatter (a
 * wave per match again, both halves' first rows in hand) — no atomics, a fixed order, the same bytes on every run.
 * nmatch * n < 2^31.  Entries of order / group_of outside their range are clamped, and a row whose place would lie outside
 * rows[0 .. nmatch * n) is not written (an order that is not a permutation): the result may be wrong, never an address.
 * Alignment as brl_league_route's: rows 8-byte, the int32 arrays 4-byte. */
int brl_xplay_route(int device, const uint8_t *terminated, const int32_t *current_player, int team, int64_t n,
                    const int32_t *order, const int32_t *group_of, int64_t nmatch, int64_t ngroups, int32_t *work,
                    int64_t *rows, int32_t *group_first, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* BRL_CROSSPLAY_H */
