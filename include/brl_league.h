/*
 * brl_league.h — C-ABI of the batched league evaluation (brl_amd/csrc/brl_league.hip, part of libbrl_hip.so): many duplicate
 * matches between pairs of networks of ONE architecture as one batch of boards, in which every board's call comes from one of
 * several networks.  The forward of such a batch is a grouped product: the boards that act are sorted by their network
 * (brl_league_route), then every hidden layer is ONE launch over all groups and the heads another (brl_league_forward).
 * The step is brl_hip.h's brl_eval_step_team, unchanged: it takes one logits row per board.
 *
 * Kept apart from brl_hip.h like brl_sl.h: these entry points have no oracle counterpart; brl_version() does not count them.
 *
 * Conventions are brl_hip.h's: 0 on success, <0 (BRL_E_*) on error with the message in brl_last_error(); every pointer is a
 * device pointer on `device`; `stream` is a hipStream_t passed as void*; nothing synchronises.  No handle.
 *
 * Layout: the batch holds nmatch matches of n boards each, match-major: board b belongs to match b / n.  The matches are
 * visited in a host-prepared order, sorted by the group (= network) that plays the acting team in them:
 *   order    int32 [nmatch]  slot k of the order is match order[k] (a permutation of 0 .. nmatch - 1)
 *   group_of int32 [nmatch]  the group of slot k, 0 <= group_of[k] < ngroups, non-decreasing in k
 * Both are static for a league and a team: built once.
 */
#ifndef BRL_LEAGUE_H
#define BRL_LEAGUE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* One "DeepMind" fp32 network by reference, as brl_mlp_ref's pointer members (nn.Linear's own layouts): the networks of a
 * league are a DEVICE-resident array of these records, one per group. */
typedef struct brl_league_net {
  const float *w[8]; /* w[l] [hidden, l == 0 ? 480 : hidden], 16-byte aligned */
  const float *b[8]; /* [hidden], 16-byte aligned */
  const float *actor_w;  /* [38, hidden], 16-byte aligned */
  const float *actor_b;  /* [38] */
  const float *critic_w; /* [1, hidden], 16-byte aligned */
  const float *critic_b; /* [1] */
} brl_league_net;

/* The boards that act for `team` (0: players {0,1}, 1: players {2,3}), grouped: board b acts when terminated[b] == 0 and
 * current_player[b] >> 1 == team (both are outputs of brl_eval_step_team).
 *   rows        int64 [nmatch * n]   rows[0 .. R): the acting boards, by slot k of the order and, inside a match, by board index
 *                                    (so: grouped by network); entries from R on are left as they are
 *   group_first int32 [ngroups + 1]  prefix sums of the groups' sizes: group g owns rows[group_first[g] .. group_first[g + 1]);
 *                                    group_first[ngroups] = R
 *   work        int32 [2 * nmatch]   scratch (per slot: its count, then its first row)
 * Three launches — counts per slot (one wave per match: ballot + popcount), an exclusive scan by one workgroup, a compacting
 * scatter — no atomics, a fixed order.  nmatch * n < 2^31.  Every array as its element type: rows 8-byte aligned, the int32
 * arrays 4-byte (BRL_E_ARG otherwise, before anything is launched). */
int brl_league_route(int device, const uint8_t *terminated, const int32_t *current_player, int team, int64_t n,
                     const int32_t *order, const int32_t *group_of, int64_t nmatch, int64_t ngroups, int32_t *work,
                     int64_t *rows, int32_t *group_first, void *stream);

/* The forward of the routed rows: for r < R = group_first[ngroups], with g the group of row r,
 *     x[r] = float(obs[rows[r]]);  h = act(h W_l^T + b_l) for the nlayers hidden layers of nets[g];
 *     out[rows[r] * ldo + 0..37] = actor(h), out[rows[r] * ldo + 38] = critic(h).
 * Rows of `out` that are not routed are not touched.  One launch for the cast, one per hidden layer (the exact-fp32 MFMA tile
 * of brl_mlp_gemm, bias + activation in its epilogue: a row's result is bit for bit brl_mlp_forward_rows' for the same
 * network), one for the heads.  R is never read by the host: the grids are sized for the bounds the caller gives,
 *     rmax >= R  and  ngroups,
 * (floor(rmax / 64) + ngroups row tiles per layer), and workgroups beyond the real work return at once.
 * nets: device array [ngroups]; nlayers 1..8, hidden a multiple of 4 and <= 1024, act 0 = ReLU / 1 = tanh — shared by all
 * networks.  obs uint8 [boards, 480], 4-byte aligned (a row is read as 4-byte words, as brl_mlp_forward_rows'); scratch:
 * rmax * (480 + 2 * hidden) floats, 16-byte aligned; rows and nets 8-byte, group_first and out 4-byte; ldo >= 39.  BRL_E_ARG
 * otherwise, before anything is launched (the arrays the records of `nets` name are on the device: not checked). */
int brl_league_forward(int device, const brl_league_net *nets, int64_t ngroups, int nlayers, int64_t hidden, int act,
                       const uint8_t *obs, const int64_t *rows, const int32_t *group_first, int64_t rmax, float *scratch,
                       int64_t scratch_len, float *out, int64_t ldo, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* BRL_LEAGUE_H */
