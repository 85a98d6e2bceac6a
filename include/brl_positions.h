/*
 * brl_positions.h — C-ABI of the position queries (brl_amd/csrc/brl_positions.hip, part of libbrl_hip.so): what a network calls
 * with a given hand after a given auction.  A position is thirteen cards, the dealer, the vulnerability and the calls made so
 * far; no deal is needed.  brl_position_rows turns a batch of positions into the observation rows and legal masks a network
 * takes, brl_position_answers turns the network's logits into the call, the top of its policy and the policy's entropy.
 *
 * Kept apart from brl_hip.h like brl_compare.h and brl_lines.h: these entry points have no oracle counterpart; brl_version()
 * does not count them.
 *
 * Conventions are brl_hip.h's: 0 on success, <0 (BRL_E_*) on error with the message in brl_last_error(); every pointer is a
 * device pointer on `device`; `stream` is a hipStream_t passed as void*; nothing synchronises.  No handle, no atomics, no
 * floating-point reduction whose order depends on timing: the same bytes on every run.  Input is not trusted: every field of a
 * position is checked on the device, and a position that fails a check reads and writes nothing outside its own rows.
 *
 * Position.  brl_position, 64 bytes.  `hand`: the caller's cards, bit = pgx card id rank * 4 + suit (the hand words of
 * brl_boards.h).  `calls[0..n_calls)`: the actions 0..37 in order from the dealer (0 Pass, 1 X, 2 XX, 3 + 5 (level - 1) + strain);
 * the entries at n_calls and beyond are BRL_POS_FILL.  The caller is seat (dealer + n_calls) & 3; seating is the identity
 * (player id = seat).
 *
 * Status.  One uint32 per position; the low byte is the first check that failed, in this order:
 *   BRL_POS_BAD_HEADER    dealer > 3, vul_ns > 1, vul_ew > 1, n_calls > 48, reserved != 0, an entry calls[j], j < n_calls, above 37,
 *                         or an entry at n_calls or beyond that is not BRL_POS_FILL
 *   BRL_POS_BAD_HAND      a bit at or above 52, or not exactly 13 of the low 52 bits
 *   BRL_POS_ILLEGAL_CALL  calls[j] is not in legal_mask (csrc/bridge_device.hpp) of the table stepped by calls[0..j); bits 8..15 = j
 *   BRL_POS_FINISHED      the table is terminated after calls[0..j], j < n_calls: nobody is to call.  Bits 8..15 = j, the index of
 *                         the call that ended the auction (j = n_calls - 1: the auction given is a complete one; j below that:
 *                         calls follow the closing pass)
 * The replay stops at the first of the last two that occurs, in call order: a position is never stepped past its point of
 * failure.  A position that is not BRL_POS_OK writes an all-zero observation row, mask row, legal word and table.
 *
 * Table.  The position's table is brl_belief.h's empty table (csrc/belief_table.hpp: all tricks zero, table index 0xFFFFFFFF,
 * seating the identity) of this deal: the caller's hand at its seat; the 39 other cards, in ascending card id, the first 13 to
 * the next seat (caller + 1) & 3, the next 13 to (caller + 2) & 3, the last 13 to (caller + 3) & 3.  It is stepped with
 * calls[0..n_calls) by table_step (csrc/bridge_device.hpp), the one copy of the auction rules, what brl_step runs.
 * The fill exists only so that the table is a valid one for brl_observe / brl_step.  The observation row and the legal mask of
 * the caller DO NOT DEPEND ON THE FILL: the row holds the vulnerability, the auction history and the observer's own 52 card bits
 * (emit_obs_row reads no other hand word), and the legal mask is a function of the table's scalars alone.
 *
 * Rows.  obs[i] is the caller's 480-byte observation at that table and mask[i] its 38 legal-action bytes, written by the
 * emitters brl_observe uses (emit_obs_row, emit_mask_row); legal[i] has bit a set where action a is legal.
 *
 * Answer.  brl_position_answer, 96 bytes, from the float32 logits of the position's row, over the legal actions:
 *   call      the evaluators' masked arg-max: categorical<8> (csrc/policy_common.hpp) in mode form — the first maximum wins, a NaN
 *             is never the maximum, a row without a legal logit above -inf gives action 0
 *   n_legal   the number of legal actions
 *   value     value[i * value_stride] (0.0 where `value` is NULL)
 *   p_a, L_a  exactly brl_compare.h's for one network, computed by the same device function (csrc/policy_dist.hpp): m the
 *             logit of `call`, e_a = exp((double) l_a - (double) m), S the sum of e_a in the two-level order (slot k of 8 adds its
 *             legal actions 5 k .. 5 k + 4 in ascending order to +0.0, the eight slot sums are added in ascending slot order),
 *             p_a = e_a / S, L_a = ((double) l_a - (double) m) - log(S); every operation one IEEE double operation, nothing contracted
 *   entropy   -sum p_a L_a, in nats: the sum of the terms p_a * (-L_a) in the same two-level order; a term with p_a == 0 is +0.0
 *             (so a position with one legal action has entropy +0.0, never -0.0)
 *   top list  rank(a) = #{legal b : p_b > p_a, or p_b == p_a and b < a}; the ranks of the legal actions are 0 .. n_legal - 1, each
 *             once, whatever the ties.  k = min(top_k, n_legal); top_action[r], top_prob[r] for r < k: the legal action of rank r
 *             and its p_a.  Formed by counting, not by sorting.  Slots k .. 7 hold action 255, probability +0.0.
 *   probs     (optional) probs[i * 38 + a] = p_a for a legal action, +0.0 for an illegal one
 *   flags     BRL_POS_NONFINITE: brl_compare.h's NONFINITE condition — a legal logit is NaN or +inf, or no legal logit is above
 *             -inf.  Then entropy, all eight top_prob and the row of probs are NaN, all eight top_action are 255, k is 0, and
 *             `call` is what categorical<8> gives.
 * A position whose status is not BRL_POS_OK gets an all-zero answer with call = 255, and a row of +0.0 in probs.
 */
#ifndef BRL_POSITIONS_H
#define BRL_POSITIONS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BRL_POS_MAX_CALLS 48
#define BRL_POS_FILL 255
#define BRL_POS_ACTIONS 38
#define BRL_POS_OBS_BYTES 480
#define BRL_POS_MAX_TOP 8

#define BRL_POS_OK 0            /* status, low byte */
#define BRL_POS_BAD_HEADER 1
#define BRL_POS_BAD_HAND 2
#define BRL_POS_ILLEGAL_CALL 3
#define BRL_POS_FINISHED 4

#define BRL_POS_NONFINITE 1     /* answer flags */

/* 64 bytes = 4 x 16, little endian, no padding */
typedef struct brl_position {
  uint64_t hand;
  uint8_t dealer;      /* 0..3 = N, E, S, W */
  uint8_t vul_ns, vul_ew;
  uint8_t n_calls;     /* 0..48 */
  uint32_t reserved;   /* zero */
  uint8_t calls[BRL_POS_MAX_CALLS];
} brl_position;

/* 96 bytes = 6 x 16, little endian, no padding */
typedef struct brl_position_answer {
  uint8_t call;        /* 255: the position's status is not BRL_POS_OK */
  uint8_t n_legal;
  uint8_t flags;       /* BRL_POS_NONFINITE */
  uint8_t k;           /* entries of the top list that hold an action */
  float value;
  double entropy;
  uint8_t top_action[BRL_POS_MAX_TOP];
  double top_prob[BRL_POS_MAX_TOP];
  uint64_t reserved;   /* zero */
} brl_position_answer;

/* obs[i], mask[i], legal[i], status[i] and, where `tables` is not NULL, tables[i] (uint64 [16], the packed table) of
 * positions[i], i < n; 1 <= n < 2^31.  positions and tables 16-byte aligned, obs and legal 8-byte aligned, status 4-byte aligned
 * (BRL_E_ARG otherwise, before anything is launched).  One launch: a one-wave workgroup takes 64 positions; a lane checks one
 * position and replays its auction in registers, leaving the table's image in LDS; the wave then writes the 64 observation and
 * mask rows and the tables. */
int brl_position_rows(int device, const brl_position *positions, int64_t n, uint8_t *obs, uint8_t *mask, uint64_t *legal,
                      uint32_t *status, uint64_t *tables, void *stream);

/* answers[i] and, where `probs` is not NULL, probs[i * 38 .. i * 38 + 38) of row i < n; 1 <= n < 2^31; 1 <= top_k <= 8.
 *   logits  float [n, ld]       row i: the network's logits for obs[i]; 38 <= ld < 2^20 (39: merged heads)
 *   value   float, or NULL      value[i * value_stride]; 0 <= value_stride < 2^20
 *   legal, status               what brl_position_rows wrote
 * logits and value 4-byte aligned, legal and probs 8-byte aligned, status 4-byte aligned, answers 16-byte aligned (BRL_E_ARG
 * otherwise, before anything is launched).  One launch, eight lanes per row; an answer leaves as six 16-byte stores. */
int brl_position_answers(int device, const float *logits, int64_t ld, const float *value, int64_t value_stride, const uint64_t *legal,
                         const uint32_t *status, int64_t n, int top_k, brl_position_answer *answers, double *probs, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* BRL_POSITIONS_H */
