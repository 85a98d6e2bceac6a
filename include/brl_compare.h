/*
 * brl_compare.h — C-ABI of the system diff (brl_amd/csrc/brl_compare.hip, part of libbrl_hip.so): where two networks X and Y call
 * differently, by auction prefix.  Every decision of a recorded match is shown to both networks — the same hand, the same
 * auction — and what each would call and how far apart their policies are is summed by the prefix that led to the decision.
 *
 * Kept apart from brl_hip.h like brl_book.h and brl_belief.h: these entry points have no oracle counterpart; brl_version() does
 * not count them.
 *
 * Conventions are brl_hip.h's: 0 on success, <0 (BRL_E_*) on error with the message in brl_last_error(); every pointer is a
 * device pointer on `device`; `stream` is a hipStream_t passed as void*; nothing synchronises.  The same bytes on every run.
 *
 * Decision.  (table A or B, record i, call index t) for t < min(n_calls, depth), 1 <= depth <= BRL_BOOK_MAX_DEPTH.  The record
 * must have BRL_BOARD_OK and not BRL_BOARD_ILLEGAL; other records are skipped (the host counts them, as the call review does).
 * The caller is seat s = (dealer + t) & 3.  The table is the empty table of the record's deal — its hands, dealer,
 * vulnerabilities and seating, all tricks zero, table index 0xFFFFFFFF: brl_belief.h's, built by the same code
 * (csrc/belief_table.hpp) — stepped with calls[0..t) by table_step (brl_step).  The observation and the 38-bit legal mask are
 * the caller's at that table (brl_observe), and X and Y each give 38 float32 logits for it.
 *
 * Key.  brl_book.h's key fields of the prefix BEFORE the call, calls[0..t): sum_{j<t} (calls[j] + 1) << (58 - 6 j), and t + 1 in
 * bits 3..0.  t <= 9, so the fields use bits 63..10 at most.  Key 0 is "no decision" (t past the auction, or a skipped record):
 * the first call of an auction has key 1.  The numeric (unsigned) order is still a prefix before its extensions: an extension
 * differs from its prefix by a non-zero field above bit 3.
 *
 * Features.  Bits 0..23 of brl_book.h's packed features of the caller's hand hands[s] (csrc/hand_features.hpp): HCP, the four
 * suit lengths, balanced, and the caller's team index in bit 23; bits 24..31 are zero.
 *
 * Calls.  call_x / call_y: the arg-max of the network's logits over the legal actions, the lowest action on a tie — what
 * categorical<8> (csrc/policy_common.hpp) returns in mode form and the evaluators play.  A NaN logit is never the maximum, and
 * where no legal logit is above -inf the call is action 0.
 *
 * Log-probabilities.  logp_x / logp_y: float32, log-probability of `played` = calls[t] under each network, by categorical<8>
 * itself in the form k_belief_logp uses: (l[played] - l[arg-max]) + (-logf(total)) — bit for bit what brl_belief_logp and the
 * rollouts' log_prob give on the same logits.
 *
 * Divergences.  kl_xy = KL(X||Y), kl_yx = KL(Y||X), js = the Jensen-Shannon divergence, float64, in nats, over the legal actions,
 * from the float32 logits.  For a network N with logits l and a legal action a, every operation one IEEE double operation in
 * the order written, nothing contracted:
 *   m    = the largest legal logit (the logit of call_N)
 *   e_a  = exp((double) l_a - (double) m)
 *   S    = the sum of e_a                                   (order below)
 *   p_a  = e_a / S
 *   L_a  = ((double) l_a - (double) m) - log(S)             (log p_a)
 * and for the pair, d_a = L^y_a - L^x_a and g(d) = log(M_a / p^x_a), M = (p^x + p^y) / 2, in the form that keeps its relative accuracy
 * where the two policies are close (log(0.5 (1 + exp d)) = d / 2 + log cosh(d / 2), cosh h = 1 + 2 sinh^2(h / 2)):
 *   g(d) = 0.5 * d + log1p(2.0 * (s * s)),  s = sinh(0.25 * |d|)          for |d| <= 1.0
 *   g(d) = log(0.5 * (1.0 + exp(-|d|))) + max(d, 0.0)                      otherwise (d = +-inf included)
 *   kl_xy = sum of  p^x_a * (L^x_a - L^y_a)                 a term with p^x_a == 0 is +0.0 (a legal -inf logit, or e_a underflowed)
 *   kl_yx = sum of  p^y_a * (L^y_a - L^x_a)                 likewise for p^y_a == 0
 *   js    = 0.5 * (sum of p^x_a * (-g(d_a))  +  sum of p^y_a * (-g(-d_a)))          the same +0.0 rule, per sum
 * Order of the six sums: lane k of 8 (slot k) holds the actions 5 k .. 5 k + 4 and adds its legal actions' terms in ascending
 * action order to +0.0; the eight slot sums are then added in ascending slot order, ((s_0 + s_1) + s_2) + ... + s_7.
 * Two properties hold exactly.  Swapping X and Y swaps kl_xy with kl_yx and leaves js bitwise the same: d_a changes sign exactly,
 * both KL sums are one function of (first, second) network, and js's last addition commutes.  Bitwise-equal logits give
 * d_a = +0.0, g = 0.0 + log1p(0.0) = +0.0, every term (+-)0.0 added to +0.0: kl_xy = kl_yx = js = +0.0.
 * kl_xy is +inf where Y gives p^y_a == 0 to an action with p^x_a > 0; js is always finite.
 *
 * NONFINITE.  Set when either network has a NaN or +inf legal logit, or no legal logit above -inf (brl_hip.h's contract for
 * non-finite network outputs).  kl_xy, kl_yx and js are then NaN, and the affected network's logp is the NaN categorical<8>
 * gives.  Such a decision counts in its entry's `n` and `nonfinite` and enters no other counter, sum, histogram or confusion cell.
 *
 * Entry.  One per distinct non-zero key: exact integer counters and float64 sums over the key's decisions in the sorted sequence
 * (the sort is stable, by key, of the dense decision index).  Order of the float64 sums, a fixed two-level order that depends on
 * the sorted sequence alone: the run of a key is cut into blocks of BRL_COMPARE_BLOCK consecutive decisions counted from the
 * run's first; a block's finite decisions are added in ascending order to +0.0; the block sums are added in ascending block
 * order to +0.0.  js_max is the maximum over the finite decisions, +0.0 without one.  No floating-point atomics.
 */
#ifndef BRL_COMPARE_H
#define BRL_COMPARE_H

#include <stdint.h>

#include "brl_book.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BRL_COMPARE_ACTIONS 38
#define BRL_COMPARE_DECISION_BYTES 64
#define BRL_COMPARE_ENTRY_BYTES 560
#define BRL_COMPARE_BLOCK 64

#define BRL_COMPARE_VALID 1       /* flags: a decision (set in every record whose key is not 0) */
#define BRL_COMPARE_AGREE 2       /*        call_x == call_y */
#define BRL_COMPARE_X_PLAYED 4    /*        call_x == played */
#define BRL_COMPARE_Y_PLAYED 8    /*        call_y == played */
#define BRL_COMPARE_NONFINITE 16  /*        see above */

/* 64 bytes = 4 x 16, little endian, no padding */
typedef struct brl_compare_decision {
  uint64_t key;
  uint64_t legal;      /* bit a: action a is legal */
  uint32_t feats;
  uint8_t played;      /* calls[t] */
  uint8_t call_x, call_y;
  uint8_t flags;       /* BRL_COMPARE_* */
  float logp_x, logp_y;
  double kl_xy, kl_yx, js;
  uint64_t reserved;   /* zero */
} brl_compare_decision;

/* 560 bytes = 35 x 16, little endian, no padding */
typedef struct brl_compare_entry {
  uint64_t key;
  uint32_t n;                      /* decisions, the non-finite ones included */
  uint32_t agree, x_played, y_played;   /* finite decisions with the flag */
  uint32_t nonfinite;
  uint32_t reserved;               /* zero */
  uint32_t calls_x[BRL_COMPARE_ACTIONS], calls_y[BRL_COMPARE_ACTIONS], played[BRL_COMPARE_ACTIONS];   /* finite decisions by call */
  uint64_t hcp_sum;                /* the callers' HCP over the finite decisions */
  uint64_t hcp_sum_disagree;       /* and over those without AGREE */
  double kl_xy_sum, kl_yx_sum, js_sum, logp_x_sum, logp_y_sum;
  double js_max;
  uint64_t reserved2;              /* zero */
} brl_compare_entry;

/* tables[j] (uint64 [16]) and hands[j] (uint64 [4], the four hand words by seat) of records[rows[j]], j < m: the empty table of
 * the record's deal.  rows int64 [m], every value in 0 .. n-1.  records, tables and hands 16-byte aligned.  One launch, a lane per
 * row; a wave stores its 64 tables and hand rows as whole 16-byte pieces. */
int brl_compare_tables(int device, const brl_board_record *records, int64_t n, const int64_t *rows, int64_t m, uint64_t *tables,
                       uint64_t *hands, void *stream);

/* decisions[rows[j] * depth + t], j < m: the decision records of call index t of the records rows[j].
 *   logits_x, logits_y  float [m, ld_x], [m, ld_y]   row j: the networks' logits for row j's observation; ld >= 38 (39: merged heads)
 *   legal               uint64 [m]                   row j's legal mask
 * The key, the features and `played` are formed in the same launch from the record's first 64 bytes (the header, the four hand
 * words, calls[0..15]), as brl_book_samples reads them.  Where (record, t) is no decision the record written is all zero.  A
 * row outside 0 .. n-1 writes nothing.  One launch, eight lanes per row; whole 16-byte stores; nothing else of `decisions` is
 * written: the caller zeroes it first. */
int brl_compare_rows(int device, const brl_board_record *records, int64_t n, const int64_t *rows, int64_t m, int t, int depth,
                     const float *logits_x, int64_t ld_x, const float *logits_y, int64_t ld_y, const uint64_t *legal,
                     brl_compare_decision *decisions, void *stream);

/* entries[e], e < K, and confusion from the decisions sorted by key:
 *   sorted       brl_compare_decision [S]  in key order (stable)
 *   entry_start  int64 [K + 1]             nondecreasing, within 0 .. S: entry e is the run sorted[entry_start[e] .. entry_start[e + 1]);
 *                                          decisions before entry_start[0] — the run of key 0 — are dropped
 *   entries      [K]                       16-byte aligned; zeroed by this call (a memset on the stream), then written; the key is
 *                                          the run's first decision's
 *   confusion    uint64 [38][38]           zeroed by this call; cell (call_x, call_y) counts the finite decisions of all entries
 * One launch, a workgroup per entry; integer atomics in LDS and, for the confusion table, in memory. */
int brl_compare_reduce(int device, const brl_compare_decision *sorted, int64_t S, const int64_t *entry_start, int64_t K,
                       brl_compare_entry *entries, uint64_t *confusion, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* BRL_COMPARE_H */
