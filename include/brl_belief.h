/*
 * brl_belief.h — C-ABI of the hand beliefs (brl_amd/csrc/brl_belief.hip, part of libbrl_hip.so): given one seat's thirteen cards
 * and an auction prefix, what the other three hands look like according to the networks that made the calls.  Deals of the 39
 * unseen cards are sampled uniformly, every sampled deal is weighted by the probability the networks give the hidden seats'
 * calls of the prefix, and the weighted deals are summed into one table per query.  This header is the specification.
 *
 * Kept apart from brl_hip.h like brl_boards.h, brl_book.h, brl_par.h and brl_review.h: these entry points have no oracle
 * counterpart; brl_version() does not count them.
 *
 * Conventions are brl_hip.h's: 0 on success, <0 (BRL_E_*) on error with the message in brl_last_error(); every pointer is a
 * device pointer on `device`; `stream` is a hipStream_t passed as void*; nothing synchronises.
 *
 * What a belief is not.  No sampled deal is scored (no double-dummy solver is involved: the sample tables' trick counts are zero
 * and nothing reads them) and nothing is searched: this is the posterior over the hidden hands under the networks' own policies,
 * the sampler a search or an information-state review would be built on, not either of them.
 *
 * Query q.  The own seat s (0..3 = N,E,S,W), the own hand word (13 bits set, bit = rank * 4 + suit as in brl_book.h), dealer,
 * vul_ns, vul_ew, the seating byte as the board records hold it (player id at seat x = (seating >> 2 x) & 3; team = id >> 1), and
 * a prefix calls[0..T), 0 <= T <= BRL_BOARD_MAX_CALLS, starting at the dealer.  The prefix is legal (it may end the auction: the
 * belief at the opening lead); the host checks that before anything is sampled.  The kernels never see the prefix as such: the
 * host turns it into one legal word and one action per (query, call index).
 *
 * Sample k of query q (k < K; q is the query's stream index, which the caller chooses: the same (seed, q, k) is the same deal
 * wherever and with whatever other queries it is drawn).
 *   - The 39 cards not in the own hand are written to c[0..39), ascending by bit index.
 *   - Fisher-Yates, j = 0..37: r = j + mulhi32(d_j, 39 - j); swap c[j], c[r].  mulhi32(d, n) = (d * n) >> 32.
 *   - d_j is draw j of a Philox4x32-10 stream (csrc/bridge_device.hpp: philox4x32_10, philox_word): word j & 3 of the block
 *     j >> 2 with counter (k, j >> 2, BRL_BELIEF_STREAM, q) and key (seed & 0xFFFFFFFF, seed >> 32).  No other stream of the
 *     library uses BRL_BELIEF_STREAM as its third counter word.
 *   - Seats (s+1)&3, (s+2)&3, (s+3)&3 receive c[0..13), c[13..26), c[26..39); seat s keeps the own hand.
 *   - The multiply-high draw is not exactly uniform: a value of 0..n-1 is drawn with probability within n / 2^32 <= 39 / 2^32 of
 *     1/n.  Nothing corrects that.
 *   - The sample's table is the empty 128-byte table of that deal (csrc/bridge_device.hpp's layout): the query's dealer,
 *     vulnerabilities and seating, no call made, table index 0xFFFFFFFF, all tricks zero.
 *
 * Weight.  For t = 0..T-1 the caller is seat (dealer + t) & 3.  If it is the own seat nothing is computed: its observation is
 * the same in every sample.  Otherwise the caller's observation goes through the network of the caller's team, and in float32
 *     logw[k] += log_softmax(logits masked to the legal actions)[calls[t]]
 *     greedy[k] &= (argmax of the masked logits == calls[t])        (the first maximum: the evaluators' masked_mode)
 * by policy_common.hpp's categorical<8>: m = the largest legal logit, total = the sum of expf(l - m) over the legal actions in
 * that function's association, log-probability = (l[calls[t]] - m) - logf(total), which is what the policy rollout records as
 * log_prob when it draws that call.  Then every table of the query is stepped with calls[t].  The legal mask depends on the
 * prefix only: one 38-bit word per (query, t).  logw starts at 0, greedy at 1.
 *
 * Non-finite values.  A legal logit that is NaN or +inf, or no legal logit above -inf, gives a NaN log-probability (as the
 * float64 log-softmax does) and makes greedy false; a -inf legal logit has probability zero; a logit that is not legal is never
 * looked at.  A query with a NaN logw, or whose largest logw is -inf, gets a weighted block that is NaN throughout (max_logw
 * included); its integer block is unaffected.
 *
 * Belief of a query, over its K samples; hidden seat h = 0, 1, 2 is seat (s + 1 + h) & 3.
 *   weighted:  w_k = exp((double)logw_k - (double)max_logw), max_logw = max_k logw_k;
 *              wsum = sum w_k, wsq = sum w_k^2 (effective sample size wsum^2 / wsq);
 *              card[h][b] = sum w_k [bit b in the hand of h], hcp[h][p], length[h][suit][len], balanced[h]: the same with
 *              brl_book.h's features of that hand (HCP 0..37, lengths of C,D,H,S 0..13, balanced = 4333 / 4432 / 5332).
 *              Sums, not shares: the host divides by wsum.
 *   greedy:    n = K, consistent = sum greedy_k, and g_card, g_hcp, g_length, g_balanced: the same tables as exact uint32
 *              counts over the samples with greedy_k = 1 — rejection sampling under the policy the evaluators play.
 * Summation order: every float64 sum is formed by one thread, alone, as ((0 + x_0) + x_1) + ... + x_{K-1} in ascending k, where
 * x_k is w_k (w_k^2 for wsq) if the sample counts for that sum and +0.0 if not.  No floating-point atomics, no dependence on
 * the launch geometry: the same bytes on every run.
 *
 * Input values are not trusted: seat and dealer are taken & 3, a vulnerability & 1, bits 52..63 of a hand word are dropped; a
 * row index, query index or action outside its range makes brl_belief_logp skip that row; every kernel writes only the rows of
 * the range it was given.
 */
#ifndef BRL_BELIEF_H
#define BRL_BELIEF_H

#include <stdint.h>

#include "brl_boards.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BRL_BELIEF_STREAM 0x42524C42u /* 'BRLB' (csrc/bridge_device.hpp: STREAM_BELIEF) */
#define BRL_BELIEF_ACTIONS 38
#define BRL_BELIEF_ENTRY_BYTES 5328

/* 16 bytes, little endian, no padding */
typedef struct brl_belief_query {
  uint64_t hand;    /* the own hand word */
  uint8_t seat;     /* the own seat */
  uint8_t dealer;
  uint8_t vul_ns;
  uint8_t vul_ew;
  uint8_t seating;
  uint8_t zero[3];
} brl_belief_query;

/* 5328 = 333 x 16 bytes, no padding */
typedef struct brl_belief_entry {
  double wsum;
  double wsq;
  float max_logw;
  uint32_t n;
  uint32_t consistent;
  uint32_t reserved;             /* zero */
  double card[3][52];
  double hcp[3][38];
  double length[3][4][14];
  double balanced[3];
  uint32_t g_card[3][52];
  uint32_t g_hcp[3][38];
  uint32_t g_length[3][4][14];
  uint32_t g_balanced[3];
  uint32_t reserved2;            /* zero */
} brl_belief_entry;

/* The Q * K samples of queries[0..Q): row i * K + k is sample k of queries[i], drawn from stream index q0 + i.  tables uint64
 * [Q * K, 16] and hands uint64 [Q * K, 4] (the four hand words by seat), both 16-byte aligned; 1 <= K, Q * K < 2^31,
 * 0 <= q0, q0 + Q <= 2^32.  One launch, a lane per sample (the 38 draws are a serial chain; the shuffled cards live in LDS, not
 * in an indexed register array); a wave then stores its 64 tables and hand rows as whole 16-byte pieces of contiguous memory. */
int brl_belief_deal(int device, const brl_belief_query *queries, int64_t Q, int64_t K, uint64_t seed, int64_t q0, uint64_t *tables,
                    uint64_t *hands, void *stream);

/* One call index of the weight: logits float32 [m, ld] (ld >= 38; row i belongs to row rows[i] of the sample arrays), rows
 * int64 [m] (any order, any subset of 0..n-1, no row twice), query_of int32 [n] (the row's query, 0..Q-1), legal uint64 [Q] and
 * action int32 [Q] (the legal word and the call of each query at this call index).  logw float32 [n] and greedy uint8 [n] are
 * updated in place for the listed rows.  One launch, eight rows per wave (categorical<8>: eight lanes and five actions per lane). */
int brl_belief_logp(int device, const float *logits, int64_t ld, const int64_t *rows, int64_t m, const int32_t *query_of, int64_t n,
                    const uint64_t *legal, const int32_t *action, int64_t Q, float *logw, uint8_t *greedy, void *stream);

/* entries[i], i < Q, from rows i * K .. i * K + K - 1 of hands uint64 [Q * K, 4], logw float32 [Q * K] and greedy uint8 [Q * K];
 * queries as given to brl_belief_deal (the own seat decides which three hands are the hidden ones).  entries 16-byte aligned.
 * One launch, a workgroup of 512 threads per query: the maximum of logw, then the samples in tiles of 512 staged in LDS (weight,
 * hand words, features, greedy flag), and one thread per sum — 443 of them — that walks the tile in ascending k, holding its
 * float64 sum and its integer count in registers. */
int brl_belief_reduce(int device, const brl_belief_query *queries, int64_t Q, int64_t K, const uint64_t *hands, const float *logw,
                      const uint8_t *greedy, brl_belief_entry *entries, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* BRL_BELIEF_H */
