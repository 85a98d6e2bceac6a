/*
 * brl_belief_smc.h — C-ABI of the resample-move stages of the hand beliefs (brl_amd/csrc/brl_belief_smc.hip, part of
 * libbrl_hip.so).  include/brl_belief.h weighs K prior deals by the hidden seats' calls; every informative call multiplies the
 * effective sample size by roughly that call's prior probability, so a long auction leaves a handful of deals with all the
 * weight.  The remedy defined here is the resample-move particle filter: after some of the weighed calls the deals of a query are
 * resampled in proportion to their weights, and the copies are moved apart again by Metropolis steps that leave the posterior of
 * the calls made so far invariant.  This header is the specification; it is opt-in, brl_belief.h's entry points are unchanged.
 *
 * Kept apart from brl_hip.h like brl_belief.h: no oracle counterpart; brl_version() does not count these entry points.
 * Conventions are brl_hip.h's: 0 on success, <0 (BRL_E_*) on error with the message in brl_last_error(); every pointer is a
 * device pointer on `device`; `stream` is a hipStream_t passed as void*; nothing synchronises.
 *
 * Particle k of query i (row i * K + k of the sample arrays of brl_belief.h) holds
 *   hands  [4]   its four hand words,
 *   table  [16]  its live 128-byte table (stepped with the calls made so far),
 *   logl   f32   the total log-likelihood of the weighed calls so far under its current hands,
 *   logw   f32   the weight accumulated since the query's last resampling: what brl_belief_logp adds to.  The host gives logl
 *                the same increments (a second brl_belief_logp on it),
 *   greedy u8    brl_belief.h's flag.
 *
 * Schedule.  Fixed by the host from the prefix alone (nothing is read back inside the loop, there is no adaptive trigger):
 * with resample_every = R >= 1, query i resamples after every R-th of its own weighed (hidden-seat) calls, after the tables have
 * been stepped with that call; the stage t of a resampling is the index of that call.  A query with fewer than R hidden calls
 * never resamples.
 *
 * Resample, stage t, a query with stream index q (brl_belief.h's q), over its K particles.
 *   max  = the largest logw_k.  If a logw_k is NaN, or max is -inf or +inf, the query is left as it is: a_j = j, every output is
 *          the input row, logw' = logw — so the final entry is the NaN block brl_belief_reduce defines.  Otherwise
 *   W_k  = exp((double)logw_k - (double)max)                         (float64; in [0, 1], and 1 for some k)
 *   C_k  = the cumulative sum of W in this fixed two-level order, segments of BRL_BELIEF_SMC_SEGMENT = 64 consecutive particles:
 *            I_k = W_k                    if k % 64 == 0,      I_k = I_{k-1} + W_k  otherwise    (serial inside a segment)
 *            O_0 = 0,  O_{s+1} = O_s + I_{64 s + 63}                                             (serial over the segments)
 *            C_k = O_{k / 64} + I_k                                                              (one more addition)
 *          every + a float64 addition, round to nearest.  C is non-decreasing.  The order is a property of this definition, not
 *          of the launch: segments may be summed side by side, nothing depends on the workgroup's size.  numpy: W padded,
 *          reshaped [-1, 64], cumsum along axis 1, the offsets a cumsum of the rows' last entries.
 *   S    = C_{K-1}
 *   u    = ((double)w + 0.5) * 2^-32,  w = word 0 of the Philox4x32-10 block with counter (t, 0, BRL_BELIEF_RESAMPLE_STREAM, q)
 *          and key (seed & 0xFFFFFFFF, seed >> 32)
 *   x_j  = (((double)j + u) * S) / (double)K          (float64, these three operations in this order; non-decreasing in j)
 *   a_j  = the smallest k with C_k > x_j; K - 1 if there is none (rounding could only produce that beyond K = 2^18)
 * (systematic resampling: one draw per query and stage, particle k is drawn floor or ceil of K W_k / S times, the ancestors are
 * non-decreasing).  Outputs, written out of place, for j < K:
 *   hands'[j] = hands[a_j], tables'[j] = tables[a_j] (the whole 128 bytes), logl'[j] = logl[a_j], greedy'[j] = greedy[a_j],
 *   logw'[j] = +0.0, ancestor[j] = a_j (kept for the tests).
 * The device's exp may differ from another library's in the last place, so ancestors are reproducible on the device (the same
 * bytes on every run) and agree with a float64 restatement wherever x_j is not within rounding of a C_k.
 * A query not in the launch's list is not touched, neither are its output rows.
 *
 * Propose, move m (0 <= m < 256) after the resampling of stage t, particle k of stream index q:
 *   (w0, w1, w2, w3) = the Philox block with counter (k, (t << 8) | m, BRL_BELIEF_MOVE_STREAM, q), the seed as key.
 *   The hidden seats are h = 0, 1, 2: seat (s + 1 + h) & 3.  mulhi32(w0, 3) = 0, 1, 2 picks the pair (first, second) = (h0, h1),
 *   (h0, h2), (h1, h2).  i = mulhi32(w1, 13) picks the i-th card, ascending by bit index, of the first seat's hand; mulhi32(w2, 13)
 *   the same of the second seat's.  The proposal is the deal with those two cards exchanged; the own hand and the third hidden
 *   hand are kept.  A hand word without such a card (fewer than 13 cards: never from brl_belief_deal) makes the proposal the deal
 *   itself.  Bits 52..63 of a hand word are dropped.  The proposal is symmetric: the reverse exchange is proposed from the
 *   proposed deal with the same probability (up to the multiply-high draw's 13 / 2^32).
 *   The proposal's table is the empty table of that deal, built by the code brl_belief_deal uses (csrc/belief_table.hpp).
 *
 * Replay, by the host with the existing entry points: the proposal tables go through calls 0..t exactly as the live ones did —
 * brl_observe, the caller's team's forward on exactly the query's K rows, brl_belief_logp into logl_new / greedy_new (which
 * start at 0 / 1), brl_step — so the proposal's likelihood comes from the same route, row by row, as the particle's own.
 *
 * Accept.  v = ((double)w3 + 0.5) * 2^-32 with w3 of the same block.  The particle takes the proposal iff
 *       log(v) < (double)logl_new - (double)logl
 * evaluated in float64 (log is the float64 natural logarithm, good to an ulp; the subtraction of two float32 values is exact in
 * float64 unless it overflows).  A NaN on either side compares false and rejects (-inf - -inf included); logl = -inf with a
 * finite logl_new accepts.  Taking the proposal replaces hands, table, logl and greedy by the proposal's; logw is not touched:
 * the move leaves the target invariant.  Per query, counters[i][0] grows by the particles proposed to and counters[i][1] by those
 * that accepted: 64-bit integer adds, nothing else.
 *
 * End.  brl_belief_reduce, unchanged, on the final hands / logw / greedy: brl_belief_entry does not change.  Under resampling the
 * consistent particles are the greedy-consistent ones among the soft particles, no longer a rejection sample of the prior, and
 * wsum^2 / wsq counts only the weight since the last resampling: the number of distinct deals shows degeneracy.
 *
 * Input values are not trusted: a list entry outside 0..Q-1 is skipped, seat & 3, hand bits 52..63 dropped; every kernel writes
 * only rows of the queries it was given.  A list names no query twice.  No floating-point atomics; the same bytes on every run.
 */
#ifndef BRL_BELIEF_SMC_H
#define BRL_BELIEF_SMC_H

#include <stdint.h>

#include "brl_belief.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BRL_BELIEF_RESAMPLE_STREAM 0x42524C53u /* 'BRLS' (csrc/bridge_device.hpp: STREAM_BELIEF_RESAMPLE) */
#define BRL_BELIEF_MOVE_STREAM 0x42524C4Du     /* 'BRLM' (csrc/bridge_device.hpp: STREAM_BELIEF_MOVE) */
#define BRL_BELIEF_SMC_SEGMENT 64
#define BRL_BELIEF_SMC_MAX_MOVES 256
#define BRL_BELIEF_SMC_MAX_LIST 65535

/* Resampling of the queries list[0..L) (int32 indices into the Q queries of the sample arrays, 1 <= L <= 65535) at stage
 * `stage` (0 .. 2^24 - 1).  stream_of int64 [Q]: the stream index q of every query (its low 32 bits).  tables uint64 [Q * K, 16],
 * hands uint64 [Q * K, 4], logl / logw float32 [Q * K], greedy uint8 [Q * K]; the outputs have the same shapes and overlap no
 * input; ancestor int32 [Q * K].  tables, hands and their outputs 16-byte aligned; 1 <= K, Q * K < 2^31.
 * One launch, a workgroup of 1024 threads per listed query.  The largest logw first.  Then, over tiles of 4096 particles, the
 * weights go to LDS, one thread per segment forms I in place and one thread carries O across the segments: once to get S and —
 * where K exceeds one tile — once more to have every C_k at hand.  Per tile the outputs j whose x_j lie below the tile's last C
 * (their range by bisection over j, x being monotone) search C in LDS by bisection, and the workgroup copies their ancestors'
 * tables and hand rows as whole 16-byte pieces, eight (two) neighbouring lanes per row, the stores contiguous, four loads of a
 * thread in flight before its first store. */
int brl_belief_resample(int device, const int32_t *list, int64_t L, const int64_t *stream_of, int64_t Q, int64_t K, uint64_t seed,
                        int64_t stage, const uint64_t *tables, const uint64_t *hands, const float *logl, const float *logw,
                        const uint8_t *greedy, uint64_t *tables_out, uint64_t *hands_out, float *logl_out, float *logw_out,
                        uint8_t *greedy_out, int32_t *ancestor, void *stream);

/* The proposals of move `move` after the resampling of stage `stage` for the queries list[0..L): queries as given to
 * brl_belief_deal (own seat, dealer, vulnerabilities, seating), hands uint64 [Q * K, 4] the particles' current hands.  The
 * proposals are written compactly, by position in the list: row p * K + k of tables_new uint64 [L * K, 16] and hands_new uint64
 * [L * K, 4] is the proposal for particle k of query list[p] (all rows of a skipped list entry are left alone).  One launch, a
 * wave per 64 particles of one listed query, a lane per particle; the table image is built in LDS and the wave stores its tables
 * and hand rows as whole 16-byte pieces, as brl_belief_deal does. */
int brl_belief_propose(int device, const brl_belief_query *queries, const int32_t *list, int64_t L, const int64_t *stream_of, int64_t Q,
                       int64_t K, uint64_t seed, int64_t stage, int64_t move, const uint64_t *hands, uint64_t *tables_new,
                       uint64_t *hands_new, void *stream);

/* The acceptance of those proposals: tables_new / hands_new as brl_belief_propose wrote them and the host replayed them (the
 * tables stepped through calls 0..stage), logl_new float32 [L * K] and greedy_new uint8 [L * K] from the replay; tables, hands,
 * logl, greedy: the particles, updated in place where the proposal is taken; counters uint64 [Q, 2] (proposals, accepted),
 * added to.  One launch, a wave per 64 particles of one listed query: a lane decides for its particle, the wave then copies the
 * accepted rows as whole 16-byte pieces (a select-and-copy: rejected particles' rows are neither read nor written). */
int brl_belief_accept(int device, const int32_t *list, int64_t L, const int64_t *stream_of, int64_t Q, int64_t K, uint64_t seed,
                      int64_t stage, int64_t move, const uint64_t *tables_new, const uint64_t *hands_new, const float *logl_new,
                      const uint8_t *greedy_new, uint64_t *tables, uint64_t *hands, float *logl, uint8_t *greedy, uint64_t *counters,
                      void *stream);

#ifdef __cplusplus
}
#endif

#endif /* BRL_BELIEF_SMC_H */
