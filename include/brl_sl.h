/*
 * brl_sl.h — C-ABI of the supervised pre-trainer's device path (brl_amd/csrc/brl_sl.hip, part of libbrl_hip.so):
 * the batch source and the loss head of the reference's sl.py (imitation of recorded auctions).
 *
 * Kept apart from brl_hip.h on purpose: that header is the environment's frozen boundary, which the CPU oracle's shim
 * exports symbol for symbol.  These entry points have no oracle counterpart; brl_version() does not count them.
 *
 * Conventions are brl_hip.h's: 0 on success, <0 (BRL_E_*) on error with the message in brl_last_error(); every pointer
 * is a device pointer on `device`; `stream` is a hipStream_t passed as void*; nothing synchronises.  No handle.
 *
 * The trajectory set (brl_amd/sl_data.py builds it from the text files):
 *   hands   uint64 [n_traj, 4]  each seat's 13 cards as bits of the observation's hand section (bit rank * 4 + suit,
 *                               suits C,D,H,S, ranks 2..A); seat 0 deals.
 *   offsets int64  [n_traj + 1] trajectory t's calls are calls[offsets[t] .. offsets[t + 1])
 *   calls   uint8  [total]      pgx action ids 0..37 (0 pass, 1 double, 2 redouble, 3 + 5 * (level - 1) + strain bids);
 *                               every auction is legal and ends exactly at its last call (checked at load).
 */
#ifndef BRL_SL_H
#define BRL_SL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The (trajectory, call index) pairs of one batch of the example stream (sl.py:100-117).  Example g = *counter + i
 * (i < batch) is trajectory perm_e(g % n_traj) of epoch e = g / n_traj, where perm_e is a keyed bijection of [0, n_traj)
 * (a 4-round Feistel network on the next even power of two, Philox rounds keyed by (seed, e), cycle-walking), and call
 * index pos = (u * n_calls) >> 32 for the Philox draw u of (seed, g).  *counter is only read: a later launch of the step
 * advances it (brl_sl_loss).  traj int64 [batch], pos int32 [batch]. */
int brl_sl_sample(int device, const int64_t *counter, const int64_t *offsets, int64_t n_traj, uint64_t seed, int64_t batch,
                  int64_t *traj, int32_t *pos, void *stream);

/* The examples of explicit (trajectory, call index) pairs: the table dealt from hands[traj] (dealer seat 0, nobody
 * vulnerable), calls[0 .. pos) of that trajectory applied, then obs float [batch, 480] (0.0 / 1.0) of the seat to act,
 * mask uint8 [batch, 38] its legal calls and label int32 [batch] the call it made.  obs 16-byte aligned (a row leaves as 16-byte
 * pieces; BRL_E_ARG otherwise), every other array as its element type.  traj / pos out of range are clamped
 * into the set (a pair must name a decision point: 0 <= pos < n_calls). */
int brl_sl_replay(int device, const uint64_t *hands, const int64_t *offsets, const uint8_t *calls, int64_t n_traj,
                  const int64_t *traj, const int32_t *pos, int64_t batch, float *obs, uint8_t *mask, int32_t *label,
                  void *stream);

/* sl.py's loss (:169-184) and metrics (:195-205, 288-300) of one batch, one workgroup, fixed-order sums:
 * logits float [batch, >= 38] (row stride logits_stride), label int32 [batch], mask uint8 [batch, 38].
 * out float [5] = total (target_loss - ent_coef * entropy), target_loss (-mean over [batch, 38] of onehot * log_softmax),
 * entropy (mean of the masked policy's, 0 log 0 = 0), accuracy (argmax of the unmasked logits == label; first maximum
 * on ties), illegal_prob (mean of the unmasked softmax's mass on illegal calls).
 * dlogits float [batch, 38] (NULL: metrics only) = d total / d logits.
 * counter (may be NULL): *counter += advance after the sums (the example stream's cursor, read by brl_sl_sample). */
int brl_sl_loss(int device, const float *logits, int64_t logits_stride, const int32_t *label, const uint8_t *mask,
                int64_t batch, float ent_coef, float *dlogits, float *out, int64_t *counter, int64_t advance, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* BRL_SL_H */
