/*
 * brl_distill.h — C-ABI of policy distillation's device path (brl_amd/csrc/brl_distill.hip, part of libbrl_hip.so): the soft
 * targets of an ensemble of K teachers and the loss head that fits a student's masked policy and value to them
 * (brl_amd/distill.py).
 *
 * Kept apart from brl_hip.h like brl_sl.h and brl_compare.h: these entry points have no oracle counterpart; brl_version() does
 * not count them.
 *
 * Conventions are brl_hip.h's: 0 on success, <0 (BRL_E_*) on error with the message in brl_last_error(); every pointer is a
 * device pointer on `device`; `stream` is a hipStream_t passed as void*; nothing synchronises.  The same bits on every run.
 *
 * Definition.  Per row b: the student's logits z[38] and value u; for each teacher k < K (1 <= K <= BRL_DISTILL_MAX_TEACHERS)
 * its logits t_k[38] and value v_k; mixture weights w_k > 0 that the host normalised in float64 to sum 1 and passes as
 * float32; the legal mask m[38] (uint8; Pass is always legal); a temperature tau > 0.  Everything below is float32, one IEEE
 * operation per operation written, nothing contracted, sums over j = 0 .. 37 and over k = 0 .. K - 1 ascending.
 *
 *   msoftmax(x / tau), the masked softmax: y_j = x_j / tau, mx = the largest legal y_j (a NaN stays: nan_math.hpp),
 *     s = sum over legal j of expf(y_j - mx), lsm_j = (y_j - mx) - logf(s), probability expf(lsm_j) on legal j and 0 on
 *     illegal j — the way k_sl_loss forms it.
 *   teacher target   q_j  = sum_k w_k * expf(lsm_kj)          (the arithmetic mixture: "a random member is at the table")
 *   target value     v*   = sum_k w_k * v_k
 *   log q_j          in log space: a_k = logf(w_k) + lsm_kj, M = max_k a_k, log q_j = M + logf(sum_k expf(a_k - M)), as a
 *                    running maximum with a rescaled sum; an a_k of -inf adds nothing.  For K = 1 it is lsm_0j bit for bit.
 *   teacher entropy  hq   = -sum over legal j with q_j > 0 of q_j * log q_j                         (0 log 0 = 0)
 *   student          p_j  = expf(lsm_j(z / tau)) on legal j, 0 elsewhere
 *   policy loss      ce   = -sum over legal j with q_j > 0 of q_j * lsm_j(z / tau)
 *                    L_pol = (tau * tau) * (ce - hq)                                    (= tau^2 KL(q || p))
 *   value loss       L_val = (u - v*) * (u - v*)
 *   total            = mean_b(c_pol L_pol + c_val L_val)
 *   gradients        dz_j = ((c_pol * tau) / B) * (p_j - q_j) on legal j, exactly 0.0f on illegal j
 *                    du   = ((2 * c_val) / B) * (u - v*)
 *
 * One shared code path.  Both kernels form lsm and the sum over the legal calls of q_j * (a log value) through the SAME two
 * device functions (distill_lsm, distill_cross in brl_distill.hip), in one order.  That is what makes the K = 1 identity
 * exact: when z equals t_0 bit for bit, at any tau, p equals q and lsm equals log q bit for bit, so the row's L_pol is exactly
 * 0, every dz of the row is exactly 0 and the row counts as an agreement.  A second copy of that arithmetic in either kernel
 * would lose this.
 *
 * Metrics row, 8 floats: total, mean L_pol, mean L_val, mean hq, mean entropy of p (-sum p_j lsm_j, 0 log 0 = 0),
 * agreement, illegal mass, and one reserved 0.  Agreement is the share of rows where the first maximum of z over the legal
 * calls is the first maximum of q over the legal calls (a NaN is never a maximum).  Illegal mass is the mean mass of the
 * UNMASKED softmax(z) (no temperature) on the illegal calls, sl.py's illegal_actions_prob.  The rows' float32 terms are added
 * as float64: rows in ascending order inside each block of BRL_DISTILL_BLOCK rows (one lane per row, then a fixed pairwise
 * tree), blocks by a fixed stride and a fixed tree in a second launch.  No floating-point atomics: the same inputs give the
 * same bits on every run, with or without the gradient, whatever the grid.
 *
 * Non-finite inputs (DESIGN, "Non-finite values"): nothing is clamped or replaced.  A NaN on a legal logit of a teacher makes
 * the row's q NaN on every legal call, its hq NaN, and with them the row's L_pol and its dz on the legal calls; a NaN on a
 * legal student logit does the same to L_pol and dz; a NaN value (u or a v_k) makes v*, L_val and du NaN.  The sums that hold
 * such a term are NaN; no other row's q, dz or du changes by a bit.  dz on an illegal call is 0.0f even then, and logits on
 * illegal calls are not read by the masked terms.  A legal teacher logit of -inf gives that teacher probability 0 there and
 * adds 0; a row in which every legal logit of a teacher is -inf is NaN (-inf - -inf).
 */
#ifndef BRL_DISTILL_H
#define BRL_DISTILL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BRL_DISTILL_ACTIONS 38
#define BRL_DISTILL_MAX_TEACHERS 8
#define BRL_DISTILL_BLOCK 64   /* rows per workgroup: one row per lane of one wave */
#define BRL_DISTILL_METRICS 8

/* The targets of `batch` rows: q float [batch, 38], vstar float [batch], hq float [batch].
 * Teacher k's logits of row b are t_logits[k * k_stride + b * row_stride + 0..37] and its value is
 * t_values[k * vk_stride + b * v_stride] (strides in floats), so the [K, n, 39] stack of InferenceSnapshot.heads is passed
 * as (heads, n * 39, 39, heads + 38, n * 39, 39).  weights float [K], mask uint8 [batch, 38].  A grid over the rows. */
int brl_distill_targets(int device, const float *t_logits, int64_t k_stride, int64_t row_stride, const float *t_values,
                        int64_t vk_stride, int64_t v_stride, const float *weights, const uint8_t *mask, int64_t batch,
                        int32_t num_teachers, float tau, float *q, float *vstar, float *hq, void *stream);

/* The loss, its metrics and gradients of `batch` rows: z float [batch, >= 38] (row stride z_stride), u float (stride
 * u_stride), q / vstar / hq as brl_distill_targets wrote them, mask uint8 [batch, 38].  dz float [batch, 38] and du float
 * [batch] = d total / d z and d total / d u; dz == NULL (then du is not written either): metrics only, bit-equal to the
 * gradient call's.  out float [8]: the metrics row.  work: at least BRL_DISTILL_METRICS doubles per block of
 * BRL_DISTILL_BLOCK rows (8 * ceil(batch / 64)), which the two launches of this call own until the second has run (the
 * per-block partial sums). */
int brl_distill_loss(int device, const float *z, int64_t z_stride, const float *u, int64_t u_stride, const float *q,
                     const float *vstar, const float *hq, const uint8_t *mask, int64_t batch, float tau, float c_pol,
                     float c_val, float *dz, float *du, float *out, double *work, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* BRL_DISTILL_H */
