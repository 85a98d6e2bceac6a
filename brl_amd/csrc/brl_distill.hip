// brl_distill.hip — translation unit of libbrl_hip.so: policy distillation's device path, declared in include/brl_distill.h (the
// definition lives there).  Three kernels, no host work, so that brl_amd/distill.py captures whole training steps in a
// hipGraph:
//   k_distill_targets  the ensemble's soft targets of a collected batch: q, v*, the teachers' entropy hq — a grid over the rows
//   k_distill_loss     tau^2 KL(q || p) + the value loss of a minibatch, d total / d z and d total / d u, per-block float64 partials
//   k_distill_finish   the partials in a fixed order -> the metrics row
// Layout (k_sl_loss's): a workgroup is one wave and takes BRL_DISTILL_BLOCK = 64 rows.  The rows' logits are staged in LDS with
// coalesced loads at a pitch of 39 floats — lane l then reads dword 39 l + j: 39 is odd, so the 32 lanes of a half-wave sit on 32
// different banks (at the rows' own pitch of 38 they would sit two to a bank) —, one lane works through one row, and what the lane
// produced per call (q, dz) goes back through LDS into coalesced stores.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/brl_distill.h"
#include "abi_common.hpp"
#include "nan_math.hpp"

namespace {

constexpr int NA = BRL_DISTILL_ACTIONS;
constexpr int ROWS = BRL_DISTILL_BLOCK;
constexpr int NM = BRL_DISTILL_METRICS;
constexpr int PITCH = 39;        // floats per staged row
constexpr int MASK_PITCH = 44;   // bytes per staged mask row: 11 dwords, odd
constexpr int FINISH_THREADS = 256;

static_assert(ROWS == 64, "one row per lane of one wave");

inline unsigned blocks_of(int64_t n) { return (unsigned)((n + ROWS - 1) / ROWS); }

// ---- the two functions BOTH kernels go through (include/brl_distill.h, "One shared code path") -----------------------------------
struct Lsm {
  float mx, lse;
};

// the masked log-softmax of row / tau: the largest legal y_j = row[j] / tau and logf of the legal calls' sum of expf(y_j - mx)
__device__ __forceinline__ Lsm distill_lsm(const float *row, uint64_t lm, float tau) {
  float mx = -INFINITY;
#pragma unroll
  for (int j = 0; j < NA; j++) mx = ((lm >> j) & 1ull) ? max_nan(mx, row[j] / tau) : mx;
  float s = 0.0f;
#pragma unroll
  for (int j = 0; j < NA; j++) s += ((lm >> j) & 1ull) ? expf(row[j] / tau - mx) : 0.0f;
  return Lsm{mx, logf(s)};
}

__device__ __forceinline__ float lsm_at(float x, float tau, const Lsm &r) { return (x / tau - r.mx) - r.lse; }

// sum over the legal calls with q_j > 0 of q_j * logv_j (0 log 0 = 0; !(q <= 0): a NaN probability stays in the sum)
__device__ __forceinline__ float distill_cross(const float *qrow, const float *logv, uint64_t lm) {
  float acc = 0.0f;
#pragma unroll
  for (int j = 0; j < NA; j++) {
    const float qj = qrow[j];
    acc += (((lm >> j) & 1ull) && !(qj <= 0.0f)) ? qj * logv[j] : 0.0f;
  }
  return acc;
}

// ---- staging ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void stage_rows(float *tile, const float *src, int64_t stride, int rows, int tid) {
  for (int e = tid; e < rows * NA; e += ROWS) {
    const int r = e / NA, j = e - r * NA;
    tile[r * PITCH + j] = src[(int64_t)r * stride + j];
  }
}

__device__ __forceinline__ void stage_mask(uint8_t *tile, const uint8_t *src, int rows, int tid) {
  for (int e = tid; e < rows * NA; e += ROWS) {
    const int r = e / NA, j = e - r * NA;
    tile[r * MASK_PITCH + j] = src[e];
  }
}

__device__ __forceinline__ void unstage_rows(float *dst, const float *tile, int rows, int tid) {
  for (int e = tid; e < rows * NA; e += ROWS) {
    const int r = e / NA, j = e - r * NA;
    dst[e] = tile[r * PITCH + j];
  }
}

__device__ __forceinline__ uint64_t legal_bits(const uint8_t *mk) {
  uint64_t lm = 0ull;
#pragma unroll
  for (int j = 0; j < NA; j++) lm |= (mk[j] != 0) ? (1ull << j) : 0ull;
  return lm;
}

// ---- targets --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ROWS) void k_distill_targets(const float *tl, int64_t ks, int64_t rs, const float *tv, int64_t vks,
                                                         int64_t vs, const float *w, const uint8_t *mask, int64_t B, int K, float tau,
                                                         float *q, float *vstar, float *hq) {
  __shared__ float tt[ROWS * PITCH];   // teacher k's logits
  __shared__ float qt[ROWS * PITCH];   // q so far
  __shared__ float at[ROWS * PITCH];   // the running maximum of a_k, then log q
  __shared__ float st[ROWS * PITCH];   // the rescaled sum of expf(a_k - maximum)
  __shared__ uint8_t mk[ROWS * MASK_PITCH];
  const int tid = (int)threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * ROWS;
  const int rows = (int)((B - base < ROWS) ? B - base : ROWS);
  const bool mine = tid < rows;
  stage_mask(mk, mask + base * NA, rows, tid);
  float *qrow = qt + tid * PITCH, *arow = at + tid * PITCH, *srow = st + tid * PITCH;
  for (int j = 0; j < NA; j++) {
    qrow[j] = 0.0f;
    arow[j] = -INFINITY;
    srow[j] = 0.0f;
  }
  __syncthreads();
  const uint64_t lm = mine ? legal_bits(mk + tid * MASK_PITCH) : 0ull;
  float vacc = 0.0f;
  for (int k = 0; k < K; k++) {
    __syncthreads();   // the lanes are done with teacher k - 1's tile
    stage_rows(tt, tl + (int64_t)k * ks + base * rs, rs, rows, tid);
    __syncthreads();
    if (mine) {
      const float wk = w[k], lw = logf(wk);
      const float *trow = tt + tid * PITCH;
      const Lsm r = distill_lsm(trow, lm, tau);
#pragma unroll
      for (int j = 0; j < NA; j++) {
        if (!((lm >> j) & 1ull)) continue;
        const float l = lsm_at(trow[j], tau, r);
        qrow[j] += wk * expf(l);
        const float a = lw + l;
        if (!(a == -INFINITY)) {   // (a NaN goes on)
          const float m = arow[j], m2 = max_nan(m, a);
          srow[j] = srow[j] * expf(m - m2) + expf(a - m2);
          arow[j] = m2;
        }
      }
      vacc += wk * tv[(int64_t)k * vks + (base + tid) * vs];
    }
  }
  if (mine) {
#pragma unroll
    for (int j = 0; j < NA; j++) arow[j] = arow[j] + logf(srow[j]);   // log q_j
    hq[base + tid] = -distill_cross(qrow, arow, lm);
    vstar[base + tid] = vacc;
  }
  __syncthreads();
  unstage_rows(q + base * NA, qt, rows, tid);
}

// ---- loss, gradients, per-block partials ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ROWS) void k_distill_loss(const float *z, int64_t zs, const float *u, int64_t us, const float *q,
                                                      const float *vstar, const float *hq, const uint8_t *mask, int64_t B, float tau,
                                                      float c_pol, float c_val, float *dz, float *du, double *work) {
  __shared__ float zt[ROWS * PITCH];   // z, then dz
  __shared__ float qt[ROWS * PITCH];
  __shared__ float lt[ROWS * PITCH];   // lsm(z / tau)
  __shared__ uint8_t mk[ROWS * MASK_PITCH];
  __shared__ double red[6][ROWS];
  const int tid = (int)threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * ROWS;
  const int rows = (int)((B - base < ROWS) ? B - base : ROWS);
  stage_mask(mk, mask + base * NA, rows, tid);
  stage_rows(zt, z + base * zs, zs, rows, tid);
  stage_rows(qt, q + base * NA, NA, rows, tid);
  __syncthreads();
  double t_pol = 0.0, t_val = 0.0, t_hq = 0.0, t_ent = 0.0, t_agree = 0.0, t_ill = 0.0;
  if (tid < rows) {
    const int64_t b = base + tid;
    float *zrow = zt + tid * PITCH, *lrow = lt + tid * PITCH;
    const float *qrow = qt + tid * PITCH;
    const uint64_t lm = legal_bits(mk + tid * MASK_PITCH);
    const float gz = (c_pol * tau) / (float)B, gu = (2.0f * c_val) / (float)B;
    // the unmasked softmax of z (the illegal mass) and the first maxima of z and of q over the legal calls
    float mx2 = zrow[0], zbest = -INFINITY, qbest = -INFINITY;
    int az = 0, aq = 0;
#pragma unroll
    for (int j = 0; j < NA; j++) {
      const float zj = zrow[j], qj = qrow[j];
      const bool legal = (lm >> j) & 1ull;
      mx2 = max_nan(mx2, zj);
      az = (legal && zj > zbest) ? j : az;
      zbest = (legal && zj > zbest) ? zj : zbest;
      aq = (legal && qj > qbest) ? j : aq;
      qbest = (legal && qj > qbest) ? qj : qbest;
    }
    float s2 = 0.0f;
#pragma unroll
    for (int j = 0; j < NA; j++) s2 += expf(zrow[j] - mx2);
    const float lse2 = logf(s2);
    float ill = 0.0f;
#pragma unroll
    for (int j = 0; j < NA; j++) ill += ((lm >> j) & 1ull) ? 0.0f : expf((zrow[j] - mx2) - lse2);
    // the masked policy at tau: lsm, the entropy of p, p - q (z_j is dead once its lsm is formed: dz takes its place)
    const Lsm r = distill_lsm(zrow, lm, tau);
    float H = 0.0f;
#pragma unroll
    for (int j = 0; j < NA; j++) {
      const bool legal = (lm >> j) & 1ull;
      const float l = lsm_at(zrow[j], tau, r);
      const float p = legal ? expf(l) : 0.0f;
      H -= (legal && !(p <= 0.0f)) ? p * l : 0.0f;
      lrow[j] = l;
      zrow[j] = legal ? gz * (p - qrow[j]) : 0.0f;
    }
    const float ce = -distill_cross(qrow, lrow, lm);
    const float h = hq[b];
    const float lpol = (tau * tau) * (ce - h);
    const float d = u[b * us] - vstar[b];
    if (dz != nullptr) du[b] = gu * d;
    t_pol = (double)lpol;
    t_val = (double)(d * d);
    t_hq = (double)h;
    t_ent = (double)H;
    t_agree = (az == aq) ? 1.0 : 0.0;
    t_ill = (double)ill;
  }
  red[0][tid] = t_pol; red[1][tid] = t_val; red[2][tid] = t_hq; red[3][tid] = t_ent; red[4][tid] = t_agree; red[5][tid] = t_ill;
  __syncthreads();
  for (int wd = ROWS / 2; wd > 0; wd >>= 1) {   // fixed pairwise tree: deterministic
    if (tid < wd) {
#pragma unroll
      for (int k = 0; k < 6; k++) red[k][tid] += red[k][tid + wd];
    }
    __syncthreads();
  }
  if (tid < NM) work[(int64_t)blockIdx.x * NM + tid] = (tid < 6) ? red[tid][0] : 0.0;
  if (dz != nullptr) unstage_rows(dz + base * NA, zt, rows, tid);
}

// ---- the blocks' partials, in a fixed order --------------------------------------------------------------------------------------
__global__ __launch_bounds__(FINISH_THREADS) void k_distill_finish(const double *work, int64_t nblocks, int64_t B, float c_pol,
                                                                  float c_val, float *out) {
  __shared__ double red[6][FINISH_THREADS];
  const int tid = (int)threadIdx.x;
  double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int64_t i = tid; i < nblocks; i += FINISH_THREADS) {
#pragma unroll
    for (int k = 0; k < 6; k++) acc[k] += work[i * NM + k];
  }
#pragma unroll
  for (int k = 0; k < 6; k++) red[k][tid] = acc[k];
  __syncthreads();
  for (int wd = FINISH_THREADS / 2; wd > 0; wd >>= 1) {
    if (tid < wd) {
#pragma unroll
      for (int k = 0; k < 6; k++) red[k][tid] += red[k][tid + wd];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const double n = (double)B;
    const double pol = red[0][0] / n, val = red[1][0] / n;
    out[0] = (float)((double)c_pol * pol + (double)c_val * val);
    out[1] = (float)pol;
    out[2] = (float)val;
    out[3] = (float)(red[2][0] / n);
    out[4] = (float)(red[3][0] / n);
    out[5] = (float)(red[4][0] / n);
    out[6] = (float)(red[5][0] / n);
    out[7] = 0.0f;
  }
}

}  // namespace

// =====================================================================================
// C-ABI (include/brl_distill.h)
// =====================================================================================
extern "C" int brl_distill_targets(int device, const float *t_logits, int64_t k_stride, int64_t row_stride, const float *t_values,
                                   int64_t vk_stride, int64_t v_stride, const float *weights, const uint8_t *mask, int64_t batch,
                                   int32_t num_teachers, float tau, float *q, float *vstar, float *hq, void *stream) {
  NEED(t_logits && t_values && weights && mask, "NULL input array");
  NEED(q && vstar && hq, "NULL output array");
  NEED(batch > 0 && batch <= ((int64_t)1 << 36), "batch");
  NEED(num_teachers >= 1 && num_teachers <= BRL_DISTILL_MAX_TEACHERS, "num_teachers");
  NEED(row_stride >= BRL_DISTILL_ACTIONS && v_stride >= 1 && k_stride >= 0 && vk_stride >= 0, "strides");
  NEED(tau > 0.0f && tau < INFINITY, "tau");
  HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(k_distill_targets, dim3(blocks_of(batch)), dim3(ROWS), 0, (hipStream_t)stream, t_logits, k_stride, row_stride,
                     t_values, vk_stride, v_stride, weights, mask, batch, (int)num_teachers, tau, q, vstar, hq);
  HIP_TRY(hipGetLastError());
  return BRL_OK;
}

extern "C" int brl_distill_loss(int device, const float *z, int64_t z_stride, const float *u, int64_t u_stride, const float *q,
                                const float *vstar, const float *hq, const uint8_t *mask, int64_t batch, float tau, float c_pol,
                                float c_val, float *dz, float *du, float *out, double *work, void *stream) {
  NEED(z && u && q && vstar && hq && mask && out && work, "NULL array");
  NEED((dz == nullptr) == (du == nullptr), "dz and du come together");
  NEED(batch > 0 && batch <= ((int64_t)1 << 36), "batch");
  NEED(z_stride >= BRL_DISTILL_ACTIONS && u_stride >= 1, "strides");
  NEED(tau > 0.0f && tau < INFINITY, "tau");
  HIP_TRY(hipSetDevice(device));
  const int64_t nblocks = (int64_t)blocks_of(batch);
  hipLaunchKernelGGL(k_distill_loss, dim3((unsigned)nblocks), dim3(ROWS), 0, (hipStream_t)stream, z, z_stride, u, u_stride, q, vstar, hq,
                     mask, batch, tau, c_pol, c_val, dz, du, work);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_distill_finish, dim3(1), dim3(FINISH_THREADS), 0, (hipStream_t)stream, work, nblocks, batch, c_pol, c_val, out);
  HIP_TRY(hipGetLastError());
  return BRL_OK;
}
