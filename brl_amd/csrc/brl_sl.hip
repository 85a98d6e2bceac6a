// brl_sl.hip — translation unit of libbrl_hip.so: the supervised pre-trainer's device path (sl.py), declared in
// include/brl_sl.h.  Three launches per batch, no host work, so that brl_amd/sl.py captures whole training steps in a hipGraph:
//   k_sl_sample  the (trajectory, call index) pairs of the example stream: a keyed per-epoch permutation + a Philox draw
//   k_sl_replay  those examples: deal, replay the auction prefix, emit the observation row / legal mask / label (the
//                environment's own table logic and row emission, bridge_device.hpp)
//   k_sl_loss    cross-entropy + masked-policy entropy, the metrics, and d total / d logits, one workgroup, fixed-order sums
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/brl_sl.h"
#include "abi_common.hpp"
#include "wave_common.hpp"

namespace {

constexpr uint32_t STREAM_SL_PERM = 0x42534C50u;  // 'BSLP': the Feistel rounds of an epoch's permutation
constexpr uint32_t STREAM_SL_POS = 0x42534C43u;   // 'BSLC': the call-index draw of an example
constexpr int SL_MAX_CALLS = 320;                 // the longest legal auction has 319 calls
constexpr int SL_K = 4;                           // examples per wave in k_sl_replay

inline unsigned blocks_of(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

// ---- the example stream ------------------------------------------------------------------------------------------------------
// perm_e: a 4-round Feistel network on [0, 2^(2 half)) with 2^(2 half) >= n, cycle-walked back into [0, n) (a bijection of
// [0, n) for every key; the walk is short: the domain is less than 4 n).
__device__ __forceinline__ uint32_t sl_feistel(uint32_t x, uint32_t half, uint32_t e, const Rng &g) {
  const uint32_t m = (1u << half) - 1u;
  uint32_t L = x >> half, R = x & m;
#pragma unroll
  for (uint32_t r = 0; r < 4; r++) {
    uint32_t o[4];
    philox4x32_10(R, r, e, STREAM_SL_PERM, g.k0, g.k1, o);
    const uint32_t nl = R;
    R = L ^ (o[0] & m);
    L = nl;
  }
  return (L << half) | R;
}

__global__ __launch_bounds__(256) void k_sl_sample(const int64_t *counter, const int64_t *offsets, int64_t n, uint32_t half, Rng g,
                                                   int64_t batch, int64_t *traj, int32_t *pos) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= batch) return;
  const int64_t gi = counter[0] + i;
  const uint32_t e = (uint32_t)(gi / n);
  uint32_t x = (uint32_t)(gi - (int64_t)e * n);
  do {
    x = sl_feistel(x, half, e, g);
  } while ((int64_t)x >= n);
  uint32_t o[4];
  philox4x32_10((uint32_t)gi, (uint32_t)((uint64_t)gi >> 32), 0u, STREAM_SL_POS, g.k0, g.k1, o);
  const int64_t nc = offsets[x + 1] - offsets[x];
  traj[i] = (int64_t)x;
  pos[i] = (int32_t)(((uint64_t)o[0] * (uint64_t)nc) >> 32);
}

// ---- replay: one wave per SL_K examples (k_step's layout: lane l runs the table logic of example l % SL_K, the 128-B table
// image lives in LDS, the whole wave writes each row) -----------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK_THREADS) void k_sl_replay(const uint64_t *hands, const int64_t *offsets, const uint8_t *calls,
                                                             int64_t n_traj, const int64_t *traj, const int32_t *pos, int64_t batch,
                                                             float *obs, uint8_t *mask, int32_t *label) {
  __shared__ __attribute__((aligned(16))) uint8_t lds_img[WAVES_PER_BLOCK * SL_K * TABLE_BYTES];
  __shared__ __attribute__((aligned(16))) uint8_t lds_calls[WAVES_PER_BLOCK * SL_K * SL_MAX_CALLS];
  const LaneConst c = make_lane_const();
  const int wave = (int)(threadIdx.x >> 6);
  const int64_t row0 = ((int64_t)blockIdx.x * WAVES_PER_BLOCK + wave) * SL_K;
  uint8_t *wimg = lds_img + wave * SL_K * TABLE_BYTES;
  uint8_t *wcalls = lds_calls + wave * SL_K * SL_MAX_CALLS;

  // this lane's example (lane % SL_K): the trajectory, where its calls start, how many of them the prefix has
  const int tl = c.lane % SL_K;
  const int64_t row = row0 + tl;
  const bool valid = row < batch;
  int64_t t = valid ? traj[row] : 0;
  t = (t < 0) ? 0 : ((t >= n_traj) ? n_traj - 1 : t);
  const int64_t start = offsets[t];
  const int64_t ncalls = offsets[t + 1] - start;
  int64_t p = valid ? (int64_t)pos[row] : 0;
  p = (p >= ncalls) ? ncalls - 1 : p;
  p = (p >= SL_MAX_CALLS) ? SL_MAX_CALLS - 1 : p;  // (the LDS staging area; a checked set never gets here)
  p = (p < 0) ? 0 : p;
  const int np = (int)p;

  // the wave's images: history words zero, hand words from the set, scalars zero (written back below)
  uint64_t *wimg64 = reinterpret_cast<uint64_t *>(wimg);
  for (int i = c.lane; i < SL_K * 16; i += 64) {
    const int j = i >> 4, w = i & 15;
    const uint64_t tj = (uint64_t)__shfl((int64_t)t, j, 64);
    wimg64[i] = (w >= W_HAND && w < W_HAND + 4) ? (hands[tj * 4 + (w - W_HAND)] << 4) : 0ull;
  }
  // the prefix calls and the label of each example, staged in LDS (independent byte loads; the logic below reads LDS)
  for (int i = c.lane; i < SL_K * SL_MAX_CALLS; i += 64) {
    const int j = i / SL_MAX_CALLS, k = i - j * SL_MAX_CALLS;
    const int64_t sj = __shfl(start, j, 64);
    const int pj = __shfl(np, j, 64);
    if (k <= pj) wcalls[i] = calls[sj + k];
  }
  wave_lds_fence();

  // the auction prefix: dealer 0, nobody vulnerable, player id = seat (identity _shuffled_players), no tricks.  A prefix of a
  // checked auction never ends it, so there are no rewards and no terminal state.
  Tbl tb;
  tb.sc = (0xE4u << SC_SHUF);
  tb.sch = 0; tb.fd = 0; tb.t2 = 0; tb.t0 = 0; tb.t1 = 0; tb.lut = 0xFFFFFFFFu; tb.bctr = 0; tb.r01 = 0; tb.r23 = 0;
  const uint8_t *mine = wcalls + tl * SL_MAX_CALLS;
  uint32_t *hist = reinterpret_cast<uint32_t *>(wimg + tl * TABLE_BYTES);
  if (c.lane < SL_K) {
    for (int k = 0; k < np; k++) {
      uint32_t a = mine[k];
      a = (a < (uint32_t)BRL_NUM_ACTIONS) ? a : 0u;
      const int hb = auction_step(tb, (int)a, cur_seat(tb));
      if (hb >= 0) atomicOr(hist + (hb >> 5), 1u << (hb & 31));  // ds_or_b32
    }
    store_scalars(tb, wimg + tl * TABLE_BYTES);
  }
  wave_lds_fence();

  const int seat = cur_seat(tb);
  const uint32_t pack = (uint32_t)seat | (vul_nibble(tb, seat) << 2);
  const uint64_t legal = legal_mask(tb);
  if (c.lane < SL_K && valid) label[row] = (int32_t)mine[np];
#pragma unroll
  for (int j = 0; j < SL_K; j++) {
    if (row0 + j < batch) {
      const uint32_t pk = __builtin_amdgcn_readlane(pack, j);
      emit_obs_row_cast(wimg + j * TABLE_BYTES, (int)(pk & 3u), pk >> 2, obs + (row0 + j) * BRL_OBS_SIZE, 0, c);
      emit_mask_row(readlane64(legal, j), mask + (row0 + j) * BRL_NUM_ACTIONS, c);
    }
  }
}

// ---- loss, metrics and d total / d logits: one workgroup, thread i takes samples i, i + 256, ... ---------------------------
// Each round of 256 samples is first staged in LDS with coalesced loads (logits and mask rows); the four passes over a row then
// read LDS instead of waiting on global loads.
constexpr int LOSS_THREADS = 256;
constexpr int NA = BRL_NUM_ACTIONS;

__global__ __launch_bounds__(LOSS_THREADS) void k_sl_loss(const float *logits, int64_t ls, const int32_t *label, const uint8_t *mask,
                                                         int64_t B, float ent_coef, float *dlogits, float *out, int64_t *counter,
                                                         int64_t advance) {
  __shared__ double red[4][LOSS_THREADS];
  __shared__ float zt[LOSS_THREADS * NA];
  __shared__ uint8_t mt[LOSS_THREADS * NA];
  const int tid = (int)threadIdx.x;
  double s_tgt = 0.0, s_ent = 0.0, s_acc = 0.0, s_ill = 0.0;  // per thread, in sample order
  for (int64_t base = 0; base < B; base += LOSS_THREADS) {
    const int rows = (int)((B - base < LOSS_THREADS) ? B - base : LOSS_THREADS);
    __syncthreads();
    for (int e = tid; e < rows * NA; e += LOSS_THREADS) {
      const int r = e / NA, j = e - r * NA;
      zt[e] = logits[(base + r) * ls + j];
      mt[e] = mask[(base + r) * NA + j];
    }
    __syncthreads();
    if (tid >= rows) continue;
    const int64_t b = base + tid;
    // passes over the row (re-read from LDS, not held in registers): maxima / legal bits, sums, terms; the derivative's two
    const float *lg = zt + tid * NA;
    const uint8_t *mk = mt + tid * NA;
    int y = label[b];
    y = (y < 0 || y >= NA) ? 0 : y;
    uint64_t lm = 0ull;  // legal calls as bits
    float mx2 = lg[0], mx = -INFINITY;
    int am = 0;          // argmax of the unmasked logits, first maximum
#pragma unroll 2
    for (int j = 0; j < NA; j++) {
      const float z = lg[j];
      const bool legal = mk[j] != 0;
      lm |= legal ? (1ull << j) : 0ull;
      am = (z > mx2) ? j : am;
      mx2 = fmaxf(mx2, z);
      mx = legal ? fmaxf(mx, z) : mx;
    }
    // unmasked softmax (the target term, accuracy, illegal mass) and the masked one (the entropy), sl.py:176-182
    float s2 = 0.0f, s = 0.0f;
#pragma unroll 2
    for (int j = 0; j < NA; j++) {
      const float z = lg[j];
      s2 += expf(z - mx2);
      s += ((lm >> j) & 1ull) ? expf(z - mx) : 0.0f;
    }
    const float lse2 = logf(s2), lse = logf(s);
    float H = 0.0f, ill = 0.0f;
#pragma unroll 2
    for (int j = 0; j < NA; j++) {
      const float z = lg[j];
      const bool legal = (lm >> j) & 1ull;
      const float lsm = (z - mx) - lse;
      const float p = legal ? expf(lsm) : 0.0f;
      H -= !(p <= 0.0f) ? p * lsm : 0.0f;  // 0 log 0 = 0 (!(p <= 0): a NaN probability stays in the sum)
      ill += legal ? 0.0f : expf((z - mx2) - lse2);
    }
    const float ly = (lg[y] - mx2) - lse2;
    s_tgt += (double)(-ly);
    s_ent += (double)H;
    s_acc += (am == y) ? 1.0 : 0.0;
    s_ill += (double)ill;
    if (dlogits != nullptr) {
      // d/dz_j of -mean(onehot * log_softmax) over [B, 38]: (softmax_j - onehot_j) / (38 B); of -ent_coef * mean(H): ent_coef
      // * p_j (log p_j + H) / B on legal j (an illegal logit sits at finfo.min: its probability and derivative are 0).
      // In float64, rounded once at the store: softmax_y - 1 on a row the network is sure of, and log p_j + H on a flat row,
      // cancel to float32's rounding noise, and a row's derivative is then wrong at ITS scale however small the batch's error.
      // The sums are taken again (the float32 ones above stay what the metrics are made of): H = log s - sum e_j a_j / s.
      const double dmx2 = (double)mx2, dmx = (double)mx;
      double ds2 = 0.0, ds = 0.0, dea = 0.0;
#pragma unroll 2
      for (int j = 0; j < NA; j++) {
        const double z = (double)lg[j];
        ds2 += exp(z - dmx2);
        if ((lm >> j) & 1ull) {
          const double a = z - dmx, e = exp(a);
          ds += e;
          dea += !(e <= 0.0) ? e * a : 0.0;  // 0 log 0 = 0, a NaN stays
        }
      }
      const double dlse2 = log(ds2), dlse = log(ds);
      const double dH = dlse - dea / ds;
      const double d38B = 1.0 / (38.0 * (double)B), dB = (double)ent_coef / (double)B;
#pragma unroll 2
      for (int j = 0; j < NA; j++) {
        const double z = (double)lg[j];
        const bool legal = (lm >> j) & 1ull;
        const double p2 = exp((z - dmx2) - dlse2);
        const double lsm = (z - dmx) - dlse;
        const double p = legal ? exp(lsm) : 0.0;
        const double dt = (p2 - ((j == y) ? 1.0 : 0.0)) * d38B;
        const double de = legal ? dB * (p * (lsm + dH)) : 0.0;
        dlogits[b * NA + j] = (float)(dt + de);
      }
    }
  }
  red[0][tid] = s_tgt; red[1][tid] = s_ent; red[2][tid] = s_acc; red[3][tid] = s_ill;
  __syncthreads();
  for (int w = LOSS_THREADS / 2; w > 0; w >>= 1) {  // fixed pairwise tree: deterministic
    if (tid < w) {
#pragma unroll
      for (int k = 0; k < 4; k++) red[k][tid] += red[k][tid + w];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const double tgt = red[0][0] / (38.0 * (double)B), ent = red[1][0] / (double)B;
    out[0] = (float)(tgt - (double)ent_coef * ent);
    out[1] = (float)tgt;
    out[2] = (float)ent;
    out[3] = (float)(red[2][0] / (double)B);
    out[4] = (float)(red[3][0] / (double)B);
    if (counter != nullptr) counter[0] += advance;
  }
}

}  // namespace

// =====================================================================================
// C-ABI (include/brl_sl.h)
// =====================================================================================
extern "C" int brl_sl_sample(int device, const int64_t *counter, const int64_t *offsets, int64_t n_traj, uint64_t seed, int64_t batch,
                             int64_t *traj, int32_t *pos, void *stream) {
  NEED(counter && offsets && traj && pos, "NULL array");
  NEED(n_traj > 0 && n_traj <= ((int64_t)1 << 31), "n_traj");
  NEED(batch > 0, "batch");
  HIP_TRY(hipSetDevice(device));
  uint32_t half = 1;
  while (((int64_t)1 << (2 * half)) < n_traj) half++;
  const Rng g{(uint32_t)seed, (uint32_t)(seed >> 32)};
  hipLaunchKernelGGL(k_sl_sample, dim3(blocks_of(batch, 256)), dim3(256), 0, (hipStream_t)stream, counter, offsets, n_traj, half, g,
                     batch, traj, pos);
  HIP_TRY(hipGetLastError());
  return BRL_OK;
}

extern "C" int brl_sl_replay(int device, const uint64_t *hands, const int64_t *offsets, const uint8_t *calls, int64_t n_traj,
                             const int64_t *traj, const int32_t *pos, int64_t batch, float *obs, uint8_t *mask, int32_t *label,
                             void *stream) {
  NEED(hands && offsets && calls && traj && pos, "NULL input array");
  NEED(obs && mask && label, "NULL output array");
  NEED(n_traj > 0 && batch > 0, "n_traj / batch");
  NEED(((uintptr_t)obs & 15u) == 0, "obs must be 16-byte aligned");
  HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(k_sl_replay, dim3(blocks_of(batch, WAVES_PER_BLOCK * SL_K)), dim3(BLOCK_THREADS), 0, (hipStream_t)stream, hands,
                     offsets, calls, n_traj, traj, pos, batch, obs, mask, label);
  HIP_TRY(hipGetLastError());
  return BRL_OK;
}

extern "C" int brl_sl_loss(int device, const float *logits, int64_t logits_stride, const int32_t *label, const uint8_t *mask,
                           int64_t batch, float ent_coef, float *dlogits, float *out, int64_t *counter, int64_t advance, void *stream) {
  NEED(logits && label && mask && out, "NULL array");
  NEED(batch > 0, "batch");
  NEED(logits_stride >= BRL_NUM_ACTIONS, "logits_stride");
  HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(k_sl_loss, dim3(1), dim3(LOSS_THREADS), 0, (hipStream_t)stream, logits, logits_stride, label, mask, batch,
                     ent_coef, dlogits, out, counter, advance);
  HIP_TRY(hipGetLastError());
  return BRL_OK;
}
