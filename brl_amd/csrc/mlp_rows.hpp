// mlp_rows.hpp — the two ends of the policy network's fp32 forward for selected rows, as device functions shared by
// brl_mlp_forward.hip (one network: brl_mlp_forward_rows) and brl_league.hip (rows grouped by network: brl_league_forward):
// the observation bytes of a board -> one float row, and the 38 + 1 heads of four rows with the scatter back to the boards.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/brl_hip.h"

namespace mlp_rows {

constexpr int NHEADS = BRL_NUM_ACTIONS + 1;   // 38 logits + the value

// x[r] = float(obs[src]): one 128-thread workgroup per row, 4 observation bytes -> one 16-byte store
// (r = the row of x, src = the board it is read from; called by every thread of the row's 128-thread workgroup)
__device__ __forceinline__ void obs_row_f32(const uint8_t *obs, int64_t src, float *x, int64_t r) {
  const int t = (int)threadIdx.x;
  if (t < BRL_OBS_SIZE / 4) {
    const uint32_t w = reinterpret_cast<const uint32_t *>(obs + src * BRL_OBS_SIZE)[t];
    reinterpret_cast<float4 *>(x + r * BRL_OBS_SIZE)[t] =
        make_float4((float)(w & 0xFFu), (float)((w >> 8) & 0xFFu), (float)((w >> 16) & 0xFFu), (float)(w >> 24));
  }
}

// The heads: out[rows[r]][hd] = h[r] . w_hd + b_hd for hd = 0..38 (38 actor rows, then the critic row).  Workgroup (x, y) owns 4
// rows of h (in registers: lane l holds columns 4 l + 256 j .. + 3) and the 13 heads 13 y .. 13 y + 12; wave w takes its heads
// w, w + 4, w + 8 (, w + 12): ALL of their weights are requested before anything is used (the kernel is a chain of L2 round trips,
// not arithmetic), 16 partial dot products per lane, reduced across the wave by a halving butterfly (16 + 8 + 4 + 2 + 2 shuffles
// instead of 16 x 6).
constexpr int HR = 4, HG = 13, HPW = 4;   // rows per workgroup, heads per workgroup, heads per wave (at most)
// (r0 = the first of the workgroup's rows, a multiple of HR below m; h0 = the first of its heads, a multiple of HG)
__device__ __forceinline__ void heads_rows_block(const float *h, int64_t ldh, int hidden, const float *actor_w, const float *actor_b,
                                                 const float *critic_w, const float *critic_b, const int64_t *rows, int64_t m,
                                                 float *out, int64_t ldo, int64_t r0, int h0) {
  const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
  float4 wv[HPW][4], hv[HR][4];
#pragma unroll
  for (int i = 0; i < HPW; i++) {
    const int l = w + 4 * i, hd = h0 + l;
    const bool ok = l < HG && hd < NHEADS;
    const float *wr = (hd < BRL_NUM_ACTIONS) ? actor_w + (int64_t)(ok ? hd : 0) * hidden : critic_w;
    // (unconditional loads from clamped addresses, zeros selected afterwards: a guard around a load makes hipcc branch around it
    //  and wait for each one — 32 memory round trips in a row instead of one, 12.6 us instead of 5)
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int k = 4 * lane + 256 * j;
      wv[i][j] = *reinterpret_cast<const float4 *>(wr + ((k < hidden) ? k : 0));
    }
  }
#pragma unroll
  for (int r = 0; r < HR; r++) {
    const int64_t row = (r0 + r < m) ? r0 + r : m - 1;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int k = 4 * lane + 256 * j;
      hv[r][j] = *reinterpret_cast<const float4 *>(h + row * ldh + ((k < hidden) ? k : 0));
    }
  }
  // columns beyond `hidden` and heads this wave does not own contribute zeros (the weights are zeroed: one side is enough)
#pragma unroll
  for (int i = 0; i < HPW; i++) {
    const int l = w + 4 * i;
    const bool ok = l < HG && h0 + l < NHEADS;
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (!ok || 4 * lane + 256 * j >= hidden) wv[i][j] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  float v[HPW * HR];   // [head i][row r]
#pragma unroll
  for (int i = 0; i < HPW; i++)
#pragma unroll
    for (int r = 0; r < HR; r++) {
      float s = 0.0f;
#pragma unroll
      for (int j = 0; j < 4; j++) {
        s = fmaf(hv[r][j].x, wv[i][j].x, s);
        s = fmaf(hv[r][j].y, wv[i][j].y, s);
        s = fmaf(hv[r][j].z, wv[i][j].z, s);
        s = fmaf(hv[r][j].w, wv[i][j].w, s);
      }
      v[i * HR + r] = s;
    }
  // halving butterfly: after the step with lane bit `off`, a lane keeps the half of the values its bit selects; four steps leave one
  // value per lane (index = lane bits 5..2), two more add what lanes differing in bits 1..0 hold — a fixed order
#pragma unroll
  for (int step = 0; step < 4; step++) {
    const int off = 32 >> step, half = (HPW * HR / 2) >> step;
    const bool hi = (lane & off) != 0;
#pragma unroll
    for (int i = 0; i < half; i++) {
      const float send = hi ? v[i] : v[i + half], keep = hi ? v[i + half] : v[i];
      v[i] = keep + __shfl_xor(send, off, 64);
    }
  }
  float s = v[0];
  s += __shfl_xor(s, 2, 64);
  s += __shfl_xor(s, 1, 64);
  if ((lane & 3) == 0) {
    const int idx = lane >> 2, i = idx / HR, r = idx % HR, l = w + 4 * i, hd = h0 + l;
    if (l < HG && hd < NHEADS && r0 + r < m) {
      const int64_t row = r0 + r;
      out[(rows ? rows[row] : row) * ldo + hd] = s + ((hd < BRL_NUM_ACTIONS) ? actor_b[hd] : critic_b[0]);
    }
  }
}

}  // namespace mlp_rows
