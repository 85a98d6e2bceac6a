// handle.hpp — the library's handle and the host-side launch helpers every translation unit with handle-taking entry points shares.
#pragma once
#include "abi_common.hpp"   // HIP_TRY, NEED, brl_fail
#include "wave_common.hpp"

struct brl_handle {
  int device;
  int4 *lut_keys;
  int4 *lut_values;
  uint4 *lut_hands;
  int64_t lut_len;
  float *neg_log_n;
  uint64_t seed;
  uint64_t env_offset;
  DevCtx *ctx_dev;  // device mirror of (LUT, seed, env_offset), read by the policy sub-step
  int tables_per_wave;
  int ws;  // 1: wave-specialised fused rollout k_rollout_ws<32,12,1> (default); 0: k_rollout_random<K> (BRL_ROLLOUT_WS=0)
  int fs;  // 1: flag-synchronised k_rollout_fs where it applies (default); 0: always k_rollout_ws (BRL_ROLLOUT_FS=0)
};
static inline int fail(int code, const char *fmt, const char *detail) { return brl_fail(code, fmt, detail); }

static inline Rng rng_of(const brl_handle *h) { return Rng{(uint32_t)h->seed, (uint32_t)(h->seed >> 32)}; }
static inline LutRef lut_of(const brl_handle *h) { return LutRef{h->lut_keys, h->lut_values, (uint32_t)h->lut_len, h->lut_hands}; }
static inline unsigned wave_grid(int64_t n, int K) {
  int64_t per_block = (int64_t)WAVES_PER_BLOCK * K;
  return (unsigned)((n + per_block - 1) / per_block);
}
static inline unsigned thread_grid(int64_t n, int bs) { return (unsigned)((n + bs - 1) / bs); }

#define LAUNCH_K(h, kernel, n, stream, ...)                                                                  \
  do {                                                                                                       \
    hipStream_t _s = (hipStream_t)(stream);                                                                  \
    switch ((h)->tables_per_wave) {                                                                          \
      case 1: hipLaunchKernelGGL(kernel<1>, dim3(wave_grid(n, 1)), dim3(BLOCK_THREADS), 0, _s, __VA_ARGS__); break; \
      case 2: hipLaunchKernelGGL(kernel<2>, dim3(wave_grid(n, 2)), dim3(BLOCK_THREADS), 0, _s, __VA_ARGS__); break; \
      case 8: hipLaunchKernelGGL(kernel<8>, dim3(wave_grid(n, 8)), dim3(BLOCK_THREADS), 0, _s, __VA_ARGS__); break; \
      default: hipLaunchKernelGGL(kernel<4>, dim3(wave_grid(n, 4)), dim3(BLOCK_THREADS), 0, _s, __VA_ARGS__); break; \
    }                                                                                                        \
    HIP_TRY(hipGetLastError());                                                                              \
  } while (0)

// What the per-step kernels' stores ask of the caller's arrays beyond their element types (include/brl_hip.h, brl_step): an
// observation row leaves as 8-byte pieces per lane (emit_obs_row), a table's four rewards as ONE 16-byte store (wave_step_outputs).
// Checked in front of COMMON: a refusal touches neither the handle nor the runtime.
static inline bool ptr_aligned(const void *p, uintptr_t a) { return (((uintptr_t)p) & (a - 1)) == 0; }
static inline bool step_outputs_aligned(const void *state_in, const void *state_out, const void *obs, const void *rewards,
                                        const void *i32a, const void *i32b) {
  return ptr_aligned(state_in, 8) && ptr_aligned(state_out, 8) && ptr_aligned(obs, 8) && ptr_aligned(rewards, 16) &&
         ptr_aligned(i32a, 4) && ptr_aligned(i32b, 4);
}
#define STEP_ALIGN_MSG "state / obs not 8-byte aligned, rewards not 16-byte, int32 / float columns not 4-byte"

// brl_table_info as the evaluators' step moves it (k_eval_step): a board's four rewards leave — and, on the step table B ends,
// come back — as ONE 16-byte piece; last_bid / last_bidder as their element type.  t may be NULL (the single-table form).
static inline bool table_info_aligned(const brl_table_info *t) {
  return t == nullptr || (ptr_aligned(t->rewards, 16) && ptr_aligned(t->last_bid, 4) && ptr_aligned(t->last_bidder, 4));
}
#define TABLE_ALIGN_MSG "table_a / table_b: rewards not 16-byte aligned, last_bid / last_bidder not 4-byte"

#define COMMON(h, n)                 \
  NEED((h) != nullptr, "handle");    \
  NEED((n) >= 0, "n");               \
  if ((n) == 0) return BRL_OK;       \
  HIP_TRY(hipSetDevice((h)->device))
