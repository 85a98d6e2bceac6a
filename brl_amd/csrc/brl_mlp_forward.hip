// brl_mlp_forward.hip — translation unit of libbrl_hip.so: the policy network's fp32 forward for selected rows with the library's
// own kernels end to end, behind ONE C-ABI call (brl_mlp_forward_rows, include/brl_hip.h): observation bytes of the selected
// boards -> float, the hidden layers through brl_mlp_gemm (bias + activation in the epilogue, nn.Linear's own weight layout), the
// 38 + 1 heads with the scatter back to the boards' rows.  Written for the small-batch iterations of the evaluators
// (src/evaluation.py:120-197: the last boards of a duplicate evaluation), which are bound by host launches, not by the GPU.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "abi_common.hpp"
#include "mlp_rows.hpp"

namespace {

using namespace mlp_rows;

__global__ __launch_bounds__(128) void k_obs_rows_f32(const uint8_t *obs, const int64_t *rows, float *x) {
  const int64_t r = blockIdx.x;
  obs_row_f32(obs, rows ? rows[r] : r, x, r);
}

__global__ __launch_bounds__(256) void k_heads_rows(const float *h, int64_t ldh, int hidden, const float *actor_w, const float *actor_b,
                                                    const float *critic_w, const float *critic_b, const int64_t *rows, int64_t m,
                                                    float *out, int64_t ldo) {
  heads_rows_block(h, ldh, hidden, actor_w, actor_b, critic_w, critic_b, rows, m, out, ldo, (int64_t)blockIdx.x * HR, (int)blockIdx.y * HG);
}

}  // namespace

// (K divided over several workgroups per tile — tiles x slices = 512 workgroups, the last slice to arrive adding the partial tiles
//  in index order — was built and measured for the layers of m <= 512 rows: 11.3 us per layer against 12.5 at m = 256, slower at
//  m = 512: a layer this small is a chain of ~5 dependent memory round trips either way; profiles/r04/r04_experiments.txt section 11.)
extern "C" int brl_mlp_forward_rows(int device, const brl_mlp_ref *net, const uint8_t *obs, const int64_t *rows, int64_t m,
                                    float *scratch, int64_t scratch_len, float *out, int64_t ldo, void *stream) {
  NEED(net && obs && scratch && out && m > 0, "net / obs / scratch / out / m");
  NEED(net->nlayers >= 1 && net->nlayers <= 8, "nlayers (1..8)");
  NEED(net->in_features == BRL_OBS_SIZE, "in_features (480)");
  NEED(net->hidden > 0 && net->hidden % 4 == 0 && net->hidden <= 1024, "hidden (a multiple of 4, <= 1024)");
  NEED(net->act == 0 || net->act == 1, "act (0 ReLU, 1 tanh)");
  NEED(net->actor_w && net->actor_b && net->critic_w && net->critic_b, "NULL head arrays");
  for (int l = 0; l < net->nlayers; l++) NEED(net->w[l] && net->b[l], "NULL layer arrays");
  NEED(ldo >= NHEADS, "ldo (>= 39)");
  NEED(m < (1 << 24), "m below 2^24");
  const int64_t H = net->hidden;
  NEED(scratch_len >= m * (BRL_OBS_SIZE + 2 * H) && (((uintptr_t)scratch) & 15) == 0, "scratch: m * (480 + 2 * hidden) floats, 16-byte aligned");
  NEED((((uintptr_t)net->actor_w | (uintptr_t)net->critic_w) & 15) == 0, "head weights not 16-byte aligned");
  // the layers are brl_mlp_gemm's operands: refused HERE, before the cast launch, not by the product behind it
  for (int l = 0; l < net->nlayers; l++)
    NEED((((uintptr_t)net->w[l] | (uintptr_t)net->b[l]) & 15) == 0, "w[l] / b[l] not 16-byte aligned");
  NEED((((uintptr_t)obs | (uintptr_t)net->actor_b | (uintptr_t)net->critic_b | (uintptr_t)out) & 3) == 0 && (((uintptr_t)rows) & 7) == 0,
       "obs / actor_b / critic_b / out not 4-byte aligned (rows: 8-byte)");
  HIP_TRY(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  float *x = scratch, *act[2] = {scratch + m * BRL_OBS_SIZE, scratch + m * BRL_OBS_SIZE + m * H};
  hipLaunchKernelGGL(k_obs_rows_f32, dim3((unsigned)m), dim3(128), 0, s, obs, rows, x);
  const float *cur = x;
  int64_t k = BRL_OBS_SIZE;
  for (int l = 0; l < net->nlayers; l++) {
    float *dst = act[l & 1];
    const int rc = brl_mlp_gemm(device, BRL_GEMM_NT, BRL_GEMM_EPI_BIAS_ACT, cur, k, net->w[l], k, dst, H, m, H, k, net->act, net->b[l],
                                nullptr, 0, nullptr, nullptr, stream);
    if (rc) return rc;
    cur = dst;
    k = H;
  }
  hipLaunchKernelGGL(k_heads_rows, dim3((unsigned)((m + HR - 1) / HR), (NHEADS + HG - 1) / HG), dim3(256), 0, s, cur, H, (int)H,
                     net->actor_w, net->actor_b, net->critic_w, net->critic_b, rows, m, out, ldo);
  HIP_TRY(hipGetLastError());
  return BRL_OK;
}
