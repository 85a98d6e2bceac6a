// brl_league.hip — translation unit of libbrl_hip.so: the batched league evaluation (include/brl_league.h).  Many duplicate matches
// between pairs of networks of one architecture are ONE batch of boards (match-major); per iteration the boards whose team acts
// are sorted by the network that plays that team in their match (brl_league_route) and forwarded as a grouped product
// (brl_league_forward): the cast, every hidden layer and the heads are one launch each over ALL groups.  The layer is
// mg::gemm_tile (csrc/mlp_gemm.hpp) on a group's slice of the dense activation buffer; the ends of the forward are
// csrc/mlp_rows.hpp, shared with brl_mlp_forward_rows — a routed row's logits are that entry point's, bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/brl_league.h"
#include "abi_common.hpp"
#include "mlp_gemm.hpp"
#include "mlp_rows.hpp"
#include "route_common.hpp"

namespace {

using namespace mlp_rows;
using route::board_acts;

// ---- route -------------------------------------------------------------------------------------------------------------------------
constexpr int RW = 4;   // waves (= order slots) per workgroup of the count and scatter kernels

// the match of slot k (clamped into the batch: a bad `order` can make the result wrong, never an address)
__device__ __forceinline__ int64_t slot_match(const int32_t *order, int64_t k, int64_t nmatch) {
  return route::clamp_index(order[k], nmatch);
}

// work[k] = acting boards of slot k's match: one wave per slot, 64 boards per ballot
__global__ __launch_bounds__(64 * RW) void k_route_count(const uint8_t *terminated, const int32_t *current_player, int team, int64_t n,
                                                         const int32_t *order, int64_t nmatch, int32_t *work) {
  const int lane = (int)threadIdx.x & 63;
  const int64_t k = (int64_t)blockIdx.x * RW + (threadIdx.x >> 6);
  if (k >= nmatch) return;
  const int64_t base = slot_match(order, k, nmatch) * n;
  int c = 0;
  for (int64_t i0 = 0; i0 < n; i0 += 64) {
    const int64_t i = i0 + lane;
    const bool a = i < n && board_acts(terminated, current_player, base + i, team);
    c += __popcll(__ballot(a));
  }
  if (lane == 0) work[k] = c;
}

// work[nmatch + k] = the first row of slot k, group_first = the groups' first rows and the total: route::scan on counts that
// k_route_count wrote in the order already
__global__ __launch_bounds__(1024) void k_route_scan(const int32_t *group_of, int64_t nmatch, int ngroups, int32_t *work,
                                                     int32_t *group_first) {
  route::scan<false>(nullptr, group_of, nmatch, ngroups, work, group_first);
}

// rows[first row of slot k ..] = the acting boards of its match, ascending
__global__ __launch_bounds__(64 * RW) void k_route_scatter(const uint8_t *terminated, const int32_t *current_player, int team, int64_t n,
                                                           const int32_t *order, int64_t nmatch, const int32_t *work, int64_t *rows) {
  const int lane = (int)threadIdx.x & 63;
  const int64_t k = (int64_t)blockIdx.x * RW + (threadIdx.x >> 6);
  if (k >= nmatch) return;
  const int64_t base = slot_match(order, k, nmatch) * n;
  int64_t pos = work[nmatch + k];
  for (int64_t i0 = 0; i0 < n; i0 += 64) {
    const int64_t i = i0 + lane;
    const bool a = i < n && board_acts(terminated, current_player, base + i, team);
    const unsigned long long bal = __ballot(a);
    if (a) rows[pos + __popcll(bal & ((1ull << lane) - 1ull))] = base + i;
    pos += __popcll(bal);
  }
}

// ---- forward -----------------------------------------------------------------------------------------------------------------------
// Work unit u of a launch whose units hold 2^SH rows of ONE group: group g owns the units [f(g), f(g + 1)) with
// f(g) = (group_first[g] >> SH) + g, which are at least ceil(size_g / 2^SH) (floor((r + s) / T) + 1 >= ceil(s / T) for a group of
// s rows that starts r rows into a unit) — so floor(R / 2^SH) + ngroups units hold every group's tiles whatever the sizes are, and
// the host needs a bound of R only.  The group of a unit: binary search for the last g with f(g) <= u (f is strictly increasing).
// Returns false for a unit without rows.  Everything is wave-uniform (the loads are scalar).
// (rmax: the caller's bound of R — a unit that reaches beyond it does not exist when the bound holds, and touches nothing when it does not)
template <int SH>
__device__ __forceinline__ bool unit_group(const int32_t *group_first, int ngroups, int u, int rmax, int &g, int &first, int &size, int &local) {
  int lo = 0, hi = ngroups;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if ((group_first[mid] >> SH) + mid <= u) lo = mid;
    else hi = mid;
  }
  g = __builtin_amdgcn_readfirstlane(lo);
  first = __builtin_amdgcn_readfirstlane(group_first[g]);
  size = __builtin_amdgcn_readfirstlane(group_first[g + 1]) - first;
  local = u - ((first >> SH) + g);
  return ((int64_t)local << SH) < size && first + size <= rmax;
}

__device__ __forceinline__ const float *uniform_ptr(const float *p) {
  const uint64_t v = (uint64_t)p;
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
  return (const float *)(((uint64_t)hi << 32) | lo);
}

// x[r] = float(obs[rows[r]]) for r < R: a grid for the host's bound of R, workgroups beyond R return
__global__ __launch_bounds__(128) void k_league_obs(const uint8_t *obs, const int64_t *rows, const int32_t *group_first, int ngroups, float *x) {
  const int64_t r = blockIdx.x;   // (< the host's bound: the grid)
  if (r >= group_first[ngroups]) return;
  obs_row_f32(obs, rows[r], x, r);
}

// One hidden layer of every group: workgroup b = (row unit b / tiles_n, column tile b % tiles_n).  A, C and M of the tile's
// mg::Args are the unit's (at most) 64 rows of the dense activation buffers, B and bias the layer of the group's network; the
// tile itself is k_gemm64n's (nothing is added to its K loop).
template <int NB>
__global__ __launch_bounds__(mg::THREADS) void k_league_layer(const brl_league_net *nets, const int32_t *group_first, int ngroups, int layer,
                                                              const float *a, int k, float *c, int hidden, int act, int tiles_n, int rmax) {
  __shared__ __attribute__((aligned(16))) float lds[mg::lds_floats<NB>()];
  const int b = (int)blockIdx.x, u = b / tiles_n, tn = b - u * tiles_n;
  int g, first, size, local;
  if (!unit_group<6>(group_first, ngroups, u, rmax, g, first, size, local)) return;
  const int64_t row0 = (int64_t)first + 64 * (int64_t)local;
  mg::Args G{};
  G.A = a + row0 * k; G.lda = k;
  G.B = uniform_ptr(nets[g].w[layer]); G.ldb = k;
  G.C = c + row0 * hidden; G.ldc = hidden;
  G.M = (size - 64 * local < 64) ? size - 64 * local : 64; G.N = hidden; G.K = k;
  G.act = act;
  G.bias = uniform_ptr(nets[g].b[layer]);
  mg::gemm_tile<true, true, mg::EPI_BIAS_ACT, NB>(G, lds, tn, tiles_n);
}

// The heads of every group: workgroup (x, y) = (unit x of 4 rows of one group, heads 13 y ..) — k_heads_rows with the group's weights
__global__ __launch_bounds__(256) void k_league_heads(const brl_league_net *nets, const int32_t *group_first, int ngroups, const float *h,
                                                      int hidden, const int64_t *rows, float *out, int64_t ldo, int rmax) {
  int g, first, size, local;
  if (!unit_group<2>(group_first, ngroups, (int)blockIdx.x, rmax, g, first, size, local)) return;
  const brl_league_net *net = nets + g;
  heads_rows_block(h + (int64_t)first * hidden, hidden, hidden, uniform_ptr(net->actor_w), uniform_ptr(net->actor_b),
                   uniform_ptr(net->critic_w), uniform_ptr(net->critic_b), rows + first, size, out, ldo, (int64_t)local * HR,
                   (int)blockIdx.y * HG);
}

}  // namespace

extern "C" int brl_league_route(int device, const uint8_t *terminated, const int32_t *current_player, int team, int64_t n,
                                const int32_t *order, const int32_t *group_of, int64_t nmatch, int64_t ngroups, int32_t *work,
                                int64_t *rows, int32_t *group_first, void *stream) {
  if (int e = route::check_args(terminated, current_player, team, n, order, group_of, nmatch, ngroups, work, rows, group_first)) return e;
  HIP_TRY(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  const unsigned blocks = (unsigned)((nmatch + RW - 1) / RW);
  hipLaunchKernelGGL(k_route_count, dim3(blocks), dim3(64 * RW), 0, s, terminated, current_player, team, n, order, nmatch, work);
  hipLaunchKernelGGL(k_route_scan, dim3(1), dim3(1024), 0, s, group_of, nmatch, (int)ngroups, work, group_first);
  hipLaunchKernelGGL(k_route_scatter, dim3(blocks), dim3(64 * RW), 0, s, terminated, current_player, team, n, order, nmatch, work, rows);
  HIP_TRY(hipGetLastError());
  return BRL_OK;
}

extern "C" int brl_league_forward(int device, const brl_league_net *nets, int64_t ngroups, int nlayers, int64_t hidden, int act,
                                  const uint8_t *obs, const int64_t *rows, const int32_t *group_first, int64_t rmax, float *scratch,
                                  int64_t scratch_len, float *out, int64_t ldo, void *stream) {
  NEED(nets && obs && rows && group_first && scratch && out, "NULL array");
  NEED(ngroups > 0 && ngroups < ((int64_t)1 << 24) && rmax > 0 && rmax < ((int64_t)1 << 24), "ngroups / rmax (1 .. 2^24)");
  NEED(nlayers >= 1 && nlayers <= 8, "nlayers (1..8)");
  NEED(hidden > 0 && hidden % 4 == 0 && hidden <= 1024, "hidden (a multiple of 4, <= 1024)");
  NEED(act == 0 || act == 1, "act (0 ReLU, 1 tanh)");
  NEED(ldo >= NHEADS, "ldo (>= 39)");
  NEED(scratch_len >= rmax * (BRL_OBS_SIZE + 2 * hidden) && (((uintptr_t)scratch) & 15) == 0, "scratch: rmax * (480 + 2 * hidden) floats, 16-byte aligned");
  // (the cast reads an observation row as 4-byte words, as brl_mlp_forward_rows does; the arrays the records of `nets` name live on
  //  the device and cannot be checked here)
  NEED((((uintptr_t)obs | (uintptr_t)group_first | (uintptr_t)out) & 3) == 0 && ((((uintptr_t)rows) | ((uintptr_t)nets)) & 7) == 0,
       "obs / group_first / out not 4-byte aligned (rows, nets: 8-byte)");
  HIP_TRY(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  const int G = (int)ngroups, H = (int)hidden;
  float *x = scratch, *actv[2] = {scratch + rmax * BRL_OBS_SIZE, scratch + rmax * BRL_OBS_SIZE + rmax * hidden};
  hipLaunchKernelGGL(k_league_obs, dim3((unsigned)rmax), dim3(128), 0, s, obs, rows, group_first, G, x);
  // brl_mlp_gemm's rule for the tile width: 64 x 32 tiles up to one 64 x 64 tile per CU (the results are the same either way)
  const int64_t units = rmax / 64 + ngroups;
  const int nb = (units * ((hidden + 63) / 64) <= 256) ? 1 : 2;
  const int tiles_n = (H + 32 * nb - 1) / (32 * nb);
  const float *cur = x;
  int k = BRL_OBS_SIZE;
  for (int l = 0; l < nlayers; l++) {
    float *dst = actv[l & 1];
    if (nb == 2) hipLaunchKernelGGL(k_league_layer<2>, dim3((unsigned)(units * tiles_n)), dim3(mg::THREADS), 0, s, nets, group_first, G, l, cur, k, dst, H, act, tiles_n, (int)rmax);
    else hipLaunchKernelGGL(k_league_layer<1>, dim3((unsigned)(units * tiles_n)), dim3(mg::THREADS), 0, s, nets, group_first, G, l, cur, k, dst, H, act, tiles_n, (int)rmax);
    cur = dst;
    k = H;
  }
  hipLaunchKernelGGL(k_league_heads, dim3((unsigned)(rmax / HR + ngroups), (NHEADS + HG - 1) / HG), dim3(256), 0, s, nets, group_first, G,
                     cur, H, rows, out, ldo, (int)rmax);
  HIP_TRY(hipGetLastError());
  return BRL_OK;
}
