// brl_crossplay.hip — translation unit of libbrl_hip.so: the route of cross-play (include/brl_crossplay.h).  A batch of duplicate
// matches in which every PLAYER has a network of its own: per iteration the boards whose team acts are sorted by the network of
// the player to call (brl_xplay_route); the grouped forward is brl_league_forward and the step brl_eval_step_team, both unchanged.
// The unit of the order is a slot = (match, half), half = current_player & 1; count and scatter run a wave per MATCH, read the
// batch once per 64 boards and take one ballot per half.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/brl_crossplay.h"
#include "abi_common.hpp"
#include "route_common.hpp"

namespace {

constexpr int RW = 4;   // waves (= matches) per workgroup of the count and scatter kernels

// the half (0 / 1) in which board b acts for `team`, -1 when it does not act: ONE read of terminated / current_player
__device__ __forceinline__ int acting_half(const uint8_t *terminated, const int32_t *current_player, int64_t b, int team) {
  const int32_t cp = current_player[b];
  return route::acts(terminated[b], cp, team) ? (cp & 1) : -1;
}

// work[2 m + h] = acting boards of match m in half h: one wave per match, 64 boards per pair of ballots
__global__ __launch_bounds__(64 * RW) void k_xroute_count(const uint8_t *terminated, const int32_t *current_player, int team, int64_t n,
                                                          int64_t nmatch, int32_t *work) {
  const int lane = (int)threadIdx.x & 63;
  const int64_t m = (int64_t)blockIdx.x * RW + (threadIdx.x >> 6);
  if (m >= nmatch) return;
  const int64_t base = m * n;
  int c0 = 0, c1 = 0;
  for (int64_t i0 = 0; i0 < n; i0 += 64) {
    const int64_t i = i0 + lane;
    const int h = i < n ? acting_half(terminated, current_player, base + i, team) : -1;
    c0 += __popcll(__ballot(h == 0));
    c1 += __popcll(__ballot(h == 1));
  }
  if (lane == 0) {
    work[2 * m] = c0;
    work[2 * m + 1] = c1;
  }
}

// work[nslots + s] = the first row of slot s = order[k], group_first = the groups' first rows and the total: route::scan along the
// order, on counts that k_xroute_count wrote by slot
__global__ __launch_bounds__(1024) void k_xroute_scan(const int32_t *order, const int32_t *group_of, int64_t nslots, int ngroups,
                                                      int32_t *work, int32_t *group_first) {
  route::scan<true>(order, group_of, nslots, ngroups, work, group_first);
}

// rows[first row of slot 2 m + h ..] = the boards of match m that act in half h, ascending: both halves in one pass of the match
// (nboards = nmatch * n: a place outside rows is not written — it cannot arise when `order` is a permutation)
__global__ __launch_bounds__(64 * RW) void k_xroute_scatter(const uint8_t *terminated, const int32_t *current_player, int team, int64_t n,
                                                            int64_t nmatch, const int32_t *work, int64_t *rows) {
  const int lane = (int)threadIdx.x & 63;
  const int64_t m = (int64_t)blockIdx.x * RW + (threadIdx.x >> 6);
  if (m >= nmatch) return;
  const int64_t base = m * n, nboards = nmatch * n;
  int64_t pos0 = work[2 * nmatch + 2 * m], pos1 = work[2 * nmatch + 2 * m + 1];
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int64_t i0 = 0; i0 < n; i0 += 64) {
    const int64_t i = i0 + lane;
    const int h = i < n ? acting_half(terminated, current_player, base + i, team) : -1;
    const unsigned long long bal0 = __ballot(h == 0), bal1 = __ballot(h == 1);
    if (h >= 0) {
      const int64_t dst = h ? pos1 + __popcll(bal1 & below) : pos0 + __popcll(bal0 & below);
      if (dst >= 0 && dst < nboards) rows[dst] = base + i;
    }
    pos0 += __popcll(bal0);
    pos1 += __popcll(bal1);
  }
}

}  // namespace

extern "C" int brl_xplay_route(int device, const uint8_t *terminated, const int32_t *current_player, int team, int64_t n,
                               const int32_t *order, const int32_t *group_of, int64_t nmatch, int64_t ngroups, int32_t *work,
                               int64_t *rows, int32_t *group_first, void *stream) {
  if (int e = route::check_args(terminated, current_player, team, n, order, group_of, nmatch, ngroups, work, rows, group_first)) return e;
  HIP_TRY(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  const unsigned blocks = (unsigned)((nmatch + RW - 1) / RW);
  hipLaunchKernelGGL(k_xroute_count, dim3(blocks), dim3(64 * RW), 0, s, terminated, current_player, team, n, nmatch, work);
  hipLaunchKernelGGL(k_xroute_scan, dim3(1), dim3(1024), 0, s, order, group_of, 2 * nmatch, (int)ngroups, work, group_first);
  hipLaunchKernelGGL(k_xroute_scatter, dim3(blocks), dim3(64 * RW), 0, s, terminated, current_player, team, n, nmatch, work, rows);
  HIP_TRY(hipGetLastError());
  return BRL_OK;
}
