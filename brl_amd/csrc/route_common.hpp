// route_common.hpp — what the routes of a batch of duplicate matches share (brl_league.hip: by the acting team's network;
// brl_crossplay.hip: by the acting player's): which boards act, the clamp that keeps a bad host table from becoming an address, the
// scan between the count and scatter kernels, and the exports' argument checks.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "abi_common.hpp"

namespace route {

// a board acts for `team` when it is not finished and its player to call is one of the team's two (outputs of brl_eval_step_team)
__device__ __forceinline__ bool acts(uint8_t terminated, int32_t current_player, int team) {
  return terminated == 0 && (current_player >> 1) == team;
}

__device__ __forceinline__ bool board_acts(const uint8_t *terminated, const int32_t *current_player, int64_t b, int team) {
  return acts(terminated[b], current_player[b], team);
}

// v clamped into 0 .. count - 1 (an entry of `order` / `group_of` out of range can make the result wrong, never an address)
__device__ __forceinline__ int64_t clamp_index(int64_t v, int64_t count) {
  return v < 0 ? 0 : (v < count ? v : count - 1);
}

// The scan of a route, for the ONE workgroup of 1024 threads that runs it.  Position k of the visiting order owns the slot
// s(k) = k (VIA_ORDER false: brl_league_route, whose counts are already in the order) or order[k] (VIA_ORDER true:
// brl_xplay_route), whose count is work[s(k)].  Writes work[nslots + s(k)] = the first row of position k (exclusive scan of the
// counts along the order), group_first[g] = the first row of group g's first position (of the next group's for a group without
// positions) and group_first[ngroups] = the total.  A thread owns a run of positions, the runs' offsets come from a scan in LDS;
// every group_first entry is written by exactly one thread (the one that owns the position where the group changes).
template <bool VIA_ORDER>
__device__ __forceinline__ void scan(const int32_t *order, const int32_t *group_of, int64_t nslots, int ngroups, int32_t *work,
                                     int32_t *group_first) {
  __shared__ int part[1024];
  const int tid = (int)threadIdx.x;
  const int64_t per = (nslots + 1023) / 1024, a0 = (int64_t)tid * per, a = a0 < nslots ? a0 : nslots, b = a + per < nslots ? a + per : nslots;
  auto slot = [&](int64_t k) { return VIA_ORDER ? clamp_index(order[k], nslots) : k; };
  auto group = [&](int64_t k) { return (int)clamp_index(group_of[k], ngroups); };
  int c = 0;
  for (int64_t k = a; k < b; k++) c += work[slot(k)];
  part[tid] = c;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {   // inclusive scan
    const int v = (tid >= off) ? part[tid - off] : 0;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  int pos = part[tid] - c;
  for (int64_t k = a; k < b; k++) {
    const int64_t s = slot(k);
    work[nslots + s] = pos;
    const int g = group(k);
    for (int gg = (k == 0) ? 0 : group(k - 1) + 1; gg <= g; gg++) group_first[gg] = pos;
    pos += work[s];
  }
  if (tid == 1023)
    for (int gg = group(nslots - 1) + 1; gg <= ngroups; gg++) group_first[gg] = part[1023];
}

// the argument checks of both route exports (they take the same arguments): BRL_OK, or the error recorded for brl_last_error()
inline int check_args(const uint8_t *terminated, const int32_t *current_player, int team, int64_t n, const int32_t *order,
                      const int32_t *group_of, int64_t nmatch, int64_t ngroups, const int32_t *work, const int64_t *rows,
                      const int32_t *group_first) {
  NEED(terminated && current_player && order && group_of && work && rows && group_first, "NULL array");
  NEED((((uintptr_t)current_player | (uintptr_t)order | (uintptr_t)group_of | (uintptr_t)work | (uintptr_t)group_first) & 3) == 0 &&
           (((uintptr_t)rows) & 7) == 0, "int32 arrays not 4-byte aligned, rows not 8-byte");
  NEED(team == 0 || team == 1, "team (0 / 1)");
  NEED(n > 0 && nmatch > 0 && ngroups > 0, "n / nmatch / ngroups");
  NEED(nmatch * n < ((int64_t)1 << 31) && nmatch < ((int64_t)1 << 24) && ngroups < ((int64_t)1 << 24), "nmatch * n below 2^31, nmatch and ngroups below 2^24");
  return BRL_OK;
}

}  // namespace route
