// route_common.hpp — what the routes of a batch of duplicate matches share (brl_league.hip: by the acting team's network;
// brl_crossplay.hip: by the acting player's): which boards act, and the clamp that keeps a bad host table from becoming an address.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

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

}  // namespace route
