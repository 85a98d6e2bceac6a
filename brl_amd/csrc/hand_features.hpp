// hand_features.hpp — the features of one hand word (bit = rank * 4 + suit, suits C,D,H,S), as include/brl_book.h defines them:
// the one copy the bidding-system book (brl_book.hip) and the hand beliefs (brl_belief.hip) share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace brl {

// feature word: bits 0..5 HCP, bits 6..21 the four suit lengths C,D,H,S (four bits each), bit 22 balanced
constexpr int F_LEN = 6, F_BAL = 22;

__device__ __forceinline__ uint32_t hand_features(uint64_t w) {
  const uint32_t top = (uint32_t)(w >> 36);   // ranks 9..12: J,Q,K,A, a nibble each
  const uint32_t hcp = __popc(top & 0xFu) + 2u * __popc(top & 0xF0u) + 3u * __popc(top & 0xF00u) + 4u * __popc(top & 0xF000u);
  uint32_t f = hcp;
  uint64_t shape = 0;   // how many suits have each length, four bits per length
#pragma unroll
  for (int s = 0; s < 4; s++) {
    const uint32_t len = (uint32_t)__popcll((w >> s) & 0x1111111111111ull);
    f |= len << (F_LEN + 4 * s);
    shape += 1ull << (4 * len);
  }
  const bool bal = shape == ((1ull << 16) | (3ull << 12)) || shape == ((2ull << 16) | (1ull << 12) | (1ull << 8)) ||
                   shape == ((1ull << 20) | (2ull << 12) | (1ull << 8));   // 4333, 4432, 5332
  return f | ((uint32_t)bal << F_BAL);
}

}  // namespace brl
