// belief_table.hpp — the empty table of a sampled deal and a wave's stores of its table images: the one copy brl_belief.hip
// (k_belief_deal) and brl_belief_smc.hip (k_belief_propose) share.  include/brl_belief.h: the query's dealer, vulnerabilities and
// seating, no call made, table index 0xFFFFFFFF, all tricks zero — with the words and helpers k_init_explicit uses.
#pragma once
#include <stdint.h>

#include "bridge_device.hpp"

namespace brl {

constexpr int BELIEF_LANES = 64;        // samples of a one-wave block
constexpr int BELIEF_IMG_STRIDE = 144;  // a lane's 128-byte table image, padded: 16-byte aligned and not a multiple of the 256-byte bank cycle

// what a table needs of a query beside the hands
struct BeliefSeat {
  uint32_t seat, dealer, vns, vew, seating;
};

__device__ __forceinline__ BeliefSeat belief_seat(const uint4 qv) {
  return {qv.z & 3u, (qv.z >> 8) & 3u, (qv.z >> 16) & 1u, (qv.z >> 24) & 1u, qv.w & 0xFFu};
}

// the empty table of the deal (own at q.seat, h[0..3) at the next three seats) into a lane's image
__device__ __forceinline__ void belief_empty_table(uint8_t *img, const BeliefSeat &q, uint64_t own, const uint64_t h[3]) {
  uint64_t *img64 = reinterpret_cast<uint64_t *>(img);
#pragma unroll
  for (int w = 0; w < W_HAND; w++) img64[w] = 0ull;
  img64[W_HAND + q.seat] = own << 4;
  img64[W_HAND + ((q.seat + 1u) & 3u)] = h[0] << 4;
  img64[W_HAND + ((q.seat + 2u) & 3u)] = h[1] << 4;
  img64[W_HAND + ((q.seat + 3u) & 3u)] = h[2] << 4;
  Tbl t;
  t.sc = q.dealer | (q.vns << SC_VULNS) | (q.vew << SC_VULEW) | (q.seating << SC_SHUF);
  t.sch = 0;
  t.fd = 0;
  t.lut = 0xFFFFFFFFu;
  t.bctr = 0;
  t.r01 = 0;
  t.r23 = 0;
  pack_tricks(t, 0u, 0u, 0u, 0u);
  store_scalars(t, img);
}

// the wave's images (sample smp of the block at s_img + smp * BELIEF_IMG_STRIDE) to rows row0 .. row0 + count - 1 of tables and
// hands: 64 x 128 contiguous table bytes and 64 x 32 hand bytes, 16 per lane and store
__device__ __forceinline__ void belief_store_images(const uint8_t *s_img, int lane, int64_t row0, int64_t count, uint4 *tables, uint4 *hands) {
#pragma unroll
  for (int it = 0; it < TABLE_BYTES / 16; it++) {
    const int p = it * BELIEF_LANES + lane, smp = p >> 3, piece = p & 7;
    const uint4 v = *reinterpret_cast<const uint4 *>(s_img + smp * BELIEF_IMG_STRIDE + piece * 16);
    if (smp < count) tables[row0 * (TABLE_BYTES / 16) + p] = v;
  }
#pragma unroll
  for (int it = 0; it < 2; it++) {
    const int p = it * BELIEF_LANES + lane, smp = p >> 1, half = p & 1;
    const uint64_t *src = reinterpret_cast<const uint64_t *>(s_img + smp * BELIEF_IMG_STRIDE) + W_HAND + 2 * half;
    const uint64_t a = src[0] >> 4, b = src[1] >> 4;
    if (smp < count) hands[row0 * 2 + p] = make_uint4((uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32));
  }
}

}  // namespace brl
