// brl_review.hip — translation unit of libbrl_hip.so: the call review (include/brl_review.h, which holds the definition).
// k_review_expand turns one table's board records into branch tables: a WAVE takes one record — the direction opposite to
// k_board_records' walk —, one of its lanes walks the record's calls from a record image in LDS and keeps the prefix table in a
// 128-byte table image, and at every call index the wave derives the prefix's 38 children with table_step and writes the decision's
// 38 x 128 contiguous bytes as whole 16-byte pieces.  (A lane per record, 64 records per wave, was the first form: a 1000-board
// table is then 16 waves that each write 64 records' decisions one after the other — 1.09 ms for 33.7 MB)
// k_review_reduce reads the tables back once the evaluators' loop has played them out: a wave per decision, a lane per slot,
// terminal_reward and imp.hpp's conversion for the value, wave reductions for the summary.  No atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/brl_review.h"
#include "abi_common.hpp"
#include "bridge_device.hpp"
#include "imp.hpp"

namespace {

using namespace brl;

constexpr int REC = (int)sizeof(brl_board_record);   // 368
constexpr int REC_CHUNKS = REC / 16;                 // 23
constexpr int CALLS_OFF = 48;
constexpr int ACTIONS = BRL_REVIEW_ACTIONS;
constexpr int CHILD_PIECES = ACTIONS * (TABLE_BYTES / 16);   // 304 16-byte pieces per decision
constexpr int EXPAND_WAVES = 4;                              // records per 256-thread block of k_review_expand, one per wave
static_assert(REC == 368 && offsetof(brl_board_record, calls) == CALLS_OFF && offsetof(brl_board_record, hands) == 16, "record layout");
static_assert(sizeof(brl_review_decision) == 16 && sizeof(brl_review_summary) == 8, "review layouts");

// the scalar words of a table as they lie in memory (load_scalars' / store_scalars' layout), as values: no field is selected by a
// run-time index
struct Words {
  uint64_t w11, w12, w13, w14, w15;
};

__device__ __forceinline__ Words scalar_words(const Tbl &t) {
  Words w;
  w.w11 = (uint64_t)t.sc | ((uint64_t)t.sch << 32);
  w.w12 = (uint64_t)t.fd | ((uint64_t)t.t2 << 32);
  w.w13 = (uint64_t)t.t0 | ((uint64_t)t.t1 << 32);
  w.w14 = (uint64_t)t.lut | ((uint64_t)t.bctr << 32);
  w.w15 = (uint64_t)t.r01 | ((uint64_t)t.r23 << 32);
  return w;
}

__global__ __launch_bounds__(256) void k_review_expand(const uint8_t *records, const uint8_t *dda, int64_t n, int depth, const int64_t *first,
                                                       int64_t d0, int64_t d1, brl_review_decision *decisions, uint64_t *tables) {
  __shared__ __attribute__((aligned(16))) uint8_t rec_img[EXPAND_WAVES * REC];
  __shared__ __attribute__((aligned(16))) uint8_t tab_img[EXPAND_WAVES * TABLE_BYTES];
  const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
  const int64_t rec = (int64_t)blockIdx.x * EXPAND_WAVES + wave;
  // (everything below is per wave: the waves of a block share nothing and never meet at a barrier)
  if (rec >= n) return;
  const int64_t base = first[rec], room = first[rec + 1] - base;   // the slots the caller gave this record
  if (room <= 0 || base >= d1 || base + room <= d0) return;        // none of them in [d0, d1)

  // the record's 23 16-byte pieces into this wave's image
  uint8_t *my = rec_img + wave * REC;
  if (lane < REC_CHUNKS) reinterpret_cast<uint4 *>(my)[lane] = reinterpret_cast<const uint4 *>(records + rec * REC)[lane];
  wave_lds_fence();
  const uint32_t h0 = reinterpret_cast<const uint32_t *>(my)[0], h1 = reinterpret_cast<const uint32_t *>(my)[1];
  const uint32_t h2 = reinterpret_cast<const uint32_t *>(my)[2];
  const int n_calls = (int)(h0 & 0xFFFFu), dealer = (int)((h0 >> 16) & 3u);
  const uint32_t vns = (h0 >> 24) & 1u, vew = h1 & 1u, flags = (h1 >> 8) & 0xFFu, seating = h2 >> 24;
  const bool reviewable = (flags & BRL_BOARD_OK) != 0 && (flags & BRL_BOARD_ILLEGAL) == 0;
  int cnt = reviewable ? (n_calls < depth ? n_calls : depth) : 0;
  cnt = cnt < BRL_BOARD_MAX_CALLS ? cnt : BRL_BOARD_MAX_CALLS;
  cnt = (int64_t)cnt < room ? cnt : (int)room;

  // the empty table of the record's deal in this wave's table image
  uint8_t *pre = tab_img + wave * TABLE_BYTES;
  uint64_t *pre64 = reinterpret_cast<uint64_t *>(pre);
  if (lane == 0) {
    Tbl t;
    t.sc = (uint32_t)dealer | (vns << SC_VULNS) | (vew << SC_VULEW) | (seating << SC_SHUF);
    t.sch = 0;
    t.fd = 0;
    t.lut = 0xFFFFFFFFu;
    t.bctr = 0;
    t.r01 = 0;
    t.r23 = 0;
    uint32_t v[4];
    const uint8_t *row = dda + rec * 20;
#pragma unroll
    for (int seat = 0; seat < 4; seat++) {
      v[seat] = 0;
#pragma unroll
      for (int den = 0; den < 5; den++) v[seat] |= ((uint32_t)row[seat * 5 + den] & 15u) << (4 * (4 - den));
    }
    pack_tricks(t, v[0], v[1], v[2], v[3]);
#pragma unroll
    for (int k = 0; k < W_HAND; k++) pre64[k] = 0ull;
#pragma unroll
    for (int s = 0; s < 4; s++) pre64[W_HAND + s] = reinterpret_cast<const uint64_t *>(my + 16)[s] << 4;
    store_scalars(t, pre);
  }
  wave_lds_fence();

  for (int t = 0; t < cnt; t++) {
    const int64_t d = base + t;
    if (d >= d1) break;
    const int call = (int)my[CALLS_OFF + t];
    const int played = call < ACTIONS ? call : 0;
    if (d >= d0) {   // ---- the 38 children of this prefix: 304 16-byte pieces, contiguous in memory
      const int64_t dj = d - d0;
      if (lane == 0) {
        const uint32_t seat = ((uint32_t)dealer + (uint32_t)t) & 3u;
        const uint32_t team = ((seating >> (2u * seat)) & 3u) >> 1;
        *reinterpret_cast<uint4 *>(decisions + dj) = make_uint4((uint32_t)rec, (uint32_t)t | (seat << 16) | (team << 24), (uint32_t)played, 0u);
      }
      uint4 *dst = reinterpret_cast<uint4 *>(tables + dj * (ACTIONS * 16));
#pragma unroll
      for (int it = 0; it < (CHILD_PIECES + 63) / 64; it++) {
        const int p = it * 64 + lane;
        const int a = p >> 3, q = p & 7;       // piece q of child a: words 2 q and 2 q + 1
        Tbl c;
        load_scalars(c, pre);
        const int hb = table_step(c, a < ACTIONS ? a : 0);
        const Words w = scalar_words(c);
        const int qq = q < 5 ? q : 4;
        uint64_t lo = pre64[2 * qq], hi = pre64[2 * qq + 1];
        lo = q == 5 ? pre64[10] : (q == 6 ? w.w12 : (q == 7 ? w.w14 : lo));
        hi = q == 5 ? w.w11 : (q == 6 ? w.w13 : (q == 7 ? w.w15 : hi));
        // the call's history bit, as the step kernels OR it into their image (bits 4 .. 427: words 0 .. 6)
        lo |= (hb >= 0 && (hb >> 6) == 2 * q) ? (1ull << (hb & 63)) : 0ull;
        hi |= (hb >= 0 && (hb >> 6) == 2 * q + 1) ? (1ull << (hb & 63)) : 0ull;
        if (p < CHILD_PIECES) dst[p] = make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
      }
    }
    wave_lds_fence();
    if (lane == 0) {   // ---- the walk: the prefix of t + 1
      Tbl c;
      load_scalars(c, pre);
      const int hb = table_step(c, played);
      if (hb >= 0 && hb < 64 * W_HAND) pre64[hb >> 6] |= 1ull << (hb & 63);
      store_scalars(c, pre);
    }
    wave_lds_fence();
  }
}

__global__ __launch_bounds__(256) void k_review_reduce(const uint64_t *tables, const brl_review_decision *decisions, int64_t nd,
                                                       const brl_board_record *other, int64_t n, int8_t *values,
                                                       brl_review_summary *summary) {
  const int lane = (int)(threadIdx.x & 63u);
  const int64_t d = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (d >= nd) return;   // (wave-uniform)
  const uint4 dec = *reinterpret_cast<const uint4 *>(decisions + d);
  const int64_t board = (int64_t)(int32_t)dec.x;
  const int seat = (int)((dec.y >> 16) & 3u), played = (int)(dec.z & 0xFFu);
  const int other_score = (board >= 0 && board < n) ? other[board].score_ns : 0;
  const bool slot = lane < ACTIONS;
  Tbl t;
  load_scalars(t, reinterpret_cast<const uint8_t *>(tables + (d * ACTIONS + (slot ? lane : 0)) * 16));
  const bool legal = slot && bits(t.sc, SC_TERM, 1) && !bits(t.sc, SC_ILLEGAL, 1);
  Tbl u = t;
  terminal_reward(u);   // rewards by player id; North's player holds North-South's score (0 for a pass-out)
  const int score_ns = reward_of(u, player_at(u, 0));
  // the reviewed table's North-South pair sits East-West at the other table: its score there is -score_ns
  const int imp_ns = (int)imp_vector((float)score_ns, (float)(-other_score)).x;
  const int value = legal ? ((seat & 1) ? -imp_ns : imp_ns) : BRL_REVIEW_VOID;
  if (slot) values[d * ACTIONS + lane] = (int8_t)value;
  int best_imp = value;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) best_imp = max(best_imp, __shfl_xor(best_imp, off, 64));
  const uint64_t legal_mask = __ballot(legal), at_best = __ballot(legal && value == best_imp);
  const int p = played < ACTIONS ? played : 0;
  const int played_imp = __shfl(value, p, 64);
  const int best = (((at_best >> p) & 1ull) || at_best == 0ull) ? played : __ffsll((unsigned long long)at_best) - 1;
  if (lane == 0) {
    const uint32_t loss = (uint32_t)(best_imp - played_imp) & 0xFFu;
    const uint32_t w0 = (uint32_t)played | ((uint32_t)__popcll(legal_mask) << 8) | (((uint32_t)played_imp & 0xFFu) << 16) |
                        (((uint32_t)best_imp & 0xFFu) << 24);
    *reinterpret_cast<uint2 *>(summary + d) = make_uint2(w0, (uint32_t)best | (loss << 8));
  }
}

}  // namespace

extern "C" int brl_review_expand(int device, const brl_board_record *records, const uint8_t *dda, int64_t n, int32_t depth,
                                 const int64_t *first, int64_t d0, int64_t d1, brl_review_decision *decisions, uint64_t *tables,
                                 void *stream) {
  NEED(records && dda && first && decisions && tables, "NULL array");
  NEED(n > 0 && n < ((int64_t)1 << 31), "n (1 .. 2^31)");
  NEED(depth >= 1, "depth (>= 1)");
  NEED(d0 >= 0 && d1 > d0 && (d1 - d0) * BRL_REVIEW_ACTIONS < ((int64_t)1 << 31), "0 <= d0 < d1, (d1 - d0) * 38 below 2^31");
  NEED(((((uintptr_t)records) | ((uintptr_t)decisions) | ((uintptr_t)tables)) & 15) == 0 && (((uintptr_t)first) & 7) == 0,
       "records / decisions / tables 16-byte aligned, first 8-byte aligned");
  HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(k_review_expand, dim3((unsigned)((n + EXPAND_WAVES - 1) / EXPAND_WAVES)), dim3(64 * EXPAND_WAVES), 0, (hipStream_t)stream,
                     reinterpret_cast<const uint8_t *>(records), dda, n, (int)depth, first, d0, d1, decisions, tables);
  HIP_TRY(hipGetLastError());
  return BRL_OK;
}

extern "C" int brl_review_reduce(int device, const uint64_t *tables, const brl_review_decision *decisions, int64_t nd,
                                 const brl_board_record *other, int64_t n, int8_t *values, brl_review_summary *summary, void *stream) {
  NEED(tables && decisions && other && values && summary, "NULL array");
  NEED(nd > 0 && nd * BRL_REVIEW_ACTIONS < ((int64_t)1 << 31), "nd (1 .., nd * 38 below 2^31)");
  NEED(n > 0 && n < ((int64_t)1 << 31), "n (1 .. 2^31)");
  NEED(((((uintptr_t)tables) | ((uintptr_t)decisions) | ((uintptr_t)other)) & 15) == 0 && (((uintptr_t)summary) & 7) == 0,
       "tables / decisions / other 16-byte aligned, summary 8-byte aligned");
  HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(k_review_reduce, dim3((unsigned)((nd + 3) / 4)), dim3(256), 0, (hipStream_t)stream, tables, decisions, nd, other, n,
                     values, summary);
  HIP_TRY(hipGetLastError());
  return BRL_OK;
}
