// brl_compare.hip — translation unit of libbrl_hip.so: the system diff (include/brl_compare.h, which holds the definition).
// k_compare_tables builds the empty tables of the listed records' deals with the beliefs' builder (belief_table.hpp).
// k_compare_rows writes one call index's decision records: eight lanes per row, categorical<8> (policy_common.hpp) in mode form
// per network for the call and the played call's log-probability as k_belief_logp forms it, then the float64 divergences on
// the same lane layout (five actions per lane, the eight slot sums added in ascending slot order; each network's p_a and L_a by
// policy_dist.hpp, which the position queries share).
// k_compare_reduce sums a key's run of sorted decisions into its entry: a workgroup per entry, a thread per block of 64
// decisions, the block sums added in ascending order by one thread per sum; integers through LDS atomics.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/brl_compare.h"
#include "abi_common.hpp"
#include "belief_table.hpp"
#include "bridge_device.hpp"
#include "hand_features.hpp"
#include "policy_common.hpp"
#include "policy_dist.hpp"

namespace {

using namespace brl;

constexpr int REC_CHUNKS = (int)sizeof(brl_board_record) / 16;   // 23
constexpr int DEC_CHUNKS = BRL_COMPARE_DECISION_BYTES / 16;      // 4
constexpr int ENTRY_CHUNKS = BRL_COMPARE_ENTRY_BYTES / 16;       // 35
constexpr int ACTIONS = BRL_COMPARE_ACTIONS;
constexpr int F_TEAM = 23;
constexpr uint64_t DECK = (1ull << 52) - 1;
static_assert(sizeof(brl_board_record) == 368 && offsetof(brl_board_record, hands) == 16 && offsetof(brl_board_record, calls) == 48,
              "record layout");
static_assert(sizeof(brl_compare_decision) == BRL_COMPARE_DECISION_BYTES && offsetof(brl_compare_decision, feats) == 16 &&
                  offsetof(brl_compare_decision, played) == 20 && offsetof(brl_compare_decision, logp_x) == 24 &&
                  offsetof(brl_compare_decision, kl_xy) == 32 && offsetof(brl_compare_decision, js) == 48,
              "decision layout");
static_assert(sizeof(brl_compare_entry) == BRL_COMPARE_ENTRY_BYTES && BRL_COMPARE_ENTRY_BYTES % 16 == 0 &&
                  offsetof(brl_compare_entry, calls_x) == 32 && offsetof(brl_compare_entry, hcp_sum) == 488 &&
                  offsetof(brl_compare_entry, kl_xy_sum) == 504 && offsetof(brl_compare_entry, js_max) == 544,
              "entry layout");
static_assert(ACTIONS == BRL_NUM_ACTIONS && BRL_BOOK_MAX_DEPTH == 10, "constants");

// ---- the empty tables -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BELIEF_LANES) void k_compare_tables(const uint4 *records, int64_t n, const int64_t *rows, int64_t m, uint4 *tables,
                                                                 uint4 *hands) {
  __shared__ __attribute__((aligned(16))) uint8_t s_img[BELIEF_LANES * BELIEF_IMG_STRIDE];
  const int lane = (int)threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * BELIEF_LANES;
  const int64_t row = row0 + lane < m ? row0 + lane : m - 1;   // (an idle lane repeats the last row and stores nothing)
  int64_t rec = rows[row];
  rec = rec < 0 ? 0 : (rec >= n ? n - 1 : rec);
  const uint4 hd = records[rec * REC_CHUNKS], ne = records[rec * REC_CHUNKS + 1], sw = records[rec * REC_CHUNKS + 2];
  const BeliefSeat qs = {0u, (hd.x >> 16) & 3u, (hd.x >> 24) & 1u, hd.y & 1u, hd.z >> 24};
  const uint64_t own = ((uint64_t)ne.x | ((uint64_t)ne.y << 32)) & DECK;
  const uint64_t h[3] = {((uint64_t)ne.z | ((uint64_t)ne.w << 32)) & DECK, ((uint64_t)sw.x | ((uint64_t)sw.y << 32)) & DECK,
                         ((uint64_t)sw.z | ((uint64_t)sw.w << 32)) & DECK};
  belief_empty_table(s_img + lane * BELIEF_IMG_STRIDE, qs, own, h);
  wave_lds_fence();
  belief_store_images(s_img, lane, row0, m - row0, tables, hands);
}

// ---- one call index's decisions ---------------------------------------------------------------------------------------------------
// KL(first || second) over this lane's actions: p * (L - Lo), +0.0 where p == 0
__device__ __forceinline__ double kl_own(const double p[NI], const double L[NI], const double Lo[NI]) {
#pragma clang fp contract(off)
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < NI; i++) {
    const double t = p[i] * (L[i] - Lo[i]);
    s += (p[i] > 0.0) ? t : 0.0;
  }
  return s;
}

// KL(first || M) over this lane's actions: p * -g(Lo - L), g(d) = log(0.5 (1 + exp d)) in brl_compare.h's two forms; +0.0 where p == 0
__device__ __forceinline__ double klm_own(const double p[NI], const double L[NI], const double Lo[NI]) {
#pragma clang fp contract(off)
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < NI; i++) {
    const double d = Lo[i] - L[i];
    const double ad = fabs(d), sh = sinh(0.25 * ad);
    const double g = (ad <= 1.0) ? 0.5 * d + log1p(2.0 * (sh * sh)) : log(0.5 * (1.0 + exp(-ad))) + fmax(d, 0.0);
    const double t = p[i] * (-g);
    s += (p[i] > 0.0) ? t : 0.0;
  }
  return s;
}

__global__ __launch_bounds__(256) void k_compare_rows(const uint4 *records, int64_t n, const int64_t *rows, int64_t m, int t, int depth,
                                                      const float *lx, int64_t ldx, const float *ly, int64_t ldy, const uint64_t *legal,
                                                      uint4 *decisions) {
  const int lane = (int)(threadIdx.x & 63u), tl = lane % ROW_LANES, slot = lane / ROW_LANES;
  const int64_t j = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * ROW_LANES + tl;
  const bool in = j < m;
  int64_t rec = in ? rows[j] : -1;
  const bool listed = in && rec >= 0 && rec < n;
  rec = listed ? rec : 0;
  // the record's first 64 bytes: slot k (and k + 4) loads piece k & 3 — the header, hands N,E, hands S,W, calls[0..15]
  const uint4 v = records[rec * REC_CHUNKS + (slot & 3)];
  const uint32_t w0 = __shfl(v.x, tl, 64), w1 = __shfl(v.y, tl, 64), w2 = __shfl(v.z, tl, 64);
  const int n_calls = (int)(w0 & 0xFFFFu), dealer = (int)((w0 >> 16) & 3u);
  const uint32_t flags_rec = (w1 >> 8) & 0xFFu, seating = w2 >> 24;
  const int s = (dealer + t) & 3, src = tl + ROW_LANES * (1 + (s >> 1));
  const uint32_t hx = __shfl(v.x, src, 64), hy = __shfl(v.y, src, 64), hz = __shfl(v.z, src, 64), hw = __shfl(v.w, src, 64);
  const uint64_t hand = ((s & 1) ? ((uint64_t)hw << 32 | hz) : ((uint64_t)hy << 32 | hx)) & DECK;
  const uint32_t c[3] = {__shfl(v.x, tl + 3 * ROW_LANES, 64), __shfl(v.y, tl + 3 * ROW_LANES, 64), __shfl(v.z, tl + 3 * ROW_LANES, 64)};
  uint64_t full = 0;   // the book's key of calls[0..9]; the fill byte 0xFF gives a zero field
#pragma unroll
  for (int k = 0; k < BRL_BOOK_MAX_DEPTH; k++) full |= (uint64_t)(((c[k >> 2] >> (8 * (k & 3))) + 1u) & 63u) << (58 - 6 * k);
  const int played = (int)((c[t >> 2] >> (8 * (t & 3))) & 0xFFu);
  const bool ok = (flags_rec & BRL_BOARD_OK) != 0 && (flags_rec & BRL_BOARD_ILLEGAL) == 0;
  const bool valid = listed && ok && t < (n_calls < depth ? n_calls : depth) && played < ACTIONS;
  const uint64_t key = (t ? (full & (~0ull << (64 - 6 * t))) : 0ull) | (uint64_t)(t + 1);
  const uint32_t team = ((seating >> (2 * s)) & 3u) >> 1;
  const uint32_t feats = hand_features(hand) | (team << F_TEAM);
  const uint64_t cand = valid ? (legal[j] & ALL_ACTIONS) : 1ull;

  // each network's masked arg-max and, in the form k_belief_logp uses, the played call's log-probability
  const int64_t ox = valid ? j * ldx : 0, oy = valid ? j * ldy : 0;
  float mode_x, mode_y;
  const int cx = categorical<ROW_LANES>(lx, ox, 0, valid, cand, 1, 0u, lane, mode_x);
  const int cy = categorical<ROW_LANES>(ly, oy, 0, valid, cand, 1, 0u, lane, mode_y);
  const int a = valid ? played : 0;
  const float logp_x = (lx[ox + a] - lx[ox + cx]) + mode_x;   // == (la - mx) - logf(total)
  const float logp_y = (ly[oy + a] - ly[oy + cy]) + mode_y;

  // the divergences
  double px[NI], Lx[NI], py[NI], Ly[NI];
  bool bad_x, bad_y;
  net_dist(lx + ox, cand, cx, slot, tl, px, Lx, bad_x);
  net_dist(ly + oy, cand, cy, slot, tl, py, Ly, bad_y);
  double kl_xy = slot_sum(kl_own(px, Lx, Ly), tl), kl_yx = slot_sum(kl_own(py, Ly, Lx), tl);
  const double jx = slot_sum(klm_own(px, Lx, Ly), tl), jy = slot_sum(klm_own(py, Ly, Lx), tl);
  double js;
  {
#pragma clang fp contract(off)
    js = 0.5 * (jx + jy);
  }
  const bool nonfinite = bad_x || bad_y;
  if (nonfinite) kl_xy = kl_yx = js = (double)NAN;

  const uint32_t flags = BRL_COMPARE_VALID | (cx == cy ? BRL_COMPARE_AGREE : 0) | (cx == a ? BRL_COMPARE_X_PLAYED : 0) |
                         (cy == a ? BRL_COMPARE_Y_PLAYED : 0) | (nonfinite ? BRL_COMPARE_NONFINITE : 0);
  const uint64_t kxy = (uint64_t)__double_as_longlong(kl_xy), kyx = (uint64_t)__double_as_longlong(kl_yx),
                 jsb = (uint64_t)__double_as_longlong(js);
  uint4 piece;
  if (slot == 0)
    piece = make_uint4((uint32_t)key, (uint32_t)(key >> 32), (uint32_t)cand, (uint32_t)(cand >> 32));
  else if (slot == 1)
    piece = make_uint4(feats, (uint32_t)a | ((uint32_t)cx << 8) | ((uint32_t)cy << 16) | (flags << 24), __float_as_uint(logp_x),
                       __float_as_uint(logp_y));
  else if (slot == 2)
    piece = make_uint4((uint32_t)kxy, (uint32_t)(kxy >> 32), (uint32_t)kyx, (uint32_t)(kyx >> 32));
  else
    piece = make_uint4((uint32_t)jsb, (uint32_t)(jsb >> 32), 0u, 0u);
  if (!valid) piece = make_uint4(0u, 0u, 0u, 0u);
  if (listed && slot < DEC_CHUNKS) decisions[(rec * depth + t) * DEC_CHUNKS + slot] = piece;
}

// ---- the entries ------------------------------------------------------------------------------------------------------------------
constexpr int RT = 256, BLOCK = BRL_COMPARE_BLOCK, SUMS = 5;
constexpr int C_N = 0, C_AGREE = 1, C_XP = 2, C_YP = 3, C_NONFINITE = 4, C_HIST = 6, COUNTERS = C_HIST + 3 * ACTIONS;   // the words behind the key
static_assert(offsetof(brl_compare_entry, n) == 8 + 4 * C_N && offsetof(brl_compare_entry, nonfinite) == 8 + 4 * C_NONFINITE &&
                  offsetof(brl_compare_entry, calls_x) == 8 + 4 * C_HIST && offsetof(brl_compare_entry, hcp_sum) == 8 + 4 * COUNTERS,
              "counter words");

__global__ __launch_bounds__(RT) void k_compare_reduce(const uint4 *sorted, int64_t S, const int64_t *start, uint8_t *entries,
                                                       unsigned long long *confusion) {
  __shared__ double s_part[SUMS][RT];
  __shared__ double s_max[RT];
  __shared__ uint32_t s_conf[ACTIONS * ACTIONS];
  __shared__ __attribute__((aligned(16))) uint8_t s_entry[BRL_COMPARE_ENTRY_BYTES];
  const int t = (int)threadIdx.x;
  const int64_t e = (int64_t)blockIdx.x;
  int64_t lo = start[e], hi = start[e + 1];
  lo = lo < 0 ? 0 : (lo > S ? S : lo);
  hi = hi < lo ? lo : (hi > S ? S : hi);
  if (hi == lo) return;   // (an empty run: the entry stays zero)
  uint32_t *cnt = reinterpret_cast<uint32_t *>(s_entry + 8);
  unsigned long long *hcp = reinterpret_cast<unsigned long long *>(s_entry + offsetof(brl_compare_entry, hcp_sum));
  for (int w = t; w < BRL_COMPARE_ENTRY_BYTES / 4; w += RT) reinterpret_cast<uint32_t *>(s_entry)[w] = 0u;
  for (int w = t; w < ACTIONS * ACTIONS; w += RT) s_conf[w] = 0u;
  __syncthreads();

  double acc = 0.0, top = -INFINITY;   // thread k < SUMS: sum k; thread SUMS: the maximum
  for (int64_t base = lo; base < hi; base += (int64_t)RT * BLOCK) {
    const int64_t b0 = base + (int64_t)t * BLOCK, b1 = b0 + BLOCK < hi ? b0 + BLOCK : hi;
    double part[SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0}, pmax = -INFINITY;
    uint32_t n = 0, agree = 0, xp = 0, yp = 0, bad = 0;
    unsigned long long h_all = 0, h_dis = 0;
    for (int64_t i = b0; i < b1; i++) {   // ascending: the block's order
      const uint4 q1 = sorted[i * DEC_CHUNKS + 1], q2 = sorted[i * DEC_CHUNKS + 2], q3 = sorted[i * DEC_CHUNKS + 3];
      const uint32_t fl = q1.y >> 24, a = q1.y & 0xFFu, cx = (q1.y >> 8) & 0xFFu, cy = (q1.y >> 16) & 0xFFu;
      n++;
      if (fl & BRL_COMPARE_NONFINITE) {
        bad++;
        continue;
      }
      const double js = __longlong_as_double((long long)((uint64_t)q3.x | ((uint64_t)q3.y << 32)));
      part[0] += __longlong_as_double((long long)((uint64_t)q2.x | ((uint64_t)q2.y << 32)));
      part[1] += __longlong_as_double((long long)((uint64_t)q2.z | ((uint64_t)q2.w << 32)));
      part[2] += js;
      part[3] += (double)__uint_as_float(q1.z);
      part[4] += (double)__uint_as_float(q1.w);
      pmax = fmax(pmax, js);
      agree += (fl & BRL_COMPARE_AGREE) != 0;
      xp += (fl & BRL_COMPARE_X_PLAYED) != 0;
      yp += (fl & BRL_COMPARE_Y_PLAYED) != 0;
      h_all += q1.x & 63u;
      h_dis += (fl & BRL_COMPARE_AGREE) ? 0u : (q1.x & 63u);
      if (cx < (uint32_t)ACTIONS && cy < (uint32_t)ACTIONS && a < (uint32_t)ACTIONS) {
        atomicAdd(cnt + C_HIST + cx, 1u);
        atomicAdd(cnt + C_HIST + ACTIONS + cy, 1u);
        atomicAdd(cnt + C_HIST + 2 * ACTIONS + a, 1u);
        atomicAdd(s_conf + cx * ACTIONS + cy, 1u);
      }
    }
    if (n) {
      atomicAdd(cnt + C_N, n);
      if (agree) atomicAdd(cnt + C_AGREE, agree);
      if (xp) atomicAdd(cnt + C_XP, xp);
      if (yp) atomicAdd(cnt + C_YP, yp);
      if (bad) atomicAdd(cnt + C_NONFINITE, bad);
      if (h_all) atomicAdd(hcp, h_all);
      if (h_dis) atomicAdd(hcp + 1, h_dis);
    }
#pragma unroll
    for (int k = 0; k < SUMS; k++) s_part[k][t] = part[k];
    s_max[t] = pmax;
    __syncthreads();
    const int64_t left = hi - base;
    const int blocks = (int)(left >= (int64_t)RT * BLOCK ? RT : (left + BLOCK - 1) / BLOCK);
    if (t < SUMS) {
      for (int b = 0; b < blocks; b++) acc += s_part[t][b];   // ascending: the blocks' order
    } else if (t == SUMS) {
      for (int b = 0; b < blocks; b++) top = fmax(top, s_max[b]);
    }
    __syncthreads();
  }

  if (t < SUMS) *reinterpret_cast<double *>(s_entry + offsetof(brl_compare_entry, kl_xy_sum) + 8 * t) = acc;
  if (t == SUMS) *reinterpret_cast<double *>(s_entry + offsetof(brl_compare_entry, js_max)) = cnt[C_N] == cnt[C_NONFINITE] ? 0.0 : top;
  if (t == SUMS + 1) {
    const uint4 q0 = sorted[lo * DEC_CHUNKS];
    *reinterpret_cast<uint2 *>(s_entry) = make_uint2(q0.x, q0.y);
  }
  __syncthreads();
  if (t < ENTRY_CHUNKS) reinterpret_cast<uint4 *>(entries + e * BRL_COMPARE_ENTRY_BYTES)[t] = reinterpret_cast<const uint4 *>(s_entry)[t];
  for (int w = t; w < ACTIONS * ACTIONS; w += RT) {
    const uint32_t v = s_conf[w];
    if (v) atomicAdd(confusion + w, (unsigned long long)v);
  }
}

}  // namespace

extern "C" int brl_compare_tables(int device, const brl_board_record *records, int64_t n, const int64_t *rows, int64_t m, uint64_t *tables,
                                  uint64_t *hands, void *stream) {
  NEED(records && rows && tables && hands, "NULL array");
  NEED(n > 0 && m > 0 && n < ((int64_t)1 << 31) && m < ((int64_t)1 << 31), "n, m (1 .. 2^31)");
  NEED(((((uintptr_t)records) | ((uintptr_t)tables) | ((uintptr_t)hands)) & 15) == 0 && (((uintptr_t)rows) & 7) == 0,
       "records / tables / hands 16-byte aligned, rows 8-byte aligned");
  HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(k_compare_tables, dim3((unsigned)((m + BELIEF_LANES - 1) / BELIEF_LANES)), dim3(BELIEF_LANES), 0, (hipStream_t)stream,
                     reinterpret_cast<const uint4 *>(records), n, rows, m, reinterpret_cast<uint4 *>(tables), reinterpret_cast<uint4 *>(hands));
  HIP_TRY(hipGetLastError());
  return BRL_OK;
}

extern "C" int brl_compare_rows(int device, const brl_board_record *records, int64_t n, const int64_t *rows, int64_t m, int t, int depth,
                                const float *logits_x, int64_t ld_x, const float *logits_y, int64_t ld_y, const uint64_t *legal,
                                brl_compare_decision *decisions, void *stream) {
  NEED(records && rows && logits_x && logits_y && legal && decisions, "NULL array");
  NEED(n > 0 && m > 0 && n < ((int64_t)1 << 31) && m < ((int64_t)1 << 31), "n, m (1 .. 2^31)");
  NEED(depth >= 1 && depth <= BRL_BOOK_MAX_DEPTH && t >= 0 && t < depth, "depth (1 .. 10), t (0 .. depth - 1)");
  NEED(ld_x >= ACTIONS && ld_y >= ACTIONS && ld_x < ((int64_t)1 << 20) && ld_y < ((int64_t)1 << 20), "ld (38 ..)");
  NEED(((((uintptr_t)records) | ((uintptr_t)decisions)) & 15) == 0 && ((((uintptr_t)rows) | ((uintptr_t)legal)) & 7) == 0 &&
           ((((uintptr_t)logits_x) | ((uintptr_t)logits_y)) & 3) == 0,
       "records / decisions 16-byte, rows / legal 8-byte, logits 4-byte aligned");
  HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(k_compare_rows, dim3((unsigned)((m + 4 * ROW_LANES - 1) / (4 * ROW_LANES))), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const uint4 *>(records), n, rows, m, t, depth, logits_x, ld_x, logits_y, ld_y, legal,
                     reinterpret_cast<uint4 *>(decisions));
  HIP_TRY(hipGetLastError());
  return BRL_OK;
}

extern "C" int brl_compare_reduce(int device, const brl_compare_decision *sorted, int64_t S, const int64_t *entry_start, int64_t K,
                                  brl_compare_entry *entries, uint64_t *confusion, void *stream) {
  NEED(sorted && entry_start && entries && confusion, "NULL array");
  NEED(S > 0 && S < ((int64_t)1 << 40), "S (1 .. 2^40)");
  NEED(K > 0 && K < ((int64_t)1 << 31), "K (1 .. 2^31)");
  NEED(((((uintptr_t)sorted) | ((uintptr_t)entries)) & 15) == 0 && ((((uintptr_t)entry_start) | ((uintptr_t)confusion)) & 7) == 0,
       "sorted / entries 16-byte, entry_start / confusion 8-byte aligned");
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipMemsetAsync(entries, 0, (size_t)K * sizeof(brl_compare_entry), (hipStream_t)stream));
  HIP_TRY(hipMemsetAsync(confusion, 0, (size_t)ACTIONS * ACTIONS * sizeof(uint64_t), (hipStream_t)stream));
  hipLaunchKernelGGL(k_compare_reduce, dim3((unsigned)K), dim3(RT), 0, (hipStream_t)stream, reinterpret_cast<const uint4 *>(sorted), S,
                     entry_start, reinterpret_cast<uint8_t *>(entries), reinterpret_cast<unsigned long long *>(confusion));
  HIP_TRY(hipGetLastError());
  return BRL_OK;
}
