// brl_book.hip — translation unit of libbrl_hip.so: the bidding-system book (include/brl_book.h).  k_book_samples turns board
// records into one (key, features) pair per call of the first `depth` calls; the host sorts the keys (torch) and k_book_reduce
// sums the sorted samples into one entry of integer counters per distinct key.  Integer arithmetic only: the same bytes on every
// run, whatever the order in which the workgroups' atomic adds arrive.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/brl_book.h"
#include "abi_common.hpp"
#include "hand_features.hpp"

namespace {

constexpr int REC_CHUNKS = (int)sizeof(brl_board_record) / 16;   // 23
static_assert(sizeof(brl_board_record) == 368 && offsetof(brl_board_record, hands) == 16 && offsetof(brl_board_record, calls) == 48,
              "record layout");
static_assert(sizeof(brl_book_team) == 400 && sizeof(brl_book_entry) == BRL_BOOK_ENTRY_BYTES && BRL_BOOK_ENTRY_BYTES % 16 == 0 &&
                  offsetof(brl_book_entry, team) == 16 && offsetof(brl_book_team, imp_sum) == 384,
              "entry layout");

// feature word (brl_book.h): the hand's part is hand_features.hpp's
using brl::F_BAL;
using brl::F_LEN;
using brl::hand_features;
constexpr int F_TEAM = 23, F_IMP = 24;

// Four lanes per record: lane q loads bytes 16 q .. 16 q + 15 — the header, hands N,E, hands S,W, calls[0..15] — and owns the
// seat (dealer + q) & 3, which makes the calls p = q, q + 4, q + 8.
__global__ __launch_bounds__(256) void k_book_samples(const uint4 *records, int64_t n, const int32_t *imp, int imp_sign, int depth,
                                                      uint64_t *keys, uint32_t *feats) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t rec = g >> 2;
  const bool live = rec < n;
  const int q = (int)(g & 3), lane = (int)(threadIdx.x & 63), base = lane & ~3;
  const uint4 v = records[(live ? rec : n - 1) * REC_CHUNKS + q];   // (an idle lane reads the last record and writes nothing)
  const uint32_t w0 = __shfl(v.x, base), w1 = __shfl(v.y, base), w2 = __shfl(v.z, base);
  const int n_calls = (int)(w0 & 0xFFFFu), dealer = (int)((w0 >> 16) & 3u);
  const bool ok = ((w1 >> 8) & BRL_BOARD_OK) != 0;
  const uint32_t seating = w2 >> 24;
  const int s = (dealer + q) & 3, src = base + 1 + (s >> 1);
  const uint32_t hx = __shfl(v.x, src), hy = __shfl(v.y, src), hz = __shfl(v.z, src), hw = __shfl(v.w, src);
  const uint64_t hand = (s & 1) ? ((uint64_t)hw << 32 | hz) : ((uint64_t)hy << 32 | hx);
  const uint32_t c[3] = {__shfl(v.x, base + 3), __shfl(v.y, base + 3), __shfl(v.z, base + 3)};
  uint64_t full = 0;   // the key of calls[0..9]; the fill byte 0xFF gives a zero field
#pragma unroll
  for (int j = 0; j < BRL_BOOK_MAX_DEPTH; j++) full |= (uint64_t)(((c[j >> 2] >> (8 * (j & 3))) + 1u) & 63u) << (58 - 6 * j);
  const uint32_t team = ((seating >> (2 * s)) & 3u) >> 1;
  int bidder_imp = (imp != nullptr && live) ? imp[rec] * imp_sign : 0;
  bidder_imp = (s & 1) ? -bidder_imp : bidder_imp;
  const uint32_t f = hand_features(hand) | (team << F_TEAM) | ((uint32_t)bidder_imp << F_IMP);
  const int m = n_calls < depth ? n_calls : depth;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const int p = q + 4 * k;
    if (live && p < depth) {
      const bool sample = ok && p < m;
      keys[rec * depth + p] = sample ? (full & (~0ull << (58 - 6 * p))) : 0ull;
      feats[rec * depth + p] = sample ? f : 0u;
    }
  }
}

// ---- the reduction ------------------------------------------------------------------------------------------------------------
constexpr int CHUNK = BRL_BOOK_CHUNK, THREADS = 256, PER = CHUNK / THREADS;
constexpr int TEAM_WORDS = (int)sizeof(brl_book_team) / 4;   // 100: 96 counters and two 64-bit sums
constexpr int SLOT_WORDS = 2 * TEAM_WORDS;
constexpr int BINS = 96, ITEMS = 2 * (BINS + 2);             // what a flush looks at, per slot
// runs that need a histogram in one chunk: at most 15 of 64 samples or more beside the two that cross its ends, or 16
constexpr int MAX_SLOTS = 18;
constexpr uint32_t CROSSES = 0x8000u;
constexpr int W_COUNT = 0, W_BAL = 1, W_HCP = 2, W_LEN = 40, W_IMP = 96, W_SQ = 98;
static_assert(offsetof(brl_book_team, hcp) == 4 * W_HCP && offsetof(brl_book_team, length) == 4 * W_LEN &&
                  offsetof(brl_book_team, imp_sq_sum) == 4 * W_SQ, "counter words");

__device__ __forceinline__ int f_imp(uint32_t f) { return (int)f >> F_IMP; }
__device__ __forceinline__ uint32_t f_len(uint32_t f, int s) { return (f >> (F_LEN + 4 * s)) & 15u; }

__device__ __forceinline__ int wave_sum(int x) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d);
  return x;
}

__global__ __launch_bounds__(THREADS) void k_book_reduce(const uint32_t *feats, const int32_t *eidx, int64_t S, const uint64_t *ekeys,
                                                         int64_t K, uint8_t *entries) {
  __shared__ uint32_t s_feat[CHUNK];
  __shared__ uint16_t s_start[CHUNK], s_end[CHUNK];   // by the run's number in the chunk: [start, end) | CROSSES
  __shared__ uint8_t s_slot[CHUNK];                   // by the run's number: its histogram
  __shared__ __attribute__((aligned(8))) uint32_t s_hist[MAX_SLOTS * SLOT_WORDS];
  __shared__ int32_t s_slot_entry[MAX_SLOTS];
  __shared__ int s_nslots;

  const int t = (int)threadIdx.x;
  const int64_t c0 = (int64_t)blockIdx.x * CHUNK;
  const int64_t left = S - c0;
  const int cn = (int)(left < CHUNK ? left : CHUNK);   // samples in this chunk, >= 1
  const int32_t e_base = eidx[c0];
  if (t == 0) s_nslots = 0;

  int32_t e[PER];
  int r[PER];
  bool valid[PER], head[PER];
#pragma unroll
  for (int k = 0; k < PER; k++) {
    const int j = k * THREADS + t;
    const int64_t i = c0 + j;
    const bool in = j < cn;
    e[k] = in ? eidx[i] : -1;
    r[k] = (int)(e[k] - e_base);
    valid[k] = in && e[k] >= 0 && (int64_t)e[k] < K && (unsigned)r[k] < (unsigned)CHUNK;
    const bool starts = i == 0 || (in && eidx[i - 1] != e[k]);
    const bool ends = i + 1 >= S || (in && eidx[i + 1] != e[k]);
    head[k] = valid[k] && starts;
    s_feat[j] = in ? feats[i] : 0u;
    if (valid[k]) {
      if (starts || j == 0) s_start[r[k]] = (uint16_t)((uint32_t)j | (starts ? 0u : CROSSES));
      if (ends || j == cn - 1) s_end[r[k]] = (uint16_t)((uint32_t)(j + 1) | (ends ? 0u : CROSSES));
    }
  }
  __syncthreads();

  // which runs get a histogram: the first lane of each asks for one
  int st[PER], en[PER];
  bool hist[PER];
#pragma unroll
  for (int k = 0; k < PER; k++) {
    const int j = k * THREADS + t;
    st[k] = en[k] = 0;
    hist[k] = false;
    if (valid[k]) {
      const uint32_t a = s_start[r[k]], b = s_end[r[k]];
      st[k] = (int)(a & (CROSSES - 1u));
      en[k] = (int)(b & (CROSSES - 1u));
      en[k] = en[k] > cn ? cn : en[k];
      st[k] = st[k] > j ? j : st[k];   // (indices that are not nondecreasing: stay inside the chunk)
      hist[k] = ((a | b) & CROSSES) != 0 || en[k] - st[k] >= 64;
      if (hist[k] && j == st[k]) {
        const int slot = atomicAdd(&s_nslots, 1);
        s_slot[r[k]] = (uint8_t)(slot < MAX_SLOTS ? slot : 0xFF);
        if (slot < MAX_SLOTS) s_slot_entry[slot] = e[k];
      }
    }
  }
  __syncthreads();
  const int nslots = s_nslots < MAX_SLOTS ? s_nslots : MAX_SLOTS;
  for (int w = t; w < nslots * SLOT_WORDS; w += THREADS) s_hist[w] = 0u;
  __syncthreads();

#pragma unroll
  for (int k = 0; k < PER; k++) {
    const int j = k * THREADS + t;
    const uint32_t f = s_feat[j];
    const uint32_t team = (f >> F_TEAM) & 1u, hcp = f & 63u, bal = (f >> F_BAL) & 1u;
    const int imp = f_imp(f);
    uint8_t *const out = entries + (int64_t)(valid[k] ? e[k] : 0) * BRL_BOOK_ENTRY_BYTES;
    if (head[k]) *reinterpret_cast<uint64_t *>(out) = ekeys[e[k]];
    const int slot = (valid[k] && hist[k]) ? (int)s_slot[r[k]] : 0xFF;
    const bool in_hist = slot < MAX_SLOTS;

    // ---- a long run, or one shared with a neighbouring workgroup: LDS atomics into its histogram
    // a wave whose 64 samples all belong to one such run adds its totals once instead of lane by lane
    const int r_first = __shfl(r[k], 0);
    const bool whole_wave = __ballot(in_hist && r[k] == r_first) == ~0ull;
    if (whole_wave) {
      const uint64_t t1 = __ballot(team != 0u), b = __ballot(bal != 0u);
      const int n1 = __popcll(t1), b1 = __popcll(b & t1), b0 = __popcll(b & ~t1);
      const int i0 = wave_sum(team ? 0 : imp), i1 = wave_sum(team ? imp : 0);
      const int q0 = wave_sum(team ? 0 : imp * imp), q1 = wave_sum(team ? imp * imp : 0);
      if ((t & 63) == 0) {
        uint32_t *h = s_hist + slot * SLOT_WORDS;
        if (n1 != 64) atomicAdd(h + W_COUNT, (uint32_t)(64 - n1));
        if (n1 != 0) atomicAdd(h + TEAM_WORDS + W_COUNT, (uint32_t)n1);
        if (b0) atomicAdd(h + W_BAL, (uint32_t)b0);
        if (b1) atomicAdd(h + TEAM_WORDS + W_BAL, (uint32_t)b1);
        if (i0) atomicAdd(reinterpret_cast<unsigned long long *>(h + W_IMP), (unsigned long long)(long long)i0);
        if (i1) atomicAdd(reinterpret_cast<unsigned long long *>(h + TEAM_WORDS + W_IMP), (unsigned long long)(long long)i1);
        if (q0) atomicAdd(reinterpret_cast<unsigned long long *>(h + W_SQ), (unsigned long long)q0);
        if (q1) atomicAdd(reinterpret_cast<unsigned long long *>(h + TEAM_WORDS + W_SQ), (unsigned long long)q1);
      }
    }
    if (in_hist) {
      uint32_t *h = s_hist + slot * SLOT_WORDS + (int)team * TEAM_WORDS;
      if (!whole_wave) {
        atomicAdd(h + W_COUNT, 1u);
        if (bal) atomicAdd(h + W_BAL, 1u);
        if (imp) {
          atomicAdd(reinterpret_cast<unsigned long long *>(h + W_IMP), (unsigned long long)(long long)imp);
          atomicAdd(reinterpret_cast<unsigned long long *>(h + W_SQ), (unsigned long long)(imp * imp));
        }
      }
      atomicAdd(h + W_HCP + (hcp < 38u ? hcp : 37u), 1u);
#pragma unroll
      for (int s = 0; s < 4; s++) {
        const uint32_t len = f_len(f, s);
        atomicAdd(h + W_LEN + 14 * s + (len < 14u ? len : 13u), 1u);
      }
    }

    // ---- a short run inside the chunk: this workgroup's alone.  Each lane looks through its run; the first lane to hold a
    // bin's value stores the bin's total.
    if (valid[k] && !hist[k]) {
      uint32_t n_team = 0, n_bal = 0, n_hcp = 0, n_len[4] = {0, 0, 0, 0};
      int64_t sum = 0;
      uint64_t sq = 0;
      bool first_team = true, first_hcp = true, first_len[4] = {true, true, true, true};
      for (int i = st[k]; i < en[k]; i++) {
        const uint32_t g = s_feat[i];
        if (((g >> F_TEAM) & 1u) != team) continue;
        const bool before = i < j;
        n_team++;
        first_team &= !before;
        n_bal += (g >> F_BAL) & 1u;
        const int gi = f_imp(g);
        sum += gi;
        sq += (uint64_t)(gi * gi);
        if ((g & 63u) == hcp) {
          n_hcp++;
          first_hcp &= !before;
        }
#pragma unroll
        for (int s = 0; s < 4; s++)
          if (f_len(g, s) == f_len(f, s)) {
            n_len[s]++;
            first_len[s] &= !before;
          }
      }
      uint32_t *h = reinterpret_cast<uint32_t *>(out + offsetof(brl_book_entry, team)) + (int)team * TEAM_WORDS;
      if (first_team) {
        h[W_COUNT] = n_team;
        if (n_bal) h[W_BAL] = n_bal;
        if (sum) *reinterpret_cast<int64_t *>(h + W_IMP) = sum;
        if (sq) *reinterpret_cast<uint64_t *>(h + W_SQ) = sq;
      }
      if (first_hcp) h[W_HCP + (hcp < 38u ? hcp : 37u)] = n_hcp;
#pragma unroll
      for (int s = 0; s < 4; s++) {
        const uint32_t len = f_len(f, s);
        if (first_len[s]) h[W_LEN + 14 * s + (len < 14u ? len : 13u)] = n_len[s];
      }
    }
  }
  __syncthreads();

  // ---- the histograms' nonzero bins, one global add each
  for (int item = t; item < nslots * ITEMS; item += THREADS) {
    const int slot = item / ITEMS, w = item - slot * ITEMS;
    const int team = w / (BINS + 2), x = w - team * (BINS + 2);
    const uint32_t *h = s_hist + slot * SLOT_WORDS + team * TEAM_WORDS;
    uint8_t *dst = entries + (int64_t)s_slot_entry[slot] * BRL_BOOK_ENTRY_BYTES + offsetof(brl_book_entry, team) + team * sizeof(brl_book_team);
    if (x < BINS) {
      const uint32_t v = h[x];
      if (v) atomicAdd(reinterpret_cast<uint32_t *>(dst) + x, v);
    } else {
      const int u = x - BINS;   // imp_sum, imp_sq_sum
      const unsigned long long v = *reinterpret_cast<const unsigned long long *>(h + W_IMP + 2 * u);
      if (v) atomicAdd(reinterpret_cast<unsigned long long *>(dst + 4 * W_IMP) + u, v);
    }
  }
}

}  // namespace

extern "C" int brl_book_samples(int device, const brl_board_record *records, int64_t n, const int32_t *imp, int imp_sign, int depth,
                                uint64_t *keys, uint32_t *feats, void *stream) {
  NEED(records && keys && feats, "NULL array");
  NEED(n > 0 && n < ((int64_t)1 << 29), "n (1 .. 2^29)");
  NEED(depth >= 1 && depth <= BRL_BOOK_MAX_DEPTH, "depth (1 .. 10)");
  NEED(imp_sign == 1 || imp_sign == -1, "imp_sign (+1 / -1)");
  NEED((((uintptr_t)records) & 15) == 0 && (((uintptr_t)keys) & 7) == 0 && (((uintptr_t)feats) & 3) == 0,
       "records 16-byte aligned, keys 8-byte aligned");
  HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(k_book_samples, dim3((unsigned)((n * 4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const uint4 *>(records), n, imp, imp_sign, depth, keys, feats);
  HIP_TRY(hipGetLastError());
  return BRL_OK;
}

extern "C" int brl_book_reduce(int device, const uint32_t *feats, const int32_t *entry_index, int64_t S, const uint64_t *entry_keys,
                               int64_t K, brl_book_entry *entries, void *stream) {
  NEED(feats && entry_index && entry_keys && entries, "NULL array");
  NEED(S > 0 && S < ((int64_t)1 << 40), "S (1 .. 2^40)");
  NEED(K > 0 && K < ((int64_t)1 << 31), "K (1 .. 2^31)");
  NEED((((uintptr_t)entries) & 15) == 0 && (((uintptr_t)entry_keys) & 7) == 0, "entries 16-byte aligned, entry_keys 8-byte aligned");
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipMemsetAsync(entries, 0, (size_t)K * sizeof(brl_book_entry), (hipStream_t)stream));
  hipLaunchKernelGGL(k_book_reduce, dim3((unsigned)((S + CHUNK - 1) / CHUNK)), dim3(THREADS), 0, (hipStream_t)stream, feats,
                     entry_index, S, entry_keys, K, reinterpret_cast<uint8_t *>(entries));
  HIP_TRY(hipGetLastError());
  return BRL_OK;
}
