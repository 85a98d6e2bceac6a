// brl_belief.hip — translation unit of libbrl_hip.so: the hand beliefs (include/brl_belief.h, which holds the definition).
// k_belief_deal draws the sample deals: a lane per sample runs the 38-draw Fisher-Yates chain on a card column in LDS, builds the
// empty table of its deal in a table image, and the wave stores its 64 tables and hand rows as whole 16-byte pieces.
// k_belief_logp adds one call's log-probability to the rows that were forwarded: categorical<8> (policy_common.hpp) in mode form
// gives the arg-max and -logf(total); the called action's term is added to it, which is the rollout's log_prob bit for bit.
// k_belief_reduce sums a query's samples: a workgroup per query, one thread per sum, ascending k, no atomics on floating point.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/brl_belief.h"
#include "abi_common.hpp"
#include "belief_table.hpp"
#include "bridge_device.hpp"
#include "hand_features.hpp"
#include "policy_common.hpp"

namespace {

using namespace brl;

static_assert(sizeof(brl_belief_query) == 16 && offsetof(brl_belief_query, seat) == 8 && offsetof(brl_belief_query, seating) == 12,
              "query layout");
static_assert(sizeof(brl_belief_entry) == BRL_BELIEF_ENTRY_BYTES && BRL_BELIEF_ENTRY_BYTES % 16 == 0 &&
                  offsetof(brl_belief_entry, card) == 32 && offsetof(brl_belief_entry, g_card) == 3560 &&
                  offsetof(brl_belief_entry, max_logw) == 16 && offsetof(brl_belief_entry, reserved2) == 5324,
              "entry layout");
static_assert(BRL_BELIEF_STREAM == STREAM_BELIEF && BRL_BELIEF_ACTIONS == BRL_NUM_ACTIONS, "constants");

constexpr uint64_t DECK = (1ull << 52) - 1;
constexpr int HIDDEN = 39;

// ---- the deals ------------------------------------------------------------------------------------------------------------------
constexpr int DEAL_LANES = BELIEF_LANES, IMG_STRIDE = BELIEF_IMG_STRIDE;

__global__ __launch_bounds__(DEAL_LANES) void k_belief_deal(const uint4 *queries, int64_t Q, int64_t K, uint32_t k0, uint32_t k1, int64_t q0,
                                                            uint4 *tables, uint4 *hands) {
  __shared__ uint8_t s_cards[HIDDEN * DEAL_LANES];                                   // card j of lane l at j * 64 + l
  __shared__ __attribute__((aligned(16))) uint8_t s_img[DEAL_LANES * IMG_STRIDE];
  const int lane = (int)threadIdx.x;
  const int64_t total = Q * K, row0 = (int64_t)blockIdx.x * DEAL_LANES;
  const int64_t row = row0 + lane < total ? row0 + lane : total - 1;   // (an idle lane repeats the last sample and stores nothing)
  const int64_t qi = row / K, k = row - qi * K;
  const uint4 qv = queries[qi];
  const uint64_t own = ((uint64_t)qv.x | ((uint64_t)qv.y << 32)) & DECK;
  const BeliefSeat qs = belief_seat(qv);

  uint8_t *c = s_cards + lane;
  uint64_t rest = ~own & DECK;
#pragma unroll 1
  for (int j = 0; j < HIDDEN; j++) {   // ascending by bit index (a hand word without 13 cards — refused by the host — runs out: card 0)
    c[j * DEAL_LANES] = (uint8_t)(rest ? __ffsll((unsigned long long)rest) - 1 : 0);
    rest &= rest - 1ull;
  }
  const uint32_t stream_q = (uint32_t)(q0 + qi);
#pragma unroll 1
  for (int blk = 0; blk < (HIDDEN + 2) / 4; blk++) {
    uint32_t r[4];
    philox4x32_10((uint32_t)k, (uint32_t)blk, STREAM_BELIEF, stream_q, k0, k1, r);
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int j = blk * 4 + i;
      if (j < HIDDEN - 1) {
        const int at = j + (int)__umulhi(philox_word(r, (uint32_t)i), (uint32_t)(HIDDEN - j));   // j .. 38
        const uint8_t a = c[j * DEAL_LANES], b = c[at * DEAL_LANES];
        c[j * DEAL_LANES] = b;
        c[at * DEAL_LANES] = a;
      }
    }
  }
  uint64_t h[3];
#pragma unroll
  for (int s = 0; s < 3; s++) {
    h[s] = 0ull;
#pragma unroll 1
    for (int i = 0; i < 13; i++) h[s] |= 1ull << (c[(s * 13 + i) * DEAL_LANES] & 63u);
  }

  // the empty table of the deal (belief_table.hpp), then the wave's 64 tables and hand rows as whole 16-byte pieces
  belief_empty_table(s_img + lane * IMG_STRIDE, qs, own, h);
  wave_lds_fence();
  belief_store_images(s_img, lane, row0, total - row0, tables, hands);
}

// ---- one call of the weight -----------------------------------------------------------------------------------------------------
constexpr int LOGP_ROWS = 8;   // rows per wave: categorical<8>

__global__ __launch_bounds__(256) void k_belief_logp(const float *logits, int64_t ld, const int64_t *rows, int64_t m, const int32_t *query_of,
                                                     int64_t n, const uint64_t *legal, const int32_t *action, int64_t Q, float *logw,
                                                     uint8_t *greedy) {
  const int lane = (int)(threadIdx.x & 63u);
  const int64_t i = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * LOGP_ROWS + (lane & (LOGP_ROWS - 1));
  bool valid = i < m;
  const int64_t r = valid ? rows[i] : -1;
  valid = valid && r >= 0 && r < n;
  const int64_t q = valid ? (int64_t)query_of[r] : -1;
  valid = valid && q >= 0 && q < Q;
  const int a = valid ? action[q] : 0;
  valid = valid && a >= 0 && a < BRL_NUM_ACTIONS;
  const uint64_t cand = valid ? (legal[q] & ALL_ACTIONS) : 1ull;
  // mode form: the arg-max over the legal actions, and (l[arg-max] - m) - logf(total) = -logf(total)
  float lp_mode;
  const int amax = categorical<LOGP_ROWS>(logits, i * ld, 0, valid, cand, 1, 0u, lane, lp_mode);
  if (valid && lane < LOGP_ROWS) {
    const float mx = logits[i * ld + amax], la = logits[i * ld + a];
    const float lp = (la - mx) + lp_mode;   // == (la - mx) - logf(total)
    logw[r] += lp;
    greedy[r] = (uint8_t)((greedy[r] != 0) && amax == a && lp == lp);
  }
}

// ---- the belief of a query ------------------------------------------------------------------------------------------------------
constexpr int RED_THREADS = 512, TILE = 512;
constexpr int B_CARD = 0, B_HCP = 156, B_LEN = 270, B_BAL = 438, B_WSUM = 441, B_WSQ = 442, BINS = 443;
constexpr int OFF_SUMS = 32, OFF_COUNTS = 3560;
static_assert(offsetof(brl_belief_entry, hcp) == OFF_SUMS + 8 * B_HCP && offsetof(brl_belief_entry, length) == OFF_SUMS + 8 * B_LEN &&
                  offsetof(brl_belief_entry, balanced) == OFF_SUMS + 8 * B_BAL && offsetof(brl_belief_entry, g_hcp) == OFF_COUNTS + 4 * B_HCP &&
                  offsetof(brl_belief_entry, g_length) == OFF_COUNTS + 4 * B_LEN && offsetof(brl_belief_entry, g_balanced) == OFF_COUNTS + 4 * B_BAL,
              "the sums' order");

__global__ __launch_bounds__(RED_THREADS) void k_belief_reduce(const uint4 *queries, int64_t K, const uint4 *hands, const float *logw,
                                                               const uint8_t *greedy, uint8_t *entries) {
  __shared__ __attribute__((aligned(16))) double s_w[TILE];
  __shared__ __attribute__((aligned(16))) uint32_t s_x[9 * TILE];   // [hidden seat][hand word low, high, features][sample of the tile]
  __shared__ __attribute__((aligned(16))) uint8_t s_g[TILE];
  __shared__ float s_max[RED_THREADS];
  __shared__ int s_nan;
  const int t = (int)threadIdx.x;
  const int64_t q = (int64_t)blockIdx.x, first = q * K;
  const uint32_t seat = queries[q].z & 3u;

  // the largest logw (NaN entries set a flag and are passed over)
  float mx = -INFINITY;
  bool nan = false;
  for (int64_t k = t; k < K; k += RED_THREADS) {
    const float v = logw[first + k];
    nan |= v != v;
    mx = fmaxf(mx, v);
  }
  if (t == 0) s_nan = 0;
  s_max[t] = mx;
  __syncthreads();
  if (nan) atomicOr(&s_nan, 1);
#pragma unroll
  for (int off = RED_THREADS / 2; off >= 1; off >>= 1) {
    if (t < off) s_max[t] = fmaxf(s_max[t], s_max[t + off]);
    __syncthreads();
  }
  mx = s_max[0];
  const bool bad = s_nan != 0 || !(fabsf(mx) < INFINITY);

  // this thread's sum: which word of which hidden seat it looks at, and what it wants to see there
  int hd = 0, word = 2;
  uint32_t shift = 0, mask = 0, value = 1;   // (threads without a sum: never a hit)
  if (t < B_HCP) {
    hd = t / 52;
    const int card = t - hd * 52;
    word = card >> 5, shift = (uint32_t)(card & 31), mask = 1, value = 1;
  } else if (t < B_LEN) {
    hd = (t - B_HCP) / 38;
    shift = 0, mask = 63, value = (uint32_t)(t - B_HCP - hd * 38);
  } else if (t < B_BAL) {
    hd = (t - B_LEN) / 56;
    const int r = t - B_LEN - hd * 56, suit = r / 14;
    shift = (uint32_t)(F_LEN + 4 * suit), mask = 15, value = (uint32_t)(r - suit * 14);
  } else if (t < B_WSUM) {
    hd = t - B_BAL;
    shift = (uint32_t)F_BAL, mask = 1, value = 1;
  } else if (t < BINS) {
    value = 0;   // every sample
  }
  const bool squares = t == B_WSQ;
  const uint32_t *col = s_x + (hd * 3 + word) * TILE;
  double acc = 0.0;
  uint32_t count = 0;
  for (int64_t base = 0; base < K; base += TILE) {
    const int cnt = (int)(K - base < TILE ? K - base : TILE);
    if (t < cnt) {
      const int64_t row = first + base + t;
      s_w[t] = exp((double)logw[row] - (double)mx);
      s_g[t] = (uint8_t)(greedy[row] != 0);
      const uint4 a = hands[row * 2], b = hands[row * 2 + 1];
#pragma unroll
      for (int h = 0; h < 3; h++) {
        const uint32_t x = (seat + 1u + (uint32_t)h) & 3u;
        const uint32_t lo = x == 0 ? a.x : (x == 1 ? a.z : (x == 2 ? b.x : b.z));
        const uint32_t hi = (x == 0 ? a.y : (x == 1 ? a.w : (x == 2 ? b.y : b.w))) & (uint32_t)(DECK >> 32);
        s_x[(h * 3 + 0) * TILE + t] = lo;
        s_x[(h * 3 + 1) * TILE + t] = hi;
        s_x[(h * 3 + 2) * TILE + t] = hand_features((uint64_t)lo | ((uint64_t)hi << 32));
      }
    } else if (t < TILE) {   // behind the last sample: weight +0.0, not consistent — such a slot adds +0.0 and counts nothing
      s_w[t] = 0.0;
      s_g[t] = 0;
    }
    __syncthreads();
    // ascending k, the summation order of the definition; eight samples' LDS reads are issued together (one read per step left
    // the loop waiting for LDS 4096 times: 598 us per launch whatever Q)
    for (int k0 = 0; k0 < cnt; k0 += 8) {
      const uint4 c0 = *reinterpret_cast<const uint4 *>(col + k0), c1 = *reinterpret_cast<const uint4 *>(col + k0 + 4);
      const uint2 g2 = *reinterpret_cast<const uint2 *>(s_g + k0);
      const uint32_t cw[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
      const uint64_t g = (uint64_t)g2.x | ((uint64_t)g2.y << 32);
      double w[8];
#pragma unroll
      for (int i = 0; i < 8; i++) w[i] = s_w[k0 + i];
#pragma unroll
      for (int i = 0; i < 8; i++) {
        const bool hit = ((cw[i] >> shift) & mask) == value;
        acc += hit ? (squares ? w[i] * w[i] : w[i]) : 0.0;
        count += (uint32_t)(hit && ((g >> (8 * i)) & 1ull) != 0ull);
      }
    }
    __syncthreads();
  }

  uint8_t *out = entries + q * BRL_BELIEF_ENTRY_BYTES;
  const double sum = bad ? (double)NAN : acc;
  if (t < B_WSUM) {
    *reinterpret_cast<double *>(out + OFF_SUMS + 8 * t) = sum;
    *reinterpret_cast<uint32_t *>(out + OFF_COUNTS + 4 * t) = count;
  } else if (t == B_WSUM) {
    *reinterpret_cast<double *>(out + offsetof(brl_belief_entry, wsum)) = sum;
    *reinterpret_cast<float *>(out + offsetof(brl_belief_entry, max_logw)) = bad ? NAN : mx;
    *reinterpret_cast<uint32_t *>(out + offsetof(brl_belief_entry, n)) = (uint32_t)K;
    *reinterpret_cast<uint32_t *>(out + offsetof(brl_belief_entry, consistent)) = count;
    *reinterpret_cast<uint32_t *>(out + offsetof(brl_belief_entry, reserved)) = 0u;
  } else if (t == B_WSQ) {
    *reinterpret_cast<double *>(out + offsetof(brl_belief_entry, wsq)) = sum;
    *reinterpret_cast<uint32_t *>(out + offsetof(brl_belief_entry, reserved2)) = 0u;
  }
}

}  // namespace

extern "C" int brl_belief_deal(int device, const brl_belief_query *queries, int64_t Q, int64_t K, uint64_t seed, int64_t q0, uint64_t *tables,
                               uint64_t *hands, void *stream) {
  NEED(queries && tables && hands, "NULL array");
  NEED(Q > 0 && K > 0 && Q < ((int64_t)1 << 31) && K < ((int64_t)1 << 31) && Q * K < ((int64_t)1 << 31), "Q, K (>= 1, Q * K below 2^31)");
  NEED(q0 >= 0 && q0 + Q <= ((int64_t)1 << 32), "q0 (0 .., q0 + Q at most 2^32)");
  NEED(((((uintptr_t)queries) | ((uintptr_t)tables) | ((uintptr_t)hands)) & 15) == 0, "queries / tables / hands 16-byte aligned");
  HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(k_belief_deal, dim3((unsigned)((Q * K + DEAL_LANES - 1) / DEAL_LANES)), dim3(DEAL_LANES), 0, (hipStream_t)stream,
                     reinterpret_cast<const uint4 *>(queries), Q, K, (uint32_t)seed, (uint32_t)(seed >> 32), q0,
                     reinterpret_cast<uint4 *>(tables), reinterpret_cast<uint4 *>(hands));
  HIP_TRY(hipGetLastError());
  return BRL_OK;
}

extern "C" int brl_belief_logp(int device, const float *logits, int64_t ld, const int64_t *rows, int64_t m, const int32_t *query_of, int64_t n,
                               const uint64_t *legal, const int32_t *action, int64_t Q, float *logw, uint8_t *greedy, void *stream) {
  NEED(logits && rows && query_of && legal && action && logw && greedy, "NULL array");
  NEED(ld >= BRL_BELIEF_ACTIONS && ld < ((int64_t)1 << 20), "ld (38 ..)");
  NEED(m > 0 && n > 0 && Q > 0 && m < ((int64_t)1 << 31) && n < ((int64_t)1 << 31) && Q < ((int64_t)1 << 31), "m, n, Q (1 .. 2^31)");
  NEED((((uintptr_t)logits) & 3) == 0 && (((uintptr_t)rows) & 7) == 0 && (((uintptr_t)legal) & 7) == 0, "logits 4-byte, rows / legal 8-byte aligned");
  HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(k_belief_logp, dim3((unsigned)((m + 4 * LOGP_ROWS - 1) / (4 * LOGP_ROWS))), dim3(256), 0, (hipStream_t)stream, logits, ld,
                     rows, m, query_of, n, legal, action, Q, logw, greedy);
  HIP_TRY(hipGetLastError());
  return BRL_OK;
}

extern "C" int brl_belief_reduce(int device, const brl_belief_query *queries, int64_t Q, int64_t K, const uint64_t *hands, const float *logw,
                                 const uint8_t *greedy, brl_belief_entry *entries, void *stream) {
  NEED(queries && hands && logw && greedy && entries, "NULL array");
  NEED(Q > 0 && K > 0 && Q < ((int64_t)1 << 31) && K < ((int64_t)1 << 31) && Q * K < ((int64_t)1 << 31), "Q, K (>= 1, Q * K below 2^31)");
  NEED(((((uintptr_t)queries) | ((uintptr_t)hands) | ((uintptr_t)entries)) & 15) == 0, "queries / hands / entries 16-byte aligned");
  HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(k_belief_reduce, dim3((unsigned)Q), dim3(RED_THREADS), 0, (hipStream_t)stream, reinterpret_cast<const uint4 *>(queries),
                     K, reinterpret_cast<const uint4 *>(hands), logw, greedy, reinterpret_cast<uint8_t *>(entries));
  HIP_TRY(hipGetLastError());
  return BRL_OK;
}
