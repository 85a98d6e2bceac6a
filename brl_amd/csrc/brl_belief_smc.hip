// brl_belief_smc.hip — translation unit of libbrl_hip.so: the resample-move stages of the hand beliefs
// (include/brl_belief_smc.h, which holds the definition).
// k_belief_resample: a workgroup per listed query.  The weights of a tile of 4096 particles go to LDS, a thread per 64-particle
// segment forms the segment's running sum in place, one thread carries the offset over the segments — the header's two-level
// order —, and the outputs search the tile's cumulative sums by bisection; their ancestors' rows are copied as 16-byte pieces.
// k_belief_propose: a lane per particle exchanges one card between two hidden hands and builds the empty table of the proposed
// deal with k_belief_deal's own builder (belief_table.hpp).
// k_belief_accept: a lane decides for its particle, the wave copies the accepted rows.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/brl_belief_smc.h"
#include "abi_common.hpp"
#include "belief_table.hpp"
#include "bridge_device.hpp"

namespace {

using namespace brl;

static_assert(BRL_BELIEF_RESAMPLE_STREAM == STREAM_BELIEF_RESAMPLE && BRL_BELIEF_MOVE_STREAM == STREAM_BELIEF_MOVE, "constants");

constexpr uint64_t DECK = (1ull << 52) - 1;
constexpr int PIECES = TABLE_BYTES / 16;   // 16-byte pieces of a table; a hand row has two

// the hand word of seat x from a hand row's two pieces (selects, no indexed array)
__device__ __forceinline__ uint64_t hand_at(const uint4 a, const uint4 b, uint32_t x) {
  const uint32_t lo = x == 0 ? a.x : (x == 1 ? a.z : (x == 2 ? b.x : b.z));
  const uint32_t hi = x == 0 ? a.y : (x == 1 ? a.w : (x == 2 ? b.y : b.w));
  return ((uint64_t)lo | ((uint64_t)hi << 32)) & DECK;
}

__device__ __forceinline__ double unit_draw(uint32_t w) { return ((double)w + 0.5) * 0x1p-32; }

// ---- resample -------------------------------------------------------------------------------------------------------------------
constexpr int RS_THREADS = 1024, SEG = BRL_BELIEF_SMC_SEGMENT, RS_TILE = 4096, RS_SEGS = RS_TILE / SEG, RS_CHUNK = 4096;
static_assert(SEG == 64 && RS_SEGS <= 64, "a segment per lane of the first wave");

// a tile's sums in LDS, one double of padding per segment: the segments' threads then walk 520 bytes apart, on different banks
__device__ __forceinline__ int c_at(int i) { return i + (i >> 6); }

__global__ __launch_bounds__(RS_THREADS) void k_belief_resample(const int32_t *list, const int64_t *stream_of, int64_t Q, int64_t K, uint32_t k0,
                                                                uint32_t k1, uint32_t stage, const uint4 *tables, const uint4 *hands,
                                                                const float *logl, const float *logw, const uint8_t *greedy, uint4 *tables_out,
                                                                uint4 *hands_out, float *logl_out, float *logw_out, uint8_t *greedy_out,
                                                                int32_t *ancestor) {
  __shared__ double s_c[RS_TILE + RS_SEGS];
  __shared__ double s_off[RS_SEGS];
  __shared__ double s_carry;
  __shared__ int s_anc[RS_CHUNK];
  __shared__ float s_max[RS_THREADS];
  __shared__ int s_nan;
  const int t = (int)threadIdx.x;
  const int64_t qi = (int64_t)list[blockIdx.x];
  if (qi < 0 || qi >= Q) return;   // (the whole workgroup)
  const int64_t first = qi * K;

  // the largest logw (NaN entries set a flag and are passed over), as k_belief_reduce
  float mx = -INFINITY;
  bool nan = false;
  for (int64_t k = t; k < K; k += RS_THREADS) {
    const float v = logw[first + k];
    nan |= v != v;
    mx = fmaxf(mx, v);
  }
  if (t == 0) s_nan = 0;
  s_max[t] = mx;
  __syncthreads();
  if (nan) atomicOr(&s_nan, 1);
#pragma unroll
  for (int off = RS_THREADS / 2; off >= 1; off >>= 1) {
    if (t < off) s_max[t] = fmaxf(s_max[t], s_max[t + off]);
    __syncthreads();
  }
  mx = s_max[0];
  if (s_nan != 0 || !(fabsf(mx) < INFINITY)) {   // left as it is: the identity, logw kept
    for (int64_t i = t; i < K * PIECES; i += RS_THREADS) tables_out[first * PIECES + i] = tables[first * PIECES + i];
    for (int64_t i = t; i < K * 2; i += RS_THREADS) hands_out[first * 2 + i] = hands[first * 2 + i];
    for (int64_t k = t; k < K; k += RS_THREADS) {
      logl_out[first + k] = logl[first + k];
      logw_out[first + k] = logw[first + k];
      greedy_out[first + k] = greedy[first + k];
      ancestor[first + k] = (int32_t)k;
    }
    return;
  }

  // C of particles base .. base + cnt - 1 into s_c (at c_at), the offset of the tile's first segment given; s_carry = its last C
  auto build_tile = [&](int64_t base, int cnt, double carry) {
    for (int i = t; i < cnt; i += RS_THREADS) s_c[c_at(i)] = exp((double)logw[first + base + i] - (double)mx);
    __syncthreads();
    const int nseg = (cnt + SEG - 1) / SEG;
    if (t < nseg) {   // I: serial inside the segment, eight LDS reads issued together
      const int n = cnt - t * SEG < SEG ? cnt - t * SEG : SEG;
      double *seg = s_c + c_at(t * SEG);
      double acc = 0.0;   // (0 + W_k is W_k: the weights are never -0)
      for (int i0 = 0; i0 < n; i0 += 8) {
        double w[8];
#pragma unroll
        for (int i = 0; i < 8; i++) w[i] = i0 + i < n ? seg[i0 + i] : 0.0;
#pragma unroll
        for (int i = 0; i < 8; i++) {
          if (i0 + i < n) {
            acc += w[i];
            seg[i0 + i] = acc;
          }
        }
      }
    }
    __syncthreads();
    if (t == 0) {   // O: serial over the segments
      double o = carry;
      for (int s = 0; s < nseg; s++) {
        s_off[s] = o;
        const int last = (s + 1) * SEG < cnt ? (s + 1) * SEG - 1 : cnt - 1;
        o += s_c[c_at(last)];
      }
      s_carry = o;
    }
    __syncthreads();
    for (int i = t; i < cnt; i += RS_THREADS) s_c[c_at(i)] = s_off[i >> 6] + s_c[c_at(i)];
    __syncthreads();
  };

  const int64_t ntiles = (K + RS_TILE - 1) / RS_TILE;
  double carry = 0.0;
  for (int64_t tile = 0; tile < ntiles; tile++) {
    const int64_t base = tile * RS_TILE;
    build_tile(base, (int)(K - base < RS_TILE ? K - base : RS_TILE), carry);
    carry = s_carry;
  }
  const double S = carry, dK = (double)K;

  uint32_t r[4];
  philox4x32_10(stage, 0u, STREAM_BELIEF_RESAMPLE, (uint32_t)stream_of[qi], k0, k1, r);
  const double u = unit_draw(r[0]);
  auto x_of = [&](int64_t j) { return (((double)j + u) * S) / dK; };

  int64_t jlo = 0;
  carry = 0.0;
  for (int64_t tile = 0; tile < ntiles; tile++) {
    const int64_t base = tile * RS_TILE;
    const int cnt = (int)(K - base < RS_TILE ? K - base : RS_TILE);
    if (ntiles > 1) build_tile(base, cnt, carry);   // (one tile: it is still there)
    carry = s_carry;
    // the outputs below the tile's last C: x is monotone in j (every thread finds the same end)
    int64_t jhi = K;
    if (tile + 1 < ntiles) {
      int64_t lo = jlo, hi = K;
      while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (x_of(mid) < carry) lo = mid + 1;
        else hi = mid;
      }
      jhi = lo;
    }
    for (int64_t jbase = jlo; jbase < jhi; jbase += RS_CHUNK) {
      const int n = (int)(jhi - jbase < RS_CHUNK ? jhi - jbase : RS_CHUNK);
      for (int jj = t; jj < n; jj += RS_THREADS) {
        const double x = x_of(jbase + jj);
        int lo = 0, hi = cnt - 1;   // the smallest i with C_i > x; the last one if there is none
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (s_c[c_at(mid)] > x) hi = mid;
          else lo = mid + 1;
        }
        const int64_t a = base + lo, out = first + jbase + jj;
        s_anc[jj] = (int)a;
        ancestor[out] = (int32_t)a;
        logl_out[out] = logl[first + a];
        greedy_out[out] = greedy[first + a];
        logw_out[out] = 0.0f;
      }
      __syncthreads();
      // the gather: a query is one workgroup, so what hides the loads' latency is loads in flight — four per thread before a store
      const int64_t out0 = first + jbase;
      const int n8 = n * PIECES;
      auto piece = [&](int i) {   // (behind the end: the last piece again, not stored)
        const int c = i < n8 ? i : n8 - 1;
        return tables[(first + s_anc[c >> 3]) * PIECES + (c & 7)];
      };
      for (int i0 = t; i0 < n8; i0 += 4 * RS_THREADS) {
        const int i1 = i0 + RS_THREADS, i2 = i0 + 2 * RS_THREADS, i3 = i0 + 3 * RS_THREADS;
        const uint4 v0 = piece(i0), v1 = piece(i1), v2 = piece(i2), v3 = piece(i3);
        tables_out[out0 * PIECES + i0] = v0;
        if (i1 < n8) tables_out[out0 * PIECES + i1] = v1;
        if (i2 < n8) tables_out[out0 * PIECES + i2] = v2;
        if (i3 < n8) tables_out[out0 * PIECES + i3] = v3;
      }
      for (int i = t; i < n * 2; i += RS_THREADS) hands_out[out0 * 2 + i] = hands[(first + s_anc[i >> 1]) * 2 + (i & 1)];
      __syncthreads();
    }
    jlo = jhi;
  }
}

// ---- propose --------------------------------------------------------------------------------------------------------------------
// the i-th card of a hand word, ascending by bit index, as a one-bit word; 0 if the hand has no such card
__device__ __forceinline__ uint64_t nth_card(uint64_t hand, uint32_t i) {
#pragma unroll 1
  for (uint32_t n = 0; n < i; n++) hand &= hand - 1ull;
  return hand & (~hand + 1ull);
}

__global__ __launch_bounds__(BELIEF_LANES) void k_belief_propose(const uint4 *queries, const int32_t *list, const int64_t *stream_of, int64_t Q,
                                                                 int64_t K, uint32_t k0, uint32_t k1, uint32_t stage_move, const uint4 *hands,
                                                                 uint4 *tables_new, uint4 *hands_new) {
  __shared__ __attribute__((aligned(16))) uint8_t s_img[BELIEF_LANES * BELIEF_IMG_STRIDE];
  const int lane = (int)threadIdx.x;
  const int64_t p = (int64_t)blockIdx.y, qi = (int64_t)list[p];
  if (qi < 0 || qi >= Q) return;
  const int64_t kb = (int64_t)blockIdx.x * BELIEF_LANES;
  const int64_t k = kb + lane < K ? kb + lane : K - 1;   // (an idle lane repeats the last particle and stores nothing)
  const BeliefSeat qs = belief_seat(queries[qi]);
  const uint4 a = hands[(qi * K + k) * 2], b = hands[(qi * K + k) * 2 + 1];
  const uint64_t own = hand_at(a, b, qs.seat);
  uint64_t h[3] = {hand_at(a, b, (qs.seat + 1u) & 3u), hand_at(a, b, (qs.seat + 2u) & 3u), hand_at(a, b, (qs.seat + 3u) & 3u)};

  uint32_t r[4];
  philox4x32_10((uint32_t)k, stage_move, STREAM_BELIEF_MOVE, (uint32_t)stream_of[qi], k0, k1, r);
  const uint32_t pair = __umulhi(r[0], 3u);            // (h0, h1), (h0, h2), (h1, h2)
  const bool first0 = pair != 2u, second1 = pair == 0u;
  const uint64_t x = first0 ? h[0] : h[1], y = second1 ? h[1] : h[2];
  const uint64_t cx = nth_card(x, __umulhi(r[1], 13u)), cy = nth_card(y, __umulhi(r[2], 13u));
  if (cx != 0ull && cy != 0ull) {
    const uint64_t nx = (x ^ cx) | cy, ny = (y ^ cy) | cx;
    h[0] = first0 ? nx : h[0];
    h[1] = first0 ? (second1 ? ny : h[1]) : nx;
    h[2] = second1 ? h[2] : ny;
  }
  belief_empty_table(s_img + lane * BELIEF_IMG_STRIDE, qs, own, h);
  wave_lds_fence();
  belief_store_images(s_img, lane, p * K + kb, K - kb, tables_new, hands_new);
}

// ---- accept ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BELIEF_LANES) void k_belief_accept(const int32_t *list, const int64_t *stream_of, int64_t Q, int64_t K, uint32_t k0,
                                                                uint32_t k1, uint32_t stage_move, const uint4 *tables_new, const uint4 *hands_new,
                                                                const float *logl_new, const uint8_t *greedy_new, uint4 *tables, uint4 *hands,
                                                                float *logl, uint8_t *greedy, unsigned long long *counters) {
  const int lane = (int)threadIdx.x;
  const int64_t p = (int64_t)blockIdx.y, qi = (int64_t)list[p];
  if (qi < 0 || qi >= Q) return;
  const int64_t kb = (int64_t)blockIdx.x * BELIEF_LANES, k = kb + lane;
  const int64_t src0 = p * K + kb, dst0 = qi * K + kb;
  bool take = false;
  if (k < K) {
    uint32_t r[4];
    philox4x32_10((uint32_t)k, stage_move, STREAM_BELIEF_MOVE, (uint32_t)stream_of[qi], k0, k1, r);
    const float ln = logl_new[src0 + lane];
    take = log(unit_draw(r[3])) < (double)ln - (double)logl[dst0 + lane];   // (a NaN on either side: false)
    if (take) {
      logl[dst0 + lane] = ln;
      greedy[dst0 + lane] = greedy_new[src0 + lane];
    }
  }
  const uint64_t mask = __ballot(take);
#pragma unroll
  for (int it = 0; it < PIECES; it++) {
    const int i = it * BELIEF_LANES + lane;
    if ((mask >> (i >> 3)) & 1ull) tables[dst0 * PIECES + i] = tables_new[src0 * PIECES + i];
  }
#pragma unroll
  for (int it = 0; it < 2; it++) {
    const int i = it * BELIEF_LANES + lane;
    if ((mask >> (i >> 1)) & 1ull) hands[dst0 * 2 + i] = hands_new[src0 * 2 + i];
  }
  if (lane == 0) {
    atomicAdd(counters + qi * 2, (unsigned long long)(K - kb < BELIEF_LANES ? K - kb : BELIEF_LANES));
    atomicAdd(counters + qi * 2 + 1, (unsigned long long)__popcll(mask));
  }
}

bool shape_ok(int64_t L, int64_t Q, int64_t K) {
  return L > 0 && L <= BRL_BELIEF_SMC_MAX_LIST && Q > 0 && K > 0 && Q < ((int64_t)1 << 31) && K < ((int64_t)1 << 31) && Q * K < ((int64_t)1 << 31);
}

}  // namespace

#define ALIGNED16(a, b) (((((uintptr_t)(a)) | ((uintptr_t)(b))) & 15) == 0)

extern "C" int brl_belief_resample(int device, const int32_t *list, int64_t L, const int64_t *stream_of, int64_t Q, int64_t K, uint64_t seed,
                                   int64_t stage, const uint64_t *tables, const uint64_t *hands, const float *logl, const float *logw,
                                   const uint8_t *greedy, uint64_t *tables_out, uint64_t *hands_out, float *logl_out, float *logw_out,
                                   uint8_t *greedy_out, int32_t *ancestor, void *stream) {
  NEED(list && stream_of && tables && hands && logl && logw && greedy && tables_out && hands_out && logl_out && logw_out && greedy_out && ancestor,
       "NULL array");
  NEED(shape_ok(L, Q, K), "L (1 .. 65535), Q, K (>= 1, Q * K below 2^31)");
  NEED(stage >= 0 && stage < ((int64_t)1 << 24), "stage (0 .. 2^24 - 1)");
  NEED(ALIGNED16(tables, hands) && ALIGNED16(tables_out, hands_out), "tables / hands 16-byte aligned");
  NEED(tables != tables_out && hands != hands_out && logl != logl_out && logw != logw_out && greedy != greedy_out, "out of place");
  HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(k_belief_resample, dim3((unsigned)L), dim3(RS_THREADS), 0, (hipStream_t)stream, list, stream_of, Q, K, (uint32_t)seed,
                     (uint32_t)(seed >> 32), (uint32_t)stage, reinterpret_cast<const uint4 *>(tables), reinterpret_cast<const uint4 *>(hands), logl,
                     logw, greedy, reinterpret_cast<uint4 *>(tables_out), reinterpret_cast<uint4 *>(hands_out), logl_out, logw_out, greedy_out,
                     ancestor);
  HIP_TRY(hipGetLastError());
  return BRL_OK;
}

extern "C" int brl_belief_propose(int device, const brl_belief_query *queries, const int32_t *list, int64_t L, const int64_t *stream_of, int64_t Q,
                                  int64_t K, uint64_t seed, int64_t stage, int64_t move, const uint64_t *hands, uint64_t *tables_new,
                                  uint64_t *hands_new, void *stream) {
  NEED(queries && list && stream_of && hands && tables_new && hands_new, "NULL array");
  NEED(shape_ok(L, Q, K) && L * K < ((int64_t)1 << 31), "L (1 .. 65535), Q, K (>= 1, Q * K and L * K below 2^31)");
  NEED(stage >= 0 && stage < ((int64_t)1 << 24) && move >= 0 && move < BRL_BELIEF_SMC_MAX_MOVES, "stage (0 .. 2^24 - 1), move (0 .. 255)");
  NEED(ALIGNED16(queries, hands) && ALIGNED16(tables_new, hands_new), "queries / hands / tables_new / hands_new 16-byte aligned");
  HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(k_belief_propose, dim3((unsigned)((K + BELIEF_LANES - 1) / BELIEF_LANES), (unsigned)L), dim3(BELIEF_LANES), 0,
                     (hipStream_t)stream, reinterpret_cast<const uint4 *>(queries), list, stream_of, Q, K, (uint32_t)seed, (uint32_t)(seed >> 32),
                     (uint32_t)((stage << 8) | move), reinterpret_cast<const uint4 *>(hands), reinterpret_cast<uint4 *>(tables_new),
                     reinterpret_cast<uint4 *>(hands_new));
  HIP_TRY(hipGetLastError());
  return BRL_OK;
}

extern "C" int brl_belief_accept(int device, const int32_t *list, int64_t L, const int64_t *stream_of, int64_t Q, int64_t K, uint64_t seed,
                                 int64_t stage, int64_t move, const uint64_t *tables_new, const uint64_t *hands_new, const float *logl_new,
                                 const uint8_t *greedy_new, uint64_t *tables, uint64_t *hands, float *logl, uint8_t *greedy, uint64_t *counters,
                                 void *stream) {
  NEED(list && stream_of && tables_new && hands_new && logl_new && greedy_new && tables && hands && logl && greedy && counters, "NULL array");
  NEED(shape_ok(L, Q, K) && L * K < ((int64_t)1 << 31), "L (1 .. 65535), Q, K (>= 1, Q * K and L * K below 2^31)");
  NEED(stage >= 0 && stage < ((int64_t)1 << 24) && move >= 0 && move < BRL_BELIEF_SMC_MAX_MOVES, "stage (0 .. 2^24 - 1), move (0 .. 255)");
  NEED(ALIGNED16(tables, hands) && ALIGNED16(tables_new, hands_new) && (((uintptr_t)counters) & 7) == 0,
       "tables / hands / tables_new / hands_new 16-byte, counters 8-byte aligned");
  HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(k_belief_accept, dim3((unsigned)((K + BELIEF_LANES - 1) / BELIEF_LANES), (unsigned)L), dim3(BELIEF_LANES), 0,
                     (hipStream_t)stream, list, stream_of, Q, K, (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)((stage << 8) | move),
                     reinterpret_cast<const uint4 *>(tables_new), reinterpret_cast<const uint4 *>(hands_new), logl_new, greedy_new,
                     reinterpret_cast<uint4 *>(tables), reinterpret_cast<uint4 *>(hands), logl, greedy,
                     reinterpret_cast<unsigned long long *>(counters));
  HIP_TRY(hipGetLastError());
  return BRL_OK;
}
