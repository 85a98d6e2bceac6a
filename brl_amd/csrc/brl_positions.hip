// brl_positions.hip — translation unit of libbrl_hip.so: the position queries (include/brl_positions.h, which holds the definition).
// k_position_rows: a one-wave block takes 64 positions.  A lane checks one position, deals the 39 other cards, builds the empty
// table in its LDS image (belief_table.hpp) and replays the auction with table_step, the scalars in registers and the history
// bits in the image; the wave then writes the 64 observation and mask rows with brl_observe's emitters and the 64 tables as whole
// 16-byte pieces.  k_position_answers: eight lanes per row — categorical<8> (policy_common.hpp) in mode form for the call, the
// float64 p_a / L_a of policy_dist.hpp (the system diff's), the entropy in the same two-level order, the top list by rank counting;
// an answer is put together in LDS and leaves as six 16-byte stores.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/brl_positions.h"
#include "abi_common.hpp"
#include "belief_table.hpp"
#include "bridge_device.hpp"
#include "policy_common.hpp"
#include "policy_dist.hpp"

namespace {

using namespace brl;

static_assert(sizeof(brl_position) == 64 && offsetof(brl_position, dealer) == 8 && offsetof(brl_position, n_calls) == 11 &&
                  offsetof(brl_position, reserved) == 12 && offsetof(brl_position, calls) == 16,
              "position layout");
static_assert(sizeof(brl_position_answer) == 96 && offsetof(brl_position_answer, value) == 4 && offsetof(brl_position_answer, entropy) == 8 &&
                  offsetof(brl_position_answer, top_action) == 16 && offsetof(brl_position_answer, top_prob) == 24 &&
                  offsetof(brl_position_answer, reserved) == 88,
              "answer layout");
static_assert(BRL_POS_ACTIONS == BRL_NUM_ACTIONS && BRL_POS_OBS_BYTES == BRL_OBS_SIZE && BRL_POS_MAX_TOP == ROW_LANES, "constants");

constexpr uint64_t DECK = (1ull << 52) - 1;
constexpr int POS_CHUNKS = (int)sizeof(brl_position) / 16;             // 4
constexpr int ANS_CHUNKS = (int)sizeof(brl_position_answer) / 16;      // 6
constexpr int CALL_BYTES = BRL_POS_MAX_CALLS;                          // a lane's calls in LDS: three 16-byte pieces
constexpr uint32_t IDENTITY_SEATING = 0xE4u;                           // player id at seat s = s

// ---- the rows -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BELIEF_LANES) void k_position_rows(const uint4 *positions, int64_t n, uint8_t *obs, uint8_t *mask, uint64_t *legal,
                                                                uint32_t *status, uint4 *tables) {
  __shared__ __attribute__((aligned(16))) uint8_t s_img[BELIEF_LANES * BELIEF_IMG_STRIDE];
  __shared__ __attribute__((aligned(16))) uint8_t s_calls[BELIEF_LANES * CALL_BYTES];
  const LaneConst c = make_lane_const();
  const int lane = c.lane;
  const int64_t row0 = (int64_t)blockIdx.x * BELIEF_LANES;
  const int count = (int)(n - row0 < BELIEF_LANES ? n - row0 : BELIEF_LANES);
  const int64_t row = lane < count ? row0 + lane : n - 1;   // (an idle lane repeats the last position and stores nothing)

  // phase one: this lane's position
  const uint4 hd = positions[row * POS_CHUNKS];
  uint4 cv[3];
#pragma unroll
  for (int k = 0; k < 3; k++) cv[k] = positions[row * POS_CHUNKS + 1 + k];
  uint8_t *my_calls = s_calls + lane * CALL_BYTES, *img = s_img + lane * BELIEF_IMG_STRIDE;
#pragma unroll
  for (int k = 0; k < 3; k++) reinterpret_cast<uint4 *>(my_calls)[k] = cv[k];
  const uint64_t hand = (uint64_t)hd.x | ((uint64_t)hd.y << 32);
  const uint32_t dealer = hd.z & 0xFFu, vns = (hd.z >> 8) & 0xFFu, vew = (hd.z >> 16) & 0xFFu, n_calls = hd.z >> 24;
  bool header = dealer <= 3u && vns <= 1u && vew <= 1u && n_calls <= (uint32_t)BRL_POS_MAX_CALLS && hd.w == 0u;
  const uint32_t cw[12] = {cv[0].x, cv[0].y, cv[0].z, cv[0].w, cv[1].x, cv[1].y, cv[1].z, cv[1].w, cv[2].x, cv[2].y, cv[2].z, cv[2].w};
#pragma unroll
  for (int j = 0; j < BRL_POS_MAX_CALLS; j++) {
    const uint32_t b = (cw[j >> 2] >> (8 * (j & 3))) & 0xFFu;
    header &= ((uint32_t)j < n_calls) ? b < (uint32_t)BRL_NUM_ACTIONS : b == (uint32_t)BRL_POS_FILL;
  }
  const bool cards = (hand >> 52) == 0ull && __popcll((unsigned long long)hand) == 13;
  uint32_t st = !header ? (uint32_t)BRL_POS_BAD_HEADER : (!cards ? (uint32_t)BRL_POS_BAD_HAND : (uint32_t)BRL_POS_OK);

  // the empty table: the caller's hand at its seat, the other 39 cards in ascending card id to the next three seats
  const bool go = st == (uint32_t)BRL_POS_OK;
  const uint32_t seat = go ? (dealer + n_calls) & 3u : 0u;
  const uint64_t own = go ? hand : 0ull;
  uint64_t rest = go ? (~hand & DECK) : 0ull, h[3];
#pragma unroll
  for (int s = 0; s < 3; s++) {
    h[s] = 0ull;
#pragma unroll 1
    for (int i = 0; i < 13; i++) {
      const uint64_t low = rest & (0ull - rest);
      h[s] |= low;
      rest ^= low;
    }
  }
  const BeliefSeat qs = {seat, go ? dealer : 0u, go ? vns : 0u, go ? vew : 0u, IDENTITY_SEATING};
  belief_empty_table(img, qs, own, h);
  Tbl t;
  load_scalars(t, img);

  // the auction, by table_step: the scalars in registers, the history bits into the image
  const int len = go ? (int)n_calls : 0;
#pragma unroll 1
  for (int j = 0; j < len; j++) {
    const int a = (int)my_calls[j];   // (checked above: 0..37)
    if (bits(t.sc, SC_TERM, 1)) {     // calls behind the closing pass
      st = (uint32_t)BRL_POS_FINISHED | ((uint32_t)(j - 1) << 8);
      break;
    }
    if (!((legal_mask(t) >> a) & 1ull)) {
      st = (uint32_t)BRL_POS_ILLEGAL_CALL | ((uint32_t)j << 8);
      break;
    }
    const int hb = table_step(t, a);
    if (hb >= 0) img[hb >> 3] |= (uint8_t)(1u << (hb & 7));
  }
  if (st == (uint32_t)BRL_POS_OK && bits(t.sc, SC_TERM, 1)) st = (uint32_t)BRL_POS_FINISHED | ((uint32_t)(len - 1) << 8);

  const bool ok = st == (uint32_t)BRL_POS_OK;
  uint64_t lg = 0ull;
  uint32_t pack = 0u;   // observer seat | vulnerability nibble << 2; 0 with a zero image: an all-zero row
  if (ok) {
    store_scalars(t, img);
    const int oseat = cur_seat(t);
    lg = legal_mask(t);
    pack = (uint32_t)oseat | (vul_nibble(t, oseat) << 2);
  } else {
    uint4 *z = reinterpret_cast<uint4 *>(img);
#pragma unroll
    for (int k = 0; k < TABLE_BYTES / 16; k++) z[k] = make_uint4(0u, 0u, 0u, 0u);
  }
  if (lane < count) {
    legal[row] = lg;
    status[row] = st;
  }
  wave_lds_fence();

  // phase two: the wave's rows, by brl_observe's emitters, and its tables as whole 16-byte pieces
#pragma unroll 1
  for (int j = 0; j < count; j++) {
    const uint32_t p = __builtin_amdgcn_readlane(pack, j);
    emit_obs_row(s_img + j * BELIEF_IMG_STRIDE, (int)(p & 3u), p >> 2, obs + (row0 + j) * BRL_OBS_SIZE, c);
    emit_mask_row(readlane64(lg, j), mask + (row0 + j) * BRL_NUM_ACTIONS, c);
  }
  if (tables != nullptr) {
#pragma unroll
    for (int it = 0; it < TABLE_BYTES / 16; it++) {
      const int q = it * BELIEF_LANES + lane, smp = q >> 3, piece = q & 7;
      const uint4 v = *reinterpret_cast<const uint4 *>(s_img + smp * BELIEF_IMG_STRIDE + piece * 16);
      if (smp < count) tables[row0 * (TABLE_BYTES / 16) + q] = v;
    }
  }
}

// ---- the answers --------------------------------------------------------------------------------------------------------------------
constexpr int ANS_ROWS = 4 * ROW_LANES;   // rows of a 256-thread block

__global__ __launch_bounds__(256) void k_position_answers(const float *logits, int64_t ld, const float *value, int64_t value_stride,
                                                          const uint64_t *legal, const uint32_t *status, int64_t n, int top_k, uint4 *answers,
                                                          double *probs) {
  __shared__ __attribute__((aligned(16))) uint8_t s_ans[ANS_ROWS * sizeof(brl_position_answer)];
  const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6), tl = lane % ROW_LANES, slot = lane / ROW_LANES;
  const int64_t j = ((int64_t)blockIdx.x * 4 + wave) * ROW_LANES + tl;
  const bool in = j < n;
  const bool valid = in && (status[j] & 0xFFu) == (uint32_t)BRL_POS_OK;
  const uint64_t cand = valid ? (legal[j] & ALL_ACTIONS) : 1ull;
  const int64_t off = valid ? j * ld : 0;
  float mode_lp;
  const int call = categorical<ROW_LANES>(logits, off, 0, valid, cand, 1, 0u, lane, mode_lp);
  double p[NI], L[NI];
  bool bad;
  net_dist(logits + off, cand, call, slot, tl, p, L, bad);
  double own = 0.0;
  {
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < NI; i++) {
      const double term = p[i] * (-L[i]);
      own += (p[i] > 0.0) ? term : 0.0;
    }
  }
  const double entropy = slot_sum(own, tl);
  const int n_legal = __popcll((unsigned long long)cand);
  const int k = bad ? 0 : (top_k < n_legal ? top_k : n_legal);

  // rank(a) of this lane's actions, by counting over the row's 38
  int rank[NI] = {0, 0, 0, 0, 0};
#pragma unroll
  for (int s = 0; s < 64 / ROW_LANES; s++) {
#pragma unroll
    for (int i = 0; i < NI; i++) {
      const double pb = __shfl(p[i], s * ROW_LANES + tl, 64);
      const int b = s * NI + i;
      const bool legal_b = b < BRL_NUM_ACTIONS && ((cand >> (b & 63)) & 1ull);
#pragma unroll
      for (int q = 0; q < NI; q++) {
        const int a = slot * NI + q;
        rank[q] += (legal_b && (pb > p[q] || (pb == p[q] && b < a))) ? 1 : 0;
      }
    }
  }

  // the answer, put together in LDS: the fixed fields and the empty top list, then the ranked actions into their slots
  uint8_t *ans = s_ans + (wave * ROW_LANES + tl) * sizeof(brl_position_answer);
  const double nan = (double)NAN;
  if (slot == 0) {
    const float v = (valid && value != nullptr) ? value[j * value_stride] : 0.0f;
    const uint32_t w0 = valid ? ((uint32_t)call | ((uint32_t)n_legal << 8) | ((bad ? (uint32_t)BRL_POS_NONFINITE : 0u) << 16) | ((uint32_t)k << 24)) : 255u;
    *reinterpret_cast<uint2 *>(ans) = make_uint2(w0, __float_as_uint(v));
    *reinterpret_cast<double *>(ans + offsetof(brl_position_answer, entropy)) = valid ? (bad ? nan : entropy) : 0.0;
  } else if (slot == 1) {
    *reinterpret_cast<uint64_t *>(ans + offsetof(brl_position_answer, top_action)) = valid ? ~0ull : 0ull;
  } else if (slot == 2) {
    *reinterpret_cast<uint64_t *>(ans + offsetof(brl_position_answer, reserved)) = 0ull;
  }
  reinterpret_cast<double *>(ans + offsetof(brl_position_answer, top_prob))[slot] = (valid && bad) ? nan : 0.0;
  wave_lds_fence();
#pragma unroll
  for (int q = 0; q < NI; q++) {
    const int a = slot * NI + q;
    const bool is_legal = a < BRL_NUM_ACTIONS && ((cand >> (a & 63)) & 1ull);
    if (valid && is_legal && rank[q] < k) {   // (ranks are distinct: one writer per slot)
      ans[offsetof(brl_position_answer, top_action) + rank[q]] = (uint8_t)a;
      reinterpret_cast<double *>(ans + offsetof(brl_position_answer, top_prob))[rank[q]] = p[q];
    }
    if (in && probs != nullptr && a < BRL_NUM_ACTIONS) probs[j * BRL_NUM_ACTIONS + a] = !valid ? 0.0 : (bad ? nan : (is_legal ? p[q] : 0.0));
  }
  wave_lds_fence();
  if (in && slot < ANS_CHUNKS) answers[j * ANS_CHUNKS + slot] = reinterpret_cast<const uint4 *>(ans)[slot];
}

}  // namespace

extern "C" int brl_position_rows(int device, const brl_position *positions, int64_t n, uint8_t *obs, uint8_t *mask, uint64_t *legal,
                                 uint32_t *status, uint64_t *tables, void *stream) {
  NEED(positions && obs && mask && legal && status, "NULL array");
  NEED(n > 0 && n < ((int64_t)1 << 31), "n (1 .. 2^31)");
  NEED(((((uintptr_t)positions) | ((uintptr_t)tables)) & 15) == 0 && ((((uintptr_t)obs) | ((uintptr_t)legal)) & 7) == 0 &&
           (((uintptr_t)status) & 3) == 0,
       "positions / tables 16-byte, obs / legal 8-byte, status 4-byte aligned");
  HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(k_position_rows, dim3((unsigned)((n + BELIEF_LANES - 1) / BELIEF_LANES)), dim3(BELIEF_LANES), 0, (hipStream_t)stream,
                     reinterpret_cast<const uint4 *>(positions), n, obs, mask, legal, status, reinterpret_cast<uint4 *>(tables));
  HIP_TRY(hipGetLastError());
  return BRL_OK;
}

extern "C" int brl_position_answers(int device, const float *logits, int64_t ld, const float *value, int64_t value_stride,
                                    const uint64_t *legal, const uint32_t *status, int64_t n, int top_k, brl_position_answer *answers,
                                    double *probs, void *stream) {
  NEED(logits && legal && status && answers, "NULL array");
  NEED(n > 0 && n < ((int64_t)1 << 31), "n (1 .. 2^31)");
  NEED(ld >= BRL_POS_ACTIONS && ld < ((int64_t)1 << 20), "ld (38 ..)");
  NEED(value_stride >= 0 && value_stride < ((int64_t)1 << 20), "value_stride (0 ..)");
  NEED(top_k >= 1 && top_k <= BRL_POS_MAX_TOP, "top_k (1 .. 8)");
  NEED(((((uintptr_t)logits) | ((uintptr_t)value) | ((uintptr_t)status)) & 3) == 0 && ((((uintptr_t)legal) | ((uintptr_t)probs)) & 7) == 0 &&
           (((uintptr_t)answers) & 15) == 0,
       "logits / value / status 4-byte, legal / probs 8-byte, answers 16-byte aligned");
  HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(k_position_answers, dim3((unsigned)((n + ANS_ROWS - 1) / ANS_ROWS)), dim3(256), 0, (hipStream_t)stream, logits, ld, value,
                     value_stride, legal, status, n, top_k, reinterpret_cast<uint4 *>(answers), probs);
  HIP_TRY(hipGetLastError());
  return BRL_OK;
}
