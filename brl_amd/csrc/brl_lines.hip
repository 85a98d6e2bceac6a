// brl_lines.hip — translation unit of libbrl_hip.so: the auction lines (include/brl_lines.h, which holds the definition).
// k_lines_expand is one step of a beam search over auctions: a WAVE takes one board.  Per live line a lane takes one action:
// the float64 masked log-softmax (line_log_softmax: the sums run over the lanes in index order through readlane, so the order of
// operations is the definition's), the rank of every child among its siblings, and the line's K first children go to a candidate
// list in LDS — K + 1 entries per slot, the last one for a finished or void line as itself.  Every candidate then counts the
// candidates that precede it under the total order (at most 272 broadcast reads of LDS per candidate, 5 candidates per lane), the
// ones with fewer than K predecessors are the new beam, and the wave builds them: 16 lanes a table word each, table_step for the
// scalar words, max_calls lanes a call each.  No atomics, no cross-lane float reduction whose order depends on timing.
// k_lines_finish reads a finished table as k_board_records does; k_lines_imp is the K x K sum of the expected IMP.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/brl_lines.h"
#include "abi_common.hpp"
#include "bridge_device.hpp"
#include "imp.hpp"

namespace {

using namespace brl;

constexpr int ACTIONS = 38;
constexpr int MAXK = BRL_LINES_MAX_K;
constexpr int CANDS = MAXK * (MAXK + 1);   // 272
constexpr int EXPAND_WAVES = 4;            // boards per 256-thread block of k_lines_expand, one per wave
constexpr uint32_t NONE = 0xFFFFu;
constexpr uint32_t DEAD = BRL_LINE_EMPTY | BRL_LINE_FINISHED | BRL_LINE_VOID;
static_assert(sizeof(brl_line_request) == 16 && sizeof(brl_line_result) == 16 && sizeof(brl_lines_board) == 64, "lines layouts");

__device__ __forceinline__ float lane_f32(float v, int src) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src)); }

__device__ __forceinline__ double lane_f64(double v, int src) {
  const uint64_t u = (uint64_t)__double_as_longlong(v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)u, src);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(u >> 32), src);
  return __longlong_as_double((long long)((uint64_t)lo | ((uint64_t)hi << 32)));
}

// The term of include/brl_lines.h on the lanes of a wave: lane a < 38 holds logit l of action a, `legal` is wave-uniform.
// Returns term(lane) (meaningful on the legal lanes); `greedy`: the evaluators' masked arg-max of the row (policy_common.hpp's
// mode: first strict float32 maximum over the legal actions, a NaN never, none -> 0); `void_row`: the row has no distribution.
// Every sum is sequential in index order and identical on all lanes.
struct Terms {
  double term;
  int greedy;
  bool void_row;
};

__device__ __forceinline__ Terms line_log_softmax(float l, uint64_t legal, int lane) {
  float mx = -INFINITY;
  int amax = 64;
  bool bad = false;
  for (int a = 0; a < ACTIONS; a++) {
    const float v = lane_f32(l, a);
    const bool in = (legal >> a) & 1ull;
    bad |= in && (v != v || v == INFINITY);
    if (in && v > mx) {   // first maximum wins, like argmax; false for a NaN
      mx = v;
      amax = a;
    }
  }
  bad |= mx == -INFINITY;
  const bool mine = lane < ACTIONS && ((legal >> (lane & 63)) & 1ull);
  const double d = (double)l - (double)mx;
  const double e = mine ? exp(d) : 0.0;
  double z = 0.0;
  for (int a = 0; a < ACTIONS; a++) {
    const double v = lane_f64(e, a);
    z = ((legal >> a) & 1ull) ? z + v : z;
  }
  Terms r;
  r.term = d - log(z);
  r.greedy = amax >= ACTIONS ? 0 : amax;
  r.void_row = bad;
  return r;
}

// candidate d precedes candidate c: void lines last, score descending, then (parent slot, action) ascending
__device__ __forceinline__ bool precedes(uint32_t vd, double sd, uint32_t kd, uint32_t vc, double sc, uint32_t kc) {
  return vd != vc ? vd < vc : (sd > sc || (sd == sc && kd < kc));
}

struct BeamIn {
  const uint64_t *tables;
  const uint8_t *calls;
  const double *score;
  const uint8_t *flags;
};

struct BeamOut {
  uint64_t *tables;
  uint8_t *calls;
  double *score;
  uint8_t *flags;
  brl_line_request *request;
  uint8_t *done;
};

__global__ __launch_bounds__(64 * EXPAND_WAVES) void k_lines_expand(BeamIn in, int64_t n, int K, int max_calls, const float *logits1,
                                                                    int64_t ldo1, const float *logits2, int64_t ldo2, BeamOut out) {
  __shared__ double c_score[EXPAND_WAVES][CANDS];
  __shared__ uint16_t c_key[EXPAND_WAVES][CANDS];   // parent slot << 6 | action + 1 (0: the line itself); NONE: no candidate
  __shared__ uint8_t c_bits[EXPAND_WAVES][CANDS];   // bit 0 void, bit 1 greedy
  __shared__ uint16_t sel[EXPAND_WAVES][MAXK];      // the candidate in slot r of the new beam; NONE: empty
  const int lane = (int)(threadIdx.x & 63u), wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t b = (int64_t)blockIdx.x * EXPAND_WAVES + wave;
  // (everything below is per wave and wave-uniform unless it names `lane`: the waves of a block share nothing and never meet at
  // a barrier)
  if (b >= n) return;
  double *cs = c_score[wave];
  uint16_t *ck = c_key[wave];
  uint8_t *cb = c_bits[wave];
  uint16_t *sl = sel[wave];
  const int per = K + 1, nc = K * per;
  if (lane < K) sl[lane] = (uint16_t)NONE;

  // ---- the candidates: per slot its K first children, or the line itself
  for (int s = 0; s < K; s++) {
    const int64_t line = b * K + s;
    const uint32_t f = (uint32_t)__builtin_amdgcn_readfirstlane((int)in.flags[line]);
    const int base = s * per;
    Tbl t;
    load_scalars(t, reinterpret_cast<const uint8_t *>(in.tables + line * 16));
    const double parent = in.score[line];
    bool self = (f & DEAD) != 0;
    uint32_t self_void = (f & BRL_LINE_VOID) ? 1u : 0u;
    int n_children = 0;
    if (!self) {   // (wave-uniform)
      const uint64_t legal = legal_mask(t);
      const int team = cur_player(t) >> 1;
      const float *row = team ? logits2 + line * ldo2 : logits1 + line * ldo1;
      const float l = row[lane < ACTIONS ? lane : 0];
      const Terms T = line_log_softmax(l, legal, lane);
      if (T.void_row) {
        self = true;
        self_void = 1u;
      } else {
        const bool mine = lane < ACTIONS && ((legal >> (lane & 63)) & 1ull);
        const double child = parent + T.term;
        int r = 0;
        for (int a = 0; a < ACTIONS; a++) {
          const double v = lane_f64(child, a);
          r += (((legal >> a) & 1ull) && (v > child || (v == child && a < lane))) ? 1 : 0;
        }
        if (mine && r < K) {
          cs[base + r] = child;
          ck[base + r] = (uint16_t)((s << 6) | (lane + 1));
          cb[base + r] = (uint8_t)(((f & BRL_LINE_GREEDY) && lane == T.greedy) ? 2u : 0u);
        }
        n_children = __popcll(legal & ALL_ACTIONS);
      }
    }
    if (lane < K && lane >= n_children) ck[base + lane] = (uint16_t)NONE;
    if (lane == 0) {
      const bool there = self && !(f & BRL_LINE_EMPTY);
      cs[base + K] = parent;
      ck[base + K] = (uint16_t)(there ? (uint32_t)(s << 6) : NONE);
      cb[base + K] = (uint8_t)(self_void | ((f & BRL_LINE_GREEDY) ? 2u : 0u));
    }
  }
  wave_lds_fence();

  // ---- the K first of the candidates: each one counts those that precede it
  for (int c = lane; c < nc; c += 64) {
    const uint32_t kc = ck[c];
    if (kc == NONE) continue;
    const double sc = cs[c];
    const uint32_t vc = cb[c] & 1u;
    int before = 0;
    for (int d = 0; d < nc; d++) {
      const uint32_t kd = ck[d];
      before += (kd != NONE && d != c && precedes(cb[d] & 1u, cs[d], kd, vc, sc, kc)) ? 1 : 0;
    }
    if (before < K) sl[before] = (uint16_t)c;
  }
  wave_lds_fence();

  // ---- the new beam
  bool any_live = false;
  for (int r = 0; r < K; r++) {
    const int64_t oline = b * K + r;
    const uint32_t ci = (uint32_t)__builtin_amdgcn_readfirstlane((int)sl[r]);
    if (ci == NONE || ci >= (uint32_t)nc) {
      if (lane < 16) out.tables[oline * 16 + lane] = 0ull;
      if (lane < max_calls) out.calls[oline * max_calls + lane] = (uint8_t)BRL_LINES_FILL;
      if (lane == 0) {
        out.score[oline] = -INFINITY;
        out.flags[oline] = (uint8_t)BRL_LINE_EMPTY;
        *reinterpret_cast<int4 *>(out.request + oline) = make_int4(-1, r, 0, 0);
      }
      continue;
    }
    const uint32_t key = ck[ci], bits_c = cb[ci];
    const int p = (int)(key >> 6) & (MAXK - 1), a = (int)(key & 63u) - 1;
    const int64_t pline = b * K + (p < K ? p : 0);
    const uint64_t *src = in.tables + pline * 16;
    Tbl t;
    load_scalars(t, reinterpret_cast<const uint8_t *>(src));
    const int len = (int)bits(t.sch, SCH_STEP, 10);
    uint64_t w = src[lane < 16 ? lane : 0];
    int hb = -1;
    if (a >= 0) hb = table_step(t, a < ACTIONS ? a : 0);
    // the scalar words as load_scalars' / store_scalars' layout has them; the call's history bit, as the step kernels OR it
    const uint64_t w11 = (uint64_t)t.sc | ((uint64_t)t.sch << 32), w12 = (uint64_t)t.fd | ((uint64_t)t.t2 << 32);
    const uint64_t w13 = (uint64_t)t.t0 | ((uint64_t)t.t1 << 32), w14 = (uint64_t)t.lut | ((uint64_t)t.bctr << 32);
    const uint64_t w15 = (uint64_t)t.r01 | ((uint64_t)t.r23 << 32);
    w = lane == 11 ? w11 : (lane == 12 ? w12 : (lane == 13 ? w13 : (lane == 14 ? w14 : (lane == 15 ? w15 : w))));
    w |= (lane < W_HAND && hb >= 0 && (hb >> 6) == lane) ? (1ull << (hb & 63)) : 0ull;
    if (lane < 16) out.tables[oline * 16 + lane] = w;
    if (lane < max_calls) {
      const uint8_t call = in.calls[pline * max_calls + lane];
      out.calls[oline * max_calls + lane] = (a >= 0 && lane == len) ? (uint8_t)a : call;
    }
    const uint32_t nf = (bits(t.sc, SC_TERM, 1) ? (uint32_t)BRL_LINE_FINISHED : 0u) | ((bits_c & 1u) ? (uint32_t)BRL_LINE_VOID : 0u) |
                        ((bits_c & 2u) ? (uint32_t)BRL_LINE_GREEDY : 0u);
    const bool live = (nf & DEAD) == 0;
    any_live |= live;
    if (lane == 0) {
      const int player = cur_player(t);
      out.score[oline] = cs[ci];
      out.flags[oline] = (uint8_t)nf;
      *reinterpret_cast<int4 *>(out.request + oline) = live ? make_int4((int)b, r, player, player >> 1) : make_int4(-1, r, 0, 0);
    }
  }
  if (lane == 0) out.done[b] = any_live ? 0 : 1;
}

__global__ __launch_bounds__(256) void k_lines_init(const uint64_t *state, int64_t n, int K, int max_calls, BeamOut out) {
  const int64_t line = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (line >= n * K) return;
  const int64_t b = line / K;
  const int s = (int)(line - b * K);
  Tbl t;
  load_scalars(t, reinterpret_cast<const uint8_t *>(state + b * 16));
  const bool term = bits(t.sc, SC_TERM, 1);
#pragma unroll
  for (int k = 0; k < 16; k++) out.tables[line * 16 + k] = s == 0 ? state[b * 16 + k] : 0ull;
  for (int k = 0; k < max_calls; k++) out.calls[line * max_calls + k] = (uint8_t)BRL_LINES_FILL;
  out.score[line] = s == 0 ? 0.0 : -INFINITY;
  out.flags[line] = (uint8_t)(s == 0 ? (BRL_LINE_GREEDY | (term ? BRL_LINE_FINISHED : 0)) : BRL_LINE_EMPTY);
  const bool live = s == 0 && !term;
  const int player = cur_player(t);
  *reinterpret_cast<int4 *>(out.request + line) = live ? make_int4((int)b, s, player, player >> 1) : make_int4(-1, s, 0, 0);
  if (s == 0) out.done[b] = term ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_lines_finish(const uint64_t *tables, const uint8_t *flags, int64_t lines, brl_line_result *results) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= lines) return;
  Tbl t;
  load_scalars(t, reinterpret_cast<const uint8_t *>(tables + i * 16));
  const uint32_t f = flags[i];
  const bool has = (f & BRL_LINE_FINISHED) && !(f & (BRL_LINE_VOID | BRL_LINE_EMPTY)) && bits(t.sc, SC_TERM, 1) && !bits(t.sc, SC_ILLEGAL, 1);
  // the contract: terminal_reward's own arithmetic, as k_board_records reads it (declarer = first of the side to name the strain)
  const uint32_t lb1 = bits(t.sc, SC_LB1, 6);
  const bool contract = has && lb1 != 0;
  const int bb = contract ? (int)lb1 - 1 : 0;
  const int level0 = (bb * 13) >> 6, den = bb - level0 * 5;
  const int side = (int)bits(t.sc, SC_LBSEAT, 2) & 1;
  const int decl = ((int)bits(t.fd, side * 15 + den * 3, 3) - 1) & 3;
  const int tricks = trick_nibble(t, decl, den);
  Tbl u = t;
  terminal_reward(u);   // rewards by player id; North's player holds North-South's score
  const int score_ns = contract ? reward_of(u, player_at(u, 0)) : 0;
  const uint32_t doubled = contract ? (bits(t.sc, SC_XX, 1) ? 2u : bits(t.sc, SC_X, 1)) : 0u;
  const uint32_t w1 = (has ? 1u : 0u) | ((contract ? (uint32_t)level0 + 1u : 0u) << 8) | ((contract ? (uint32_t)den : 0u) << 16) | (doubled << 24);
  const uint32_t w2 = (contract ? (uint32_t)decl : 0u) | ((contract ? (uint32_t)tricks : 0u) << 8);
  const int score_team1 = contract ? reward_of(u, 0) : 0;
  *reinterpret_cast<uint4 *>(results + i) = make_uint4((uint32_t)score_ns, w1, w2, (uint32_t)score_team1);
}

constexpr int IMP_THREADS = 64;

__global__ __launch_bounds__(IMP_THREADS) void k_lines_imp(const double *score_a, const uint8_t *flags_a, const brl_line_result *res_a,
                                                           const double *score_b, const uint8_t *flags_b, const brl_line_result *res_b,
                                                           int64_t n, int K, brl_lines_board *boards) {
  __shared__ double pa[MAXK][IMP_THREADS], pb[MAXK][IMP_THREADS];   // a finished line's probability, 0.0 for any other line
  __shared__ float sa[MAXK][IMP_THREADS], sb[MAXK][IMP_THREADS];    // its score from player 0's side
  const int tid = (int)threadIdx.x;
  const int64_t b = (int64_t)blockIdx.x * IMP_THREADS + tid;
  if (b >= n) return;   // (a thread reads only its own column of the arrays: no barrier)
  double mass[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // covered, open, void of A; of B (indexed by constants only)
#pragma unroll
  for (int tb = 0; tb < 2; tb++) {
    const double *score = tb ? score_b : score_a;
    const uint8_t *flags = tb ? flags_b : flags_a;
    const brl_line_result *res = tb ? res_b : res_a;
    double covered = 0.0, open = 0.0, voided = 0.0;
    for (int s = 0; s < K; s++) {
      const int64_t line = b * K + s;
      const uint32_t f = flags[line];
      const double p = (f & BRL_LINE_EMPTY) ? 0.0 : exp(score[line]);
      const bool fin = (f & DEAD) == BRL_LINE_FINISHED && res[line].has_result != 0;
      covered += fin ? p : 0.0;
      open += (f & DEAD) == 0 ? p : 0.0;
      voided += (f & BRL_LINE_VOID) && !(f & BRL_LINE_EMPTY) ? p : 0.0;
      (tb ? pb : pa)[s][tid] = fin ? p : 0.0;
      (tb ? sb : sa)[s][tid] = fin ? (float)res[line].score_team1 : 0.0f;
    }
    mass[3 * tb] = covered;
    mass[3 * tb + 1] = open;
    mass[3 * tb + 2] = voided;
  }
  // player 0's two results, as k_eval_step hands them to imp_vector
  auto term = [&](int i, int j) { return (pa[i][tid] * pb[j][tid]) * (double)imp_vector(sa[i][tid], sb[j][tid]).x; };
  double S = 0.0;
  for (int m = 0; m < K; m++) {
    S += term(m, m);
    for (int j = 0; j < m; j++) S += term(m, j) + term(j, m);
  }
  double *o = reinterpret_cast<double *>(boards + b);
  o[0] = S;
  o[1] = mass[0] * mass[3];
  o[2] = mass[0];
  o[3] = mass[3];
  o[4] = mass[1];
  o[5] = mass[4];
  o[6] = mass[2];
  o[7] = mass[5];
}

int beam_args_ok(int64_t n, int32_t k, int32_t max_calls) {
  return n > 0 && k >= 1 && k <= BRL_LINES_MAX_K && max_calls >= 1 && max_calls <= BRL_LINES_MAX_CALLS && n * k < ((int64_t)1 << 31);
}

}  // namespace

extern "C" int brl_lines_init(int device, const uint64_t *state, int64_t n, int32_t k, int32_t max_calls, uint64_t *tables, uint8_t *calls,
                              double *score, uint8_t *flags, brl_line_request *request, uint8_t *done, void *stream) {
  NEED(state && tables && calls && score && flags && request && done, "NULL array");
  NEED(beam_args_ok(n, k, max_calls), "n > 0, 1 <= k <= 16, 1 <= max_calls <= 64, n * k below 2^31");
  NEED(((((uintptr_t)state) | ((uintptr_t)tables) | ((uintptr_t)score)) & 7) == 0 && (((uintptr_t)request) & 15) == 0,
       "state / tables / score 8-byte aligned, request 16-byte aligned");
  HIP_TRY(hipSetDevice(device));
  const BeamOut out{tables, calls, score, flags, request, done};
  hipLaunchKernelGGL(k_lines_init, dim3((unsigned)((n * k + 255) / 256)), dim3(256), 0, (hipStream_t)stream, state, n, (int)k, (int)max_calls, out);
  HIP_TRY(hipGetLastError());
  return BRL_OK;
}

extern "C" int brl_lines_expand(int device, const uint64_t *tables, const uint8_t *calls, const double *score, const uint8_t *flags,
                                int64_t n, int32_t k, int32_t max_calls, const float *logits1, int64_t ldo1, const float *logits2,
                                int64_t ldo2, uint64_t *out_tables, uint8_t *out_calls, double *out_score, uint8_t *out_flags,
                                brl_line_request *request, uint8_t *done, void *stream) {
  NEED(tables && calls && score && flags && logits1 && logits2, "NULL beam / logits");
  NEED(out_tables && out_calls && out_score && out_flags && request && done, "NULL output");
  NEED(beam_args_ok(n, k, max_calls), "n > 0, 1 <= k <= 16, 1 <= max_calls <= 64, n * k below 2^31");
  NEED(ldo1 >= BRL_NUM_ACTIONS && ldo2 >= BRL_NUM_ACTIONS, "logits stride (>= 38)");
  NEED(tables != out_tables && calls != out_calls && score != out_score && flags != out_flags, "the next beam needs memory of its own");
  NEED(((((uintptr_t)tables) | ((uintptr_t)out_tables) | ((uintptr_t)score) | ((uintptr_t)out_score)) & 7) == 0 &&
           (((uintptr_t)request) & 15) == 0 && (((((uintptr_t)logits1) | ((uintptr_t)logits2))) & 3) == 0,
       "tables / score 8-byte aligned, request 16-byte aligned, logits 4-byte aligned");
  HIP_TRY(hipSetDevice(device));
  const BeamIn in{tables, calls, score, flags};
  const BeamOut out{out_tables, out_calls, out_score, out_flags, request, done};
  hipLaunchKernelGGL(k_lines_expand, dim3((unsigned)((n + EXPAND_WAVES - 1) / EXPAND_WAVES)), dim3(64 * EXPAND_WAVES), 0, (hipStream_t)stream,
                     in, n, (int)k, (int)max_calls, logits1, ldo1, logits2, ldo2, out);
  HIP_TRY(hipGetLastError());
  return BRL_OK;
}

extern "C" int brl_lines_finish(int device, const uint64_t *tables, const uint8_t *flags, int64_t lines, brl_line_result *results,
                                void *stream) {
  NEED(tables && flags && results, "NULL array");
  NEED(lines > 0 && lines < ((int64_t)1 << 31), "lines (1 .. 2^31)");
  NEED((((uintptr_t)tables) & 7) == 0 && (((uintptr_t)results) & 15) == 0, "tables 8-byte aligned, results 16-byte aligned");
  HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(k_lines_finish, dim3((unsigned)((lines + 255) / 256)), dim3(256), 0, (hipStream_t)stream, tables, flags, lines, results);
  HIP_TRY(hipGetLastError());
  return BRL_OK;
}

extern "C" int brl_lines_imp(int device, const double *score_a, const uint8_t *flags_a, const brl_line_result *results_a,
                             const double *score_b, const uint8_t *flags_b, const brl_line_result *results_b, int64_t n, int32_t k,
                             brl_lines_board *boards, void *stream) {
  NEED(score_a && flags_a && results_a && score_b && flags_b && results_b && boards, "NULL array");
  NEED(n > 0 && k >= 1 && k <= BRL_LINES_MAX_K && n * k < ((int64_t)1 << 31), "n > 0, 1 <= k <= 16, n * k below 2^31");
  NEED(((((uintptr_t)score_a) | ((uintptr_t)score_b) | ((uintptr_t)boards)) & 7) == 0 &&
           ((((uintptr_t)results_a) | ((uintptr_t)results_b)) & 15) == 0,
       "score / boards 8-byte aligned, results 16-byte aligned");
  HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(k_lines_imp, dim3((unsigned)((n + IMP_THREADS - 1) / IMP_THREADS)), dim3(IMP_THREADS), 0, (hipStream_t)stream, score_a,
                     flags_a, results_a, score_b, flags_b, results_b, n, (int)k, boards);
  HIP_TRY(hipGetLastError());
  return BRL_OK;
}
