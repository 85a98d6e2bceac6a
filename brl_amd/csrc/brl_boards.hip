// brl_boards.hip — translation unit of libbrl_hip.so: the board records (include/brl_boards.h).  A packed table keeps its auction
// as a set of events; k_board_records turns it back into the sequence of calls and adds the contract, the declarer, the deal's
// tricks and the duplicate score, all from bridge_device.hpp's own functions.  The event walk is serial per table and short (at
// most 109 events), so a LANE walks one table — 64 walks per wave instead of the per-step kernels' K — into a record image in
// LDS, and the wave then writes its 64 x 368 contiguous bytes as whole 16-byte stores.  No floating point, no atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/brl_boards.h"
#include "abi_common.hpp"
#include "bridge_device.hpp"
#include "imp.hpp"

namespace {

using namespace brl;

constexpr int REC = (int)sizeof(brl_board_record);   // 368
constexpr int REC_CHUNKS = REC / 16;                 // 23
constexpr int CALLS_OFF = 48;
static_assert(REC == 368 && REC % 16 == 0, "brl_board_record is 23 x 16 bytes");
static_assert(offsetof(brl_board_record, calls) == CALLS_OFF && offsetof(brl_board_record, hands) == 16, "record layout");

constexpr uint64_t HIST_W0 = ~0xFull;                // bits 0..3 of word 0 are unused
constexpr uint64_t HIST_W6 = (1ull << 44) - 1ull;    // the history ends at bit 8 + 12 * 35 = 428 = 6 * 64 + 44

struct Hist {
  uint64_t w[7];   // (indexed by constants only: stays in registers)
};

__device__ __forceinline__ bool hist_test(const Hist &h, int g) {
  bool r = false;
#pragma unroll
  for (int i = 0; i < 7; i++) r = ((g >> 6) == i) ? (((h.w[i] >> (g & 63)) & 1ull) != 0) : r;
  return r;
}

__device__ __forceinline__ void hist_clear(Hist &h, int g, bool doit) {
#pragma unroll
  for (int i = 0; i < 7; i++) h.w[i] &= ~((doit && (g >> 6) == i) ? (1ull << (g & 63)) : 0ull);
}

// the walk's cursor: the next call goes to calls[pos]; `prev` is the seat of the last call that was an event
struct Cursor {
  uint8_t *calls;
  int pos, prev;
};

__device__ __forceinline__ void put(Cursor &c, int call) {
  if (c.pos < BRL_BOARD_MAX_CALLS) c.calls[c.pos] = (uint8_t)call;   // (a table of garbage can ask for more: never past the row)
  c.pos++;
}

// the events of one history word, ascending: (passes by the seats in between, then the call)
__device__ __forceinline__ void walk_word(Cursor &c, uint64_t x, int base) {
  while (x) {
    const int e = base + __ffsll((unsigned long long)x) - 1 - 8;   // event index: 12 per bid
    x &= x - 1ull;
    const int bid = e / 12, r = e - bid * 12, kind = r >> 2, seat = r & 3;
    const int gap = (seat - c.prev - 1) & 3;
    for (int k = 0; k < gap; k++) put(c, 0);
    put(c, kind == 0 ? 3 + bid : kind);   // bid / 1 double / 2 redouble
    c.prev = seat;
  }
}

__global__ __launch_bounds__(64) void k_board_records(const uint64_t *state, int64_t n, uint8_t *records) {
  __shared__ __attribute__((aligned(16))) uint8_t img[64 * REC];
  const int lane = (int)threadIdx.x;
  const int64_t table0 = (int64_t)blockIdx.x * 64, table = table0 + lane;
  const bool valid = table < n;
  // the fill value everywhere; headers, hands and calls are written over it
  uint4 *img16 = reinterpret_cast<uint4 *>(img);
#pragma unroll
  for (int i = 0; i < REC_CHUNKS; i++) img16[i * 64 + lane] = make_uint4(~0u, ~0u, ~0u, ~0u);
  wave_lds_fence();

  const uint64_t *src = state + (valid ? table : 0) * 16;   // (an idle lane reads table 0 and writes nothing)
  Hist h;
#pragma unroll
  for (int i = 0; i < 7; i++) h.w[i] = src[W_HIST + i];
  h.w[0] &= HIST_W0;
  h.w[6] &= HIST_W6;
  uint64_t hands[4];
#pragma unroll
  for (int s = 0; s < 4; s++) hands[s] = src[W_HAND + s] >> 4;
  Tbl t;
  load_scalars(t, reinterpret_cast<const uint8_t *>(src));

  const int dealer = (int)bits(t.sc, SC_DEALER, 2), turn = (int)bits(t.sch, SCH_TURN, 9);
  const uint32_t lb1 = bits(t.sc, SC_LB1, 6);
  const bool term = bits(t.sc, SC_TERM, 1), illegal = bits(t.sc, SC_ILLEGAL, 1);
  const bool dbl = bits(t.sc, SC_X, 1) | bits(t.sc, SC_XX, 1);
  const bool lost = illegal && !dbl && lb1 != 0;   // an illegal bid overwrote _last_bid (brl_boards.h)
  const int actor = (dealer + turn - 1) & 3;       // who made the illegal call
  if (illegal && lb1 != 0) {   // drop the illegal call's own history bit (brl_boards.h: which bits cannot be legal ones)
    const int g = 8 + 12 * ((int)lb1 - 1);
    const bool own = ((actor ^ (int)bits(t.sc, SC_LBSEAT, 2)) & 1) == 0;
    hist_clear(h, g + 8 + actor, true);
    hist_clear(h, g + 4 + actor, own || hist_test(h, g + 4 + (actor ^ 2)));
  }

  Cursor c;
  c.calls = img + lane * REC + CALLS_OFF;
  c.pos = 0;
  const int opening = __popc((uint32_t)(h.w[0] >> 4) & 15u);
  for (int k = 0; k < opening; k++) put(c, 0);
  c.prev = (dealer + opening - 1) & 3;
  const bool events = (h.w[0] >> 8) | h.w[1] | h.w[2] | h.w[3] | h.w[4] | h.w[5] | h.w[6];
  walk_word(c, h.w[0] & ~0xFFull, 0);
  walk_word(c, h.w[1], 64);
  walk_word(c, h.w[2], 128);
  walk_word(c, h.w[3], 192);
  walk_word(c, h.w[4], 256);
  walk_word(c, h.w[5], 320);
  walk_word(c, h.w[6], 384);
  // the passes behind the last event: the table's own count, or — it was reset by an illegal call — up to the actor's seat
  const int tail = illegal ? ((actor - c.prev - 1) & 3) : (events ? (int)bits(t.sc, SC_PASS, 3) : 0);   // (no event: the passes are the opening's)
  for (int k = 0; k < tail; k++) put(c, 0);

  const int want = illegal ? turn - 1 : (term ? turn + 1 : turn);
  const bool ok = !lost && c.pos == want && c.pos < BRL_BOARD_MAX_CALLS;
  int n_calls = lost ? 0 : (c.pos < BRL_BOARD_MAX_CALLS ? c.pos : BRL_BOARD_MAX_CALLS - 1);
  if (lost)   // (the row of a table without a record is all fill)
    for (int k = 0; k < BRL_BOARD_MAX_CALLS; k += 4) *reinterpret_cast<uint32_t *>(c.calls + k) = ~0u;

  // the contract: terminal_reward's own arithmetic (declarer = first of the side to name the strain, contract_score)
  const bool contract = term && !illegal && lb1 != 0;
  const int b = contract ? (int)lb1 - 1 : 0;
  const int level0 = (b * 13) >> 6, den = b - level0 * 5;
  const int side = (int)bits(t.sc, SC_LBSEAT, 2) & 1;
  const int decl = ((int)bits(t.fd, side * 15 + den * 3, 3) - 1) & 3;
  const int tricks = trick_nibble(t, decl, den);
  Tbl u = t;
  terminal_reward(u);   // rewards by player id; North's player holds North-South's score
  const int score_ns = contract ? reward_of(u, player_at(u, 0)) : 0;
  const uint32_t flags = (term ? BRL_BOARD_TERMINATED : 0u) | ((term && !illegal && lb1 == 0) ? BRL_BOARD_PASSED_OUT : 0u) |
                         (illegal ? BRL_BOARD_ILLEGAL : 0u) | (ok ? BRL_BOARD_OK : 0u);
  const uint32_t doubled = contract ? (bits(t.sc, SC_XX, 1) ? 2u : bits(t.sc, SC_X, 1)) : 0u;
  const uint32_t w0 = (uint32_t)n_calls | ((uint32_t)dealer << 16) | (bits(t.sc, SC_VULNS, 1) << 24);
  const uint32_t w1 = bits(t.sc, SC_VULEW, 1) | (flags << 8) | ((contract ? (uint32_t)level0 + 1u : 0u) << 16) | ((contract ? (uint32_t)den : 0u) << 24);
  const uint32_t w2 = doubled | ((contract ? (uint32_t)decl : 0u) << 8) | ((contract ? (uint32_t)tricks : 0u) << 16) | (bits(t.sc, SC_SHUF, 8) << 24);
  uint4 *rec16 = reinterpret_cast<uint4 *>(img + lane * REC);
  rec16[0] = make_uint4(w0, w1, w2, (uint32_t)score_ns);
  rec16[1] = make_uint4((uint32_t)hands[0], (uint32_t)(hands[0] >> 32), (uint32_t)hands[1], (uint32_t)(hands[1] >> 32));
  rec16[2] = make_uint4((uint32_t)hands[2], (uint32_t)(hands[2] >> 32), (uint32_t)hands[3], (uint32_t)(hands[3] >> 32));
  wave_lds_fence();

  // the wave's records are contiguous in memory: chunk k of the image is chunk k of the output
  const int64_t left = n - table0;
  const int chunks = (int)(left < 64 ? left : 64) * REC_CHUNKS;
  uint4 *dst = reinterpret_cast<uint4 *>(records + table0 * REC);
#pragma unroll
  for (int i = 0; i < REC_CHUNKS; i++) {
    const int k = i * 64 + lane;
    if (k < chunks) dst[k] = img16[k];
  }
}

__global__ __launch_bounds__(256) void k_board_imp(const brl_board_record *a, const brl_board_record *b, int64_t n, int32_t *out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  // table A's North-South pair sits East-West at table B: its score there is -score_ns
  out[i] = (int32_t)imp_vector((float)a[i].score_ns, (float)(-b[i].score_ns)).x;
}

__global__ __launch_bounds__(256) void k_board_keep_a(const uint64_t *state, uint64_t *prev, const int32_t *action, const uint8_t *a_done,
                                                      uint8_t *taken, uint64_t *final_a, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (!taken[i] && a_done[i]) {
    // the row passes through memory as uint64 only; the scalar words go through a local image, so that their layout stays
    // load_scalars' / store_scalars' (bridge_device.hpp)
    __attribute__((aligned(8))) uint64_t row[16];   // (indexed by constants only: registers)
#pragma unroll
    for (int k = 0; k < 16; k++) row[k] = prev[i * 16 + k];
    Tbl t;
    load_scalars(t, reinterpret_cast<const uint8_t *>(row));
    const int a = action[i];
    const int hb = ((uint32_t)a < 38u) ? table_step(t, a) : -1;
#pragma unroll
    for (int k = 0; k < W_HAND; k++)   // the call's history bit, as the step kernels OR it into their image
      row[k] |= (hb >= 0 && (hb >> 6) == k) ? (1ull << (hb & 63)) : 0ull;
    store_scalars(t, reinterpret_cast<uint8_t *>(row));
#pragma unroll
    for (int k = 0; k < 16; k++) final_a[i * 16 + k] = row[k];
    taken[i] = 1;
  }
#pragma unroll
  for (int k = 0; k < 16; k++) prev[i * 16 + k] = state[i * 16 + k];
}

}  // namespace

extern "C" int brl_board_records(int device, const uint64_t *state, int64_t n, brl_board_record *records, void *stream) {
  NEED(state && records, "NULL array");
  NEED(n > 0 && n < ((int64_t)1 << 31), "n (1 .. 2^31)");
  NEED((((uintptr_t)records) & 15) == 0 && (((uintptr_t)state) & 7) == 0, "records 16-byte aligned, state 8-byte aligned");
  HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(k_board_records, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, (hipStream_t)stream, state, n,
                     reinterpret_cast<uint8_t *>(records));
  HIP_TRY(hipGetLastError());
  return BRL_OK;
}

extern "C" int brl_board_imp(int device, const brl_board_record *records_a, const brl_board_record *records_b, int64_t n,
                             int32_t *out_imp, void *stream) {
  NEED(records_a && records_b && out_imp, "NULL array");
  NEED(n > 0 && n < ((int64_t)1 << 31), "n (1 .. 2^31)");
  NEED(((((uintptr_t)records_a) | ((uintptr_t)records_b)) & 7) == 0 && (((uintptr_t)out_imp) & 3) == 0, "records 8-byte aligned, out_imp 4-byte");
  HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(k_board_imp, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, records_a, records_b, n, out_imp);
  HIP_TRY(hipGetLastError());
  return BRL_OK;
}

extern "C" int brl_board_keep_a(int device, const uint64_t *state, uint64_t *prev, const int32_t *action, const uint8_t *a_done,
                                uint8_t *taken, uint64_t *final_a, int64_t n, void *stream) {
  NEED(state && prev && action && a_done && taken && final_a, "NULL array");
  NEED(n > 0 && n < ((int64_t)1 << 31), "n (1 .. 2^31)");
  NEED(((((uintptr_t)state) | ((uintptr_t)prev) | ((uintptr_t)final_a)) & 15) == 0 && (((uintptr_t)action) & 3) == 0,
       "state / prev / final_a 16-byte aligned, action 4-byte");
  HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(k_board_keep_a, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, state, prev, action, a_done,
                     taken, final_a, n);
  HIP_TRY(hipGetLastError());
  return BRL_OK;
}
