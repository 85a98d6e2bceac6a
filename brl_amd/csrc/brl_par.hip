// brl_par.hip — translation unit of libbrl_hip.so: the double-dummy par (include/brl_par.h, which holds the definition).  The
// game over the 35 bids is a serial backward scan per board and short (70 outcomes, scored once), so a LANE solves one board — as
// k_board_records walks one table — and the wave moves its 64 x 20 contiguous input bytes and its 64 x 32 contiguous output
// bytes as whole 16-byte pieces through LDS.  contract_score (bridge_device.hpp) is the one scorer.  No floating point except
// imp.hpp's conversion, no atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/brl_par.h"
#include "abi_common.hpp"
#include "bridge_device.hpp"
#include "imp.hpp"

namespace {

using namespace brl;

constexpr int ROW = 20;                              // input bytes per board
constexpr int REC = (int)sizeof(brl_par_record);     // 32
constexpr int IN_CHUNKS = 64 * ROW / 16;             // 80 per wave
constexpr int INF = 1 << 30;                         // beyond every score (|score| <= 7600)
static_assert(REC == 32 && offsetof(brl_par_record, contracts_ns) == 16, "brl_par_record is 2 x 16 bytes");

// one side's tricks per strain (indexed by constants only: stays in registers, see reward_of's note)
struct Side {
  int t[5];
  int vul;
};

// o(s, b): North-South's score when the side plays level `level` in `den` — undoubled when it makes, doubled when it fails
__device__ __forceinline__ int outcome(const Side &s, int den, int level, int sign) {
  const int fails = s.t[den] < level + 6;
  return sign * contract_score(den, level, s.vul, fails, 0, s.t[den]);
}

// o(s, b) of every bid, computed once for both scans (indexed by constants only: 70 registers)
struct Outcomes {
  int ns[35], ew[35];
};

__device__ __forceinline__ Outcomes outcomes(const Side &ns, const Side &ew) {
  Outcomes o;
#pragma unroll
  for (int b = 0; b < 35; b++) {
    o.ns[b] = outcome(ns, b % 5, b / 5 + 1, 1);
    o.ew[b] = outcome(ew, b % 5, b / 5 + 1, -1);
  }
  return o;
}

struct Scan {
  int best_ns, best_ew;        // max_b V(NS, b), min_b V(EW, b)
  uint64_t mask_ns, mask_ew;   // P(NS), P(EW) for the par score r (MASKS only)
};

// the backward scan over b = 34..0: suf_ns = max_{b' > b} V(NS, b'), suf_ew = min_{b' > b} V(EW, b')
template <bool MASKS>
__device__ __forceinline__ Scan scan(const Outcomes &o, int r) {
  int suf_ns = -INF, suf_ew = INF;
  uint64_t mask_ns = 0, mask_ew = 0;
#pragma unroll
  for (int b = 34; b >= 0; b--) {
    if (MASKS) {
      mask_ns |= (o.ns[b] == r && suf_ew > r) ? (1ull << b) : 0ull;   // every overcall leaves East-West strictly worse off
      mask_ew |= (o.ew[b] == r && suf_ns < r) ? (1ull << b) : 0ull;
    }
    const int v_ns = min(o.ns[b], suf_ew), v_ew = max(o.ew[b], suf_ns);
    suf_ns = max(suf_ns, v_ns);
    suf_ew = min(suf_ew, v_ew);
  }
  return Scan{suf_ns, suf_ew, mask_ns, mask_ew};
}

__global__ __launch_bounds__(64) void k_par(const uint8_t *dda, const uint8_t *dealer, const uint8_t *vul, int64_t n, uint8_t *out) {
  __shared__ __attribute__((aligned(16))) uint8_t in_img[64 * ROW];
  __shared__ __attribute__((aligned(16))) uint8_t out_img[64 * REC];
  const int lane = (int)threadIdx.x;
  const int64_t board0 = (int64_t)blockIdx.x * 64, board = board0 + lane;
  const bool valid = board < n;
  const int64_t left = n - board0;
  const int boards = (int)(left < 64 ? left : 64);

  // the wave's rows are contiguous in memory: chunk k of the input is chunk k of the image.  The last wave's rows end on a
  // 4-byte boundary: whole 16-byte pieces first, then the dwords behind them — never a byte past row n - 1
  const int in_bytes = boards * ROW, whole = in_bytes >> 4, rest = (in_bytes & 15) >> 2;
  const uint8_t *src = dda + board0 * ROW;
#pragma unroll
  for (int i = 0; i < (IN_CHUNKS + 63) / 64; i++) {
    const int k = i * 64 + lane;
    if (k < whole) reinterpret_cast<uint4 *>(in_img)[k] = reinterpret_cast<const uint4 *>(src)[k];
  }
  if (lane < rest) reinterpret_cast<uint32_t *>(in_img)[whole * 4 + lane] = reinterpret_cast<const uint32_t *>(src)[whole * 4 + lane];
  const int dl = valid ? (int)dealer[board] & 3 : 0;
  const int vl = valid ? (int)vul[board] : 0;
  wave_lds_fence();

  // (an idle lane reads what the image holds, solves it and writes nothing)
  uint32_t w[5];
#pragma unroll
  for (int i = 0; i < 5; i++) w[i] = reinterpret_cast<const uint32_t *>(in_img)[lane * 5 + i];
  Side ns, ew;
#pragma unroll
  for (int den = 0; den < 5; den++) {
    int t[4];
#pragma unroll
    for (int seat = 0; seat < 4; seat++) {
      const int k = seat * 5 + den;
      t[seat] = (int)((w[k >> 2] >> ((k & 3) * 8)) & 15u);
    }
    ns.t[den] = max(t[0], t[2]);
    ew.t[den] = max(t[1], t[3]);
  }
  ns.vul = vl & 1;
  ew.vul = (vl >> 1) & 1;

  const Outcomes o = outcomes(ns, ew);
  const Scan a = scan<false>(o, 0);
  // the root: the first side bids its best contract or passes to the other side, which bids its best or passes the board out
  const int r_ns_first = max(a.best_ns, min(a.best_ew, 0)), r_ew_first = min(a.best_ew, max(a.best_ns, 0));
  const bool ns_deals = (dl & 1) == 0;
  const int r = ns_deals ? r_ns_first : r_ew_first, r_alt = ns_deals ? r_ew_first : r_ns_first;
  const Scan m = scan<true>(o, r);
  const uint32_t flags = ((r == 0 && (m.mask_ns | m.mask_ew) == 0) ? BRL_PAR_PASSED_OUT : 0u) | ((r != r_alt) ? BRL_PAR_DEALER_DEPENDENT : 0u);
  uint4 *rec16 = reinterpret_cast<uint4 *>(out_img + lane * REC);
  rec16[0] = make_uint4((uint32_t)r, (uint32_t)r_alt, flags, 0u);
  rec16[1] = make_uint4((uint32_t)m.mask_ns, (uint32_t)(m.mask_ns >> 32), (uint32_t)m.mask_ew, (uint32_t)(m.mask_ew >> 32));
  wave_lds_fence();

  // chunk k of the image is chunk k of the output
  const int chunks = boards * (REC / 16);
  uint4 *dst = reinterpret_cast<uint4 *>(out + board0 * REC);
#pragma unroll
  for (int i = 0; i < REC / 16; i++) {
    const int k = i * 64 + lane;
    if (k < chunks) dst[k] = reinterpret_cast<const uint4 *>(out_img)[k];
  }
}

__global__ __launch_bounds__(256) void k_par_imp(const brl_board_record *rec, const brl_par_record *par, int64_t n, int32_t sign,
                                                 int32_t *out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t flags = rec[i].flags;
  const bool result = (flags & BRL_BOARD_TERMINATED) != 0 && (flags & BRL_BOARD_ILLEGAL) == 0;
  const int32_t imp = (int32_t)imp_vector((float)rec[i].score_ns, (float)(-par[i].score_ns)).x;
  out[i] = result ? sign * imp : BRL_PAR_NO_RESULT;
}

}  // namespace

extern "C" int brl_par(int device, const uint8_t *dda, const uint8_t *dealer, const uint8_t *vul, int64_t n, brl_par_record *out,
                       void *stream) {
  NEED(dda && dealer && vul && out, "NULL array");
  NEED(n > 0 && n < ((int64_t)1 << 31), "n (1 .. 2^31)");
  NEED(((((uintptr_t)dda) | ((uintptr_t)out)) & 15) == 0, "dda / out 16-byte aligned");
  HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(k_par, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, (hipStream_t)stream, dda, dealer, vul, n,
                     reinterpret_cast<uint8_t *>(out));
  HIP_TRY(hipGetLastError());
  return BRL_OK;
}

extern "C" int brl_par_imp(int device, const brl_board_record *records, const brl_par_record *par, int64_t n, int32_t sign,
                           int32_t *out_imp, void *stream) {
  NEED(records && par && out_imp, "NULL array");
  NEED(n > 0 && n < ((int64_t)1 << 31), "n (1 .. 2^31)");
  NEED(sign == 1 || sign == -1, "sign (+1 or -1)");
  HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(k_par_imp, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, records, par, n, sign, out_imp);
  HIP_TRY(hipGetLastError());
  return BRL_OK;
}
