// policy_dist.hpp — one network's float64 distribution over a row's legal actions on the eight lanes that share the row
// (include/brl_compare.h holds the definition): the one copy brl_compare.hip (k_compare_rows) and brl_positions.hip
// (k_position_answers) share.  Lane layout: categorical<8>'s (policy_common.hpp) — lane l: row l % 8, slot l / 8, and slot k
// holds the five actions 5 k .. 5 k + 4.
#pragma once
#include <math.h>
#include <stdint.h>

#include "policy_common.hpp"

namespace brl {

constexpr int ROW_LANES = 8;    // lanes per row: categorical<8>
constexpr int NI = 5;           // actions per lane: slot k holds 5 k .. 5 k + 4

// the eight slot values of a row added in ascending slot order; the same bits on every lane of the row
__device__ __forceinline__ double slot_sum(double own, int tl) {
#pragma clang fp contract(off)
  double s = __shfl(own, tl, 64);
#pragma unroll
  for (int k = 1; k < 64 / ROW_LANES; k++) s += __shfl(own, k * ROW_LANES + tl, 64);
  return s;
}

__device__ __forceinline__ bool row_any(bool x) {
  int v = x ? 1 : 0;
#pragma unroll
  for (int off = ROW_LANES; off < 64; off <<= 1) v |= __shfl_xor(v, off, 64);
  return v != 0;
}

// p_a and L_a = log p_a of this lane's five actions (brl_compare.h); `bad`: the network's NONFINITE condition, row-wide
__device__ __forceinline__ void net_dist(const float *row, uint64_t legal, int amax, int slot, int tl, double p[NI], double L[NI],
                                         bool &bad) {
#pragma clang fp contract(off)
  const double m = (double)row[amax];
  float lf[NI];
#pragma unroll
  for (int i = 0; i < NI; i++) lf[i] = row[min(slot * NI + i, BRL_NUM_ACTIONS - 1)];
  double x[NI], e[NI], own = 0.0;
  bool nonfinite = false, live = false;
#pragma unroll
  for (int i = 0; i < NI; i++) {
    const int a = slot * NI + i;
    const bool ok = a < BRL_NUM_ACTIONS && ((legal >> (a & 63)) & 1ull);
    nonfinite |= ok && (lf[i] != lf[i] || lf[i] == INFINITY);
    live |= ok && lf[i] > -INFINITY;
    x[i] = (double)lf[i] - m;
    e[i] = ok ? exp(x[i]) : 0.0;
    own += e[i];
  }
  const double S = slot_sum(own, tl), logS = log(S);
#pragma unroll
  for (int i = 0; i < NI; i++) {
    p[i] = e[i] / S;
    L[i] = x[i] - logS;
  }
  bad = row_any(nonfinite) || !row_any(live);
}

}  // namespace brl
