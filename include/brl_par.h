/*
 * brl_par.h — C-ABI of the double-dummy par (brl_amd/csrc/brl_par.hip, part of libbrl_hip.so): a deal's double-dummy table,
 * dealer and vulnerability in, one fixed-size par record per board out — the par score, the par contracts of either side —
 * and the IMP of a board record (brl_boards.h) against its par.
 *
 * Kept apart from brl_hip.h like brl_boards.h and brl_book.h: these entry points have no oracle counterpart; brl_version() does
 * not count them.
 *
 * Conventions are brl_hip.h's: 0 on success, <0 (BRL_E_*) on error with the message in brl_last_error(); every pointer is a
 * device pointer on `device`; `stream` is a hipStream_t passed as void*; nothing synchronises.  No handle, no atomics, no
 * floating point except imp.hpp's conversion, the same bytes on every run.
 *
 * The definition.
 *
 * T[seat][strain] is the double-dummy trick count.  Seats N,E,S,W are 0..3 and strains C,D,H,S,NT are 0..4.  This is the
 * layout of Deals.tricks and BoardRecords.dda.  Sides are NS = 0 and EW = 1.  A contract is a bid index b = 0..34 with
 * level = b / 5 + 1 and strain = b % 5.
 *
 *   - Tricks of a side.  tricks(s, b) = max of T over the side's two seats for strain.  The side declares from its better
 *     seat.
 *   - Outcome.  o(s, b) is North-South's score when side s plays b.  With at least level + 6 tricks it is the UNDOUBLED
 *     making score.  Otherwise it is the DOUBLED penalty.  The side's own vulnerability applies.  The sign is + for NS and
 *     - for EW.  There are never redoubles.  (contract_score, csrc/bridge_device.hpp, is the one scorer.)
 *   - Game.  NS maximises and EW minimises.  V(s, b) is the value when s holds b and the other side s' is to act.  s' either
 *     passes, which gives o(s, b), or bids any b' > b, which gives V(s', b').  So
 *         V(NS, b) = min(o(NS, b), min_{b' > b} V(EW, b'))   and   V(EW, b) = max(o(EW, b), max_{b' > b} V(NS, b')).
 *   - Root.  The dealer's side d acts first.  It bids some b, giving V(d, b), or it passes.  After a pass the other side bids
 *     some b, giving V(d', b), or passes the board out for 0.  Par score R = the root's value for the board's dealer.
 *     R_alt = the same with the other side first.
 *   - Par contracts.  P(s) = the bids b with o(s, b) == R for which every V(s', b') with b' > b is STRICTLY worse for s'
 *     than R.  These are the contracts that score par and that the other side cannot overcall without losing.
 *
 * How it is computed.  One backward scan over b = 34..0 carries the two suffix optima max_{b' > b} V(NS, b') and
 * min_{b' > b} V(EW, b'); its end gives both roots.  A second scan, R known, sets bit b of a side's mask where o(s, b) == R
 * and the other side's suffix optimum is strictly on R's far side.
 *
 * Input values are not trusted: a trick count is taken & 15 and a dealer & 3, vul's bits above 1 are ignored, so that no
 * input can index out of bounds.  (A count of 14 or 15 is scored as that many tricks.)
 */
#ifndef BRL_PAR_H
#define BRL_PAR_H

#include <stdint.h>

#include "brl_boards.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BRL_PAR_PASSED_OUT 1         /* flags: R == 0 and no par contract */
#define BRL_PAR_DEALER_DEPENDENT 2   /*        R != R_alt */

#define BRL_PAR_NO_RESULT INT32_MIN  /* brl_par_imp: the record holds no result */

/* 32 bytes = 2 x 16, little endian, no padding */
typedef struct brl_par_record {
  int32_t score_ns;       /* R, North-South's side */
  int32_t score_ns_alt;   /* R_alt */
  uint32_t flags;         /* BRL_PAR_* */
  uint32_t zero;
  uint64_t contracts_ns;  /* bit b: b in P(NS), for the board's dealer; bits 35.. zero */
  uint64_t contracts_ew;  /* bit b: b in P(EW) */
} brl_par_record;

/* out[i] of board i < n: dda uint8 [n,20] (T[seat * 5 + strain]), dealer uint8 [n], vul uint8 [n] (bit 0: North-South
 * vulnerable, bit 1: East-West), out brl_par_record [n].  dda and out are 16-byte aligned; 1 <= n < 2^31.  One launch, a
 * board per lane: the wave moves its 64 x 20 input bytes and its 64 x 32 output bytes as whole 16-byte pieces through LDS. */
int brl_par(int device, const uint8_t *dda, const uint8_t *dealer, const uint8_t *vul, int64_t n, brl_par_record *out,
            void *stream);

/* out_imp[i] (int32) = sign * IMP(records[i].score_ns - par[i].score_ns), i < n: the IMP (src/duplicate.py:15-70) that the
 * pair sitting North-South at the record's table wins against par (sign = +1) or the pair sitting East-West (sign = -1).
 * BRL_PAR_NO_RESULT for a record that is not BRL_BOARD_TERMINATED or that is BRL_BOARD_ILLEGAL.  One launch, a thread per
 * board. */
int brl_par_imp(int device, const brl_board_record *records, const brl_par_record *par, int64_t n, int32_t sign,
                int32_t *out_imp, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* BRL_PAR_H */
