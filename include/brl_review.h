/*
 * brl_review.h — C-ABI of the call review (brl_amd/csrc/brl_review.hip, part of libbrl_hip.so): the board records of one table
 * of a duplicate match in, one branch table per (decision, alternative call) out; and, once those tables have been played to
 * the end by the evaluators' loop, the IMP every alternative would have won for the caller's side, with a summary per decision.
 *
 * Kept apart from brl_hip.h like brl_boards.h, brl_book.h and brl_par.h: these entry points have no oracle counterpart;
 * brl_version() does not count them.
 *
 * Conventions are brl_hip.h's: 0 on success, <0 (BRL_E_*) on error with the message in brl_last_error(); every pointer is a
 * device pointer on `device`; `stream` is a hipStream_t passed as void*; nothing synchronises.  No handle, no atomics, no
 * floating point except imp.hpp's conversion, the same bytes on every run.
 *
 * What a review is.  Hindsight on the ACTUAL deal under the policies' OWN continuations: at a decision of the recorded auction
 * every alternative call is tried, both sides then go on with their networks' greedy calls (the evaluators' masked arg-max), and
 * the result is scored against the recorded result of the other table.  It is not a double-dummy judgement of the call, and it
 * does not see the deal from the caller's information state.
 *
 * The definition.
 *
 *   - Reviewable record.  One with BRL_BOARD_OK and without BRL_BOARD_ILLEGAL.  A live (unfinished) record is reviewed like any
 *     other, up to its n_calls.  Every other record contributes no decision.
 *   - Decision.  (record i, call index t) for every t < min(n_calls, depth).  Decisions are numbered record by record, t
 *     ascending: decision d = first[i] + t, where first[] is the exclusive prefix sum of min(n_calls, depth) over the records
 *     (0 for a record that is not reviewable).
 *   - Caller and team.  The caller's seat is (dealer + t) & 3; its side is North-South when the seat is even.  The team is
 *     ((seating >> 2 * seat) & 3) >> 1 (players {0,1} are team 0).
 *   - Branch.  Slot d * 38 + a holds, for action a = 0..37, the empty table of the record's deal — its seating, dealer,
 *     vulnerabilities and hands, the board's 20 double-dummy tricks (dda row, [declarer seat][C,D,H,S,NT]), no table index
 *     (0xFFFFFFFF), board counter 0 — stepped with calls[0..t) and then with a, by bridge_device.hpp's table_step.  If a ends
 *     the auction the branch is final at birth.
 *   - Void.  An alternative that is not legal at the decision.  table_step ends such a table at once (SC_TERMINATED,
 *     SC_ILLEGAL): the evaluators' loop never forwards it, and the illegal bit is the void mark.  A branch table that is not
 *     terminated when it is read has no result and counts as void too.
 *   - Value.  S' = the North-South score of the branch's final table (terminal_reward, csrc/bridge_device.hpp), S_o =
 *     score_ns of the same board's record at the OTHER table.  The IMP to North-South at the reviewed table is conv(S' - S_o),
 *     brl_board_imp's conversion (imp.hpp); it holds for both tables because conv is odd.  The value is that number, negated
 *     when the caller sits East-West: -24 .. 24.  BRL_REVIEW_VOID for a void slot.
 *   - Summary.  played = calls[t]; n_legal = the slots that are not void; played_imp = the value of slot `played`; best_imp =
 *     the maximum over the slots that are not void; best = played if it attains the maximum, otherwise the lowest action that
 *     does; loss = best_imp - played_imp >= 0.
 *
 * Input values are not trusted: a dealer is taken & 3, a vulnerability & 1, a trick count & 15, a call above 37 is taken as a
 * pass, a record's decisions are at most first[i + 1] - first[i] and at most BRL_BOARD_MAX_CALLS, and every write is guarded
 * by the range it was asked for: a record of garbage cannot write outside its own slots.
 */
#ifndef BRL_REVIEW_H
#define BRL_REVIEW_H

#include <stdint.h>

#include "brl_boards.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BRL_REVIEW_ACTIONS 38   /* slots per decision */
#define BRL_REVIEW_VOID (-128)  /* value of a void slot */

/* 16 bytes, little endian, no padding */
typedef struct brl_review_decision {
  int32_t board;        /* index of the record */
  uint16_t call_index;  /* t */
  uint8_t seat;         /* the caller's seat N,E,S,W = 0..3 */
  uint8_t team;         /* the caller's team, 0 = players {0,1} */
  uint8_t played;       /* calls[t] */
  uint8_t zero[7];
} brl_review_decision;

/* 8 bytes, no padding */
typedef struct brl_review_summary {
  uint8_t played;
  uint8_t n_legal;
  int8_t played_imp;
  int8_t best_imp;
  uint8_t best;
  uint8_t loss;
  uint8_t zero[2];
} brl_review_summary;

/* The decisions d0 <= d < d1 of one table's records: decisions[d - d0] and the 38 branch tables tables[(d - d0) * 38 + a]
 * (uint64 [16] each).  records brl_board_record [n], dda uint8 [n,20], first int64 [n + 1] (see above; the caller computes it
 * from the records' bytes), depth >= 1, 0 <= d0 < d1, (d1 - d0) * 38 < 2^31; decisions and tables 16-byte aligned.  One launch,
 * a wave per record: one lane walks the record's calls from a record image in LDS, keeping the prefix table in a table image;
 * at every t in range the wave derives the prefix's 38 children and stores them as whole 16-byte pieces. */
int brl_review_expand(int device, const brl_board_record *records, const uint8_t *dda, int64_t n, int32_t depth, const int64_t *first,
                      int64_t d0, int64_t d1, brl_review_decision *decisions, uint64_t *tables, void *stream);

/* values[d * 38 + a] (int8) and summary[d] of the decisions d < nd: tables uint64 [nd * 38, 16] as the evaluators' loop left
 * them, decisions [nd] as brl_review_expand wrote them, other brl_board_record [n]: the OTHER table's records (a decision whose
 * board is not below n is scored against 0).  One launch, a wave per decision and a lane per slot; the maximum, the tie rule
 * and the loss are wave reductions.  Integer only, except imp.hpp's conversion. */
int brl_review_reduce(int device, const uint64_t *tables, const brl_review_decision *decisions, int64_t nd, const brl_board_record *other,
                      int64_t n, int8_t *values, brl_review_summary *summary, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* BRL_REVIEW_H */
