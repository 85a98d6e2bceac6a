/*
 * brl_boards.h — C-ABI of the board records (brl_amd/csrc/brl_boards.hip, part of libbrl_hip.so): packed tables in, one
 * fixed-size record per table out — the auction as a sequence of calls, the contract, the declarer, the deal's tricks and the
 * duplicate score — and the IMP of a board from the records of its two tables.
 *
 * Kept apart from brl_hip.h like brl_sl.h and brl_league.h: these entry points have no oracle counterpart; brl_version() does
 * not count them.
 *
 * Conventions are brl_hip.h's: 0 on success, <0 (BRL_E_*) on error with the message in brl_last_error(); every pointer is a
 * device pointer on `device`; `stream` is a hipStream_t passed as void*; nothing synchronises.  No handle, no atomics, the
 * same bytes on every run.
 *
 * How the sequence is rebuilt.  A packed table (uint64 [16], csrc/bridge_device.hpp) stores the auction as a SET — bit
 * 4 + s: seat s passed before the opening; 8 + 12 b + s: seat s made bid b; + 4: doubled it; + 8: redoubled it — and the calls
 * after the last of these events as a count (_pass_num).  Seats act in rotation, so the set has one order only:
 *   - the opening passes are made by the seats dealer, dealer + 1, ...: their number is the number of bits 4..7;
 *   - bids strictly increase, so the bids are made in bit order; a bid's double follows it, its redouble follows the double,
 *     and the next bid comes after them: ascending bit order IS the order of the events;
 *   - between two consecutive events by seats a and b lie (b - a - 1) & 3 passes (fewer would be the wrong seat, four more
 *     would have ended the auction);
 *   - after the last event come _pass_num passes.
 * The walk is at most 4 + 35 * 3 events and at most 319 calls (3 passes + 35 x (bid P P X P P XX P P) + the final pass).
 *
 * Self-check (BRL_BOARD_OK).  The rebuilt number of calls is compared with the table's own counter:
 *   - a live table:                                 n_calls == _turn
 *   - a table whose auction ended (no illegal call): n_calls == _turn + 1   (the call that ends an auction does not advance
 *                                                                             _turn: auction_step, csrc/bridge_device.hpp)
 *   - a table ended by an illegal call:             n_calls == _turn - 1   (the calls BEFORE the illegal one; see below)
 * and the walk must stay inside the 319 calls.  A record without BRL_BOARD_OK is not a record of an auction.
 *
 * Tables ended by an illegal call (SC_ILLEGAL).  table_step applies the call to the table before it flags it: _turn counts
 * it, _pass_num is reset by it, and an illegal double / redouble of a bid on the table sets its history bit.  The record
 * holds the L = _turn - 1 calls before it: the illegal actor is seat s = (dealer + L) & 3, and
 *   - a redouble bit of the last bid by s is never a legal one (after a legal redouble s acts again only behind a new bid):
 *     it is dropped;
 *   - a double bit of the last bid by s is dropped when s sits on the bidder's side, or when s's partner doubled that bid
 *     too (a legal auction doubles a bid once); otherwise it is s's own earlier, legal double;
 *   - the passes behind the last event are (s - seat of the last event - 1) & 3.
 * An illegal BID (too low) overwrites _last_bid and cannot be told from the history: such a table (SC_ILLEGAL with neither
 * _call_x nor _call_xx set and a bid on the table) gets n_calls = 0, an all-fill call row and no BRL_BOARD_OK.  The contract
 * fields and the score of a table ended by an illegal call are zero: no contract was reached.
 */
#ifndef BRL_BOARDS_H
#define BRL_BOARDS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BRL_BOARD_MAX_CALLS 320   /* bytes of the call row (an auction has at most 319 calls) */
#define BRL_BOARD_FILL 0xFF       /* calls[n_calls ..] */

#define BRL_BOARD_TERMINATED 1    /* flags: the auction is over */
#define BRL_BOARD_PASSED_OUT 2    /*        four passes, no contract */
#define BRL_BOARD_ILLEGAL 4       /*        ended by an illegal call, which is NOT in calls[] */
#define BRL_BOARD_OK 8            /*        the self-check above holds */

/* 368 bytes = 23 x 16, little endian, no padding */
typedef struct brl_board_record {
  uint16_t n_calls;   /* calls made so far, 0 .. 319 */
  uint8_t dealer;     /* seat N,E,S,W = 0..3 */
  uint8_t vul_ns, vul_ew;
  uint8_t flags;      /* BRL_BOARD_* */
  uint8_t level;      /* 1..7; the contract fields are zero unless the auction ended legally in a contract */
  uint8_t strain;     /* C,D,H,S,NT = 0..4 */
  uint8_t doubled;    /* 0 / 1 doubled / 2 redoubled */
  uint8_t declarer;   /* absolute seat: the first of the declaring side to name the strain */
  uint8_t tricks;     /* the deal's double-dummy tricks for (declarer, strain) */
  uint8_t seating;    /* player id at seat s = (seating >> 2 s) & 3 (players {0,1} are team 1) */
  int32_t score_ns;   /* duplicate score from North-South's side */
  uint64_t hands[4];  /* seat s's 13 cards: bit rank * 4 + suit, suits C,D,H,S, ranks 2..A (brl_sl.h's form) */
  uint8_t calls[BRL_BOARD_MAX_CALLS]; /* action ids as brl_step takes them: 0 pass, 1 double, 2 redouble, 3 + 5 (level - 1) + strain */
} brl_board_record;

/* records[i] of state[i], i < n: state uint64 [n,16] (any mix of live and finished tables; only read), records
 * brl_board_record [n], 16-byte aligned.  One launch: a lane walks one table's events into a record image in LDS, the wave
 * writes its 64 records as whole 16-byte stores. */
int brl_board_records(int device, const uint64_t *state, int64_t n, brl_board_record *records, void *stream);

/* out_imp[i] (int32) = the IMP (src/duplicate.py:15-70) the pair sitting North-South at table A wins on board i, whose other
 * pair sits North-South at table B: the conversion of records_a[i].score_ns - records_b[i].score_ns.  records_a / records_b
 * 8-byte aligned (the struct's own alignment), out_imp 4-byte. */
int brl_board_imp(int device, const brl_board_record *records_a, const brl_board_record *records_b, int64_t n, int32_t *out_imp,
                  void *stream);

/* Keeps table A's final state of a duplicate evaluation, which the evaluators' step overwrites in the launch that ends it
 * (the slot is re-dealt seat-swapped for table B at once).  Called after every step launch of the loop:
 *   state       uint64 [n,16]  the tables after the step (only read)
 *   prev        uint64 [n,16]  in: the tables before the step; out: a copy of `state` (the next call's "before")
 *   action      int32  [n]     the call each table made in the step (-1: it waited)
 *   a_done      uint8  [n]     table A's `terminated` of the evaluators' Table_info, after the step
 *   taken       uint8  [n]     in/out: 1 once final_a[i] is written (start with zeros)
 *   final_a     uint64 [n,16]  out: for a table whose a_done turned 1 in this step, prev[i] stepped by action[i] with
 *                              bridge_device.hpp's table_step — the state the step kernel had in hand before the hand-over
 * One launch, a thread per table.  state, prev and final_a 16-byte aligned (a table's row is moved as 16-byte pieces), action
 * 4-byte; BRL_E_ARG otherwise, before anything is launched. */
int brl_board_keep_a(int device, const uint64_t *state, uint64_t *prev, const int32_t *action, const uint8_t *a_done,
                     uint8_t *taken, uint64_t *final_a, int64_t n, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* BRL_BOARDS_H */
