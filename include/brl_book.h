/*
 * brl_book.h — C-ABI of the bidding-system book (brl_amd/csrc/brl_book.hip, part of libbrl_hip.so): what each call of an
 * auction shows, grouped by the sequence of calls that led to it.  Board records (brl_boards.h) in, one table of exact integer
 * counters per distinct auction prefix out.
 *
 * Kept apart from brl_hip.h like brl_boards.h and brl_league.h: these entry points have no oracle counterpart; brl_version()
 * does not count them.
 *
 * Conventions are brl_hip.h's: 0 on success, <0 (BRL_E_*) on error with the message in brl_last_error(); every pointer is a
 * device pointer on `device`; `stream` is a hipStream_t passed as void*; nothing synchronises.
 *
 * Sample.  One call p of one record, p < min(n_calls, depth), 1 <= depth <= BRL_BOOK_MAX_DEPTH.  A record without BRL_BOARD_OK
 * gives no samples; live tables and tables ended by an illegal call give the samples of the calls they hold.
 *
 * Bidder.  The seat is s = (dealer + p) & 3, the bidder's player id (seating >> 2 s) & 3, its team index id >> 1: 0 is team 1
 * (players 0, 1), 1 is team 2.
 *
 * Key.  The prefix calls[0..p], the call made included, as a uint64: sum_j (calls[j] + 1) << (58 - 6 j).  Six bits per call,
 * most significant first; a zero field ends the prefix; ten calls use bits 63..4 and calls[j] + 1 lies in 1..38.  Key 0 is
 * "no sample".  The numeric (unsigned) order of keys is the depth-first order of the prefix tree, a prefix before its
 * extensions.  The prefix starts at the dealer, so keys are relative to position (first seat, second seat, ...).
 *
 * Features of the bidder's hand word hands[s] (bit = rank * 4 + suit, suits C,D,H,S), packed into one uint32 per sample:
 *   bits  0..5   HCP 0..37: ranks 9..12 are J,Q,K,A worth 1,2,3,4
 *   bits  6..21  the four suit lengths C,D,H,S, 0..13, four bits each
 *   bit   22     balanced: the sorted shape is 4333, 4432 or 5332
 *   bit   23     the team index
 *   bits 24..31  the board's IMP from the bidder's side as an int8: imp_sign * imp[i] for a North-South bidder,
 *                -imp_sign * imp[i] for an East-West one; 0 without an imp array.  imp[i] is brl_board_imp's value (the IMP of
 *                the pair sitting North-South at table A, -24..24): imp_sign is +1 for table A's records and -1 for table B's.
 *
 * Entry.  One per distinct key, BRL_BOOK_ENTRY_BYTES = 816 = 51 x 16 bytes, little endian, no padding: the key and per team
 * index a block of counters.  All counters are exact integers: the same bytes on every run.
 */
#ifndef BRL_BOOK_H
#define BRL_BOOK_H

#include <stdint.h>

#include "brl_boards.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BRL_BOOK_MAX_DEPTH 10
#define BRL_BOOK_ENTRY_BYTES 816

/* 400 bytes */
typedef struct brl_book_team {
  uint32_t count;            /* samples */
  uint32_t balanced;         /* samples with a balanced hand */
  uint32_t hcp[38];          /* samples by high-card points */
  uint32_t length[4][14];    /* samples by the length of suit C,D,H,S */
  int64_t imp_sum;           /* sum of the bidder's-side IMP */
  uint64_t imp_sq_sum;       /* and of its square */
} brl_book_team;

typedef struct brl_book_entry {
  uint64_t key;
  uint64_t reserved;         /* zero */
  brl_book_team team[2];
} brl_book_entry;

/* keys[i * depth + p] and feats[i * depth + p], i < n, p < depth, of records[i] (16-byte aligned): the sample's key and packed
 * features, or 0 and 0 where there is no sample (p past the auction, or a record without BRL_BOARD_OK).  imp: int32 [n] or
 * NULL; imp_sign: +1 or -1.  One launch, four lanes per record, each loading 16 of the record's first 64 bytes (the header, the
 * four hand words, calls[0..15]); the other 304 call bytes are never read.  No atomics.  A duplicate match calls it once per
 * table, into the two halves of one buffer. */
int brl_book_samples(int device, const brl_board_record *records, int64_t n, const int32_t *imp, int imp_sign, int depth,
                     uint64_t *keys, uint32_t *feats, void *stream);

/* entries[e], e < K, from the samples sorted by key:
 *   feats        uint32 [S]  brl_book_samples' feats in key order
 *   entry_index  int32  [S]  nondecreasing; the entry of sample i.  It is dense: entry_index[i + 1] - entry_index[i] is 0 or 1
 *                            (what unique_consecutive's inverse is).  A sample whose index lies outside 0..K-1 — the run of
 *                            key 0 given index -1 — is dropped; nothing is ever written outside entries[0..K-1].
 *   entry_keys   uint64 [K]  the key of entry e
 *   entries      [K]         16-byte aligned; zeroed by this call (a memset on the stream), then written
 * One launch, a workgroup per BRL_BOOK_CHUNK consecutive samples.  A run of equal indices that crosses a chunk boundary or is
 * 64 samples or longer is accumulated in a histogram in LDS and flushed once per workgroup with global integer atomic adds of
 * its nonzero bins; a shorter run inside the chunk belongs to that workgroup alone, which stores the bins it touches. */
#define BRL_BOOK_CHUNK 1024
int brl_book_reduce(int device, const uint32_t *feats, const int32_t *entry_index, int64_t S, const uint64_t *entry_keys,
                    int64_t K, brl_book_entry *entries, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* BRL_BOOK_H */
