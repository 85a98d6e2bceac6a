/*
 * brl_lines.h — C-ABI of the auction lines (brl_amd/csrc/brl_lines.hip, part of libbrl_hip.so): a beam search over the auctions
 * of every board under the networks' masked softmax — the K most probable auctions with their probability —, the results of the
 * finished ones and the expected IMP of two tables' beams with a rigorous bound.
 *
 * Kept apart from brl_hip.h like brl_boards.h and brl_review.h: these entry points have no oracle counterpart; brl_version()
 * does not count them.
 *
 * Conventions are brl_hip.h's: 0 on success, <0 (BRL_E_*) on error with the message in brl_last_error(); every pointer is a
 * device pointer on `device`; `stream` is a hipStream_t passed as void*; nothing synchronises.  No handle, no atomics, no
 * floating-point reduction whose order depends on timing: the same bytes on every run.
 *
 * The definition.
 *
 *   - Line.  An auction prefix of one board with its table (uint64 [16], bridge_device.hpp's packed table).  A beam holds K
 *     slots per board, 1 <= K <= BRL_LINES_MAX_K: line (board b, slot s) is element b * K + s of every array below.
 *   - Term.  The masked log-softmax of one call, in float64 from the float32 logits of the caller's network (team 0 = players
 *     {0,1} reads logits1, team 1 logits2; row b * K + s, 38 logits, row stride ldo), over the legal mask of the line's own table
 *     (legal_mask, bridge_device.hpp: what brl_observe reports):
 *         mx = the maximum of the legal logits, taken in index order;  z = the sum of exp((double)l_j - mx) over the legal j in
 *         index order;  term(a) = ((double)l_a - mx) - log(z).
 *     One device function (line_log_softmax, brl_lines.hip) computes it.  A line's score is the float64 sum of its calls' terms in
 *     call order, starting from 0.0.
 *   - Greedy call.  The evaluators' masked arg-max (categorical<K>, mode 1, policy_common.hpp — what brl_eval_step_team plays): the
 *     FIRST legal action whose float32 logit is strictly greater than every legal logit before it; a NaN is never a maximum; a
 *     row without a legal logit above -inf gives action 0.  BRL_LINE_GREEDY says that every call of the line was that call.
 *   - Void row.  A row in which a legal logit is NaN or +inf, or in which no legal logit is above -inf (nothing is clamped or
 *     replaced: DESIGN, "Non-finite values"; comparisons follow nan_math.hpp's reading, a NaN is not skipped).  Such a row has no
 *     distribution, so the line cannot be continued: the line itself becomes BRL_LINE_VOID — table, calls and score unchanged, its
 *     score is the mass that reached the row — and is carried like a finished line from then on.  -inf on a legal action is an
 *     ordinary probability 0 (term -inf).  Logits of illegal actions are never read into any result.
 *   - One expansion step of one board.  Candidates: every finished or void line of the beam as itself (action -1, score
 *     unchanged; a passed-out deal is finished), and for every live line every legal action a as a child with score
 *     parent + term(a).  The new beam is the K first candidates under the total order
 *         void lines last;  score descending;  parent slot ascending;  action ascending,
 *     in that order in slots 0 .. K-1.  Fewer than K candidates leave the trailing slots BRL_LINE_EMPTY: table 0, calls
 *     BRL_LINES_FILL, score -inf.  (A child can reach the new beam only among its parent's K first: at most K * K + K candidates
 *     are ranked.)  A child's table is the parent's stepped by table_step (bridge_device.hpp), its calls are the parent's plus a
 *     at index t = the parent table's step count (call t of the table's auction is calls[t]; stored only if t < max_calls).
 *   - Finished.  The table is terminated (SC_TERM).  Open: a line that is neither finished, void nor empty when the search stops.
 *   - Result of a finished line.  As brl_board_records reads a table: contract, declarer (first of the side to name the strain),
 *     doubled state, the declarer's double-dummy tricks from the table, North-South's score (terminal_reward).
 *   - Expected IMP of a board.  Table A seats (team 1 North-South, team 2 East-West), table B the swapped seating; the tables are
 *     searched independently.  With p = exp(score) and u = score_team1, the result from player 0's side (at table A score_ns, at
 *     table B -score_ns), over the finished lines (not void) i of table A and j of table B:
 *         t(i,j) = (p_i * p_j) * imp(u_i + u_j)       (imp_vector of imp.hpp, as the evaluators' step calls it)
 *         S = sum over m = 0 .. K-1 of [ t(m,m) + sum over j < m of (t(m,j) + t(j,m)) ]      in this order, float64
 *         c = (sum_i p_i) * (sum_j p_j), each sum in slot order
 *     and the expected IMP of team 1 lies in [S - 24 (1 - c), S + 24 (1 - c)] (an IMP is at most 24 in magnitude and 1 - c is the
 *     mass of the pairs of auctions that were not enumerated).  The order of S is symmetric in the two tables: exchanging the two
 *     teams exchanges the tables' beams and negates every u, which negates S bit for bit and leaves c bit for bit.
 *
 * Input values are not trusted: K, max_calls and ldo are checked, a call is stored only below max_calls, a slot index read back
 * from the selection is below K by construction, and every write is to the line's own element.
 */
#ifndef BRL_LINES_H
#define BRL_LINES_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BRL_LINES_MAX_K 16       /* beam width */
#define BRL_LINES_MAX_CALLS 64   /* calls kept per line */
#define BRL_LINES_FILL 0xFF      /* calls[] behind the line's last call */

/* flags of a line */
#define BRL_LINE_EMPTY 1
#define BRL_LINE_FINISHED 2
#define BRL_LINE_VOID 4
#define BRL_LINE_GREEDY 8

/* 16 bytes, little endian, no padding */
typedef struct brl_line_request {
  int32_t board;   /* -1: the line needs no forward (empty, finished or void) */
  int32_t slot;
  int32_t player;  /* player to act, 0..3 */
  int32_t team;    /* 0 = players {0,1} */
} brl_line_request;

/* 16 bytes, little endian, no padding */
typedef struct brl_line_result {
  int32_t score_ns;
  uint8_t has_result;  /* 1: a finished line that is not void (a pass-out has level 0 and score 0) */
  uint8_t level;       /* 1..7, 0 = passed out */
  uint8_t strain;      /* C,D,H,S,NT = 0..4 */
  uint8_t doubled;     /* 0, 1 = doubled, 2 = redoubled */
  uint8_t declarer;    /* seat N,E,S,W = 0..3 */
  uint8_t tricks;
  uint8_t zero[2];
  int32_t score_team1; /* the same score from the side player 0 sits on (player 0's reward: what the evaluators accumulate) */
} brl_line_result;

/* 64 bytes: 8 doubles per board */
typedef struct brl_lines_board {
  double imp;        /* S */
  double covered;    /* c */
  double covered_a, covered_b;   /* mass of the finished lines of each table */
  double open_a, open_b;         /* mass of the lines still live */
  double void_a, void_b;         /* mass of the void lines */
} brl_lines_board;

/* Step 0's beam of n boards: slot 0 = state[b] (uint64 [n,16]: the dealt tables) with score 0.0 and BRL_LINE_GREEDY (finished
 * already if the table is), the other slots empty.  tables uint64 [n*K,16], calls uint8 [n*K,max_calls], score double [n*K],
 * flags uint8 [n*K], request [n*K], done uint8 [n] (1: no live line).  1 <= max_calls <= 64, n * K < 2^31. */
int brl_lines_init(int device, const uint64_t *state, int64_t n, int32_t k, int32_t max_calls, uint64_t *tables, uint8_t *calls,
                   double *score, uint8_t *flags, brl_line_request *request, uint8_t *done, void *stream);

/* One expansion step (above): the beam (tables, calls, score, flags) in, the next beam into the out_ arrays, which must be other
 * memory (a double buffer).  logits1 / logits2: float [n*K, ldo1 / ldo2 >= 38], the row of line (b, s) is b * K + s; only the
 * rows of live lines are read, team 0's from logits1.  request / done as brl_lines_init.  One launch, a wave per board: per live
 * line the wave forms the terms (a lane per action), ranks the line's children and leaves the K first in LDS; every candidate
 * then counts the candidates that precede it, and the wave builds the K selected lines. */
int brl_lines_expand(int device, const uint64_t *tables, const uint8_t *calls, const double *score, const uint8_t *flags, int64_t n,
                     int32_t k, int32_t max_calls, const float *logits1, int64_t ldo1, const float *logits2, int64_t ldo2,
                     uint64_t *out_tables, uint8_t *out_calls, double *out_score, uint8_t *out_flags, brl_line_request *request,
                     uint8_t *done, void *stream);

/* results[i] of the lines i < lines (tables uint64 [lines,16], flags uint8 [lines]): has_result = 0 and zeros for a line that is
 * not finished, is void or is empty.  One launch, a thread per line; integer only. */
int brl_lines_finish(int device, const uint64_t *tables, const uint8_t *flags, int64_t lines, brl_line_result *results, void *stream);

/* boards[b] of the boards b < n from the two tables' final beams (score double [n*K], flags uint8 [n*K], results [n*K] each).
 * One launch, a thread per board; float64 in the order stated above. */
int brl_lines_imp(int device, const double *score_a, const uint8_t *flags_a, const brl_line_result *results_a, const double *score_b,
                  const uint8_t *flags_b, const brl_line_result *results_b, int64_t n, int32_t k, brl_lines_board *boards,
                  void *stream);

#ifdef __cplusplus
}
#endif

#endif /* BRL_LINES_H */
