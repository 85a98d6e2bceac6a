"""One duplicate match between two saved models — the reference's ``eval.py``.

    python -m brl_amd.eval team1_model_path=a.pt team2_model_path=b.pkl [team2_model_type=FAIR] [num_eval_envs=100] [dds_path=...]
                           [deals_path=deals.json|deals.pbn] [save_boards=out.json|out.pbn]
                           [save_book=book.json|book.txt] [book_depth=4] [book_min_count=20] [par=1]
                           [review=1] [review_depth=12] [save_review=review.json]
                           [belief_board=ID belief_table=a belief_call=t] [belief_samples=4096] [save_belief=belief.json]
                           [belief_resample=N] [belief_moves=2]
                           [diff=1] [diff_depth=4] [diff_min_count=20] [save_diff=diff.json]
                           [lines=K] [lines_max_calls=64] [save_lines=lines.json]

The two teams may differ in type, so this is ``make_simple_duplicate_evaluate`` (a league of one architecture is
``python -m brl_amd.league``).  rng key 0, as in the reference.  Prints ``IMP: mean ± standard error``.
``deals_path``: play the boards of a deal file (``boards.read_deals``; ``num_eval_envs`` is then their number) instead of
dealing from the table; ``save_boards``: write every board's two auctions, contracts, scores and IMP (``boards.BoardRecords``).
``save_book``: write the bidding-system book of the match (``book.system_book``: what each call shows, by auction prefix, over
the first ``book_depth`` calls; entries with fewer than ``book_min_count`` samples are left out) as JSON or, ``.txt``, as a tree.
``par=1``: the boards are scored against their double-dummy par (``par.par_stats``): one line per team behind the ``IMP:``
line, and ``save_boards`` writes the par score, the par contracts and each table's IMP against par too.
``review=1``: the call review of the match (``review.make_call_review``): at each of the first ``review_depth`` calls of every
auction every alternative call is played out by the two loaded teams' own greedy policies and scored against the other table's
recorded result — hindsight on the actual deal, not a double-dummy judgement; one line per team behind the ``IMP:`` line, and
``save_review`` (which implies ``review=1``) writes the whole review as JSON (``review.CallReview.from_json`` reads it back).
``belief_board=ID belief_table=a|b belief_call=t``: the hand belief (``belief.make_hand_belief``) of the seat to call at
decision ``t`` of that board (its ``board_id``; the row of the match where the boards have none) at that table: what the other
three hands look like to it according to the two loaded teams, from ``belief_samples`` sampled deals — printed behind the other
lines; ``save_belief`` writes it as JSON (``belief.HandBelief.from_json`` reads it back).  ``belief_resample=N`` (with
``belief_moves=M`` Metropolis moves per particle, default 2) resamples the deals after every N-th call a hidden seat made
(``make_hand_belief``'s ``resample_every``): for prefixes that leave plain weighting with a handful of deals.
``diff=1``: the system diff of the match (``compare.make_policy_diff``): team 1's network (X) and team 2's (Y) are both shown
every decision of the first ``diff_depth`` calls of both tables' auctions — the same hand, the same auction — and the lines behind
the ``IMP:`` line say how often they would call the same, how far apart their policies are (Jensen-Shannon, overall and by call
index), how often each calls what was played, the largest confusion cells and the prefix with at least ``diff_min_count``
decisions that differs most; ``save_diff`` (which implies ``diff=1``) writes the whole diff as JSON
(``compare.PolicyDiff.from_json`` reads it back).
``lines=K`` (1 .. 16): the auction lines of the same boards (``lines.make_auction_lines``): a beam search of width K over the
auctions of both tables under the two teams' masked softmax, at most ``lines_max_calls`` calls deep; the lines behind the other
lines give the expected IMP of the policies as trained with its bound (24 x the mass not covered), the covered mass, how much of
its policy's mass the greedy auction carries and how often another auction is more probable; ``save_lines`` (which needs
``lines=K``) writes every line as JSON (``lines.AuctionLines.from_json`` reads it back).
Without these arguments the output is what it always was."""
from __future__ import annotations

import sys

EVAL_DEFAULTS = dict(  # eval.py: EVALConfig, same names and defaults
    team1_model_path=None, team2_model_path=None, team1_activation="relu", team1_model_type="DeepMind",
    team2_activation="relu", team2_model_type="DeepMind", num_eval_envs=100,
    dds_path="dds_results/test_000.npy",   # build-side: the reference reads this path unconditionally
    deals_path=None, save_boards=None, save_book=None, book_depth=4, book_min_count=20, par=0,
    review=0, review_depth=12, save_review=None,
    belief_board=None, belief_table="a", belief_call=0, belief_samples=4096, save_belief=None,
    belief_resample=0, belief_moves=2,
    diff=0, diff_depth=4, diff_min_count=20, save_diff=None,
    lines=0, lines_max_calls=64, save_lines=None,
)


def main(argv, log=print):
    import brl_amd
    from .checkpoint import load_params
    from .evaluation import make_simple_duplicate_evaluate
    from .league import parse
    cfg = parse(argv, EVAL_DEFAULTS)
    if not cfg["team1_model_path"] or not cfg["team2_model_path"]:
        raise SystemExit("team1_model_path= and team2_model_path= are required")
    review = bool(cfg["review"]) or cfg["save_review"] is not None
    diff = bool(cfg["diff"]) or cfg["save_diff"] is not None
    boards_run = (cfg["deals_path"] is not None or cfg["save_boards"] is not None or cfg["save_book"] is not None or bool(cfg["par"])
                  or review or cfg["belief_board"] is not None or diff)
    beam = int(cfg["lines"])
    if beam < 0 or beam > 16 or (cfg["save_lines"] is not None and beam == 0):
        raise SystemExit("lines=K: 1 .. 16 (0: no lines); save_lines= needs lines=K")
    deals = None
    if cfg["deals_path"] is not None:
        from .boards import read_deals
        deals = read_deals(cfg["deals_path"])
        cfg["num_eval_envs"] = deals.n
    env = brl_amd.BridgeBidding(cfg["dds_path"]) if deals is None else brl_amd.BridgeBidding(lut=(deals.lut_keys(), deals.lut_values()))
    log(f"num envs: {cfg['num_eval_envs']}")
    team1 = load_params(cfg["team1_model_path"], cfg["team1_activation"], cfg["team1_model_type"], env.device)
    team2 = load_params(cfg["team2_model_path"], cfg["team2_activation"], cfg["team2_model_type"], env.device)
    log("---------------------------------------------------")
    log(f'{cfg["team1_model_path"]} vs. {cfg["team2_model_path"]}')
    if boards_run:
        from .boards import make_board_match
        board_match = make_board_match(env, cfg["team1_activation"], cfg["team1_model_type"], cfg["team2_activation"],
                                       cfg["team2_model_type"], cfg["num_eval_envs"])
        (imp, se, _), records = board_match(team1, team2, deals if deals is not None else 0)
        if cfg["save_boards"] is not None:
            records.save(cfg["save_boards"], par=bool(cfg["par"]))
            log(f"boards: {cfg['save_boards']}")
        if cfg["save_book"] is not None:
            from .book import system_book
            system_book(records, int(cfg["book_depth"])).save(cfg["save_book"], min_count=int(cfg["book_min_count"]))
            log(f"book: {cfg['save_book']}")
    else:
        duplicate_evaluate = make_simple_duplicate_evaluate(env, cfg["team1_activation"], cfg["team1_model_type"], cfg["team2_activation"],
                                                            cfg["team2_model_type"], cfg["num_eval_envs"])
        (imp, se, _), _, _ = duplicate_evaluate(team1, team2, 0)
    log(f"IMP: {float(imp)} ± {float(se)}")
    if cfg["par"]:
        from .par import par_stats, stats_lines
        for line in stats_lines(par_stats(records)):
            log(line)
    if review:
        from .review import make_call_review
        call_review = make_call_review(env, cfg["team1_activation"], cfg["team1_model_type"], cfg["team2_activation"],
                                       cfg["team2_model_type"], depth=int(cfg["review_depth"]))
        rv = call_review(team1, team2, records)
        for line in rv.stats_lines():
            log(line)
        if cfg["save_review"] is not None:
            rv.to_json(cfg["save_review"])
            log(f"review: {cfg['save_review']}")
    if diff:
        from .compare import make_policy_diff
        policy_diff = make_policy_diff(env, cfg["team1_activation"], cfg["team1_model_type"], cfg["team2_activation"],
                                       cfg["team2_model_type"], depth=int(cfg["diff_depth"]))
        pd = policy_diff(team1, team2, records)
        for line in pd.stats_lines(min_count=int(cfg["diff_min_count"])):
            log(line)
        if cfg["save_diff"] is not None:
            pd.to_json(cfg["save_diff"])
            log(f"diff: {cfg['save_diff']}")
    if cfg["belief_board"] is not None:
        import numpy as np

        from .belief import make_hand_belief, queries_from_records
        ids = records.board_id
        if ids is not None and not isinstance(ids, np.ndarray):
            ids = ids.detach().cpu().numpy()
        rows = np.nonzero(np.asarray(ids) == int(cfg["belief_board"]))[0] if ids is not None else [int(cfg["belief_board"])]
        if len(rows) == 0 or not 0 <= int(rows[0]) < len(records):
            raise SystemExit(f"belief_board={cfg['belief_board']}: no such board in the match")
        if cfg["belief_table"] not in ("a", "b"):
            raise SystemExit(f"belief_table={cfg['belief_table']!r}: 'a' or 'b'")
        hand_belief = make_hand_belief(env, cfg["team1_activation"], cfg["team1_model_type"], cfg["team2_activation"],
                                       cfg["team2_model_type"], samples=int(cfg["belief_samples"]),
                                       resample_every=int(cfg["belief_resample"]), moves=int(cfg["belief_moves"]))
        hb = hand_belief(team1, team2, queries_from_records(records, cfg["belief_table"], int(rows[0]), int(cfg["belief_call"])))
        for line in hb.to_text(0).split("\n"):
            log(line)
        if cfg["save_belief"] is not None:
            hb.to_json(cfg["save_belief"])
            log(f"belief: {cfg['save_belief']}")
    if beam:
        from .lines import make_auction_lines
        auction_lines = make_auction_lines(env, cfg["team1_activation"], cfg["team1_model_type"], cfg["team2_activation"],
                                           cfg["team2_model_type"], cfg["num_eval_envs"], k=beam, max_calls=int(cfg["lines_max_calls"]))
        al = auction_lines(team1, team2, deals if deals is not None else 0)
        for line in al.summary_lines():
            log(line)
        if cfg["save_lines"] is not None:
            al.to_json(cfg["save_lines"])
            log(f"lines: {cfg['save_lines']}")
    return float(imp), float(se)


if __name__ == "__main__":
    main(sys.argv[1:])
