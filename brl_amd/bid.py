"""Ask a saved model what it bids — the reference's ``wb5/model_client_script.py`` (``ModelBiddingSystem.bid``) as a command.

    python -m brl_amd.bid model_path=params.pt [model_type=DeepMind] [activation=relu] [top_k=3]
                          hand=AKQ.J32.T9.87654 dealer=N vul=None auction="1C P"
    python -m brl_amd.bid model_path=params.pt positions_path=quiz.json [save_path=answers.json]

``hand``: spades.hearts.diamonds.clubs; ``dealer``: N, E, S, W; ``vul``: None, NS, EW, Both; ``auction``: the calls so far from
the dealer on (P, X, XX, 1C .. 7NT; Pass, Dbl, Rdbl and 1N are read too).  Prints the call of the seat whose turn it is, the top of
its policy with probabilities, the value and the policy's entropy (``positions.Answers.to_text``).
``positions_path``: a JSON list of ``{"hand", "dealer", "vul", "auction", "answers"?}``; every position is answered in one batch
and printed; ``answers`` maps calls to points (a bidding-contest key: several calls may score) and, where any are present, the
totals of ``positions.quiz_score`` are printed behind them.  ``save_path`` writes ``Answers.to_json``."""
from __future__ import annotations

import json
import sys

BID_DEFAULTS = dict(model_path=None, model_type="DeepMind", activation="relu", top_k=3, hand=None, dealer="N", vul="None", auction="",
                    positions_path=None, save_path=None, device=None)


def read_positions(path):
    """([Position], [key or None]) of a quiz file; ``SystemExit`` names the entry that cannot be read"""
    from .positions import Position
    with open(path) as f:
        doc = json.load(f)
    if not isinstance(doc, list) or not doc:
        raise SystemExit(f"{path}: not a non-empty JSON list of positions")
    out, keys = [], []
    for i, d in enumerate(doc):
        try:
            out.append(Position.from_label(d))
        except (ValueError, KeyError, TypeError, AttributeError) as e:
            raise SystemExit(f"{path}: position {i}: {e}") from None
        keys.append(d.get("answers"))
    return out, keys


def main(argv, log=print):
    from .league import parse
    cfg = parse(argv, BID_DEFAULTS)
    if not cfg["model_path"]:
        raise SystemExit("model_path= is required")
    if (cfg["hand"] is None) == (cfg["positions_path"] is None):
        raise SystemExit("give either hand= (with dealer= vul= auction=) or positions_path=")
    if cfg["save_path"] is not None and cfg["positions_path"] is None:
        raise SystemExit("save_path= needs positions_path=")
    from .positions import MAX_TOP, Position, quiz_score
    if not 1 <= int(cfg["top_k"]) <= MAX_TOP:
        raise SystemExit(f"top_k=: 1 .. {MAX_TOP}")
    if cfg["hand"] is not None:
        try:
            asked, keys = [Position(cfg["hand"], cfg["dealer"], cfg["vul"], cfg["auction"])], [None]
        except ValueError as e:
            raise SystemExit(f"not a position: {e}") from None
    else:
        asked, keys = read_positions(cfg["positions_path"])
    import torch

    from .checkpoint import load_params
    from .positions import Bidder
    device = cfg["device"] or ("cuda" if torch.cuda.is_available() else None)
    if device is None:
        raise SystemExit("brl_amd.bid needs a GPU: brl_amd has no CPU fallback")
    params = load_params(cfg["model_path"], cfg["activation"], cfg["model_type"], device)
    answers = Bidder(params, cfg["activation"], cfg["model_type"], top_k=int(cfg["top_k"])).ask(asked)
    for i in range(len(answers)):
        log(answers.to_text(i))
    if any(keys):
        t = quiz_score(answers, keys)["total"]
        log(f"quiz: {t['points']:g} of {t['max']:g} points on {t['positions']} positions, expected {t['expected']:.2f} under the policy, "
            f"{100 * t['top_mass']:.1f}% of its mass on the top-scored calls")
    if cfg["save_path"] is not None:
        answers.to_json(cfg["save_path"])
        log(f"answers: {cfg['save_path']}")
    return answers


if __name__ == "__main__":
    main(sys.argv[1:])
