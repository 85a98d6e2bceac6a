"""CPU: the tools that run on one rank refuse a process group of more than one (``brl_amd.dist.one_rank_only``), in one wording and
before anything touches the environment or the device; the world size alone decides (BRL_FORCE_DIST does not)."""
import pytest
import torch.distributed as dist

from brl_amd.dist import one_rank_only


class _Untouched:
    """an environment nothing may ask anything of but its device's name"""
    device = "cpu"

    def __getattr__(self, name):
        raise AssertionError(f"the environment was asked for {name!r}")


def _group(monkeypatch, world):
    """torch.distributed as it answers with a process group of ``world`` ranks up (None: no group)"""
    monkeypatch.setattr(dist, "is_available", lambda: True)
    monkeypatch.setattr(dist, "is_initialized", lambda: world is not None)
    monkeypatch.setattr(dist, "get_world_size", lambda *a: world)


def _entry_points():
    from brl_amd import belief, boards, build, compare, crossplay, lines, review
    build.build()      # (make_lineup_evaluate loads the library)
    env, net = _Untouched(), ("relu", "DeepMind")
    return {
        "board_match": lambda: boards.make_board_match(env, *net, *net, 4)(None, None, 0),
        "call_review": lambda: review.make_call_review(env, *net, *net)(None, None, None),
        "hand_belief": lambda: belief.make_hand_belief(env, *net, *net, samples=4)(None, None, [None]),
        "policy_diff": lambda: compare.make_policy_diff(env, *net, *net)(None, None, None),
        "auction_lines": lambda: lines.make_auction_lines(env, *net, *net, 4)(None, None, 0),
        "lineup_evaluate": lambda: crossplay.make_lineup_evaluate(env, *net, 4, method="loop")([None], [(0, 0, 0, 0)], 0),
    }


@pytest.mark.parametrize("world,forced", [(None, False), (1, False), (1, True)])
def test_the_helper_is_silent_without_a_second_rank(monkeypatch, world, forced):
    _group(monkeypatch, world)
    monkeypatch.setenv("BRL_FORCE_DIST", "1" if forced else "0")
    one_rank_only("anything")


def test_every_entry_point_refuses_a_second_rank_before_it_touches_anything(monkeypatch):
    calls = _entry_points()      # (built with no group up: what a tool refuses is the call)
    _group(monkeypatch, 2)
    with pytest.raises(RuntimeError, match=r"^a_tool runs on one rank \(a process group is up\): call it on one rank only, outside the group$"):
        one_rank_only("a_tool")
    for name, call in calls.items():
        with pytest.raises(RuntimeError, match=rf"^{name} runs on one rank \(a process group is up\)"):
            call()
