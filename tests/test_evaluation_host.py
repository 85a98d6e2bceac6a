"""Host-side logic of the evaluators' loop (brl_amd/evaluation.py) that needs no GPU: the ladder of batch sizes the forwards on
the boards still playing step down through (`_ActiveRows.update`), and the composition of ``log_info`` from the counters of ``brl_eval_reduce`` (`eval_log_info`)."""
import numpy as np
import pytest
import torch

from brl_amd.evaluation import _ActiveRows


def ladder(n):
    """every batch size the loop can take for n boards, by feeding every possible number of finished boards in order"""
    rows, seen = _ActiveRows(n), [n]
    idx = torch.arange(n)
    for finished in range(0, n + 1):
        rows.update((finished, idx))
        if rows.m != seen[-1]:
            seen.append(rows.m)
        live = n - finished
        assert rows.m >= min(live, n) or live == 0            # never fewer rows than boards still playing
        assert rows.m >= 256 or rows.m == n                   # (small evaluations are never cut below one tile)
        assert rows.idx is None or rows.idx.numel() == rows.m
    return seen


def test_batch_sizes_step_down_a_short_ladder():
    seen = ladder(8192)
    assert seen == [8192, 6144, 4096, 3072, 2048, 1536, 1024, 768, 512, 256]     # ten GEMM shapes per layer, not thirty-two
    seen = ladder(10000)
    assert seen[0] == 10000 and seen[-1] == 256 and len(seen) <= 12
    assert all(a > b for a, b in zip(seen, seen[1:])) and all(m % 256 == 0 for m in seen[1:])
    assert ladder(300) == [300, 256]
    assert ladder(100) == [100]                                                    # nothing below one tile: full batches


def test_batch_size_never_grows_and_ignores_missing_lists():
    rows = _ActiveRows(4096)
    idx = torch.arange(4096)
    rows.update(None)
    rows.update((4000, None))          # a post without an index list (compaction off)
    assert rows.m == 4096 and rows.idx is None
    rows.update((3000, idx))           # 1096 playing -> 1536
    assert rows.m == 1536
    rows.update((100, idx))            # an older, larger count arriving late must not grow the batch again
    assert rows.m == 1536


def test_done_watch_tags_identify_loop_and_iteration():
    """The finished-board count reaches the host as (tag << 32) | count in pinned memory (brl_live_index); a tag names the loop
    (epoch) and the iteration, fits the kernel's 31 bits, and no two iterations the host could confuse share one: the ring has 4
    slots, a slot is rewritten every 4 iterations, and a new loop on the same watch takes a new epoch."""
    from brl_amd.evaluation import _DoneWatch
    w = object.__new__(_DoneWatch)
    seen = set()
    for epoch in (1, 2, 0x7FFF):
        w.epoch = epoch
        tags = [w._tag(i) for i in range(0, 5000)]
        assert all(0 < t < (1 << 31) for t in tags)
        assert len(set(tags)) == len(tags)                      # within a loop: distinct for 65535 iterations
        assert not (seen & set(tags))                           # across loops: disjoint
        seen |= set(tags)
    assert _DoneWatch.DEPTH < _DoneWatch.RING                   # the slot polled for iteration i - DEPTH is not the one being written


# ---- the statistics behind log_info: counters (tests/eval_counts_ref.py) -> eval_log_info, against oracle/eval_stats.py ----------
# log_info entries that are one integer count / n / tables, computed in float64 and rounded to float32 once
_COUNT_ENTRIES = {True: list(range(6, 21)), False: list(range(4, 19))}


def _synthetic_evaluation(n, seed, dup):
    """finished tables, a step log and returns that no play produced: skewed per team, table and bid (tests/eval_counts_ref.py)"""
    from oracle.eval_stats import StepLog
    from tests import eval_counts_ref as er
    rng = np.random.default_rng([seed, 79])
    A = er.synthetic_table(n, seed, 0)
    B = er.synthetic_table(n, seed, 1) if dup else None
    log = StepLog(n)
    steps = rng.integers(1, 11, (n, 2))
    passes = (rng.random((n, 2)) * (steps + 1)).astype(np.int64)
    bc = er.synthetic_bid_count(n, seed, big=False, at_most_one=not dup)     # (the single-table evaluator marks a bid: 0 / 1)
    log.step_count[:], log.pass_count[:], log.bid[:] = steps, passes, bc
    log.total_illegal[:] = (rng.random((n, 2)) ** 3 * steps).astype(np.float32)
    final_steps = rng.integers(4, 40, n).astype(np.int32)
    cum = rng.integers(-24, 25, n).astype(np.float32) if dup else A["rewards"][:, 0].copy()
    return A, B, log, bc, final_steps, cum


def _host_log_info(A, B, log, bc, final_steps, cum, dup):
    from brl_amd.evaluation import EvalStats, _Shard, eval_log_info
    from tests import eval_counts_ref as er
    n = len(cum)
    counts = er.eval_counts_ref(A, B, bc, final_steps)
    stats = EvalStats(n, "cpu")
    stats.illegal_prob_sum.copy_(torch.from_numpy(log.total_illegal))
    stats.step_count.copy_(torch.from_numpy(log.step_count.astype(np.int32)))
    stats.pass_count.copy_(torch.from_numpy(log.pass_count.astype(np.int32)))
    got = eval_log_info(torch.from_numpy(counts).to(torch.float64), stats, torch.from_numpy(cum), dup, _Shard(n, None))
    return counts, got


@pytest.mark.parametrize("dup", [True, False])
@pytest.mark.parametrize("n", [5000, 257])
def test_log_info_from_counters_matches_the_reference_statistics(dup, n):
    """eval_counts_ref -> eval_log_info on CPU tensors against duplicate_log_info / single_log_info of the same arrays: a wrong
    offset in the composition of log_info moves a skewed count to an entry where the reference has another one"""
    from oracle.eval_stats import duplicate_log_info, single_log_info
    from tests import eval_counts_ref as er
    A, B, log, bc, final_steps, cum = _synthetic_evaluation(n, 11, dup)
    counts, got = _host_log_info(A, B, log, bc, final_steps, cum, dup)
    if n == 5000:
        assert er.equal_exchange_pairs(counts, dup) == []          # (of the input: with ties, change the seed)
    if dup:
        want = duplicate_log_info(cum, log, final_steps, A, B)
    else:
        want = single_log_info(cum, log, dict(A, step_count=final_steps))
    assert len(got) == len(want) == (23 if dup else 19)
    for i, (g, w) in enumerate(zip(got, want)):
        g, w = g.numpy().astype(np.float64), np.asarray(w, np.float64)
        assert g.shape == w.shape, i
        if i in _COUNT_ENTRIES[dup]:
            assert np.all(np.abs(g - w) <= 2.0 ** -23 * np.abs(w)), f"log_info[{i}]: {g} != {w}"
        else:   # means of per-board ratios and of returns, in float32 on both sides: the tolerance of the GPU tests' _assert_log_info
            assert np.allclose(g, w, rtol=1e-5, atol=1e-6), f"log_info[{i}]: {g} != {w}"


def test_evaluate_log_files_every_bid_under_its_own_key():
    """make_evaluate_log: log_info[6..9] land under .../{level}{strain} for all 35 bids, with 35 distinct values per histogram"""
    from brl_amd.evaluation import make_evaluate_log
    from brl_amd.evaluation import EvalStats, _Shard, eval_log_info
    n = 64
    counts = torch.arange(231, dtype=torch.float64) ** 2 * 3 + 100      # increasing faster than linearly: sums over the tables differ too
    stats = EvalStats(n, "cpu")
    stats.step_count.fill_(2)
    info = eval_log_info(counts, stats, torch.arange(n, dtype=torch.float32), True, _Shard(n, None))
    d = make_evaluate_log(info)
    assert len(d) == 19 + 4 * 35
    for entry, group in ((6, "actor_bid_probs"), (7, "opp_bid_probs"), (8, "actor_contract_probs"), (9, "opp_contract_probs")):
        vec = [float(v) for v in info[entry]]
        assert len(set(vec)) == 35, group
        for level in range(1, 8):
            for s, strain in enumerate(("C", "D", "H", "S", "NT")):
                assert d[f"eval/{group}/{level}{strain}"] == vec[5 * (level - 1) + s], (group, level, strain)
    assert len({tuple(float(v) for v in info[e]) for e in (6, 7, 8, 9)}) == 4
