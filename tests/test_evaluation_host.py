"""Host-side logic of the evaluators' loop (brl_amd/evaluation.py) that needs no GPU: the ladder of batch sizes the forwards on
the boards still playing step down through (`_ActiveRows.update`), the route of every forward (`_Forward.route`), and the composition of ``log_info`` from the counters of ``brl_eval_reduce`` (`eval_log_info`)."""
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


class _SnapStub:
    """a snapshot as far as the route is concerned: brl_linear_x3p from 4096 rows on (models.InferenceSnapshot.planes_for)"""

    def planes_for(self, rows):
        return rows >= 4096


class _ConstantStub:
    """the whole contract of a constant forward (evaluation._Forward's docstring)"""
    constant = True

    def __call__(self, obs_bool, obs_f32):
        raise AssertionError("the route needs no forward")


def _stub_forwards():
    """(constant, snapshot + brl_mlp_ref: "DeepMind" ReLU, brl_mlp_ref only: "DeepMind" tanh, neither: "FAIR")"""
    from brl_amd.evaluation import _Forward
    out = [_ConstantStub()]
    for snap, ref in ((_SnapStub(), object()), (None, object()), (None, None)):
        f = object.__new__(_Forward)       # (no network behind it: route and cast read these two attributes only)
        f.snap, f.ref = snap, ref
        out.append(f)
    return out


def test_route_of_every_forward_at_every_threshold(monkeypatch):
    """_Forward.route — what a forward takes as input and on which rows — on both sides of _OWN_FORWARD_ROWS = 1024 and of the
    4096-row planes threshold, for every kind of forward; and when the alternating loop's step launch writes float32 too"""
    from brl_amd import evaluation
    from brl_amd.evaluation import _Forward
    monkeypatch.setattr(evaluation, "_OWN_FORWARD_ROWS", 1024)
    constant, relu, tanh, fair = _stub_forwards()
    full, shrunk = (300, 4095, 4096, 8192), (256, 1024, 1280, 3072, 4096, 6144)
    want = {constant: (["constant"] * 4, ["constant"] * 6),
            relu: (["full_f32", "full_f32", "full_bool", "full_bool"],
                   ["rows_own", "rows_own", "rows_f32", "rows_f32", "rows_bf16", "rows_bf16"]),
            tanh: (["full_f32"] * 4, ["rows_own", "rows_own", "rows_f32", "rows_f32", "rows_f32", "rows_f32"]),
            fair: (["full_f32"] * 4, ["rows_f32"] * 6)}
    for fwd, (w_full, w_shrunk) in want.items():
        assert [_Forward.route(fwd, n, False) for n in full] == w_full
        assert [_Forward.route(fwd, m, True) for m in shrunk] == w_shrunk
    for fwd in (relu, tanh, fair):
        assert [fwd.cast(m) for m in (4095, 4096)] == [(torch.float32, 0), (torch.bfloat16 if fwd is relu else torch.float32, int(fwd is relu))]
    monkeypatch.setattr(evaluation, "_OWN_FORWARD_ROWS", 0)        # BRL_EVAL_OWN_ROWS=0: never the one-call forward
    assert [_Forward.route(relu, m, True) for m in (256, 4096)] == ["rows_f32", "rows_bf16"]
    # the step launch writes the next forward's float32 input exactly while that forward takes every board as float32
    for n in full:
        for fwd in (constant, relu, tanh, fair):
            rows = _ActiveRows(n)
            assert rows.takes_f32(fwd) == (fwd is not constant and not (fwd is relu and n >= 4096)), n
            rows.update((n - 1, torch.arange(n)))                   # an index list: from now on the forward gathers its own rows
            assert rows.idx is not None and not rows.takes_f32(fwd)


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
