"""-m gpu: the bidding-system book (brl_amd/book.py, include/brl_book.h) against its Python restatement (tests/book_ref.py),
entry for entry and counter for counter — synthetic records at the sizes and shapes where the two kernels change path, a
duplicate match end to end, and the command line.  Every comparison is exact integer equality."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import board_records_ref as R  # noqa: E402
import book_ref as B  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _upload(rec):
    return torch.from_numpy(rec.view(np.uint8).reshape(-1, 368)).to(DEV)


def _same(sb, ref, skipped=0):
    """the book equals the restatement's dict: the same prefixes in the same order and every counter"""
    keys, count, balanced, hcp, length, imp_sum, imp_sq = B.arrays(ref)
    assert len(sb) == len(ref) and np.array_equal(sb.keys, keys)
    assert np.array_equal(sb.count, count) and np.array_equal(sb.balanced, balanced)
    assert np.array_equal(sb.hcp_hist, hcp) and np.array_equal(sb.length_hist, length)
    assert np.array_equal(sb.imp_sum, imp_sum) and np.array_equal(sb.imp_sq_sum, imp_sq)
    assert sb.skipped == skipped


_SETS = {}


def _random_set(n):
    """n records of random auctions — the 319-call one, auctions stopped early (shorter than any depth) and empty ones among
    them — with random hands, dealers, seatings and IMPs; built once per size"""
    if n not in _SETS:
        rng = np.random.default_rng(500 + n)
        auctions = []
        for i in range(n):
            if i % 97 == 3:
                auctions.append(R.longest_auction())
            elif i % 11 == 5:
                auctions.append([])
            elif i % 3 == 0:
                auctions.append(R.random_auction(rng, stop=int(rng.integers(0, 12))))
            else:
                auctions.append(R.random_auction(rng, p_pass=float(rng.uniform(0.2, 0.7))))
        if n == 1:
            auctions = [R.random_auction(rng)]
        _SETS[n] = (B.make_records(auctions, rng), B.make_records(auctions[::-1], rng), rng.integers(-24, 25, size=n).astype(np.int32))
    return _SETS[n]


@pytest.mark.parametrize("depth", [1, 4, 10])
@pytest.mark.parametrize("n", [1, 5, 64, 65, 4099])
def test_book_equals_the_restatement(n, depth):
    from brl_amd import book, boards
    rec_a, rec_b, imp = _random_set(n)
    # both tables with the IMPs: imp_sign +1 and -1
    records = boards.BoardRecords(_upload(rec_a), _upload(rec_b), torch.from_numpy(imp).to(DEV))
    sb = book.system_book(records, depth)
    _same(sb, B.book_of(rec_a, rec_b, depth, imp)[0])
    assert sb.has_imp and sb.depth == depth
    # one table without
    sb = book.system_book(_upload(rec_b), depth)
    _same(sb, B.book_of(rec_b, None, depth)[0])
    assert not sb.has_imp and not sb.imp_sum.any() and not sb.imp_sq_sum.any()


@pytest.mark.parametrize("sign", [1, -1])
def test_samples_take_the_tables_sign(sign):
    """brl_book_samples alone: keys, and the features' IMP byte for imp_sign +1 / -1"""
    from brl_amd import book
    rec, _, imp = _random_set(65)
    keys, feats = book.book_samples(_upload(rec), 10, torch.from_numpy(imp).to(DEV), sign)
    keys, feats = keys.cpu().numpy().view(np.uint64).reshape(65, 10), feats.cpu().numpy().view(np.uint32).reshape(65, 10)
    for i, r in enumerate(rec):
        for p in range(10):
            if p < int(r["n_calls"]):
                seat = (int(r["dealer"]) + p) % 4
                assert int(keys[i, p]) == B.key(r["calls"][:p + 1])
                assert (int(feats[i, p]) >> 24) == ((int(imp[i]) * sign * (1 if seat % 2 == 0 else -1)) & 0xFF)
                assert (int(feats[i, p]) >> 23) & 1 == ((int(r["seating"]) >> (2 * seat)) & 3) >> 1
            else:
                assert keys[i, p] == 0 and feats[i, p] == 0


def test_no_records_and_no_calls_give_an_empty_book():
    from brl_amd import book
    rng = np.random.default_rng(1)
    sb = book.system_book(torch.zeros((0, 368), dtype=torch.uint8, device=DEV), 4)
    assert len(sb) == 0 and sb.skipped == 0 and sb.to_text() == "" and sb.continuations("") == []
    rec = B.make_records([[]] * 7, rng)
    sb = book.system_book(_upload(rec), 10)
    assert len(sb) == 0 and sb.skipped == 0
    with pytest.raises(ValueError):
        book.system_book(_upload(rec), 11)
    with pytest.raises(ValueError):
        book.system_book(_upload(rec), 0)


def test_records_without_the_ok_bit_give_no_samples():
    from brl_amd import book
    rec, _, imp = _random_set(4099)
    rng = np.random.default_rng(2)
    bad = rng.random(4099) < 0.1
    marked = rec.copy()
    marked["flags"][bad] &= ~np.uint8(8)
    sb = book.system_book(_upload(marked), 4)
    assert sb.skipped == int(bad.sum()) > 0
    # the remaining entries are those of the set without the marked records
    _same(sb, B.book_of(rec[~bad], None, 4)[0], skipped=int(bad.sum()))
    ref, skipped = B.book_of(marked, None, 4)
    _same(sb, ref, skipped)
    none = marked.copy()
    none["flags"] &= ~np.uint8(8)
    sb = book.system_book(_upload(none), 4)
    assert len(sb) == 0 and sb.skipped == 4099


def _distinct_auctions(n):
    """n unfinished ten-call auctions bid P bid P ... whose five bids enumerate the index in base 6 (each bid 1..6 steps above
    the one before: always legal): every depth-10 prefix is an entry of its own, the shallower ones are shared"""
    out = []
    for i in range(n):
        calls, bid, k = [], 2, i
        for _ in range(5):
            bid += 1 + k % 6
            k //= 6
            calls += [bid, 0]
        assert k == 0 and bid < 38
        out.append(calls)
    assert len({tuple(c) for c in out}) == n
    return out


@pytest.fixture(scope="module")
def hot_and_cold():
    rng = np.random.default_rng(77)
    hot = [[0, 0, 8, 0, 12, 0, 0, 0]] * 4099                      # P P 2C P 2NT P P P: one run per prefix, across every chunk
    cold = _distinct_auctions(4099)
    imp = rng.integers(-24, 25, size=4099).astype(np.int32)
    return B.make_records(hot, rng), B.make_records(cold, rng), imp


@pytest.mark.parametrize("which", ["hot", "cold", "interleaved"])
def test_hot_runs_singletons_and_the_two_interleaved(hot_and_cold, which):
    from brl_amd import book, boards
    hot, cold, imp = hot_and_cold
    if which == "interleaved":
        rec = np.empty(8198, hot.dtype)
        rec[0::2], rec[1::2] = hot, cold
        imp = np.repeat(imp, 2)
    else:
        rec = hot if which == "hot" else cold
    for depth in (4, 10):
        ref = B.book_of(rec, None, depth, imp)[0]
        sb = book.system_book(boards.BoardRecords(_upload(rec), None, torch.from_numpy(imp).to(DEV)), depth)
        _same(sb, ref)
        if which == "hot":
            assert len(sb) == min(depth, 8) and (sb.count.sum(1) == 4099).all()
        if which == "cold" and depth == 10:
            assert (sb.count.sum(1)[book.key_depth(sb.keys) == 10] == 1).all() and (book.key_depth(sb.keys) == 10).sum() == 4099


def test_hand_extremes():
    """37 and 0 HCP, a 13-card suit, each balanced shape and its nearest unbalanced neighbour"""
    from brl_amd import book
    shapes = [(4, 3, 3, 3), (3, 3, 3, 4), (4, 4, 3, 2), (2, 4, 3, 4), (5, 3, 3, 2), (3, 2, 5, 3),      # balanced
              (5, 4, 2, 2), (4, 4, 4, 1), (6, 3, 2, 2), (2, 2, 4, 5), (1, 4, 4, 4), (2, 6, 3, 2),      # their neighbours
              (13, 0, 0, 0), (0, 0, 0, 13), (0, 13, 0, 0), (0, 0, 13, 0), (7, 6, 0, 0), (5, 5, 3, 0)]
    hands = [B.shaped_hand(s, top) for s in shapes for top in (True, False)]
    hands.append(B.hand_word([(12, s) for s in range(4)] + [(11, s) for s in range(4)] + [(10, s) for s in range(4)] + [(9, 0)]))   # 37 HCP
    hands.append(B.hand_word([(r, s) for r in range(3) for s in range(4)] + [(3, 0)]))                                             # 0 HCP
    rng = np.random.default_rng(4)
    rows = []
    for k in range(len(hands)):
        rows.append([hands[(k + s) % len(hands)] for s in range(4)])     # every hand in every seat
    rec = B.make_records([[3 + (k * 7) % 35, 0, 0, 0] for k in range(len(rows))], rng, hands=rows)
    ref = B.book_of(rec, None, 4)[0]
    sb = book.system_book(_upload(rec), 4)
    _same(sb, ref)
    pooled = sb.hcp_hist.sum((0, 1))
    assert pooled[37] > 0 and pooled[0] > 0 and sb.length_hist.sum((0, 1))[:, 13].all() and 0 < sb.balanced.sum() < sb.count.sum()


def test_two_runs_give_the_same_bytes():
    from brl_amd import book
    rec, _, imp = _random_set(4099)
    dev_rec, dev_imp = _upload(rec), torch.from_numpy(imp).to(DEV)
    runs = []
    for _ in range(2):
        keys, feats = book.book_samples(dev_rec, 4, dev_imp, 1)
        top = torch.tensor(-2 ** 63, dtype=torch.int64, device=DEV)
        ordered, perm = torch.sort(torch.bitwise_xor(keys, top))
        unique, inverse = torch.unique_consecutive(ordered, return_inverse=True)
        has0 = int(unique[0] == top)
        entries = book.book_reduce(feats[perm], (inverse - has0).to(torch.int32), torch.bitwise_xor(unique[has0:], top).contiguous())
        runs.append(entries.cpu().numpy().tobytes())
    assert runs[0] == runs[1] and len(runs[0]) % 816 == 0 and len(runs[0]) > 0


# ---- a duplicate match, end to end ----------------------------------------------------------------------------------------------
def _nets(seeds=(1, 2)):
    from brl_amd.models import make_forward_pass
    fp = make_forward_pass("relu", "DeepMind")
    return [fp.init(s, device=DEV) for s in seeds]


def test_the_book_of_a_match(dds):
    import brl_amd
    from brl_amd import book, boards
    env = brl_amd.BridgeBidding(lut=(dds["keys"], dds["values"]), device=DEV)
    net1, net2 = _nets()
    _, records = boards.make_board_match(env, "relu", "DeepMind", "relu", "DeepMind", 640)(net1, net2, 5)
    sb = book.system_book(records, 4)
    ra, rb, imp = records.cpu("a"), records.cpu("b"), records.imp.cpu().numpy()
    ref, skipped = B.book_of(ra, rb, 4, imp)
    _same(sb, ref, skipped)
    depth = book.key_depth(sb.keys)
    # every record with a call has one depth-1 sample
    assert sb.count[depth == 1].sum() == int((ra["n_calls"] > 0).sum() + (rb["n_calls"] > 0).sum()) == 1280
    assert np.array_equal(sb.hcp_hist.sum(2), sb.count)
    assert np.array_equal(sb.length_hist.sum(3), np.repeat(sb.count[:, :, None], 4, axis=2))
    for i, k in enumerate(sb.keys):
        kids = sb.continuations(int(k))
        assert sb.count[i].sum() >= sum(c["count"] for c in kids)
    # the dealer's IMP, summed over team 1's openings: +imp when the dealer sits North-South at table A, -imp at table B
    want = 0
    for rec, sign in ((ra, 1), (rb, -1)):
        dealer = rec["dealer"].astype(np.int64)
        team1 = ((rec["seating"] >> (2 * dealer)) & 3) < 2
        want += int((imp * sign * np.where(dealer % 2 == 0, 1, -1))[team1].sum())
    assert int(sb.imp_sum[depth == 1, 0].sum()) == want
    # a subset is taken by indexing the records before the call
    north = torch.from_numpy(ra["dealer"] == 0).to(DEV)
    sub = boards.BoardRecords(records.table_a[north], records.table_b[north], records.imp[north])
    _same(book.system_book(sub, 4), B.book_of(ra[ra["dealer"] == 0], rb[ra["dealer"] == 0], 4, imp[ra["dealer"] == 0])[0])


def test_the_command_line_writes_the_book(tmp_path, dds):
    import brl_amd
    from brl_amd import book, boards, checkpoint
    from brl_amd.models import make_forward_pass
    fp = make_forward_pass("relu", "DeepMind")
    for k in range(2):
        checkpoint.save_params(fp.init(50 + k), str(tmp_path / f"params-{k:08}.pt"))
    lut = tmp_path / "lut.npy"
    np.save(lut, np.stack([dds["keys"], dds["values"]]))
    envv = dict(os.environ, PYTHONPATH=ROOT)
    base = [sys.executable, "-m", "brl_amd.eval", f"team1_model_path={tmp_path / 'params-00000000.pt'}",
            f"team2_model_path={tmp_path / 'params-00000001.pt'}", "num_eval_envs=64", f"dds_path={lut}"]
    outs = []
    for extra in ([], [f"save_book={tmp_path / 'book.json'}", "book_min_count=1"]):
        r = subprocess.run(base + extra, cwd=tmp_path, env=envv, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(r.stdout.splitlines())
    assert outs[0][-1].startswith("IMP: ")
    assert outs[1] == outs[0][:-1] + [f"book: {tmp_path / 'book.json'}"] + outs[0][-1:]
    # the tree, through the same entry point in this process
    from brl_amd import eval as eval_cli
    said = []
    eval_cli.main(base[3:] + [f"save_book={tmp_path / 'book.txt'}", "book_depth=2"], log=said.append)
    assert said == outs[0][:-1] + [f"book: {tmp_path / 'book.txt'}"] + outs[0][-1:]
    # the same match in this process
    env = brl_amd.BridgeBidding(lut=(dds["keys"], dds["values"]), device=DEV)
    team = [checkpoint.load_params(str(tmp_path / f"params-{k:08}.pt"), "relu", "DeepMind", env.device) for k in range(2)]
    _, records = boards.make_board_match(env, "relu", "DeepMind", "relu", "DeepMind", 64)(team[0], team[1], 0)
    here = book.system_book(records, 4)
    assert book.SystemBook.from_json(str(tmp_path / "book.json")) == here and len(here) > 0
    assert open(tmp_path / "book.txt").read() == book.system_book(records, 2).to_text(min_count=20)
