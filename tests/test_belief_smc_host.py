"""CPU: the resample-move stages of the hand beliefs (include/brl_belief_smc.h) — the header against the binding, the two stream
constants, the numpy restatement (tests/belief_smc_ref.py) of the resampling and of the proposal on hand-made cases, the schedule
``belief.resample_stages`` derives from a prefix, and ``HandBelief``'s text and JSON with and without the new arrays."""
import json
import os
import re

import numpy as np
import pytest

from brl_amd import belief
from tests import belief_ref as BR
from tests import belief_smc_ref as SR
from tests import book_ref as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECK = (1 << 52) - 1


# ---- the header and the binding -------------------------------------------------------------------------------------------------
def test_the_header_states_what_the_binding_reads():
    text = open(os.path.join(ROOT, "include", "brl_belief_smc.h")).read()
    assert f"#define BRL_BELIEF_RESAMPLE_STREAM 0x{belief.RESAMPLE_STREAM:08X}u" in text
    assert f"#define BRL_BELIEF_MOVE_STREAM 0x{belief.MOVE_STREAM:08X}u" in text
    assert f"#define BRL_BELIEF_SMC_SEGMENT {SR.SEGMENT}\n" in text and f"#define BRL_BELIEF_SMC_MAX_MOVES {belief.MAX_MOVES}\n" in text
    assert (SR.RESAMPLE_STREAM, SR.MOVE_STREAM) == (belief.RESAMPLE_STREAM, belief.MOVE_STREAM)
    assert "brl_belief" not in open(os.path.join(ROOT, "include", "brl_hip.h")).read()
    # the entry does not change: the end is brl_belief_reduce's
    assert "BRL_BELIEF_ENTRY_BYTES 5328" in open(os.path.join(ROOT, "include", "brl_belief.h")).read() and belief.ENTRY_DTYPE.itemsize == 5328


def test_the_two_stream_constants_are_no_other_streams():
    streams = []
    for unit in ("bridge_device.hpp", "brl_sl.hip"):
        streams += re.findall(r"constexpr uint32_t (STREAM_\w+) = (0x[0-9A-Fa-f]+)u;", open(os.path.join(ROOT, "brl_amd", "csrc", unit)).read())
    values = dict((name, int(v, 16)) for name, v in streams)
    assert len(values) == len(streams) >= 7 and len(set(values.values())) == len(values)
    assert values["STREAM_BELIEF_RESAMPLE"] == belief.RESAMPLE_STREAM and values["STREAM_BELIEF_MOVE"] == belief.MOVE_STREAM
    assert values["STREAM_BELIEF"] == belief.STREAM
    # no other translation unit defines a stream of its own that these two could meet
    for name in os.listdir(os.path.join(ROOT, "brl_amd", "csrc")):
        if name not in ("bridge_device.hpp", "brl_sl.hip"):
            assert not re.findall(r"constexpr uint32_t STREAM_\w+ =", open(os.path.join(ROOT, "brl_amd", "csrc", name)).read()), name


# ---- the restated resampling -------------------------------------------------------------------------------------------------------
def test_the_cumulative_sum_is_the_headers_two_level_order():
    rng = np.random.default_rng(2)
    for K in (1, 63, 64, 65, 257, 4096, 4097):
        W = rng.random(K)
        C = SR.cumulative(W)
        want, offset = np.zeros(K), 0.0
        for s in range(0, K, 64):                       # the definition, one addition at a time
            inner = 0.0
            for k in range(s, min(K, s + 64)):
                inner = W[k] if k == s else inner + W[k]
                want[k] = offset + inner
            offset = offset + inner
        assert np.array_equal(C, want) and (np.diff(C) >= 0).all(), K
        assert np.array_equal(C[:64], np.cumsum(W[:64]))
        assert abs(C[-1] - W.sum()) <= K * 2.0 ** -52 * C[-1]


def test_equal_weights_resample_to_the_identity():
    """C_k = k + 1 and x_j = j + u exactly (K a power of two or not: (j + u) K / K is within rounding of j + u, u is at least
    2^-33 away from an integer), so a_j = j"""
    for K in (1, 2, 64, 257, 4096, 5000):
        for lw in (0.0, -7.25):
            for u in (SR.offset_u(5, 3, 2), float(SR.unit(0)), float(SR.unit(0xFFFFFFFF))):
                a, C, x = SR.resample(np.full(K, lw, np.float32), u)
                assert np.array_equal(C, np.arange(1, K + 1)) and np.array_equal(a, np.arange(K)), (K, lw, u)
    assert 0.0 < float(SR.unit(0)) < float(SR.unit(0xFFFFFFFF)) < 1.0


def test_every_index_is_drawn_floor_or_ceil_of_its_share():
    rng = np.random.default_rng(3)
    for K in (1, 64, 257, 4096):
        for spread in (0.5, 3.0, 40.0):
            logw = (rng.normal(size=K) * spread).astype(np.float32)
            a, C, x = SR.resample(logw, SR.offset_u(1, K, 7))
            assert (np.diff(a) >= 0).all() and a.min() >= 0 and a.max() < K
            W = np.exp(logw.astype(np.float64) - logw.max())
            share = K * W / C[-1]
            count = np.bincount(a, minlength=K)
            near = np.abs(share - np.round(share)) <= (2 * K + 8) * 2.0 ** -52 * np.maximum(share, 1.0)      # a share that is an integer within rounding
            ok = (count == np.floor(share)) | (count == np.ceil(share)) | (near & (np.abs(count - share) <= 1.0 + 1e-9))
            assert ok.all() and count.sum() == K, (K, spread)
    # one dominant sample takes every draw; a NaN weight or no weight at all leaves the query alone
    lw = np.full(300, -2000.0, np.float32)
    lw[17] = -3.0
    assert (SR.resample(lw, 0.3)[0] == 17).all()
    lw[5] = np.nan
    assert SR.resample(lw, 0.3)[0] is None and SR.resample(np.full(9, -np.inf, np.float32), 0.3)[0] is None


def test_the_offset_is_philox_with_the_documented_counter():
    w = BR.philox4x32_10(11, 0, SR.RESAMPLE_STREAM, 6, 7, 9)[0]
    assert SR.offset_u(7 + (9 << 32), 6, 11) == (float(w) + 0.5) / 2.0 ** 32
    ws = SR.move_words(7 + (9 << 32), 6, 11, 1, [4])
    assert [int(x[0]) for x in ws] == [int(x) for x in BR.philox4x32_10(4, (11 << 8) | 1, SR.MOVE_STREAM, 6, 7, 9)]


# ---- the restated proposal ---------------------------------------------------------------------------------------------------------
def test_a_proposal_exchanges_two_cards_between_two_hidden_hands():
    rng = np.random.default_rng(4)
    own_hands = [B.shaped_hand([3, 3, 3, 4]), B.shaped_hand([0, 4, 4, 5], top=False), B.shaped_hand([13, 0, 0, 0]), B.random_hands(rng)[0]]
    seen_pairs, seen_i, seen_j = set(), set(), set()
    for n, own in enumerate(own_hands):
        for seat in range(4):
            K = 400
            h = BR.sample_hands(seat, own, 11, n, np.arange(K))
            new, pick, w3 = SR.propose(seat, h, seed=11, q=n, t=3, m=1)
            assert (new[:, seat] == np.uint64(own)).all()                                   # the own hand
            assert (np.bitwise_or.reduce(new, axis=1) == np.uint64(DECK)).all()              # still a partition of the deck
            assert all(bin(int(x)).count("1") == 13 for x in new.reshape(-1))
            for k in range(K):
                changed = [s for s in range(4) if new[k, s] != h[k, s]]
                first, second = ((seat + 1 + x) & 3 for x in SR.PAIRS[pick[k, 0]])
                assert changed == sorted((first, second)) and seat not in changed           # exactly two hidden seats
                gone, came = int(h[k, first]) & ~int(new[k, first]), int(new[k, first]) & ~int(h[k, first])
                assert bin(gone).count("1") == 1 and bin(came).count("1") == 1               # exactly one card each way
                assert gone == SR.nth_card(h[k, first], pick[k, 1]) and came == SR.nth_card(h[k, second], pick[k, 2])
                assert int(new[k, second]) == (int(h[k, second]) ^ came) | gone
            seen_pairs |= set(pick[:, 0].tolist())
            seen_i |= set(pick[:, 1].tolist())
            seen_j |= set(pick[:, 2].tolist())
            # another move, stage or query index is another draw; the same one is the same
            assert not np.array_equal(SR.propose(seat, h, 11, n, 3, 0)[1], pick) and not np.array_equal(SR.propose(seat, h, 11, n, 4, 1)[1], pick)
            assert np.array_equal(SR.propose(seat, h, 11, n, 3, 1)[0], new)
    assert seen_pairs == {0, 1, 2} and seen_i == set(range(13)) and seen_j == set(range(13))
    # a hand word with too few cards: the proposal is the deal itself; bits 52..63 are dropped
    short = np.array([[1 << 0, 1 << 1, (1 << 2) | (1 << 60), 1 << 3]] * 2000, np.uint64)
    new, pick, _ = SR.propose(0, short, 1, 0, 0, 0)
    moved = (new != (short & np.uint64(DECK))).any(axis=1)
    assert (pick[moved, 1:] == 0).all() and moved.any() and (~moved).any() and not (new >> np.uint64(52)).any()


def test_the_acceptance_in_float64():
    inf, nan = np.inf, np.nan
    w3 = np.array([0, 0xFFFFFFFF, 0x80000000, 0x80000000, 5, 5, 5, 5, 5], np.uint64)
    logl = np.array([0.0, 0.0, -1.0, -1.0, nan, 0.0, -inf, 0.0, -inf], np.float32)
    new = np.array([-30.0, 0.0, -1.5, -2.0, 0.0, nan, -3.0, -inf, -inf], np.float32)
    # log(2^-33) = -22.9 against -30: no; log(1 - 2^-33) < 0: yes; log(0.5 + 2^-33) = -0.693 against -0.5 yes, against -1 no
    assert SR.accept(w3, logl, new).tolist() == [False, True, True, False, False, False, True, False, False]


# ---- the schedule ------------------------------------------------------------------------------------------------------------------
OWN = B.shaped_hand([3, 3, 3, 4])
TWELVE = ["1C", "1D", "1H", "1S", "2C", "2D", "2H", "2S", "3C", "3D", "3H", "3S"]


def test_the_schedule_follows_from_the_prefix():
    q = belief.BeliefQuery("S", OWN, "N", "None", TWELVE)          # South calls at 2, 6, 10; nine hidden calls
    hidden = [0, 1, 3, 4, 5, 7, 8, 9, 11]
    assert belief.resample_stages(q, 1) == hidden == SR.stages(2, 0, 12, 1)
    assert belief.resample_stages(q, 2) == [1, 4, 7, 9] == SR.stages(2, 0, 12, 2)
    assert belief.resample_stages(q, 9) == [11] and belief.resample_stages(q, 10) == [] == SR.stages(2, 0, 12, 10)
    assert belief.resample_stages(q, 0) == []
    # no prefix; a prefix whose only call is the own seat's
    assert belief.resample_stages(belief.BeliefQuery("S", OWN, "S", "None", []), 1) == []
    assert belief.resample_stages(belief.BeliefQuery("S", OWN, "S", "None", ["1C"]), 1) == [] == SR.stages(2, 2, 1, 1)
    # every dealer and seat against the restatement
    for dealer in range(4):
        for seat in range(4):
            for R in (1, 2, 3, 5):
                for T in (0, 1, 4, 12):
                    got = belief.resample_stages(belief.BeliefQuery(seat, OWN, dealer, "None", TWELVE[:T]), R)
                    assert got == SR.stages(seat, dealer, T, R)
    with pytest.raises(ValueError, match="resample_every"):
        belief.resample_stages(q, -1)
    with pytest.raises(ValueError, match="call 1"):              # an illegal prefix is refused here too
        belief.resample_stages(belief.BeliefQuery("S", OWN, "N", "None", ["1H", "1D"]), 1)


# ---- the result --------------------------------------------------------------------------------------------------------------------
def test_text_and_json_with_and_without_the_new_arrays(tmp_path):
    K = 300
    q0 = belief.BeliefQuery("W", OWN, "N", "Both", ["1S", "P"])
    q1 = belief.BeliefQuery("N", OWN, "E", "None", [])
    h0, h1 = BR.sample_hands(3, OWN, 0, 0, np.arange(K)), BR.sample_hands(0, OWN, 0, 1, np.arange(K))
    e = np.zeros(2, belief.ENTRY_DTYPE)
    for i, (seat, h) in enumerate(((3, h0), (0, h1))):
        for name, v in BR.reduce64(seat, h, np.zeros(K, np.float32), np.arange(K) % 3 == 0).items():
            e[name][i] = v
    plain = belief.HandBelief(e, [q0, q1], seed=4)
    assert plain.resamples is None and plain.proposals is None and plain.accepted is None and plain.distinct is None
    smc = {"resamples": [2, 0], "proposals": [1200, 0], "accepted": [455, 0], "distinct": [171, 300]}
    hb = belief.HandBelief(e, [q0, q1], seed=4, smc=smc)
    assert hb.resamples.tolist() == [2, 0] and hb.distinct.tolist() == [171, 300] and hb.accepted.dtype == np.int64
    assert hb.of(0)["distinct"] == 171 and "distinct" not in plain.of(0)
    # the text: only the second line differs, and it names the greedy column for what it now is
    a, b = plain.to_text(0).split("\n"), hb.to_text(0).split("\n")
    assert a[0] == b[0] and a[2:] == b[2:] and a[1] != b[1]
    assert a[1] == f"  {K} samples, effective {plain.ess[0]:.1f}, consistent with the greedy policy 100"
    assert "2 resamplings" in b[1] and "distinct deals 171" in b[1] and "moves taken 455 of 1200" in b[1]
    assert "greedy among soft particles 100" in b[1] and "consistent with the greedy policy" not in b[1]
    # JSON: the new arrays only when present; a file written without them reads back as it always did
    plain.to_json(tmp_path / "plain.json")
    hb.to_json(tmp_path / "smc.json")
    assert "smc" not in json.load(open(tmp_path / "plain.json")) and json.load(open(tmp_path / "smc.json"))["smc"] == smc
    back_plain, back = belief.HandBelief.from_json(tmp_path / "plain.json"), belief.HandBelief.from_json(tmp_path / "smc.json")
    assert back_plain.same_as(plain) and back_plain.resamples is None and back_plain.to_text(0) == plain.to_text(0)
    assert back.same_as(hb) and back.to_text(0) == hb.to_text(0) and back.seed == 4
    assert all(np.array_equal(getattr(back, name), getattr(hb, name)) for name in belief.SMC_FIELDS)
    without = {k: v for k, v in json.load(open(tmp_path / "smc.json")).items() if k != "smc"}
    assert without == json.load(open(tmp_path / "plain.json"))
