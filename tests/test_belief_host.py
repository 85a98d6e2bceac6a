"""CPU: the hand beliefs' header against the binding and the dtypes, the Python restatement (tests/belief_ref.py) of the sampler and
of the reduction on hand-made cases, query parsing, and ``HandBelief``'s text and JSON on hand-made entries."""
import os
import re

import numpy as np
import pytest

from brl_amd import belief, boards
from tests import belief_ref as BR
from tests import board_records_ref as R
from tests import book_ref as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECK = (1 << 52) - 1


def bid(level, strain):
    return 3 + 5 * (level - 1) + "CDHSN".index(strain)


def _entry(d):
    e = np.zeros(1, belief.ENTRY_DTYPE)
    for name, v in d.items():
        e[name][0] = v
    return e


# ---- the header and the binding -------------------------------------------------------------------------------------------------
def test_the_header_states_what_the_binding_and_the_host_read():
    text = open(os.path.join(ROOT, "include", "brl_belief.h")).read()
    assert f"#define BRL_BELIEF_ACTIONS {belief.ACTIONS}\n" in text and f"#define BRL_BELIEF_STREAM 0x{belief.STREAM:08X}u" in text
    assert f"#define BRL_BELIEF_ENTRY_BYTES {belief.ENTRY_DTYPE.itemsize}\n" in text and belief.QUERY_DTYPE.itemsize == 16
    assert (BR.STREAM, BR.HIDDEN) == (belief.STREAM, 39)
    for dt, struct in ((belief.QUERY_DTYPE, "brl_belief_query"), (belief.ENTRY_DTYPE, "brl_belief_entry")):
        body = re.search(r"typedef struct " + struct + r" \{(.*?)\} " + struct, text, re.S).group(1)
        fields = re.findall(r"^\s*(\w+) (\w+)((?:\[\d+\])*);", body, re.M)
        assert [f[1] for f in fields] == list(dt.names), struct
        for ctype, name, dims in fields:                    # every field's type and shape
            base, shape = dt.fields[name][0].base, dt.fields[name][0].shape
            assert base == np.dtype({"uint64_t": "<u8", "uint8_t": "u1", "double": "<f8", "float": "<f4", "uint32_t": "<u4"}[ctype]), name
            assert tuple(int(x) for x in re.findall(r"\d+", dims)) == shape, name
    assert [belief.QUERY_DTYPE.fields[n][1] for n in belief.QUERY_DTYPE.names] == [0, 8, 9, 10, 11, 12, 13]
    assert belief.ENTRY_DTYPE.fields["card"][1] == 32 and belief.ENTRY_DTYPE.fields["g_card"][1] == 3560
    assert "brl_belief" not in open(os.path.join(ROOT, "include", "brl_hip.h")).read()
    # the stream constant is no other stream's
    dev = open(os.path.join(ROOT, "brl_amd", "csrc", "bridge_device.hpp")).read()
    streams = re.findall(r"constexpr uint32_t (STREAM_\w+) = (0x[0-9A-Fa-f]+)u;", dev)
    streams += re.findall(r"constexpr uint32_t (STREAM_\w+) = (0x[0-9A-Fa-f]+)u;", open(os.path.join(ROOT, "brl_amd", "csrc", "brl_sl.hip")).read())
    values = [int(v, 16) for _, v in streams]
    assert dict(streams)["STREAM_BELIEF"].lower() == f"0x{belief.STREAM:08x}" and len(set(values)) == len(values) >= 5


# ---- the restated sampler ----------------------------------------------------------------------------------------------------------
OWN = B.shaped_hand([3, 3, 3, 4])                   # 37 points: the hidden hands hold three jacks
LOW = B.shaped_hand([3, 3, 3, 4], top=False)        # no points: the hidden hands hold all 40


def test_every_sample_partitions_the_deck_and_keeps_the_own_hand():
    rng = np.random.default_rng(5)
    own_hands = [OWN, B.shaped_hand([0, 4, 4, 5], top=False), B.shaped_hand([13, 0, 0, 0])] + [B.random_hands(rng)[0] for _ in range(3)]
    for i, own in enumerate(own_hands):
        for seat in range(4):
            h = BR.sample_hands(seat, own, seed=11, q=i, ks=np.arange(200))
            assert (h[:, seat] == np.uint64(own)).all()
            assert (np.bitwise_or.reduce(h, axis=1) == np.uint64(DECK)).all()
            assert all(bin(int(x)).count("1") == 13 for x in h.reshape(-1))
    # seats rotate with the own seat: the same shuffled cards go to (s + 1, 2, 3) & 3
    a, b = BR.sample_hands(0, OWN, 3, 0, np.arange(50)), BR.sample_hands(2, OWN, 3, 0, np.arange(50))
    for h in range(3):
        assert np.array_equal(a[:, (0 + 1 + h) & 3], b[:, (2 + 1 + h) & 3])
    # a different k, q or seed is a different deal
    base = BR.sample_hands(1, OWN, 3, 0, np.arange(64))
    assert len({x.tobytes() for x in base}) == 64
    assert not (BR.sample_hands(1, OWN, 3, 1, np.arange(64)) == base).all(axis=1).any()
    assert not (BR.sample_hands(1, OWN, 4, 0, np.arange(64)) == base).all(axis=1).any()
    assert not (BR.sample_hands(1, OWN, 3 + (1 << 32), 0, np.arange(64)) == base).all(axis=1).any()      # the seed's high word counts
    # the samples do not depend on which others are drawn with them
    assert np.array_equal(BR.sample_hands(1, OWN, 3, 0, [63, 5]), base[[63, 5]])


def test_the_stream_is_philox_with_the_documented_counter():
    """the first block of sample 0 of stream 0 under key (0, 0) is Random123's known answer for counter (0, 0, STREAM, 0) only if
    STREAM were 0: check the function itself on the all-zero vector, then that the counter words sit where the header says"""
    z = BR.philox4x32_10(0, 0, 0, 0, 0, 0)
    assert [int(x) for x in z] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    d = BR.draws(7 + (9 << 32), 5, [3])
    for j in (0, 3, 4, 37):
        want = BR.philox4x32_10(3, j >> 2, BR.STREAM, 5, 7, 9)[j & 3]
        assert int(d[0, j]) == int(want)


def test_the_sample_tables_are_the_encoders():
    h = BR.sample_hands(3, OWN, 1, 2, np.arange(4))
    seating = 2 | (0 << 2) | (3 << 4) | (1 << 6)
    tb = BR.sample_tables(1, 1, 0, seating, h)
    for k in range(4):
        want = R.encode(1, [], vul_ns=1, vul_ew=0, seating=(2, 0, 3, 1), hands=[int(x) for x in h[k]]).pack()
        assert np.array_equal(tb[k], want)


def test_the_prior_is_uniform():
    """T = 0: every hidden card is in each hidden hand with probability 1/3.  Over K samples a card's share has standard deviation
    sigma = sqrt((1/3)(2/3) / K) = sqrt(2 / 9K); all 3 x 39 shares lie within 5 sigma.  The mean HCP of each hidden hand is
    (40 - own HCP) / 3 within 5 of its standard errors.  (K and the seed are fixed; the restatement passes with them.)"""
    K, seed = 4096, 0
    h = BR.sample_hands(2, OWN, seed, 0, np.arange(K))
    e = BR.reduce64(2, h, np.zeros(K, np.float32), np.ones(K, np.uint8))
    assert e["wsum"] == K and e["wsq"] == K and e["consistent"] == K
    share = e["card"] / K
    hidden = np.array([not (OWN >> b) & 1 for b in range(52)])
    sigma = np.sqrt(2.0 / (9.0 * K))
    assert (share[:, ~hidden] == 0).all() and np.allclose(share[:, hidden].sum(0), 1.0)
    print(f"largest deviation of a card share from 1/3: {np.abs(share[:, hidden] - 1 / 3).max() / sigma:.2f} sigma")
    assert (np.abs(share[:, hidden] - 1.0 / 3.0) <= 5 * sigma).all()
    _, own_hcp, _, _ = BR.features(np.uint64(OWN))
    _, hcp, _, _ = BR.features(h[:, [3, 0, 1]])
    se = hcp.std(axis=0, ddof=1) / np.sqrt(K)
    assert (np.abs(hcp.mean(axis=0) - (40 - int(own_hcp)) / 3.0) <= 5 * se).all()
    assert np.allclose((e["hcp"] * np.arange(38)).sum(-1) / K, hcp.mean(axis=0))


# ---- the restated reduction on hand-made weights -----------------------------------------------------------------------------------
def test_the_reduction_on_hand_made_weights():
    K = 300
    h = BR.sample_hands(0, OWN, 2, 0, np.arange(K))
    bits, hcp, lengths, bal = BR.features(h[:, 1:4])
    # equal weights: the soft sums are the plain counts, whatever the common log-weight
    for lw in (0.0, -7.25):
        e = BR.reduce64(0, h, np.full(K, lw, np.float32), np.ones(K))
        assert e["wsum"] == K and e["wsq"] == K and e["max_logw"] == np.float32(lw)
        assert np.array_equal(e["card"], bits.sum(0)) and np.array_equal(e["card"], e["g_card"])
        assert np.array_equal(e["hcp"], e["g_hcp"]) and np.array_equal(e["length"], e["g_length"]) and np.array_equal(e["balanced"], e["g_balanced"])
        assert (e["hcp"].sum(-1) == K).all() and (e["length"].sum(-1) == K).all()
    # one dominant sample: the belief is that sample
    lw = np.full(K, -2000.0, np.float32)                  # exp(-1997) is 0 in float64
    lw[17] = -3.0
    e = BR.reduce64(0, h, lw, np.zeros(K))
    assert e["wsum"] == 1.0 and e["wsq"] == 1.0 and np.array_equal(e["card"], bits[17]) and e["max_logw"] == np.float32(-3.0)
    assert e["hcp"][np.arange(3), hcp[17]].tolist() == [1.0] * 3 and np.array_equal(e["balanced"], bal[17].astype(float))
    # consistent = 0: the integer block is empty, the soft block is not
    assert e["consistent"] == 0 and not e["g_card"].any() and not e["g_hcp"].any() and e["n"] == K
    # two samples at a known ratio
    lw = np.full(K, -np.inf, np.float32)
    lw[3], lw[4] = 0.0, np.float32(np.log(0.5))
    e = BR.reduce64(0, h, lw, np.arange(K) == 4)
    half = np.exp(np.float64(np.float32(np.log(0.5))))
    assert e["wsum"] == 1.0 + half and e["wsq"] == 1.0 + half * half
    assert np.array_equal(e["card"], bits[3] + half * bits[4]) and np.array_equal(e["g_card"], bits[4]) and e["consistent"] == 1
    # a NaN weight: the weighted block is NaN throughout, the integers are not touched
    lw = np.zeros(K, np.float32)
    lw[9] = np.nan
    greedy = np.arange(K) % 3 == 0
    e = BR.reduce64(0, h, lw, greedy)
    assert all(np.isnan(np.asarray(e[name])).all() for name in BR.FLOAT_FIELDS) and np.isnan(e["max_logw"])
    assert e["consistent"] == 100 and np.array_equal(e["g_card"], bits[greedy].sum(0))
    # every weight zero (all -inf): no belief either
    e = BR.reduce64(0, h, np.full(K, -np.inf, np.float32), greedy)
    assert np.isnan(e["wsum"]) and np.isnan(e["card"]).all()
    # the comparison helper accepts what it is given and refuses an integer that is off by one
    dev = _entry(BR.reduce64(0, h, np.zeros(K, np.float32), greedy))[0]
    assert BR.compare_entry(dev, BR.reduce64(0, h, np.zeros(K, np.float32), greedy), K) == 0.0
    dev["g_hcp"][1, 9] += 1
    with pytest.raises(AssertionError):
        BR.compare_entry(dev, BR.reduce64(0, h, np.zeros(K, np.float32), greedy), K)


def test_the_features_are_the_books():
    rng = np.random.default_rng(8)
    for _ in range(50):
        w = B.random_hands(rng)[0]
        names = boards.hand_names(w)
        bits, hcp, lengths, bal = BR.features(np.uint64(w))
        assert int(hcp) == sum(B.POINTS.get(c[1], 0) for c in names)
        assert lengths.tolist() == [sum(1 for c in names if c[0] == s) for s in "CDHS"]
        assert bool(bal) == (sorted(lengths.tolist()) in B.BALANCED)


# ---- queries -------------------------------------------------------------------------------------------------------------------
def test_queries_are_parsed_and_illegal_prefixes_refused():
    q = belief.BeliefQuery("S", "AQ5.KT93.8.QJ762", "N", "NS", ["1H", "P"], seating=(2, 0, 3, 1))
    assert (q.seat, q.dealer, q.vul_ns, q.vul_ew, q.calls) == (2, 0, 1, 0, [bid(1, "H"), 0])
    assert q.seating == 2 | (0 << 2) | (3 << 4) | (1 << 6) and q.team_at(0) == 1 and q.team_at(1) == 0
    assert boards.pbn_deal([q.hand] * 4).split()[1] == "AQ5.KT93.8.QJ762" and belief.hand_text(q.hand) == "AQ5.KT93.8.QJ762"
    same = belief.BeliefQuery(2, q.hand, 0, (1, 0), [bid(1, "H"), "P"], seating=q.seating)
    assert same == q and belief.BeliefQuery.from_label(q.label()) == q
    plan = q.plan()
    assert [p[0] for p in plan] == [0, 1] and plan[0][1] == (1 << 38) - 1 - 6 and plan[1][2] == 0
    assert plan[1][1] == 1 | 2 | (((1 << 38) - 1) >> (3 + 3) << (3 + 3))         # pass, double, every bid above 1H
    arr = belief.query_array([q])
    assert arr.tobytes() == int(q.hand).to_bytes(8, "little") + bytes([2, 0, 1, 0, q.seating, 0, 0, 0])
    for bad_hand in ("AQ5.KT93.8.QJ76", "AQ5.KT93.8.QJ7622", "AQ5.KT93.8", "AQ5.KT93.8.QJ76Z", (1 << 14) - 1):
        with pytest.raises(ValueError, match="hand"):
            belief.BeliefQuery(0, bad_hand, 0, "None", [])
    for kw, what in ((dict(seat=4), "seat"), (dict(dealer="X"), "dealer"), (dict(vul="All"), "vul"), (dict(seating=(0, 1, 2, 2)), "seating"),
                     (dict(calls=["1Z"]), "call")):
        args = dict(seat=0, hand=OWN, dealer=0, vul="None", calls=[])
        args.update(kw)
        with pytest.raises(ValueError, match=what):
            belief.BeliefQuery(**args)
    # an illegal prefix is refused with the query and the call named, before anything is sampled
    cases = [(["1H", "1D"], r"query 3: call 1 \(1D\)"), (["X"], r"query 3: call 0 \(X\)"), (["1H", "P", "X"], r"call 2 \(X\)"),
             (["1H", "X", "P", "XX"], r"call 3 \(XX\)"), (["P", "P", "P", "P", "P"], r"call 4 \(P\).*over"), ([38], r"call 0 \(38\)")]
    for calls, pattern in cases:
        with pytest.raises(ValueError, match=pattern):
            belief.BeliefQuery(0, OWN, 1, "None", calls).plan(3)
    # a prefix that ends the auction is accepted: the belief at the opening lead
    done = belief.BeliefQuery(0, OWN, 1, "None", ["1NT", "X", "XX", "P", "P", "P"]).plan()
    assert len(done) == 6 and (done[2][1] >> 2) & 1 and [p[0] for p in done] == [1, 2, 3, 0, 1, 2]
    assert len(belief.BeliefQuery(0, OWN, 1, "None", R.longest_auction()).plan()) == 319
    # the host's legal words are the encoder's
    rng = np.random.default_rng(12)
    for _ in range(30):
        calls = R.random_auction(rng)
        d = int(rng.integers(0, 4))
        got = belief.BeliefQuery(0, OWN, d, "None", calls).plan()
        assert [(s, w) for s, w, _ in got] == [(s, w) for s, w in BR.legal_words(d, calls)]


def test_queries_from_records():
    rng = np.random.default_rng(3)
    rec = B.make_records([[bid(1, "S"), 0, bid(2, "S"), 0, 0, 0], [0, 0, 0, 0]], rng)
    records = boards.BoardRecords(rec)
    (q,) = belief.queries_from_records(records, "a", 0, 2)
    r = rec[0]
    seat = (int(r["dealer"]) + 2) & 3
    assert q == belief.BeliefQuery(seat, int(r["hands"][seat]), int(r["dealer"]), (int(r["vul_ns"]), int(r["vul_ew"])),
                                   ["1S", "P"], int(r["seating"]))
    qs = belief.queries_from_records(records, "a", [0, 1, 1], [6, 0, 4])
    assert [len(x.calls) for x in qs] == [6, 0, 4] and qs[1].seat == int(rec[1]["dealer"])
    with pytest.raises(ValueError, match="call index"):
        belief.queries_from_records(records, "a", 1, 5)


# ---- the result --------------------------------------------------------------------------------------------------------------------
def test_hand_belief_text_and_json(tmp_path):
    K = 500
    q0 = belief.BeliefQuery("W", LOW, "N", "Both", ["1S", "P"])
    q1 = belief.BeliefQuery("N", LOW, "E", "None", [])
    h0, h1 = BR.sample_hands(3, LOW, 0, 0, np.arange(K)), BR.sample_hands(0, LOW, 0, 1, np.arange(K))
    _, hcp, _, _ = BR.features(h0[:, 0])
    lw = (0.5 * (hcp - 10)).astype(np.float32)             # North, the opener's seat, is stronger in the soft belief
    greedy = hcp >= 12
    e = np.concatenate([_entry(BR.reduce64(3, h0, lw, greedy)), _entry(BR.reduce64(0, h1, np.r_[np.nan, np.zeros(K - 1)], np.zeros(K)))])
    hb = belief.HandBelief(e, [q0, q1], seed=0)
    assert len(hb) == 2 and hb.seats.tolist() == [[0, 1, 2], [1, 2, 3]] and hb.n.tolist() == [K, K]
    assert hb.consistent.tolist() == [int(greedy.sum()), 0]
    assert hb.card_prob.shape == (2, 3, 52) and hb.hcp_hist.shape == (2, 3, 38) and hb.length_hist.shape == (2, 3, 4, 14)
    assert np.allclose(hb.card_prob[0].sum(0)[[not (LOW >> b) & 1 for b in range(52)]], 1.0)
    assert np.allclose(hb.hcp_hist[0].sum(-1), 1.0) and np.allclose(hb.length_mean[0].sum(-1), 13.0)
    assert hb.hcp_mean[0, 0] > hcp.mean() + 1 and hb.greedy_hcp_mean[0, 0] >= 12 and 1 < hb.ess[0] < K
    assert np.isclose(hb.greedy_hcp_mean[0, 0], hcp[greedy].mean())
    assert np.isnan(hb.card_prob[1]).all() and np.isnan(hb.greedy_card_prob[1]).all() and np.isnan(hb.ess[1])
    d = hb.of(0)
    assert list(d["hidden"]) == ["N", "E", "S"] and d["n"] == K and d["consistent"] == int(greedy.sum())
    lo, hi = d["hidden"]["N"]["soft"]["hcp_range"]
    assert 0 <= lo <= d["hidden"]["N"]["soft"]["hcp_mean"] <= hi <= 37 and len(d["hidden"]["N"]["soft"]["cards"]) == 39
    text = hb.to_text(0)
    assert text.startswith(f"belief 0: W holds {belief.hand_text(LOW)}; dealer N, vul Both; auction 1S P")
    assert f"{K} samples, effective {hb.ess[0]:.1f}, consistent with the greedy policy {int(greedy.sum())}" in text
    assert text.count("\n") == 7 and all(f"\n  {s}: HCP " in text for s in "NES") and "most likely honours" in text and " | " in text
    assert "nan" in hb.to_text(1) and "auction (none)" in hb.to_text(1)          # a starved belief shows
    hb.to_json(tmp_path / "belief.json")
    back = belief.HandBelief.from_json(tmp_path / "belief.json")
    assert back.same_as(hb) and back.to_text(0) == text and back.seed == 0
    other = belief.HandBelief(e[::-1].copy(), [q1, q0])
    assert not other.same_as(hb)
