"""The float64 reference of the policy sampler (tests/categorical_ref.py) checked on the CPU: against torch's
Categorical, against the plain inverse CDF, how often it leaves a sampler a choice, and the committed draws at the
two ends of the 24-bit range."""
import json
import os

import numpy as np
import pytest
import torch

from tests.categorical_cases import FAMILIES, make_rows, stepped_states
from tests.categorical_ref import BAND, TOP, U24, accept_matrix, accept_set, cdf64, inverse_cdf64, log_softmax64, mode64
from tests.conftest import GOLDEN

SEED, N, DRAWS = 19, 120, 16


@pytest.fixture(scope="module")
def rows(oracle):
    """per family: masked logits [N, 38], the candidates, and the 24-bit draws [DRAWS, N] of the oracle"""
    ref, _ = stepped_states(oracle, N, SEED)
    mask = ref["legal_action_mask"].astype(np.uint8)
    u24 = np.array([[oracle.action_draw(SEED, e, d) >> 8 for e in range(N)] for d in range(DRAWS)])
    rng = np.random.default_rng(5)
    return {f: (make_rows(rng, [f] * N, mask, True), mask, u24) for f in FAMILIES}


@pytest.mark.parametrize("family", FAMILIES)
def test_log_softmax_and_mode_match_torch_categorical(rows, family):
    logits, mask, _ = rows[family]
    masked = torch.where(torch.from_numpy(mask.astype(bool)), torch.from_numpy(logits).double(), -torch.inf)
    pi = torch.distributions.Categorical(logits=masked, validate_args=False)
    want = pi.logits.numpy()
    got = log_softmax64(logits, mask)
    fin = np.isfinite(want)
    assert np.array_equal(fin, np.isfinite(got)) and np.array_equal(got[~fin], want[~fin])
    assert np.allclose(got[fin], want[fin], rtol=1e-13, atol=1e-13)
    assert np.array_equal(mode64(logits, mask), masked.argmax(dim=1).numpy())
    assert mask[np.arange(N), mode64(logits, mask)].all()


@pytest.mark.parametrize("family", FAMILIES)
def test_accept_set_is_the_inverse_cdf_away_from_cell_edges(rows, family):
    logits, mask, u24 = rows[family]
    c = cdf64(logits, mask)
    seen = 0
    for d in range(DRAWS):
        acc = accept_matrix(logits, mask, u24[d])
        u = u24[d] * U24
        clear = (np.abs(c - u[:, None]) > BAND).all(axis=1) & (u > BAND) & (u < TOP - BAND)
        for i in np.nonzero(clear)[0]:
            assert accept_set(logits[i], mask[i], int(u24[d, i])) == {inverse_cdf64(logits[i], mask[i], u[i])}
            assert acc[i].sum() == 1
        seen += int(clear.sum())
    assert seen > 0.9 * N * DRAWS
    assert (accept_matrix(logits, mask, u24[0]) <= mask.astype(bool)).all()      # never an illegal call


@pytest.mark.parametrize("family", FAMILIES)
def test_share_of_draws_that_leave_a_choice(rows, family):
    """37 cell edges x 2 * BAND = 3e-4 of the draw range lies within BAND of an edge; the cap is 1 %"""
    logits, mask, u24 = rows[family]
    multi = sum(int((accept_matrix(logits, mask, u24[d]).sum(axis=1) > 1).sum()) for d in range(DRAWS))
    none = sum(int((accept_matrix(logits, mask, u24[d]).sum(axis=1) == 0).sum()) for d in range(DRAWS))
    assert none == 0
    assert multi <= 0.01 * N * DRAWS, (family, multi)


def test_accept_set_at_the_ends_of_the_range():
    cand = np.ones(38, np.uint8)
    logits = np.zeros(38)
    logits[37] = -30.0                       # a last call of probability 2.5e-15: no draw reaches its cell
    assert accept_set(logits, cand, (1 << 24) - 1) == {36}
    assert accept_set(logits, cand, 0) == {0}
    logits[0] = -np.inf                      # an empty first cell is never first
    assert accept_set(logits, cand, 0) == {1}
    logits = np.full(38, -40.0)              # thin cells in front of the mass: within BAND of u = 0, all acceptable
    logits[20] = 0.0
    assert accept_set(logits, cand, 0) == set(range(21))
    assert accept_set(logits, cand, 1 << 23) == {20}
    assert accept_set(logits, cand, (1 << 24) - 1) == {20}


def test_committed_extreme_draws_are_what_they_claim(oracle):
    with open(os.path.join(GOLDEN, "extreme_draws.json")) as f:
        ends = json.load(f)
    want = {"top": (1 << 24) - 1, "top_minus_1": (1 << 24) - 2, "one": 1, "zero": 0}
    assert set(ends) == set(want)
    for name, triples in ends.items():
        assert len(triples) >= 2
        for t in triples:
            assert t["u24"] == want[name] and t["env_id"] >= 66
            assert oracle.action_draw(t["seed"], t["env_id"], t["draw"]) >> 8 == want[name], t
