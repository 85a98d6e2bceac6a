"""Logit rows for the sampler tests (tests/test_categorical_host.py, tests/test_gpu_categorical.py): what a trained
bidding network produces and what breaks samplers — peaked rows, exact ties, underflowing tails, non-finite values on
calls the mask rules out.  Plain numpy; masks come from the CPU oracle."""
import numpy as np

from tests.gpu_util import random_legal_actions

FAMILIES = ("flat", "peaked8", "peaked20", "peaked40", "onehot", "ties", "single", "max_on_illegal", "poisoned",
            "neg_inf_legal")
SINGLE_LEGAL_CALLS = (37, 1, 2)   # 7NT, double, redouble from the deal: only Pass stays legal


def stepped_states(oracle, n, seed, env_offset=0, steps=3, rng=None, forced=True):
    """Oracle states `steps` legal calls past the deal and the calls made ([steps, n] int32): with `forced` every fifth
    table bids 7NT - X - XX (one legal call left: Pass); the others call at random, so that the masks vary."""
    rng = rng or np.random.default_rng(seed)
    ref = oracle.init_random(n, seed=seed, env_offset=env_offset)
    calls = np.zeros((steps, n), np.int32)
    for s in range(steps):
        act = random_legal_actions(rng, ref["legal_action_mask"])
        if forced and s < len(SINGLE_LEGAL_CALLS):
            act[::5] = SINGLE_LEGAL_CALLS[s]
        calls[s] = act
        oracle.step(ref, act)
    return ref, calls


def family_of_rows(n, shift=0):
    """row i's family: a cycle through FAMILIES starting at `shift` (batches of 1 and 3 rows still vary with shift)"""
    return [FAMILIES[(i + shift) % len(FAMILIES)] for i in range(n)]


def make_row(rng, family, mask, masked, fp16=False):
    """One float32 row of `family`.  mask: the table's 0/1 legal mask; masked: whether the policy under test ranges over
    the legal calls only (then `illegal` entries may hold anything) or over all 38.  A family a row cannot express
    (no illegal call, a single legal call, the unmasked policy for `poisoned`) falls back to `flat`."""
    legal = np.nonzero(mask)[0]
    illegal = np.nonzero(mask == 0)[0]
    cand = legal if masked else np.arange(38)
    row = (rng.standard_normal(38) * 2).astype(np.float32)
    if family.startswith("peaked"):
        row = (rng.standard_normal(38) * float(family[6:])).astype(np.float32)
    elif family == "onehot":
        row = rng.uniform(-60.0, 0.0, 38).astype(np.float32)
        row[rng.choice(legal)] = 60.0
    elif family == "ties":
        row = rng.integers(-3, 4, 38).astype(np.float32)
        if rng.random() < 0.25:
            row[:] = float(rng.integers(-3, 4))
    elif family == "single":
        keep = rng.choice(legal)
        row = np.full(38, -np.inf, np.float32)
        row[keep] = np.float32(rng.standard_normal() * 8)
    elif family == "max_on_illegal" and masked and len(illegal):
        row[rng.choice(illegal)] = row.max() + np.float32(5.0)
    elif family == "poisoned" and masked and len(illegal):
        big = 65504.0 if fp16 else 3e38
        poison = np.array([np.inf, -np.inf, np.nan, big, -big], np.float32)
        row[illegal] = poison[(np.arange(len(illegal)) + rng.integers(5)) % 5]
    elif family == "neg_inf_legal" and len(cand) > 1:
        k = rng.integers(1, len(cand))
        row[rng.choice(cand, size=k, replace=False)] = -np.inf
    return row


def make_rows(rng, families, mask, masked, fp16=False):
    return np.stack([make_row(rng, f, mask[i], masked, fp16) for i, f in enumerate(families)])
