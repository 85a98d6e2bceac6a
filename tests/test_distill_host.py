"""CPU checks of policy distillation (brl_amd/distill.py, include/brl_distill.h): the header against the binding, and the numpy
restatement of the definition (tests/distill_ref.py) against finite differences of its own total and the definition's identities."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import distill_ref as R  # noqa: E402


def test_distill_header_matches_the_binding():
    from brl_amd import _capi
    from brl_amd import build
    build.build()
    assert _capi.lib().brl_version() == 6      # (the prototypes against the argtypes: tests/test_capi_cpu.py, every header)


def _small(K, seed, B=9):
    z, u, t, v, w, mask = R.inputs(B, K, seed)
    z, t = z.astype(np.float64) / 8.0, t.astype(np.float64) / 8.0     # (+-60 logits leave finite differences nothing to resolve)
    return z, u.astype(np.float64), t, v.astype(np.float64), w.astype(np.float64) / w.astype(np.float64).sum(), mask


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("tau", [0.5, 1.0, 2.0])
def test_restated_gradients_are_the_finite_differences_of_the_total(tau, K):
    z, u, t, v, w, mask = _small(K, seed=7)
    c_pol, c_val, h = 0.7, 0.3, 1e-6
    out = R.restate(z, u, t, v, w, mask, tau, c_pol, c_val)
    f = lambda zz, uu: R.total(zz, uu, t, v, w, mask, tau, c_pol, c_val)     # noqa: E731
    fd_z = np.zeros_like(z)
    for b in range(z.shape[0]):
        for j in range(R.NA):
            zp, zm = z.copy(), z.copy()
            zp[b, j] += h
            zm[b, j] -= h
            fd_z[b, j] = (f(zp, u) - f(zm, u)) / (2 * h)
    fd_u = np.zeros_like(u)
    for b in range(u.shape[0]):
        up, um = u.copy(), u.copy()
        up[b] += h
        um[b] -= h
        fd_u[b] = (f(z, up) - f(z, um)) / (2 * h)
    assert np.abs(out["dz"] - fd_z).max() <= 1e-8, np.abs(out["dz"] - fd_z).max()
    assert np.abs(out["du"] - fd_u).max() <= 1e-8, np.abs(out["du"] - fd_u).max()
    assert (fd_z[~mask] == 0.0).all()


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("tau", [0.5, 1.0, 2.0])
def test_restatement_keeps_the_definitions_identities(tau, K):
    z, u, t, v, w, mask = R.inputs(200, K, seed=8)
    w = w.astype(np.float64) / w.astype(np.float64).sum()
    out = R.restate(z.astype(np.float64), u, t.astype(np.float64), v, w, mask, tau)
    assert (out["policy_loss"] >= -1e-12).all()                      # tau^2 KL(q || p)
    assert np.abs(out["dz"].sum(1)).max() <= 1e-15
    assert (out["dz"][~mask] == 0.0).all()
    assert np.abs(out["q"].sum(1) - 1.0).max() <= 1e-12 and (out["q"][~mask] == 0.0).all()
    ent = -np.sum(np.where(out["q"] > 0, out["q"] * np.log(np.where(out["q"] > 0, out["q"], 1.0)), 0.0), axis=1)
    assert np.abs(out["hq"] - ent).max() <= 1e-12


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("tau", [0.5, 1.0, 2.0])
def test_one_teacher_and_the_same_logits_give_zeros(tau, dtype):
    z, u, t, v, _, mask = R.inputs(200, 1, seed=9)
    out = R.restate(t[0], u, t, v, np.ones(1), mask, tau, dtype=dtype)
    assert (out["policy_loss"] == 0.0).all() and (out["dz"] == 0.0).all()
    assert out["metrics"][1] == 0.0 and out["metrics"][5] == 1.0


def test_mixture_weights_are_normalised_in_float64():
    from brl_amd.distill import mixture_weights
    assert mixture_weights(None, 1).tolist() == [1.0] and mixture_weights("3", 1).tolist() == [1.0]
    w = mixture_weights("0.75,0.25", 2)
    assert w.dtype == np.float32 and w.tolist() == [0.75, 0.25]
    assert np.array_equal(mixture_weights([3, 1], 2), w)
    for bad in ([1.0], [1.0, 0.0], [1.0, -1.0], [1.0, float("nan")]):
        with pytest.raises(ValueError):
            mixture_weights(bad, 2)
    with pytest.raises(ValueError):
        mixture_weights(None, 9)


def test_cli_names_follow_the_issue():
    from brl_amd.distill import DISTILL_DEFAULTS
    from brl_amd.train import parse_cli
    names = {"teacher_model_path", "teacher_weights", "type_of_model", "activation", "initial_model_path", "dds_path", "num_envs",
             "num_steps", "iterations", "update_epochs", "minibatch_size", "learning_rate", "tau", "policy_coef", "value_coef",
             "behaviour", "teacher_iterations", "eval_every", "num_eval_envs", "save_path", "rng_seed"}
    assert names <= set(DISTILL_DEFAULTS)
    cfg = parse_cli(["teacher_model_path=a.pt,b.pkl", "teacher_weights=0.75,0.25", "tau=2", "behaviour=student"], defaults=DISTILL_DEFAULTS)
    assert cfg["teacher_model_path"] == "a.pt,b.pkl" and cfg["teacher_weights"] == "0.75,0.25" and cfg["tau"] == 2.0
    with pytest.raises(SystemExit):
        parse_cli(["anchor_coef=1"], defaults=DISTILL_DEFAULTS)
