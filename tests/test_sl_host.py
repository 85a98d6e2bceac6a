"""CPU checks of the supervised pre-trainer (brl_amd/sl.py, brl_amd/sl_data.py, include/brl_sl.h): the trajectory parser and
its rejects, the packed hands, the example stream's numpy restatement, the loss and its gradient in float64 against torch
autograd, the config, the missing-data exit, the checkpoint round trip and the binding's argument types."""
import ctypes
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sl_teacher as T  # noqa: E402
from brl_amd import sl_data  # noqa: E402


def _deal(seed=0):
    return np.random.default_rng(seed).permutation(52)


def test_parser_strips_the_play_and_keeps_pass_outs():
    d0, d1 = _deal(0), _deal(1)
    calls = [0, 3 + 5, 1, 2, 0, 0, 0]   # P 2C X XX P P P
    text = T.line(d0, calls, np.random.default_rng(2)) + "\n" + T.line(d1, [0, 0, 0, 0]) + "\n"
    assert len(text.split("\n")[0].split()) == 52 + len(calls) + 52
    assert len(text.split("\n")[1].split()) == 56
    ts = sl_data.parse_trajectories(text)
    assert ts.n == 2
    assert ts.offsets.tolist() == [0, len(calls), len(calls) + 4]
    assert ts.calls.tolist() == calls + [0, 0, 0, 0]
    assert ts.calls.dtype == np.uint8 and ts.hands.dtype == np.uint64 and ts.offsets.dtype == np.int64


def test_packed_hands_equal_a_direct_restatement():
    text = T.random_file(40, seed=3)
    ts = sl_data.parse_trajectories(text)
    for i, ln in enumerate(text.strip().split("\n")):
        deal = [int(t) for t in ln.split()[:52]]
        for seat in range(4):
            want = 0
            for k, c in enumerate(deal):
                if k % 4 == seat:
                    want |= 1 << c
            assert int(ts.hands[i, seat]) == want
        assert sum(bin(int(h)).count("1") for h in ts.hands[i]) == 52


def test_openspiel_card_maps_back_to_the_observation_index():
    # the inverse of the oracle's card -> observation-bit map: pgx card suit * 13 + rank (S,H,D,C; A,2..K)
    for c in range(52):
        p = int(sl_data.openspiel_to_pgx_card(c))
        suit, rank = p // 13, p % 13
        assert ((rank + 12) % 13) * 4 + (3 - suit) == c


@pytest.mark.parametrize("what, mutate", [
    ("permutation", lambda toks: toks[:1] + toks[:1] + toks[2:]),                            # card 0 twice
    ("outside 52..89", lambda toks: toks[:52] + ["90"] + toks[53:]),
    ("illegal call", lambda toks: toks[:52] + ["55", "52", "55"] + toks[55:]),               # 1C P 1C
    ("does not end", lambda toks: toks[:52] + ["52", "52", "52", "52", "52"] + toks[57:]),   # a fifth pass
    ("tokens", lambda toks: toks[:-1]),                                                      # one play action short
])
def test_parser_rejects_malformed_lines_with_their_number(what, mutate):
    good = [T.line(_deal(i), [3, 0, 0, 0], np.random.default_rng(i)) for i in range(5)]
    toks = good[3].split()
    if what == "illegal call":
        toks = toks[:52] + ["55", "52", "55", "52", "52", "52"] + toks[56:]
    elif what == "does not end":
        toks = toks[:52] + ["55", "52", "52", "52", "52"] + toks[56:]
    else:
        toks = mutate(toks)
    lines = good[:3] + [" ".join(toks)] + good[4:]
    with pytest.raises(sl_data.MalformedTrajectory, match=r"^line 4: .*" + re.escape(what)):
        sl_data.parse_trajectories("\n".join(lines) + "\n")


def test_parser_rejects_an_auction_that_ends_before_its_last_call():
    toks = T.line(_deal(0), [0, 0, 0, 0]).split() + ["52"]        # five passes, no play
    text = T.line(_deal(1), [0, 0, 0, 0]) + "\n" + " ".join(toks) + "\n"
    with pytest.raises(sl_data.MalformedTrajectory, match="line 2"):
        sl_data.parse_trajectories(text)


def test_parser_accepts_random_legal_auctions_and_the_longest_one():
    ts = sl_data.parse_trajectories(T.random_file(300, seed=5))
    assert ts.n == 300 and int(ts.n_calls().max()) == 319 and int(ts.n_calls().min()) == 4


def test_sampler_restatement_is_a_bijection_per_epoch():
    offsets = np.cumsum(np.r_[0, np.random.default_rng(0).integers(4, 30, 777)])
    n = 777
    t0, p0 = T.sample(offsets, 42, 0, 3 * n)
    for e in range(3):
        assert sorted(t0[e * n:(e + 1) * n].tolist()) == list(range(n))
    assert not np.array_equal(t0[:n], t0[n:2 * n])                    # another order in the next epoch
    t1, p1 = T.sample(offsets, 42, 0, 3 * n)
    assert np.array_equal(t0, t1) and np.array_equal(p0, p1)          # deterministic
    t2, p2 = T.sample(offsets, 42, n - 5, 10)                          # the stream crosses the epoch boundary
    assert np.array_equal(t2, t0[n - 5:n + 5]) and np.array_equal(p2, p0[n - 5:n + 5])
    nc = offsets[t0 + 1] - offsets[t0]
    assert (p0 >= 0).all() and (p0 < nc).all()
    t3, _ = T.sample(offsets, 43, 0, n)
    assert not np.array_equal(t3, t0[:n])                              # the seed keys the order


@pytest.mark.parametrize("ent_coef", [0.0, 0.01])
def test_loss_and_gradient_match_torch_autograd_float64(ent_coef):
    rng = np.random.default_rng(7)
    B = 64
    z = rng.normal(0, 3, (B, 38))
    z[:4] *= 20                                                        # +-60-magnitude logits
    mask = rng.random((B, 38)) < 0.5
    mask[:, 0] = True
    mask[5:9] = False
    mask[5:9, 0] = True                                                # rows with a single legal call
    label = np.array([rng.choice(np.nonzero(m)[0]) for m in mask])
    out, d = T.loss64(z, label, mask, ent_coef)
    zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    lt = torch.tensor(label)
    mt = torch.tensor(mask)
    tgt = -(torch.nn.functional.one_hot(lt, 38) * torch.log_softmax(zt, -1)).mean()
    lsm = torch.log_softmax(torch.where(mt, zt, torch.finfo(torch.float64).min), -1)
    p = lsm.exp()
    H = -torch.where(p > 0, p * lsm, torch.zeros_like(p)).sum(-1)
    total = tgt - ent_coef * H.mean()
    total.backward()
    assert np.allclose(out[:3], [total.item(), tgt.item(), H.mean().item()], rtol=1e-12, atol=1e-14)
    assert np.allclose(d, zt.grad.numpy(), rtol=1e-10, atol=1e-15)


def test_sl_defaults_equal_the_reference_config():
    from brl_amd.sl import SL_DEFAULTS
    want = dict(iterations=400000, train_batch=128, learning_rate=1e-4, eval_every=10000, data_path=None, save_path=None,
                num_examples=3, eval_batch=10000, rng_seed=42, entropy_coef=0, type_of_model="DeepMind", activation="relu")
    assert SL_DEFAULTS == want
    from brl_amd.train import DEFAULTS, parse_cli
    cfg = parse_cli(["iterations=40", "entropy_coef=0.01", "data_path=/x"], defaults=SL_DEFAULTS)
    assert cfg["iterations"] == 40 and cfg["entropy_coef"] == 0.01 and cfg["data_path"] == "/x"
    assert parse_cli(["seed=3"]) == dict(DEFAULTS, seed=3)             # the PPO trainer's CLI as before


def test_missing_data_path_exits_1_with_the_hint(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "brl_amd.sl", f"data_path={tmp_path}"], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 1
    assert "Please generate your own supervised training data" in r.stderr and "train.txt" in r.stderr


@pytest.mark.parametrize("model", ["DeepMind", "FAIR"])
def test_params_pickle_round_trips_through_load_params(tmp_path, model):
    from brl_amd import checkpoint
    from brl_amd.models import make_forward_pass
    from brl_amd.sl import save_pickle
    net = make_forward_pass("relu", model).init(5)
    path = str(tmp_path / "params-20.pkl")
    save_pickle(net, path)
    back = checkpoint.load_params(path, "relu", model)
    for (ka, a), (kb, b) in zip(net.state_dict().items(), back.state_dict().items()):
        assert ka == kb and torch.equal(a, b)
    with open(path, "rb") as f:
        tree = pickle.load(f)
    assert "actor_critic/linear" in tree and tree["actor_critic/linear"]["w"].shape[0] == 480


def test_sl_header_matches_the_binding():
    from brl_amd import _capi
    from brl_amd import build
    build.build()
    text = open(os.path.join(ROOT, "include", "brl_sl.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decls = re.findall(r"\bint\s+(brl_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S)
    assert sorted(n for n, _ in decls) == ["brl_sl_loss", "brl_sl_replay", "brl_sl_sample"]
    scalar = {"int": 4, "int32_t": 4, "uint32_t": 4, "int64_t": 8, "uint64_t": 8, "float": "f"}

    def c_kind(arg):
        if "*" in arg:
            return "ptr"
        words = arg.split()
        return scalar[" ".join(words[:-1])]

    def py_kind(t):
        if t is ctypes.c_float:
            return "f"
        if t is ctypes.c_void_p:
            return "ptr"
        return ctypes.sizeof(t)

    L = _capi.lib()
    for name, args in decls:
        want = [c_kind(a.strip()) for a in args.split(",")]
        got = [py_kind(t) for t in getattr(L, name).argtypes]
        assert want == got, f"{name}: header {want} != ctypes {got}"
        assert name not in _capi.EXPORTS
    assert L.brl_version() == 6
