"""-m gpu: ``evaluation._Forward.whole`` — the one forward of every row that the evaluators' loops and the analysis tools share —
against each formulation it replaced, written out here, bit for bit: the tools' ``brl_obs_cast`` + ``fwd(None, x)`` in the dtype
``fwd.cast(m)`` names, the loops' ``fwd(obs, obs.to(torch.float32))``, and ``fwd(obs, None)`` where the route takes the bool rows.
On networks with non-zero biases (tests/nets.py), on both sides of ``InferenceSnapshot.X3_ROWS`` = 4096, where a snapshot's route
changes from "full_f32" to "full_bool"."""
import pytest
import torch

from tests.nets import observations, perturbed

pytestmark = pytest.mark.gpu

ROWS = (1, 3, 4095, 4096, 4099)


@pytest.fixture(scope="module")
def env(dds):
    import brl_amd
    return brl_amd.BridgeBidding(lut=(dds["keys"], dds["values"]))


def _forward(kind, m):
    from brl_amd.evaluation import _Forward, _PassOnly
    from brl_amd.models import make_forward_pass
    if kind == "pass":
        return _PassOnly(m, "cuda")
    fp = make_forward_pass(kind, "DeepMind")
    fwd = _Forward(fp, perturbed(fp.init(11, device="cuda"), 21))
    assert (fwd.snap is not None) == (kind == "relu")      # relu: the snapshot; tanh: the module forwards
    return fwd


def _same_bytes(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _check(fwd, m, want_route, env, monkeypatch):
    from brl_amd import _capi
    from brl_amd.evaluation import _Forward
    obs = observations(m, 100 + m, "cuda")
    assert _Forward.route(fwd, m, False) == want_route
    casts = []
    cast = _Forward._obs_cast
    monkeypatch.setattr(_Forward, "_obs_cast", staticmethod(lambda o, e, dt, fmt: casts.append(dt) or cast(o, e, dt, fmt)))
    f32 = _Forward._f32
    monkeypatch.setattr(_Forward, "_f32", staticmethod(lambda o, e: casts.append("f32") or f32(o, e)))
    with torch.no_grad():
        got = _Forward.whole(fwd, obs, env)
        # the route it took: a cast exactly where the route reads one (with the environment, brl_obs_cast in the dtype cast(m) names)
        with_env = {"full_f32": ["f32", torch.float32], "full_bool": [torch.bfloat16], "constant": []}[want_route]
        assert casts == with_env
        reads_f32 = want_route == "full_f32"
        assert got.dtype == torch.float32 and got.stride(1) == 1 and got.shape[0] == m and got.shape[1] >= 38
        x32 = obs.to(torch.float32)
        del casts[:]
        others = {"no environment": _Forward.whole(fwd, obs)}
        assert casts == (["f32"] if reads_f32 else [])      # (torch's own cast; the bool rows themselves on the other routes)
        del casts[:]
        others.update({"the caller's x": _Forward.whole(fwd, obs, x=x32), "environment and x": _Forward.whole(fwd, obs, env, x32)})
        assert casts == ([] if want_route != "full_bool" else [torch.bfloat16])      # (a given x is taken, not cast again)
        # the formulations it replaced
        dtype, fmt = (torch.float32, 0) if fwd.constant else fwd.cast(m)
        assert (dtype == torch.bfloat16) == (want_route == "full_bool")
        x = torch.empty((m, 480), dtype=dtype, device="cuda")
        _capi.check(_capi.lib().brl_obs_cast(env._h, obs.data_ptr(), m, _capi.ptr(x), fmt, _capi.stream()))
        others["brl_obs_cast + fwd(None, x)"] = fwd(None, x)
        others["fwd(obs, obs.to(float32))"] = fwd(obs, x32)
        if not reads_f32:
            others["fwd(obs, None)"] = fwd(obs, None)
        # ... and the pair: one object for one forward, the two results for two
        one = _Forward.whole_pair(fwd, fwd, obs, env)
        assert one[0] is one[1]
        twin = _forward("relu", m)
        others["the pair's first"], second = _Forward.whole_pair(fwd, twin, obs)
        others["the pair's first, with the environment"] = _Forward.whole_pair(fwd, twin, obs, env)[0]
        assert _same_bytes(second, _Forward.whole(twin, obs))
        torch.cuda.synchronize()
    assert bool(torch.isfinite(got).all()) and float(got[:, :38].abs().max()) > 0
    for name, out in others.items():
        assert _same_bytes(out, got), (name, want_route, m)


@pytest.mark.parametrize("m", ROWS)
@pytest.mark.parametrize("kind", ["relu", "tanh", "pass"])
def test_whole_is_every_formulation_it_replaced_bit_for_bit(env, monkeypatch, kind, m):
    from brl_amd.models import InferenceSnapshot
    assert InferenceSnapshot.X3_ROWS == 4096
    want = "constant" if kind == "pass" else "full_bool" if kind == "relu" and m >= 4096 else "full_f32"
    _check(_forward(kind, m), m, want, env, monkeypatch)


def test_without_planes_4096_rows_stay_on_float32(env, monkeypatch):
    monkeypatch.setenv("BRL_INFERENCE_PLANES", "0")
    fwd = _forward("relu", 4096)
    assert fwd.snap.wp is None and fwd.snap.gemm_x3
    _check(fwd, 4096, "full_f32", env, monkeypatch)
