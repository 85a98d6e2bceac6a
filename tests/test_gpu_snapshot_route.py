"""-m gpu: InferenceSnapshot.route on both sides of every condition of its table (models.InferenceSnapshot.route_of), each
asserted TOGETHER with the numbers the routed backend gives: a route that names one kernel while another runs, or a threshold that
moved by one row, fails here.  One perturbed DeepMind network (tests/nets.py) and one float64 reference for all fp32 cases; the
bound is the project's 2e-4 max(1, max|ref|).  The 16-bit case is checked as tests/test_gpu_forward_biases.py checks 16-bit paths:
against forward16_ref within 2 x torch's own 16-bit chain's error (+ one ulp where the output was stored in 16 bits) — no 16-bit
forward is within 2e-4 of float64."""
import pytest
import torch

from tests.nets import forward16_ref, forward64, perturbed
from tests.test_gpu_forward_biases import _bound16, _err, _excess, _obs, _tol32, _ulp

pytestmark = pytest.mark.gpu
ROWS = 4096          # InferenceSnapshot.X3_ROWS, spelled out: the tests pin the number


@pytest.fixture(scope="module")
def env(dds):
    import brl_amd
    return brl_amd.BridgeBidding(lut=(dds["keys"], dds["values"]))


@pytest.fixture(scope="module")
def case():
    """(network, [4096, 480] bool observations, forward64 of them) — read-only"""
    from brl_amd.models import make_forward_pass
    net = perturbed(make_forward_pass("relu", "DeepMind").init(11, device="cuda"), 21)
    obs = _obs(ROWS)
    return net, obs, forward64(net, obs)


FP32 = {  # name: (snapshot arguments, BRL_INFERENCE_PLANES, rows, the observation as given, route, input dtype)
    "planes_bool_4095": ({}, "1", ROWS - 1, torch.bool, "library", torch.float32),
    "planes_bool_4096": ({}, "1", ROWS, torch.bool, "planes", torch.bfloat16),
    "planes_f32_4096": ({}, "1", ROWS, torch.float32, "x3", torch.float32),
    "no_planes_4096": ({}, "0", ROWS, torch.bool, "x3", torch.float32),
    "no_planes_4095": ({}, "0", ROWS - 1, torch.bool, "library", torch.float32),
    "library_4096": ({"gemm": "library"}, "1", ROWS, torch.bool, "library", torch.float32),
}


@pytest.mark.parametrize("name", list(FP32))
def test_fp32_route_and_result_on_both_sides_of_the_threshold(case, name, monkeypatch):
    from brl_amd.models import InferenceSnapshot
    kw, planes, n, given_dt, route, in_dt = FP32[name]
    monkeypatch.delenv("BRL_INFERENCE_GEMM", raising=False)
    monkeypatch.setenv("BRL_INFERENCE_PLANES", planes)
    net, obs, ref = case
    obs, ref = obs[:n], ref[:n]
    snap = InferenceSnapshot.make(net, **kw)
    assert (snap.wp is not None) == (planes == "1" and not kw) and snap.gemm_x3 == (not kw) and snap.body_nk is None
    given = obs.to(given_dt)
    x = snap._input(given)
    assert x.dtype == in_dt == snap.input_dtype(n, given_dt) and snap.route(x) == route
    assert bool(snap.planes_for(n)) == (snap.wp is not None and n >= ROWS)
    with torch.no_grad():
        out = snap.heads(given)
    e, tol = _err(out, ref), _tol32(ref)
    print(f"{name}: {route}, error {e:.2e} of {tol:.2e}")
    assert out.shape == (n, 39) and e < tol


def test_strided_bf16_input_is_refused_on_the_host(case):
    """a planes snapshot handed bf16 rows that brl_linear_x3p cannot take (a [4096, 512][:, :480] view): the table's rule 3 raises
    while it is being read — no backend has been chosen, nothing was launched.  (That such an input is not cast and run on another
    backend is a known gap; this pins what happens.)"""
    from brl_amd.models import InferenceSnapshot
    net, obs, _ = case
    snap = InferenceSnapshot.make(net)
    assert snap.wp is not None
    wide = torch.zeros((ROWS, 512), dtype=torch.bfloat16, device="cuda")
    wide[:, :480] = obs.to(torch.bfloat16)
    x = wide[:, :480]
    torch.cuda.synchronize()
    for call in (lambda: snap.route(x), lambda: snap.hidden(None, x=x), lambda: snap.heads(None, x=x)):
        with pytest.raises(RuntimeError, match=r"input in torch.bfloat16 where the layers run in torch.float32 \(bf16 input is taken by "
                                                 r"the planes path only: >= 4096 contiguous rows\)"):
            call()
    assert snap.route(x.contiguous()) == "planes"
    torch.cuda.synchronize()        # (and no fault is pending)


def test_16_bit_snapshot_route_and_head_parts_switch(env, monkeypatch):
    """a bf16 snapshot with a library handle at 1000 rows: "linear16"; `head_parts` applies and, summed in the step kernel's order plus
    `head_bf`, is within the 16-bit bound of forward16_ref, as is `heads` (+ one ulp: stored as bf16).  BRL_HEAD_PARTS=0 (read per
    call, the same snapshot): no `head_parts`, `hidden` still on "linear16" and bit for bit what it was."""
    from brl_amd.models import InferenceSnapshot, make_forward_pass
    monkeypatch.delenv("BRL_LINEAR16", raising=False)
    monkeypatch.delenv("BRL_HEAD_PARTS", raising=False)
    dt, n = torch.bfloat16, 1000
    net = perturbed(make_forward_pass("relu", "DeepMind").init(11, device="cuda"), 21)
    obs = _obs(n)
    snap = InferenceSnapshot.make(net, dt, env)
    x = snap._input(obs)
    assert snap.body_nk is not None and x.dtype == dt == snap.input_dtype(n) and snap.route(x) == "linear16"
    ref16 = forward16_ref(net, obs, dt)
    e_lib, bound, _ = _bound16(net, obs, dt, ref16)
    with torch.no_grad():
        parts = snap.head_parts(obs)
        assert parts is not None and parts.shape == (snap.head_wt.shape[1] // 128, n, snap.HEAD_PART_LD)
        lg = snap.head_bf.clone().expand(n, 39).contiguous()
        for p_ in range(parts.shape[0]):
            lg = lg + parts[p_, :, :39]
        hidden, out = snap.hidden(obs), snap.heads(obs)
        monkeypatch.setenv("BRL_HEAD_PARTS", "0")
        assert snap.head_parts(obs) is None and snap.head_parts(None, x) is None
        assert snap.route(snap._input(obs)) == "linear16" and torch.equal(snap.hidden(obs), hidden)
    ex = _excess(out, ref16, _ulp(ref16, dt))
    print(f"library chain {e_lib:.2e} -> bound {bound:.2e}; head_parts {_err(lg, ref16):.2e}, heads beyond its rounding {ex:.2e}")
    assert _err(lg, ref16) < bound and ex < bound
    # the route leaves brl_linear_act where the kernel cannot take the input: no rows, or rows with a stride (torch's chain, no parts)
    monkeypatch.delenv("BRL_HEAD_PARTS")
    assert snap.route(x[:0]) == "library" and snap.route(x[:, :240]) == "library" and snap.head_parts(None, x[:0]) is None
