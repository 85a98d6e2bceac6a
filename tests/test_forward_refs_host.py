"""tests/nets.py on the CPU: the references every bias test of the inference forwards leans on (forward64, forward16_ref), the
perturbation recipe, and the sensitivity table — how far each bias mix-up of `bias_slots` moves the outputs of the networks the GPU
tests use (tests/test_gpu_forward_biases.py asserts the same before each of its checks)."""
import copy

import pytest
import torch

from brl_amd.models import make_forward_pass
from tests.nets import assert_sees_bias_slots, bias_slots, forward16_ref, forward64, observations, perturbed, raw_net, slot_effects

NET_SEED, PERTURB_SEED, OBS_SEED = 11, 21, 5


def _net(model, activation="relu"):
    return perturbed(make_forward_pass(activation, model).init(NET_SEED), PERTURB_SEED)


def test_perturbed_moves_every_parameter_and_is_the_documented_recipe():
    """N(0, 0.01) on weights, N(0, 0.1) on biases, one host generator in parameters() order — the recipe of the FAIR update cases, so
    their seeded inputs stay what they were; the same seed gives a float32 network on any device the same numbers"""
    fp = make_forward_pass("relu", "DeepMind")
    base, net = fp.init(3), fp.init(3)
    assert perturbed(net, 7) is net
    gen = torch.Generator().manual_seed(7)
    for q0, q in zip(base.parameters(), net.parameters()):
        want = q0.detach() + torch.randn(q0.shape, generator=gen) * (0.1 if q0.dim() == 1 else 0.01)
        assert torch.equal(q.detach(), want)
    for lin in list(net.body) + [net.actor, net.critic]:
        assert float(lin.bias.detach().abs().min()) > 0.0
    other = perturbed(fp.init(3), 8)
    assert not torch.equal(other.body[0].bias, net.body[0].bias)
    wide = perturbed(fp.init(3), 7, w=0.0, b=0.3)
    assert torch.equal(wide.body[1].weight, base.body[1].weight) and float(wide.body[1].bias.detach().std()) > 0.25


@pytest.mark.parametrize("model,activation", [("DeepMind", "relu"), ("DeepMind", "tanh"), ("DeepMind_6", "relu")])
def test_forward64_is_the_module_in_float64(model, activation):
    net = _net(model, activation)
    x = observations(200, OBS_SEED)
    with torch.no_grad():
        logits, value = copy.deepcopy(net).double()(x.double())
    out = forward64(net, x)
    assert out.shape == (200, 39) and out.dtype == torch.float64
    assert float((out - torch.cat([logits, value[:, None]], 1)).abs().max()) < 1e-13
    # ... and of a network over plain tensors
    raw = raw_net([(l.weight.detach(), l.bias.detach()) for l in net.body], (net.actor.weight.detach(), net.actor.bias.detach()),
                  (net.critic.weight.detach(), net.critic.bias.detach()), net.act)
    assert torch.equal(forward64(raw, x), out)


@pytest.mark.parametrize("model", ["DeepMind", "DeepMind_6"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_forward16_ref_against_torchs_own_16_bit_chain(model, dtype):
    """torch's CPU addmm chain in `dtype` (fp32 accumulation, one rounding per layer) with the heads in fp32 on the rounded head
    parameters, against forward16_ref.  The two differ only where a hidden activation rounds the other way (the chain rounds an fp32
    sum, the reference the exact one) and in the fp32 head product: well inside half a unit in the last place of `dtype` at the
    outputs' scale (2^-9 for bf16, 2^-12 for fp16, |out| < 1).  Measured: 4.1e-4 / 6.0e-4 (bf16), 7.5e-5 / 1.0e-4 (fp16) for the
    4- / 6-layer net.  The rounding of the parameters and activations itself — forward16_ref against forward64 — is 1.8e-3 (bf16)
    and 2.3e-4 (fp16): the reference has to model it, or a 16-bit check could not be tighter than that."""
    net = _net(model)
    x = observations(512, OBS_SEED)
    ref16 = forward16_ref(net, x, dtype)
    with torch.no_grad():
        h = x.to(dtype)
        for lin in net.body:
            h = torch.addmm(lin.bias.to(dtype), h, lin.weight.to(dtype).t()).relu_()
        hw = torch.cat([net.actor.weight, net.critic.weight]).to(dtype).float()
        hb = torch.cat([net.actor.bias, net.critic.bias]).to(dtype).float()
        out = torch.addmm(hb, h.float(), hw.t())
    half_ulp = 2.0 ** -9 if dtype == torch.bfloat16 else 2.0 ** -12
    scale = max(1.0, float(ref16.abs().max()))
    gap = float((out.double() - ref16).abs().max())
    rounding = float((ref16 - forward64(net, x)).abs().max())
    print(f"{model} {dtype}: chain vs forward16_ref {gap:.2e} (bound {half_ulp * scale:.2e}); forward16_ref vs forward64 {rounding:.2e}")
    assert gap < half_ulp * scale
    assert gap < rounding < 4 * half_ulp * scale      # (the reference models the rounding: it is closer to the chain than float64 is)


# the smallest effect of a bias mix-up the GPU tests rely on (tests/test_gpu_forward_biases.py)
SENSITIVITY = {"DeepMind": 0.069, "DeepMind_6": 0.029}


@pytest.mark.parametrize("model", ["DeepMind", "DeepMind_6"])
def test_every_bias_slot_moves_the_outputs(model):
    """init(11), perturbed(21), 512 observations of density 0.12: |out| < 1, and every mutant of bias_slots — a hidden bias dropped,
    two neighbouring ones swapped, the actor's rolled, the critic's dropped — moves some output by at least SENSITIVITY[model]: 40 x
    the fp32 bound 2e-4 and 8 x a 16-bit bound of up to 3.6e-3."""
    net = _net(model)
    x = observations(512, OBS_SEED)
    L = len(net.body)
    names = [name for name, _ in bias_slots(net)]
    assert len(names) == 2 * L + 1 and len(set(names)) == len(names)
    for name, m in bias_slots(net):      # float64 copies: the network itself is never touched
        assert m.body[0].weight.dtype == torch.float64 and m.body[0].weight.data_ptr() != net.body[0].weight.data_ptr()
    assert float(forward64(net, x).abs().max()) < 1.0
    effects = slot_effects(net, x)
    print(model, {k: round(v, 4) for k, v in effects.items()})
    assert min(effects.values()) >= SENSITIVITY[model]
    assert assert_sees_bias_slots(net, x, 2e-4) == min(effects.values())
    assert_sees_bias_slots(net, x, SENSITIVITY[model] / 8)
    with pytest.raises(AssertionError, match="would not see it"):
        assert_sees_bias_slots(net, x, 0.08)          # (the 16-bit tolerance of the rollout tests on zero-bias networks)
    # on hk.Linear's zero biases every slot is invisible — the blind spot itself
    zero = make_forward_pass("relu", model).init(NET_SEED)
    assert max(slot_effects(zero, x).values()) == 0.0
