"""Networks with non-zero biases, and plain float64 forwards of the DeepMind MLP to check the inference paths against.

``ForwardPass.init`` is hk.Linear's initialisation: every bias is 0.0.  A forward that drops a bias, or adds another layer's, another
network's or the other head's, computes the same numbers on such a network.  ``perturbed`` moves every parameter; ``forward64`` and
``forward16_ref`` are the references; ``bias_slots`` yields one wrong network per way a bias can be mixed up, so that a test can first
prove, in float64, that its tolerance sees each of them (``assert_sees_bias_slots``).

A "network" here is anything with ``body`` (a sequence of layers with ``weight`` [out, in] and ``bias`` [out]), ``actor``, ``critic`` and
``act`` (torch.relu / torch.tanh): an ``ActorCritic`` module, or a ``types.SimpleNamespace`` over plain tensors (``raw_net``).
"""
from types import SimpleNamespace

import torch


def perturbed(net, seed, w=0.01, b=0.1):
    """N(0, w) added to every weight and N(0, b) to every bias of `net`, in place; -> net.  The noise is drawn on the host from a generator
    seeded with `seed`, parameter by parameter in ``net.parameters()`` order and in the parameter's dtype, so a network on the GPU and its
    copy on the host receive the same numbers."""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for q in net.parameters():
            noise = torch.randn(q.shape, generator=gen, dtype=q.dtype) * (b if q.dim() == 1 else w)
            q.add_(noise.to(q.device))
    return net


def raw_net(body, actor, critic, act):
    """a network over plain tensors: body = [(W, b), ...], actor = (W [38, h], b [38]), critic = (W [1, h], b [1])"""
    lin = lambda wb: SimpleNamespace(weight=wb[0], bias=wb[1])   # noqa: E731
    return SimpleNamespace(body=[lin(wb) for wb in body], actor=lin(actor), critic=lin(critic), act=act)


def copy64(net, device=None):
    """float64 copies of every parameter of `net` (on `device`, default: where they are) as a network over plain tensors"""
    c = lambda t: t.detach().to(device=device or t.device, dtype=torch.float64).clone()   # noqa: E731
    return raw_net([(c(l.weight), c(l.bias)) for l in net.body], (c(net.actor.weight), c(net.actor.bias)),
                   (c(net.critic.weight), c(net.critic.bias)), net.act)


def _layers(net, device, cast):
    return [(cast(l.weight.detach().to(device)), cast(l.bias.detach().to(device))) for l in list(net.body) + [net.actor, net.critic]]


def forward64(net, x):
    """the DeepMind forward (src/models.py:23-33) in float64 on x's device -> [n, 39]: 38 logits, then the value"""
    layers = _layers(net, x.device, lambda t: t.double())
    h = x.double()
    for W, b in layers[:-2]:
        h = net.act(h @ W.t() + b)
    (Wa, ba), (Wc, bc) = layers[-2:]
    return torch.cat([h @ Wa.t() + ba, h @ Wc.t() + bc], 1)


def forward16_ref(net, x, dtype):
    """float64 forward of what the 16-bit kernels are given: every weight and bias rounded to `dtype`, each hidden layer's output
    rounded to `dtype` (the kernels store 16-bit activations); the heads' product of the rounded last activation with the rounded
    head weights and bias stays in float64 -> [n, 39]"""
    layers = _layers(net, x.device, lambda t: t.to(dtype).double())
    h = x.double()
    for W, b in layers[:-2]:
        h = net.act(h @ W.t() + b).to(dtype).double()
    (Wa, ba), (Wc, bc) = layers[-2:]
    return torch.cat([h @ Wa.t() + ba, h @ Wc.t() + bc], 1)


def bias_slots(net):
    """(name, float64 copy of `net` with ONE bias mix-up) for every slot a bias can be mixed up in: each hidden bias zeroed (a bias
    never added), each adjacent pair of hidden biases swapped (another layer's bias), the actor bias rolled by one, the critic bias
    zeroed"""
    L = len(net.body)
    for i in range(L):
        m = copy64(net)
        m.body[i].bias.zero_()
        yield f"layer-{i} bias zeroed", m
    for i in range(L - 1):
        m = copy64(net)
        m.body[i].bias, m.body[i + 1].bias = m.body[i + 1].bias, m.body[i].bias
        yield f"layer-{i} and layer-{i + 1} biases swapped", m
    m = copy64(net)
    m.actor.bias = m.actor.bias.roll(1)
    yield "actor bias rolled by one", m
    m = copy64(net)
    m.critic.bias.zero_()
    yield "critic bias zeroed", m


def slot_effects(net, x):
    """{slot name: max|forward64(mutant) - forward64(net)|} over the rows of x"""
    ref = forward64(net, x)
    return {name: float((forward64(m, x) - ref).abs().max()) for name, m in bias_slots(net)}


def assert_sees_bias_slots(net, x, tol):
    """Every mutant of `bias_slots` moves the float64 outputs on x by at least 8 x `tol`: a check with tolerance `tol` on these inputs
    cannot pass a forward with that bias mix-up.  -> the smallest effect"""
    effects = slot_effects(net, x)
    name = min(effects, key=effects.get)
    assert effects[name] >= 8 * tol, f"{name} moves the outputs by {effects[name]:.3g} < 8 x {tol:.3g}: the check would not see it"
    return effects[name]


def observations(n, seed, device="cpu", p=0.12):
    """[n, 480] bool, each bit set with probability p (a bridge observation has about that density); drawn on the host"""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((n, 480), generator=g) < p).to(device)
