"""brl_amd._capture.preserved on the CPU: what a warm-up or a capture does to the parameters, the optimizer state and the counters
is undone in place (the captured graphs hold those tensors' addresses)."""
import pytest
import torch

from brl_amd._capture import preserved


def _net_and_opt():
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.ReLU(), torch.nn.Linear(5, 3))
    return net, torch.optim.Adam(net.parameters(), lr=1e-2)


def _adam_steps(net, opt, n):
    for i in range(n):
        opt.zero_grad()
        net(torch.full((4, 6), 0.5 + i)).square().sum().backward()
        opt.step()


def _state(opt):
    return {p: dict(st) for p, st in opt.state.items()}


def test_fresh_optimizer_state_created_inside_is_zeroed():
    net, opt = _net_and_opt()
    before = [p.detach().clone() for p in net.parameters()]
    with preserved(net.parameters(), opt):
        _adam_steps(net, opt, 2)
        assert not torch.equal(next(net.parameters()), before[0])
    for p, q in zip(net.parameters(), before):
        assert torch.equal(p, q)
    assert len(opt.state) == len(before)
    for st in opt.state.values():
        assert set(st) == {"step", "exp_avg", "exp_avg_sq"}
        for v in st.values():
            assert torch.count_nonzero(v) == 0


def test_stepped_optimizer_state_is_restored_in_place():
    net, opt = _net_and_opt()
    _adam_steps(net, opt, 3)
    params = [p.detach().clone() for p in net.parameters()]
    objs = _state(opt)
    ptrs = {p: {k: v.data_ptr() for k, v in st.items()} for p, st in objs.items()}
    vals = {p: {k: v.clone() for k, v in st.items()} for p, st in objs.items()}
    with preserved(net.parameters(), opt):
        _adam_steps(net, opt, 2)
    for p, q in zip(net.parameters(), params):
        assert torch.equal(p, q)
    for p, st in opt.state.items():
        for k, v in st.items():
            assert v is objs[p][k] and v.data_ptr() == ptrs[p][k]
            assert torch.equal(v, vals[p][k])


def test_state_is_restored_when_the_body_raises():
    net, opt = _net_and_opt()
    _adam_steps(net, opt, 1)
    counter = torch.tensor([7], dtype=torch.int64)
    params = [p.detach().clone() for p in net.parameters()]
    vals = {p: {k: v.clone() for k, v in st.items()} for p, st in opt.state.items()}
    with pytest.raises(RuntimeError, match="capture failed"):
        with preserved(net.parameters(), opt, tensors=(counter,)):
            _adam_steps(net, opt, 1)
            counter += 5
            raise RuntimeError("capture failed")
    assert int(counter) == 7
    for p, q in zip(net.parameters(), params):
        assert torch.equal(p, q)
    for p, st in opt.state.items():
        for k, v in st.items():
            assert torch.equal(v, vals[p][k])
