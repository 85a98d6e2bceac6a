"""hipGraph capture: every capture of this package goes through ``warm_up``, ``capture`` / ``capture_each`` and ``preserved``.

A dead reference cycle that still owns a ``torch.cuda.CUDAGraph`` (an earlier rollout / update object) is freed whenever the
collector happens to run; the graph's destructor synchronises the device (torch does that on ROCm: hipGraphExecDestroy frees
lazily), and a device synchronisation while a stream of this process is capturing aborts the process.  ``torch.cuda.graph`` no
longer collects before it captures (torch.compiler.config.force_cudagraph_gc), so every capture of this package goes through
``quiet_gc``: collect once up front — cycles die BEFORE the capture — and keep the collector off until the captures are done.

Warm-up and capture run the REAL step (optimizer included) on dummy inputs: ``preserved`` puts the training state back in place.
"""
import contextlib
import gc

import torch


@contextlib.contextmanager
def quiet_gc():
    gc.collect()
    was_enabled = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was_enabled:
            gc.enable()


def graph_kwargs() -> dict:
    """``torch.cuda.graph`` keyword arguments for a capture of this package: ``capture_error_mode="thread_local"`` ONLY while an
    NCCL / RCCL process group lives — its watchdog thread queries events beside the capturing thread, which the default
    ("global") mode reports as a capture error.  Every other capture (no process group, gloo) keeps the default, where an unsafe
    call from ANY thread fails the capture instead of going unnoticed."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_backend() == "nccl":
        return {"capture_error_mode": "thread_local"}
    return {}


def _grad(no_grad: bool):
    return torch.no_grad() if no_grad else contextlib.nullcontext()


def warm_up(fn, iters: int, no_grad: bool = False) -> None:
    """``fn()`` ``iters`` times on a fresh side stream that waits for the current stream; the current stream then waits for the
    side stream (allocator, library heuristics and lazily created state settle before a capture)"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    try:
        with torch.cuda.stream(side), _grad(no_grad):
            for _ in range(iters):
                fn()
    finally:
        torch.cuda.current_stream().wait_stream(side)


def capture_each(fns, pool=None, no_grad: bool = False) -> list:
    """one ``torch.cuda.CUDAGraph`` per callable of ``fns``, in order, all under one ``quiet_gc()`` with ``graph_kwargs()``;
    ``pool``: a memory pool the graphs share (``torch.cuda.graph_pool_handle()``), else one private pool per graph"""
    graphs = []
    with quiet_gc(), _grad(no_grad):
        kwargs = graph_kwargs()
        for fn in fns:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, pool=pool, **kwargs):
                fn()
            graphs.append(g)
    return graphs


def capture(fn, pool=None, no_grad: bool = False) -> torch.cuda.CUDAGraph:
    """one ``torch.cuda.CUDAGraph`` of ``fn()`` (``capture_each`` of one callable)"""
    return capture_each([fn], pool, no_grad)[0]


@contextlib.contextmanager
def preserved(params=(), opt=None, tensors=()):
    """Training state as it was on entry, copied back IN PLACE on exit, normal or by exception (captured graphs hold these
    tensors' addresses): the parameters, every entry of ``opt.state`` and the extra ``tensors`` (counters, flat buffers).  A tensor
    entry of the optimizer state created inside the context is zeroed (zero moments / step 0 == a fresh Adam state); a non-tensor
    entry that existed on entry is put back."""
    params, tensors, state = list(params), list(tensors), opt.state if opt is not None else {}
    saved_p = [p.detach().clone() for p in params]
    saved_s = {p: {k: (v.detach().clone() if torch.is_tensor(v) else v) for k, v in st.items()} for p, st in state.items()}
    saved_t = [t.detach().clone() for t in tensors]
    try:
        yield
    finally:
        with torch.no_grad():
            for p, q in zip(params, saved_p):
                p.copy_(q)
            for p, st in state.items():
                old = saved_s.get(p)
                for k, v in st.items():
                    if torch.is_tensor(v):
                        if old is not None and k in old:
                            v.copy_(old[k])
                        else:
                            v.zero_()
                    elif old is not None and k in old:
                        st[k] = old[k]
            for t, q in zip(tensors, saved_t):
                t.copy_(q)
