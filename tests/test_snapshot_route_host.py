"""Host-side decisions of models.InferenceSnapshot that need no GPU: which backend runs the hidden layers of a call (`route_of`), the
dtype `_input` hands the layers (`input_dtype`) and where `head_parts` applies — each enumerated over every
combination of facts against a literal restatement of the conditions the class held, in six places, before it had a route table."""
import itertools

import pytest
import torch

from brl_amd.models import InferenceSnapshot, make_forward_pass
from tests.nets import forward64, observations, perturbed

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
# (has16, has_planes, has_x3, dtype) of every snapshot that can exist: the planes need the bf16x3 products, which are fp32 only;
# brl_linear_act's layout is 16-bit only (without it — BRL_LINEAR16=0, no library handle — a 16-bit snapshot has none of the three)
SNAPSHOTS = [(False, False, False, F32), (False, False, True, F32), (False, True, True, F32),
             (True, False, False, BF16), (True, False, False, F16), (False, False, False, BF16), (False, False, False, F16)]
ROWS = (0, 1, 4095, 4096)
INPUTS = list(itertools.product(ROWS, (F32, BF16, F16), (False, True), (False, True)))      # (n, xdt, dev_ok, al16)


def old_body(has16, has_planes, has_x3, sdt, n, xdt, dev_ok, al16):
    """the five-step cascade `_body` was (dev_ok: x.is_cuda and x.dim() == 2 and x.is_contiguous())"""
    planes_for = has_planes and n >= 4096
    if has16 and dev_ok and n > 0:
        return "linear16"
    if dev_ok and planes_for and al16 and xdt == BF16 and sdt == F32:
        return "planes"
    if xdt != sdt:
        raise RuntimeError("input dtype")
    if has_x3 and dev_ok and n >= 4096 and al16:
        return "x3"
    return "library"


def old_input_dtype(has_planes, sdt, n, odim, odt, own):
    """the two branches `_input` had; own: env, own_cast, a contiguous observation on the GPU (its brl_obs_cast branch also asked for
    0/1 bytes)"""
    planes_for = has_planes and n >= 4096
    if own and odt in (torch.bool, torch.uint8):
        return BF16 if (sdt == F32 and odim == 2 and planes_for) else sdt
    if sdt == F32 and odim == 2 and planes_for:
        if odt in (torch.bool, torch.uint8):
            return BF16
        if odt == BF16:
            return odt
    return sdt


def old_head_parts(has16, switch, dev_ok, n):
    """`head_parts` ran (did not return None) where ..."""
    if not has16 or switch == "0":
        return False
    return dev_ok and n > 0


def _outcome(f, *a):
    try:
        return f(*a)
    except RuntimeError:
        return "raises"


def test_route_table_is_the_cascade_it_replaces():
    seen = set()
    for snap, x in itertools.product(SNAPSHOTS, INPUTS):
        got, want = _outcome(InferenceSnapshot.route_of, *snap, *x), _outcome(old_body, *snap, *x)
        assert got == want, (snap, x)
        seen.add(got)
    assert seen == {"linear16", "planes", "x3", "library", "raises"}
    # the refusal's text, as it was
    with pytest.raises(RuntimeError) as err:
        InferenceSnapshot.route_of(False, True, True, F32, 4096, BF16, False, True)
    assert str(err.value) == ("InferenceSnapshot: input in torch.bfloat16 where the layers run in torch.float32 (bf16 input is taken by the "
                              "planes path only: >= 4096 contiguous rows)")


def _stub(has16, has_planes, has_x3, sdt):
    """a snapshot as far as its decisions are concerned: they read the presence of the weight stores and the dtype only"""
    snap = object.__new__(InferenceSnapshot)
    snap.body_nk, snap.wp, snap.gemm_x3, snap.dtype = ([] if has16 else None), ([] if has_planes else None), has_x3, sdt
    return snap


def test_planes_for_is_rule_two_at_n_rows():
    for cfg, n in itertools.product(SNAPSHOTS, ROWS + (8192,)):
        assert _stub(*cfg).planes_for(n) == (cfg[1] and n >= 4096)
        # ... an aligned bf16 input on the device takes rule 2 exactly there
        assert (_outcome(InferenceSnapshot.route_of, *cfg, n, BF16, True, True) == "planes") == _stub(*cfg).planes_for(n)


def test_input_dtype_is_what_both_branches_of_input_gave():
    dts = (torch.bool, torch.uint8, F32, BF16, F16)
    for cfg, n, odim, odt, own in itertools.product(SNAPSHOTS, ROWS, (1, 2, 3), dts, (False, True)):
        assert _stub(*cfg).input_dtype(n, odt, odim) == old_input_dtype(cfg[1], cfg[3], n, odim, odt, own), (cfg, n, odim, odt, own)
    assert _stub(False, True, True, F32).input_dtype(4096) == BF16          # (the default: an [n, 480] bool observation)


class _X:
    """a tensor as far as `route` reads one"""
    is_cuda = True

    def __init__(self, n, xdt, dev_ok, al16):
        self.shape, self.dtype, self._ok, self._ptr = (n, 480), xdt, dev_ok, 4096 if al16 else 4104

    def dim(self):
        return 2

    def is_contiguous(self):
        return self._ok

    def data_ptr(self):
        return self._ptr


class _Applies(Exception):
    pass


def test_head_parts_apply_on_the_linear16_route_only(monkeypatch):
    """`head_parts` itself, on a stub snapshot whose "linear16" runner says that it was reached, for every snapshot, input and value of
    BRL_HEAD_PARTS.  One cell differs, by the table's own order: a 16-bit snapshot handed an `x` that brl_linear_act cannot take
    (host, strided or empty) AND in another dtype.  `head_parts` answered None there and the `hidden` every caller runs next raised;
    now the route raises that error already."""
    def reached(x, layers):
        raise _Applies

    for cfg, x, switch in itertools.product(SNAPSHOTS, INPUTS, ("1", "0")):
        n, xdt, dev_ok, al16 = x
        monkeypatch.setenv("BRL_HEAD_PARTS", switch)
        snap = _stub(*cfg)
        snap._run_linear16 = reached
        try:
            got = snap.head_parts(None, _X(n, xdt, dev_ok, al16)) is not None
        except _Applies:
            got = True
        except RuntimeError:
            got = "raises"
        want = old_head_parts(cfg[0], switch, dev_ok, n)
        if got == "raises":
            assert cfg[0] and switch != "0" and not want and xdt != cfg[3] and _outcome(old_body, *cfg, *x) == "raises", (cfg, x)
        else:
            assert got == want, (cfg, x, switch)
            assert got == (switch != "0" and _outcome(InferenceSnapshot.route_of, *cfg, *x) == "linear16")


def test_a_host_snapshot_runs_on_the_library():
    net = perturbed(make_forward_pass("relu", "DeepMind").init(11), 21)
    snap = InferenceSnapshot.make(net)
    assert snap.gemm_x3 and snap.wp is None and snap.body_nk is None      # (the planes are built on the GPU only)
    for n in ROWS:
        x = snap._input(torch.zeros((n, 480), dtype=torch.bool))
        assert x.dtype == F32 and snap.route(x) == "library" and not snap.planes_for(n)
    obs = observations(64, 5)
    ref = forward64(net, obs)
    with torch.no_grad():
        assert float((snap.heads(obs).double() - ref).abs().max()) < 2e-4 * max(1.0, float(ref.abs().max()))
        assert snap.head_parts(obs) is None
