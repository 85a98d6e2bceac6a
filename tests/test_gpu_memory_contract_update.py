"""-m gpu: the memory contract (tests/guarded.py; DESIGN.md "Memory contract") of the PPO step's own entry points — loss, heads,
statistics, minibatch gather, activation backward, bias finalize, clip + Adam (whole buffers and rank slices), the FAIR chain.
These kernels update the parameters, the Adam moments and the gradient in place, inside views of ONE flat buffer: a store one piece
past a segment lands in the next layer's weights, not in allocator slack.

Every case runs through ``both``: plain (dense allocator tensors), then guarded — every pointer at exactly the alignment
include/brl_hip.h states for it and no better, every leading dimension the signature offers 4 floats larger than dense, every
scratch / partials / workspace array exactly as long as the header says, NaN bytes in the padding of inputs — and asserts the
same bits, no guard byte changed, every output element written, every input that is not in/out unchanged.  A row log (`row_index`)
is placed with 4 rows, row 2 selected: the other rows must stay as placed.  Values are held to float64 elsewhere
(tests/test_gpu_update_float64.py, tests/test_gpu_parity.py): bit equality with the plain run is the assertion here.
Nothing here can fault by design: no pointer is below an entry point's required alignment or outside the arena."""
import ctypes as C

import pytest
import torch

from tests.guarded import both

pytestmark = pytest.mark.gpu
F32, U8, I32, I64 = torch.float32, torch.uint8, torch.int32, torch.int64
NA, NH, GRAM = 38, 39, 38 * 38


def _s():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _lib():
    from brl_amd import _capi
    return _capi.lib(), _capi.check


def _gen(*seed):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(s) for i, s in enumerate(seed)) + 1)


def _randn(gen, *shape):
    return torch.randn(shape, generator=gen)


def _loss_inputs(batch, gen):
    """one minibatch of `_loss_fn` inputs: at least one legal action per row, the action taken is legal"""
    mask = (torch.rand((batch, NA), generator=gen) < 0.6).to(U8)
    action = torch.randint(0, NA, (batch,), generator=gen)
    mask[torch.arange(batch), action] = 1
    return dict(mask=mask, action=action.to(I32), old_value=_randn(gen, batch), old_log_prob=-3 * torch.rand(batch, generator=gen),
                gae=_randn(gen, batch), targets=_randn(gen, batch))


def _place_loss(mem, li):
    return [mem.inp("mask", li["mask"], U8, 1), mem.inp("action", li["action"], I32, 4), mem.inp("old_value", li["old_value"], F32, 4),
            mem.inp("old_log_prob", li["old_log_prob"], F32, 4), mem.inp("gae", li["gae"], F32, 4), mem.inp("targets", li["targets"], F32, 4)]


def _only_row(gm, name, row, rows=4):
    """a log of `rows` rows of which the launch may write only `row`"""
    u = gm.arena.unwritten(gm.outs[name])
    assert u.shape[0] == rows and not u[row].any(), f"{name}: row {row} not written"
    assert u[[r for r in range(rows) if r != row]].all(), f"{name}: a row other than {row} was written"


def _stats_inputs(groups, gen):
    """loss partials [groups, 8] and Gram partials [groups, 1444] as brl_ppo_heads_loss_split leaves them (P^T P of 4 rows of
    non-negative probabilities per group)"""
    lp = torch.rand((groups, 8), generator=gen)
    lp[:, 5:] = 0
    pr = torch.rand((groups, 4, NA), generator=gen) * (torch.rand((groups, 4, NA), generator=gen) < 0.4)
    return lp, torch.einsum("gri,grj->gij", pr, pr).reshape(groups, GRAM).contiguous()


# ---- brl_ppo_loss, brl_ppo_stats -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 5, 67])
def test_ppo_loss_and_stats_guarded(batch):
    """brl_ppo_loss: one short group of 4 samples, two groups, 17 groups with a ragged last one; logits with row stride 38 and 40
    (NaN in columns 38, 39), masked and unmasked, illegal_probs given and NULL; partials exactly ceil(batch / 4) * 8 floats; every
    float / int32 array at exactly 4 bytes, mask at 1.  brl_ppo_stats on those partials with gram given and NULL."""
    L, check = _lib()
    gen = _gen(batch, 1)
    li, z, value = _loss_inputs(batch, gen), _randn(gen, batch, NA) * 2, _randn(gen, batch)
    gram0 = _stats_inputs(1, gen)[1].reshape(NA, NA)
    groups = (batch + 3) // 4
    for stride, masked, with_illp in ((38, 1, True), (40, 0, False), (40, 1, True)):
        def run(mem):
            lg = mem.inp("logits", z, F32, 4, ld=stride, plain_ld=stride if stride != NA else None)
            v = mem.inp("value", value, F32, 4)
            cols = _place_loss(mem, li)
            dl, dv, pa = mem.out("dlogits", (batch, NA), F32, 4), mem.out("dvalue", (batch,), F32, 4), mem.out("partials", (groups * 8,), F32, 4)
            ip = mem.out("illegal_probs", (batch, NA), F32, 4) if with_illp else None
            check(L.brl_ppo_loss(0, _p(lg), lg.stride(0), _p(v), *[_p(c) for c in cols], batch, 0.2, 0.5, 0.01, masked, 1, _p(dl), _p(dv),
                                 _p(pa), _p(ip), _s()))
            gr = mem.inp("gram", gram0, F32, 4) if with_illp else None
            st = mem.out("stats", (8,), F32, 4)
            check(L.brl_ppo_stats(0, _p(pa), batch, _p(gr), 0.5, 0.01, _p(st), _s()))
            return {"dlogits": dl, "dvalue": dv, "partials": pa, "stats": st, **({"illegal_probs": ip} if with_illp else {})}
        _, g, _ = both(run, capacity=1 << 20)
        assert bool(torch.isfinite(g["dlogits"]).all()) and bool(torch.isfinite(g["stats"]).all()), (stride, masked)
        assert (float(g["stats"][6]) > 0) == with_illp


# ---- brl_ppo_heads_loss_split, brl_ppo_stats_gram ------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden", [16, 272])
@pytest.mark.parametrize("batch", [1, 5, 67])
def test_heads_loss_split_and_stats_gram_guarded(hidden, batch):
    """brl_ppo_heads_loss_split at hidden 16 (the smallest: one K group) and 272 (16 x 17: no multiple of 64, 17 K groups that 8
    splits and 8 waves do not divide), ldh = hidden + 4 with NaN padding, ksplit 1 and 8 (the largest the entry point accepts; at
    hidden 16 seven of the eight parts have no K group and must still be written, as zeros), head_parts exactly [ksplit, batch,
    39], heads_out / gram_partials given and NULL, reward_scaling 0 and 1; h and head_w at exactly 16 bytes, everything else at 4.
    brl_ppo_stats_gram on its partials: row_index NULL, and pointing at row 2 of 4; vec_out given and NULL."""
    L, check = _lib()
    gen = _gen(hidden, batch, 2)
    li = _loss_inputs(batch, gen)
    h = _randn(gen, batch, hidden).clamp_min(0)
    hw, hb = _randn(gen, NH, hidden) / hidden ** 0.5 * 2, _randn(gen, NH) * 0.1
    groups = (batch + 3) // 4
    for ksplit, optional, rs in ((1, True, 0), (8, False, 1), (8, True, 1)):
        def run(mem):
            hs = mem.inp("h", h, F32, 16, ld=hidden + 4)
            w, b = mem.inp("head_w", hw, F32, 16), mem.inp("head_b", hb, F32, 4)
            cols = _place_loss(mem, li)
            ho = mem.out("heads_out", (batch, NH), F32, 4) if optional else None
            dh, pa = mem.out("dheads", (batch, NH), F32, 4), mem.out("partials", (groups * 8,), F32, 4)
            gp = mem.out("gram_partials", (groups, GRAM), F32, 4) if optional else None
            parts = mem.out("head_parts", (ksplit, batch, NH), F32, 4)
            check(L.brl_ppo_heads_loss_split(0, _p(hs), hs.stride(0), _p(w), _p(b), hidden, *[_p(c) for c in cols], batch, 0.2, 0.5, 0.01,
                                             1, 1, rs, _p(ho), _p(dh), _p(pa), _p(gp), _p(parts), ksplit, _s()))
            out = {"dheads": dh, "partials": pa, "head_parts": parts}
            if optional:
                out.update(heads_out=ho, gram_partials=gp)
                row = mem.out("stats_row", (1, 8), F32, 4)
                vec = mem.out("vec_out", (40,), F32, 4)
                check(L.brl_ppo_stats_gram(0, _p(pa), groups, batch, _p(gp), groups, 0.5, 0.01, 0.1, _p(row), None, _p(vec), _s()))
                ri = mem.inp("row_index", torch.tensor([2]), I32, 4)
                log = mem.out("stats_log", (4, 8), F32, 4)
                check(L.brl_ppo_stats_gram(0, _p(pa), groups, batch, _p(gp), groups, 0.5, 0.01, 0.1, _p(log), _p(ri), None, _s()))
                out.update(stats_row=row, vec_out=vec, stats_log_row=log[2:3])
            return out
        _, g, gm = both(run, capacity=1 << 21, partial=("stats_log",))
        assert bool(torch.isfinite(g["dheads"]).all()), (ksplit, rs)
        if optional:
            _only_row(gm, "stats_log", 2)
            assert torch.equal(g["stats_log_row"], g["stats_row"])
            heads = g["heads_out"].cpu().double()
            want = h.double() @ hw.double().t() + hb.double()
            assert float((heads - want).abs().max()) < 1e-4 * max(1.0, float(want.abs().max()))   # (the product's inputs were the right ones)


@pytest.mark.parametrize("rows", [1, 3])
def test_ppo_stats_rows_guarded(rows):
    """brl_ppo_stats_rows: stat_sums [rows, 8], gram_sums [rows, 1444], out_rows [rows, 8], each exactly sized, at 4 bytes."""
    L, check = _lib()
    lp, gp = _stats_inputs(rows, _gen(rows, 3))

    def run(mem):
        ss, gs = mem.inp("stat_sums", lp, F32, 4), mem.inp("gram_sums", gp, F32, 4)
        out = mem.out("out_rows", (rows, 8), F32, 4)
        check(L.brl_ppo_stats_rows(0, _p(ss), _p(gs), rows, 64, 0.5, 0.01, 0.1, _p(out), _s()))
        return {"out_rows": out}
    _, g, _ = both(run, capacity=1 << 20)
    assert bool(torch.isfinite(g["out_rows"]).all()) and bool((g["out_rows"][:, 6] > 0).all())


# ---- brl_ppo_illegal_grad ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 5, 67])
def test_illegal_grad_guarded(batch):
    """dheads [batch, 39] is in/out: columns 0..37 change, column 38 (the value's gradient) keeps its bits."""
    L, check = _lib()
    gen = _gen(batch, 4)
    heads, mask, d0 = _randn(gen, batch, NH), (torch.rand((batch, NA), generator=gen) < 0.5).to(U8), _randn(gen, batch, NH)
    vec = torch.cat([torch.nn.functional.normalize(torch.rand(NA, generator=gen), dim=0), torch.tensor([0.7, 0.0])])

    def run(mem):
        hd, mk, vc = mem.inp("heads", heads, F32, 4), mem.inp("mask", mask, U8, 1), mem.inp("vec", vec, F32, 4)
        dh = mem.inp("dheads", d0, F32, 4, inout=True)
        check(L.brl_ppo_illegal_grad(0, _p(hd), _p(mk), _p(vc), 0.3, batch, _p(dh), _s()))
        return {"dheads": dh}
    _, g, _ = both(run, capacity=1 << 20)
    got = g["dheads"].cpu()
    assert torch.equal(got[:, 38], d0[:, 38]) and not torch.equal(got[:, :38], d0[:, :38])


# ---- the heads' weight-gradient role (brl_ppo_heads_bwd, brl_act_bwd_colsum_heads_dw, brl_mlp_gemm_dh_heads_dw) ----------------
class _DwRole:
    """the role's arrays at hidden 256: dheads [batch, 39] and h [batch, 260] in; dw_partials [nsplit, 39 * 256], db_partials
    [nsplit, 39] out, each exactly sized; with the sums, row 2 of stat_sums [4, 8] / gram_sums [4, 1444]"""
    H = 256

    def __init__(self, batch, nsplit, sums, gen):
        self.batch, self.nsplit, self.sums = batch, nsplit, sums
        self.groups = (batch + 3) // 4
        self.dheads, self.h = _randn(gen, batch, NH), _randn(gen, batch, self.H).clamp_min(0)
        self.lp, self.gp = _stats_inputs(self.groups, gen)

    def place_inputs(self, mem):
        self.d = mem.inp("dheads", self.dheads, F32, 4)
        self.hs = mem.inp("h", self.h, F32, 16, ld=self.H + 4)

    def place_outputs(self, mem):
        self.dw, self.db = mem.out("dw_partials", (self.nsplit, NH * self.H), F32, 4), mem.out("db_partials", (self.nsplit, NH), F32, 4)
        self.out = {"dw_partials": self.dw, "db_partials": self.db}
        self.tail = (None, None, 0, None, None, None)
        if self.sums:
            lp, gp = mem.inp("loss_partials", self.lp, F32, 4), mem.inp("gram_partials", self.gp, F32, 4)
            ri = mem.inp("row_index", torch.tensor([2]), I32, 4)
            ss, gs = mem.out("stat_sums", (4, 8), F32, 4), mem.out("gram_sums", (4, GRAM), F32, 4)
            self.tail = (_p(lp), _p(gp), self.groups, _p(ri), _p(ss), _p(gs))
            self.out.update(stat_sums_row=ss[2:3], gram_sums_row=gs[2:3])

    partial = ("stat_sums", "gram_sums")

    def verify(self, g, gm):
        """the sums landed in row 2 alone; the partials add up to the float64 products"""
        if self.sums:
            _only_row(gm, "stat_sums", 2)
            _only_row(gm, "gram_sums", 2)
            assert float((g["stat_sums_row"].cpu().double()[0] - self.lp.double().sum(0)).abs().max()) < 1e-4
        want = self.dheads.double().t() @ self.h.double()
        got = g["dw_partials"].cpu().double().sum(0).reshape(NH, self.H)
        assert float((got - want).abs().max()) < 1e-4 * max(1.0, float(want.abs().max()))
        assert float((g["db_partials"].cpu().double().sum(0) - self.dheads.double().sum(0)).abs().max()) < 1e-4


def _nsplits(batch):
    return ((batch + 63) // 64, (batch + 63) // 64 + 1)


@pytest.mark.parametrize("batch", [1, 17, 65])
def test_heads_bwd_guarded(batch):
    """brl_ppo_heads_bwd at hidden 256 (its minimum), ldh = 260 with NaN padding, batch 1 / 17 / 65 (one short 16-row tile; a
    second tile of one row; a second 64-row split of one row), nsplit = ceil(batch / 64) and one more (at batch 1 the second split
    has no row: its partials are zeros, and h has no row to read for it); the full form with and without the statistics sums,
    and the dw_partials = db_partials = NULL form.  h, head_w, dh, tile_sums at exactly 16 bytes; tile_sums exactly
    ceil(batch / 16) * 256 floats."""
    L, check = _lib()
    H, tiles = 256, (batch + 15) // 16
    for k, (nsplit, form) in enumerate(zip(_nsplits(batch) + _nsplits(batch)[:1], ("sums", "full", "dh_only"))):
        gen = _gen(batch, nsplit, 5)
        role = _DwRole(batch, nsplit, form == "sums", gen)
        hw = _randn(gen, NH, H) / 16
        act = k % 2

        def run(mem):
            role.place_inputs(mem)
            w = mem.inp("head_w", hw, F32, 16)
            dh, ts = mem.out("dh", (batch, H), F32, 16), mem.out("tile_sums", (tiles * H,), F32, 16)
            out = {"dh": dh, "tile_sums": ts}
            if form == "dh_only":
                dw = db = None
                tail = (None, None, 0, None, None, None)
            else:
                role.place_outputs(mem)
                dw, db, tail = role.dw, role.db, role.tail
                out.update(role.out)
            check(L.brl_ppo_heads_bwd(0, _p(role.d), _p(role.hs), role.hs.stride(0), _p(w), batch, H, act, nsplit, _p(dw), _p(db), _p(dh), _p(ts),
                                      *tail, _s()))
            return out
        _, g, gm = both(run, capacity=1 << 21, partial=role.partial)
        if form != "dh_only":
            role.verify(g, gm)
        want = (g["dh"].cpu().double().reshape(batch, H))
        sums = torch.stack([want[16 * t:16 * t + 16].sum(0) for t in range(tiles)]).reshape(-1)
        assert float((g["tile_sums"].cpu().double() - sums).abs().max()) < 1e-4


# ---- brl_act_bwd_colsum, brl_act_bwd_colsum_heads_dw ---------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 17, 65])
@pytest.mark.parametrize("cols", [4, 260])
def test_act_bwd_colsum_guarded(rows, cols):
    """brl_act_bwd_colsum: one 16-byte piece per row, and 260 columns = one block of 256 + a tail block of 4; rows 1 / 17 / 65 (a
    short tile; a second tile of one row; a fifth); ld = cols + 4 with NaN in the padding of both dh and h; both activations;
    dh (in/out), h and scratch at exactly 16 bytes, scratch exactly ceil(rows / 16) * cols floats."""
    L, check = _lib()
    tiles = (rows + 15) // 16
    for act in (0, 1):
        gen = _gen(rows, cols, act, 6)
        d0, h = _randn(gen, rows, cols), (_randn(gen, rows, cols).clamp_min(0) if act == 0 else torch.tanh(_randn(gen, rows, cols)))

        def run(mem):
            dh = mem.inp("dh", d0, F32, 16, ld=cols + 4, inout=True)
            hs = mem.inp("h", h, F32, 16, ld=cols + 4)
            sc = mem.out("scratch", (tiles, cols), F32, 16)
            check(L.brl_act_bwd_colsum(0, _p(dh), _p(hs), rows, cols, dh.stride(0), act, _p(sc), _s()))
            return {"dh": dh, "scratch": sc}
        _, g, _ = both(run, capacity=1 << 20)
        want = d0 * ((h > 0).float() if act == 0 else 1 - h * h)
        assert torch.equal(g["dh"].cpu(), want)
        sums = torch.stack([want[16 * t:16 * t + 16].double().sum(0) for t in range(tiles)])
        assert float((g["scratch"].cpu().double() - sums).abs().max()) < 1e-5


@pytest.mark.parametrize("rows,cols,batch", [(1, 4, 17), (17, 260, 17), (65, 4, 65), (65, 260, 65)])
def test_act_bwd_colsum_heads_dw_guarded(rows, cols, batch):
    """brl_act_bwd_colsum_heads_dw: brl_act_bwd_colsum's shapes with the heads' weight-gradient role (hidden 256, batch 17 / 65,
    nsplit = ceil(batch / 64) and one more, with and without the statistics sums) in the same launch; every output of the role
    exactly sized."""
    L, check = _lib()
    tiles = (rows + 15) // 16
    for k, nsplit in enumerate(_nsplits(batch)):
        gen = _gen(rows, cols, nsplit, 7)
        role = _DwRole(batch, nsplit, k == 0, gen)
        d0, h = _randn(gen, rows, cols), _randn(gen, rows, cols).clamp_min(0)

        def run(mem):
            dz = mem.inp("dz", d0, F32, 16, ld=cols + 4, inout=True)
            hh = mem.inp("hh", h, F32, 16, ld=cols + 4)
            sc = mem.out("scratch", (tiles, cols), F32, 16)
            role.place_inputs(mem)
            role.place_outputs(mem)
            check(L.brl_act_bwd_colsum_heads_dw(0, _p(dz), _p(hh), rows, cols, dz.stride(0), 0, _p(sc), _p(role.d), _p(role.hs),
                                                role.hs.stride(0), batch, role.H, nsplit, _p(role.dw), _p(role.db), *role.tail, _s()))
            return {"dz": dz, "scratch": sc, **role.out}
        _, g, gm = both(run, capacity=1 << 21, partial=role.partial)
        role.verify(g, gm)
        assert torch.equal(g["dz"].cpu(), d0 * (h > 0).float())


@pytest.mark.parametrize("batch", [17, 65])
def test_mlp_gemm_dh_heads_dw_guarded(batch):
    """brl_mlp_gemm_dh_heads_dw: the NN + GATE_COLSUM product (m = batch, n = 36, k = 52: edge tiles and a K tail) with the heads'
    role at hidden 256 in the same launch; dz / w / out / gate / h at exactly 16 bytes, every leading dimension + 4."""
    from tests.gpu_util import gemm_bound, gemm_operands, gemm_ref64
    L, check = _lib()
    m, n, k = batch, 36, 52
    A, B, bias, gate = (t.cpu() for t in gemm_operands(1, m, n, k, 300 + batch))
    for i, nsplit in enumerate(_nsplits(batch)):
        role = _DwRole(batch, nsplit, i == 0, _gen(batch, nsplit, 8))

        def run(mem):
            a = mem.inp("dz", A, F32, 16, ld=k + 4)
            w = mem.inp("w", B, F32, 16, ld=n + 4)
            ga = mem.inp("gate", gate, F32, 16, ld=n + 4)
            c = mem.out("out", (m, n), F32, 16, ld=n + 4)
            cs = mem.out("colsum", ((m + 63) // 64, n), F32, 4)
            role.place_inputs(mem)
            role.place_outputs(mem)
            check(L.brl_mlp_gemm_dh_heads_dw(0, _p(a), a.stride(0), _p(w), w.stride(0), _p(c), c.stride(0), m, n, k, 0, _p(ga), ga.stride(0),
                                             _p(cs), _p(role.d), _p(role.hs), role.hs.stride(0), batch, role.H, nsplit, _p(role.dw), _p(role.db),
                                             *role.tail, _s()))
            return {"out": c, "colsum": cs, **role.out}
        _, g, gm = both(run, capacity=1 << 21, partial=role.partial)
        role.verify(g, gm)
        ref = gemm_ref64(1, 2, 0, A, B, bias, gate)
        assert float((g["out"].cpu().double() - ref).abs().max()) < gemm_bound(ref, k)


# ---- brl_bias_finalize_ex, brl_bias_finalize_rows ------------------------------------------------------------------------------
SEG_COLS, SEG_TILES = (39, 4, 260), (1, 3, 5)


def _seg_tables(parts, outs, cols=SEG_COLS, tiles=SEG_TILES):
    vp, i64 = C.c_void_p * len(parts), C.c_int64 * len(parts)
    return vp(*[t.data_ptr() for t in parts]), i64(*cols), i64(*tiles), vp(*[t.data_ptr() for t in outs])


@pytest.mark.parametrize("first_row_seg", [None, 0, 1, 3])
def test_bias_finalize_guarded(first_row_seg):
    """Three segments in one launch — 39 columns of one tile, 4 of three, 260 (five blocks of 64, the last of 4) of five — with
    partials exactly tiles * cols floats and outputs exactly cols, at 4 bytes.  brl_bias_finalize_ex (None), and _rows with
    first_row_seg 0 / 1 / 3 (= nseg: no row segment): a row segment writes row 2 of its [4, cols] log and nothing else."""
    L, check = _lib()
    gen = _gen(9, -1 if first_row_seg is None else first_row_seg)
    vals = [_randn(gen, t, c) for c, t in zip(SEG_COLS, SEG_TILES)]
    as_rows = [first_row_seg is not None and i >= first_row_seg for i in range(3)]

    def run(mem):
        parts = [mem.inp(f"partials{i}", v.reshape(-1), F32, 4) for i, v in enumerate(vals)]
        outs = [mem.out(f"out{i}", (4, c) if as_rows[i] else (c,), F32, 4) for i, c in enumerate(SEG_COLS)]
        if first_row_seg is None:
            check(L.brl_bias_finalize_ex(0, 3, *_seg_tables(parts, outs), _s()))
        else:
            ri = mem.inp("row_index", torch.tensor([2]), I32, 4)
            check(L.brl_bias_finalize_rows(0, 3, *_seg_tables(parts, outs), first_row_seg, _p(ri), _s()))
        return {f"out{i}": (o[2] if as_rows[i] else o) for i, o in enumerate(outs)}
    _, g, gm = both(run, capacity=1 << 20, partial=[f"out{i}" for i in range(3) if as_rows[i]])
    for i, v in enumerate(vals):
        if as_rows[i]:
            _only_row(gm, f"out{i}", 2)
        assert float((g[f"out{i}"].cpu().double() - v.double().sum(0)).abs().max()) < 1e-5


# ---- brl_mb_gather_bind, brl_mb_gather_dev -------------------------------------------------------------------------------------
TRAJ_ROWS = 12


def _trajectory(gen):
    n = TRAJ_ROWS
    return dict(done=(torch.rand(n, generator=gen) < 0.3).to(U8), action=torch.randint(0, NA, (n,), generator=gen).to(I32),
                value=_randn(gen, n), reward=_randn(gen, n), log_prob=-torch.rand(n, generator=gen),
                obs=(torch.rand((n, 480), generator=gen) < 0.2).to(U8), legal_action_mask=(torch.rand((n, NA), generator=gen) < 0.5).to(U8),
                adv=_randn(gen, n), tgt=_randn(gen, n))


def _bind_gather(mem, L, check, traj, perm, mbs, mb0, mb_inout=False):
    """places the trajectory (every brl_transition column its own placement), the permutation, the counter, args_dev (exactly 256
    bytes, at 8) and the seven minibatch buffers (exactly sized), and binds them -> (args_dev, mb_index, outputs)"""
    from brl_amd import _capi
    tp, keep = _capi.TransitionPtrs(), []      # (keep: the structure and args_dev hold addresses only; the tensors must outlive the launches)
    for name, dt, align in (("done", U8, 1), ("action", I32, 4), ("value", F32, 4), ("reward", F32, 4), ("log_prob", F32, 4), ("obs", U8, 4),
                            ("legal_action_mask", U8, 1)):
        keep.append(mem.inp("traj_" + name, traj[name], dt, align))
        setattr(tp, name, keep[-1].data_ptr())
    adv, tgt = mem.inp("adv", traj["adv"], F32, 4), mem.inp("tgt", traj["tgt"], F32, 4)
    pm = mem.inp("perm", perm, I64, 8)
    keep += [adv, tgt, pm]
    mb = mem.inp("mb_index", torch.tensor([mb0]), I32, 4, inout=mb_inout)
    args = mem.out("args_dev", (256,), U8, 8)
    out = {"x0": mem.out("x0", (mbs, 480), F32, 16), "mask": mem.out("mask", (mbs, NA), U8, 1), "action": mem.out("action", (mbs,), I32, 4)}
    for name in ("old_value", "old_log_prob", "gae", "targets"):
        out[name] = mem.out(name, (mbs,), F32, 4)
    check(L.brl_mb_gather_bind(0, C.byref(tp), _p(adv), _p(tgt), _p(pm), _p(mb), mbs, *[_p(out[k]) for k in (
        "x0", "mask", "action", "old_value", "old_log_prob", "gae", "targets")], perm.numel() // mbs, _p(args), _s()))
    return (args, keep), mb, out


def _gathered(traj, rows):
    return {"x0": traj["obs"][rows].float(), "mask": traj["legal_action_mask"][rows], "action": traj["action"][rows],
            "old_value": traj["value"][rows], "old_log_prob": traj["log_prob"][rows], "gae": traj["adv"][rows], "targets": traj["tgt"][rows]}


@pytest.mark.parametrize("mbs", [1, 5])
@pytest.mark.parametrize("last", [False, True])
def test_mb_gather_guarded(mbs, last):
    """brl_mb_gather_bind + brl_mb_gather_dev on a trajectory of 12 rows: obs at exactly 4 bytes (read as 4-byte words), x0 at 16,
    perm and args_dev at 8, masks at 1, the other columns at 4; *mb_index 0 and the last minibatch `perm` holds; the trajectory's
    done and reward columns are not read.  args_dev is 256 bytes of which the arguments fill the front; nothing behind it."""
    L, check = _lib()
    gen = _gen(mbs, last, 10)
    traj = _trajectory(gen)
    nsteps = TRAJ_ROWS // mbs
    perm = torch.randperm(TRAJ_ROWS, generator=gen)[:nsteps * mbs]
    mb0 = nsteps - 1 if last else 0

    def run(mem):
        (args, keep), mb, out = _bind_gather(mem, L, check, traj, perm, mbs, mb0)
        check(L.brl_mb_gather_dev(0, _p(args), mbs, _s()))
        torch.cuda.synchronize()
        return out
    _, g, _ = both(run, capacity=1 << 20, partial=("args_dev",))
    for name, want in _gathered(traj, perm[mb0 * mbs:(mb0 + 1) * mbs]).items():
        assert torch.equal(g[name].cpu(), want), name


# ---- brl_adam_clip_fin_gather --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,seg_cols", [(8, (4,)), (4100, (4,)), (4100, (4, 39))])
def test_adam_clip_fin_gather_guarded(n, seg_cols):
    """brl_adam_clip_fin_gather on flat buffers of exactly n floats at exactly 16 bytes: n = 8 (two pieces: 1022 of the 1024 sweep
    blocks have nothing), 4100 (1025 pieces: chunks of 2, the last blocks empty); one finalize segment of 4 columns, and two (4,
    then 39 + 1 float of zero padding) that tile the end of g; scratch exactly 1024 + sum ceil(cols / 64) floats.  Once with lr_dev,
    norm_out, max_norm 0.5 and the gather of the next minibatch (bound to a 12-row trajectory, mbs 5: the launch advances
    *mb_index to 1 and gathers that one), once with all of them NULL / off.  p / g / m / v and the counters are in/out."""
    L, check = _lib()
    gen = _gen(n, len(seg_cols), 11)
    seg_tiles = (3, 2)[:len(seg_cols)]
    tail = (sum(seg_cols) + 3) // 4 * 4
    p0, g0, m0, v0 = _randn(gen, n), _randn(gen, n), _randn(gen, n) * 0.1, torch.rand(n, generator=gen) * 0.01
    g0[n - tail:] = 0           # (produced by the launch; the pad stays zero)
    parts = [_randn(gen, t, c) for c, t in zip(seg_cols, seg_tiles)]
    traj, mbs = _trajectory(gen), 5
    perm = torch.randperm(TRAJ_ROWS, generator=gen)[:10]
    nscratch = 1024 + sum((c + 63) // 64 for c in seg_cols)
    for full in (True, False):
        def run(mem):
            P, G, M, V = (mem.inp(name, x, F32, 16, inout=True) for name, x in (("p", p0), ("g", g0), ("m", m0), ("v", v0)))
            step = mem.inp("step", torch.tensor([3.0]), F32, 4, inout=True)
            sc = mem.out("scratch", (nscratch,), F32, 4)
            ps = [mem.inp(f"partials{i}", x.reshape(-1), F32, 4) for i, x in enumerate(parts)]
            outs, off = [], n - tail
            for c in seg_cols:
                outs.append(G[off:off + c])
                off += c
            out = {"p": P, "g": G, "m": M, "v": V, "step": step, "scratch": sc}
            lr = norm = mb = args = keep = None
            if full:
                lr, norm = mem.inp("lr_dev", torch.tensor([3e-3]), F32, 4), mem.out("norm_out", (1,), F32, 4)
                (args, keep), mb, gathered = _bind_gather(mem, L, check, traj, perm, mbs, 0, mb_inout=True)
                out.update(gathered, norm_out=norm, mb_index=mb)
            check(L.brl_adam_clip_fin_gather(0, _p(P), _p(G), _p(M), _p(V), n, _p(step), 1e-3, _p(lr), 0.9, 0.999, 1e-8, 0.5 if full else 0.0,
                                             _p(sc), nscratch, _p(mb), _p(norm), _p(args), mbs if full else 0, len(seg_cols),
                                             *_seg_tables(ps, outs, seg_cols, seg_tiles), _s()))
            torch.cuda.synchronize()       # (`keep`, `ps`, `lr`: inputs that only this frame holds)
            return out
        _, g, _ = both(run, capacity=1 << 20, partial=("args_dev",))
        assert float(g["step"]) == 4.0
        want_g = torch.cat([g0[:n - tail]] + [x.double().sum(0).float() for x in parts] + [torch.zeros(tail - sum(seg_cols))])
        assert float((g["g"].cpu().double() - want_g.double()).abs().max()) < 1e-5
        assert not torch.equal(g["p"].cpu(), p0) and bool(torch.isfinite(g["p"]).all())
        if full:
            assert int(g["mb_index"]) == 1 and abs(float(g["norm_out"]) - float(want_g.double().norm())) < 1e-3
            for name, want in _gathered(traj, perm[mbs:2 * mbs]).items():
                assert torch.equal(g[name].cpu(), want), name


# ---- brl_adam_shard_norm, brl_adam_shard_apply ---------------------------------------------------------------------------------
@pytest.mark.parametrize("ln", [4, 1028])
@pytest.mark.parametrize("nsub", [1, 3])
def test_adam_shards_guarded(ln, nsub):
    """world 2, two buckets of two slices of `ln` floats each, 4 floats between the buckets and 4 behind the last: the gap, the
    tail and the slices of ranks outside [rank_lo, rank_hi) keep their bits in p / m / v; g is read only.  ln = 4: one piece per
    slice (with nsub 3, two of the three sub-blocks are empty and still write their partial); 1028: 257 pieces, the 256-thread
    loop's second trip.  partials exactly world * nbuckets * nsub floats: a rank range writes its rows and no others."""
    from brl_amd import _capi
    L, check = _lib()
    n = 4 * ln + 8
    geom = _capi.ShardGeom()
    geom.nbuckets, geom.world, geom.nsub = 2, 2, nsub
    geom.off[0], geom.len[0], geom.off[1], geom.len[1] = 0, ln, 2 * ln + 4, ln
    gen = _gen(ln, nsub, 12)
    p0, g0, m0, v0 = _randn(gen, n), _randn(gen, n), _randn(gen, n) * 0.1, torch.rand(n, generator=gen) * 0.01
    owned = torch.zeros((2, n), dtype=torch.bool)
    for r in range(2):
        for b in range(2):
            lo = int(geom.off[b]) + r * ln
            owned[r, lo:lo + ln] = True
    for lo, hi in ((0, 1), (1, 2), (0, 2)):
        def run(mem):
            P, M, V = (mem.inp(name, x, F32, 16, inout=True) for name, x in (("p", p0), ("m", m0), ("v", v0)))
            G = mem.inp("g", g0, F32, 16)
            step = mem.inp("step", torch.tensor([3.0]), F32, 4, inout=True)
            mb = mem.inp("mb_index", torch.tensor([0]), I32, 4, inout=True)
            mine = mem.out("partials_of_range", (2, 2 * nsub), F32, 4)
            check(L.brl_adam_shard_norm(0, _p(G), C.byref(geom), lo, hi, 0.5, _p(mine), _p(step), _p(mb), _s()))
            allp = mem.out("partials", (2, 2 * nsub), F32, 4)
            check(L.brl_adam_shard_norm(0, _p(G), C.byref(geom), 0, 2, 0.5, _p(allp), _p(step), None, _s()))
            norm = mem.out("norm_out", (1,), F32, 4)
            check(L.brl_adam_shard_apply(0, _p(P), _p(G), _p(M), _p(V), C.byref(geom), lo, hi, _p(allp), _p(step), 1e-3, None, 0.9, 0.999,
                                         1e-8, 0.5, 0.5, _p(norm), None, 0, _s()))
            return {"p": P, "m": M, "v": V, "step": step, "mb_index": mb, "partials_of_range": mine[lo:hi], "partials": allp, "norm_out": norm}
        _, g, gm = both(run, capacity=1 << 20, partial=("partials_of_range",))
        u = gm.arena.unwritten(gm.outs["partials_of_range"])
        assert not u[lo:hi].any() and u[:lo].all() and u[hi:].all()
        assert torch.equal(g["partials_of_range"], g["partials"][lo:hi]) and float(g["step"]) == 5.0 and int(g["mb_index"]) == 1
        touched = owned[lo:hi].any(0)
        for name, x0 in (("p", p0), ("m", m0), ("v", v0)):
            got = g[name].cpu()
            assert torch.equal(got[~touched], x0[~touched]), f"{name}: changed outside the slices of ranks [{lo}, {hi})"
            changed = got[touched] != x0[touched]     # (a parameter's step can be below half an ulp of it: m and v always move)
            assert bool(changed.all()) if name != "p" else float(changed.float().mean()) > 0.9, name
        want = float((0.5 * g0[owned.any(0)]).double().norm())
        assert abs(float(g["norm_out"]) - want) < 1e-4 * max(1.0, want)


# ---- brl_fair_forward, brl_fair_chain ------------------------------------------------------------------------------------------
def _fair_params(gen):
    H = 200
    ins = [480 if l == 0 else 680 if l == 6 else H for l in range(11)]
    return ([_randn(gen, H, k) / k ** 0.5 for k in ins], [_randn(gen, H) * 0.1 for _ in range(11)], _randn(gen, NH, H) / H ** 0.5,
            _randn(gen, NH) * 0.1)


def _place_fair_net(mem, params):
    """-> (brl_fair_net, the placed tensors: the structure holds addresses only)"""
    from brl_amd import _capi
    ws, bs, hw, hb = params
    net, keep = _capi.FairNet(), []
    for l in range(11):
        keep += [mem.inp(f"w{l}", ws[l], F32, 16), mem.inp(f"b{l}", bs[l], F32, 16)]
        net.w[l], net.b[l] = keep[-2].data_ptr(), keep[-1].data_ptr()
    keep += [mem.inp("head_w", hw, F32, 16), mem.inp("head_b", hb, F32, 4)]
    net.head_w, net.head_b = keep[-2].data_ptr(), keep[-1].data_ptr()
    return net, keep


@pytest.fixture(scope="module")
def fair_params():
    return _fair_params(_gen(13))


@pytest.mark.parametrize("rows", [1, 17])
def test_fair_forward_guarded(fair_params, rows):
    """brl_fair_forward: 16 rows per workgroup — one short workgroup, and a second of one row; x and the weights at exactly 16 bytes,
    head_b, logits [rows, 38] and value [rows] at 4 and exactly sized."""
    L, check = _lib()
    x = (torch.rand((rows, 480), generator=_gen(rows, 14)) < 0.2).float()

    def run(mem):
        net, keep = _place_fair_net(mem, fair_params)
        xs = mem.inp("x", x, F32, 16)
        lg, va = mem.out("logits", (rows, NA), F32, 4), mem.out("value", (rows,), F32, 4)
        check(L.brl_fair_forward(0, C.byref(net), _p(xs), rows, int(rows > 1), _p(lg), _p(va), _s()))
        torch.cuda.synchronize()
        return {"logits": lg, "value": va}
    _, g, _ = both(run, capacity=1 << 23)
    assert bool(torch.isfinite(g["logits"]).all()) and bool(torch.isfinite(g["value"]).all())


@pytest.mark.parametrize("batch,act,with_gram", [(16, 0, True), (48, 1, False), (48, 0, True)])
def test_fair_chain_guarded(fair_params, batch, act, with_gram):
    """brl_fair_chain at one and at three workgroups of 16 samples: every brl_fair_work array a placement of its own, at exactly
    16 bytes and exactly the header's size; gram_partials given and NULL; both activations.  Its logits / value against
    brl_fair_forward's on the same rows is test_gpu_parity's business; here: the same bits as on dense tensors."""
    from brl_amd import _capi
    L, check = _lib()
    gen = _gen(batch, act, 15)
    li = _loss_inputs(batch, gen)
    x = (torch.rand((batch, 480), generator=gen) < 0.2).float()
    nwg, H = batch // 16, 200
    shapes = dict(inp=(9, batch, H), dzs=(9, batch, H), gates=(4, batch, H), cat6=(batch, 680), x4=(batch, H), dz0=(batch, H), dz6=(batch, H),
                  dheads=(batch, 40), tiles=(11 * nwg * H + nwg * NH,), partials=(nwg, 8), gram_partials=(nwg, GRAM))

    def run(mem):
        net, keep = _place_fair_net(mem, fair_params)
        xs = mem.inp("x0", x, F32, 16)
        cols = _place_loss(mem, li)
        work, out = _capi.FairWork(), {}
        for name, shape in shapes.items():
            if name == "gram_partials" and not with_gram:
                continue
            out[name] = mem.out(name, shape, F32, 16)
            setattr(work, name, out[name].data_ptr())
        check(L.brl_fair_chain(0, C.byref(net), _p(xs), *[_p(c) for c in cols], batch, 0.2, 0.5, 0.01, 1, 1, 0, act, C.byref(work), _s()))
        torch.cuda.synchronize()
        return out
    _, g, _ = both(run, capacity=1 << 23)
    assert bool(torch.isfinite(g["dheads"]).all()) and bool((g["dheads"][:, 39] == 0).all())
    assert torch.equal(g["cat6"][:, H:].cpu(), x)
