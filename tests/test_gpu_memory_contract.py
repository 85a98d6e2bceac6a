"""-m gpu: what the headers promise about MEMORY — alignment, leading dimensions, strides, what is left untouched — checked the
way a sanitizer would, inside memory the process owns (tests/guarded.py; DESIGN.md "Memory contract").

Every case drives an entry point through _capi twice on the same input values:
  plain    fresh dense torch tensors, as every other test of the suite does (512-byte aligned blocks of the caching allocator);
  guarded  every pointer argument placed in ONE Arena: at the minimum alignment its header states and no better (16 where the
           header states none and the kernel moves 16-byte pieces; never below what header or code require), every leading
           dimension and stride the signature offers larger than dense by the smallest step the header allows, NaN bytes in the
           padding of inputs, a position-dependent pattern everywhere else.
and asserts: the guarded outputs equal the plain ones bit for bit; no guard byte changed (`Arena.check` names array, row and
column of the first one); every output element was written; an optional output passed as NULL leaves nothing written anywhere;
and, for the product kernels, the guarded result meets the bound the project already holds that kernel to against float64.
Nothing here can fault by design: no pointer is below an entry point's required alignment or outside the arena."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import distill_ref, sl_teacher
from tests.guarded import Arena, Guarded, Plain, _bits, both, round_up  # noqa: F401
from tests.gpu_util import gemm_bound, gemm_operands, gemm_ref64, make_env
from tests.nets import forward64, raw_net

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16, F16, U8, I16, I32, I64 = (torch.float32, torch.bfloat16, torch.float16, torch.uint8, torch.int16, torch.int32,
                                     torch.int64)


def _s():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _lib():
    from brl_amd import _capi
    return _capi.lib(), _capi.check


@pytest.fixture(scope="module")
def env(dds):
    return make_env(dds, 4)


def _rand(gen, *shape):
    return torch.rand(shape, generator=gen) * 2 - 1


# ---- brl_mlp_gemm / _group / _x3 / _x3_group -----------------------------------------------------------------------------------
GEMM_SHAPES = [(4, 4, 4), (68, 36, 52), (60, 132, 8)]      # one piece; edge tiles in m and n with a K tail; two column tiles, one K piece
X3_SHAPES = [(4, 4, 32), (132, 132, 160), (68, 260, 128)]


def _gemm_operands(layout, m, n, k, seed):
    """tests/gpu_util.py's operands (test_mlp_gemm_matches_float64's), on the host: each run places its own copy"""
    return tuple(t.cpu() for t in gemm_operands(layout, m, n, k, seed))


_gemm_ref64, _gemm_bound = gemm_ref64, gemm_bound      # the same reference and the same bound as that test


def _tile_n():
    return 64 if os.environ.get("BRL_GEMM_TILE_N") == "64" else 32   # (every shape here is <= 256 tiles: 64 x 32 unless forced)


@pytest.mark.parametrize("layout,epi", [(0, 0), (0, 1), (1, 0), (1, 2), (2, 0), (2, 3)])
def test_mlp_gemm_guarded(layout, epi):
    """brl_mlp_gemm, every layout x every epilogue it has: a / b / c / bias / gate at exactly 16 bytes, colsum / sqsum at 4 and
    sized exactly as the header says, lda / ldb / ldc / ldg = dense + 4 — an edge tile that stored a full tile width or a full 64
    rows, or folded a padding column into a sum, shows here.  colsum = NULL writes no column sums anywhere."""
    L, check = _lib()
    for (m, n, k) in GEMM_SHAPES:
        for act, with_colsum in ((0, True), (1, False)) if epi == 2 else ((0, True), (1, True)) if epi == 1 else ((0, True),):
            A, B, bias, gate = _gemm_operands(layout, m, n, k, 1000 * layout + 10 * epi + m + n + k)
            tm, wide = (m + 63) // 64, _tile_n()

            def run(mem):
                a = mem.inp("a", A, F32, 16, ld=A.shape[1] + 4)
                b = mem.inp("b", B, F32, 16, ld=B.shape[1] + 4)
                bi = mem.inp("bias", bias, F32, 16) if epi == 1 else None
                ga = mem.inp("gate", gate, F32, 16, ld=n + 4) if epi == 2 else None
                c = mem.out("c", (m, n), F32, 16, ld=n + 4)
                cs = mem.out("colsum", (tm, n), F32, 4) if epi == 2 and with_colsum else None
                sq = mem.out("sqsum", (tm * ((n + 31) // 32),), F32, 4) if epi == 3 else None
                check(L.brl_mlp_gemm(0, layout, epi, _p(a), a.stride(0), _p(b), b.stride(0), _p(c), c.stride(0), m, n, k, act, _p(bi),
                                     _p(ga), ga.stride(0) if ga is not None else 0, _p(cs), _p(sq), _s()))
                out = {"c": c}
                if cs is not None:
                    out["colsum"] = cs
                if sq is not None:          # one word per tile of the width in use; the words behind them belong to nobody
                    out["sqsum"] = sq[:tm * ((n + wide - 1) // wide)]
                return out
            _, g, gm = both(run, partial=("sqsum",))
            ref = _gemm_ref64(layout, epi, act, A, B, bias, gate)
            assert float((g["c"].cpu().double() - ref).abs().max()) < _gemm_bound(ref, k), (m, n, k)
            if epi == 2 and with_colsum:
                want = torch.stack([g["c"].cpu()[64 * t:64 * t + 64].double().sum(0) for t in range(tm)])
                assert float((g["colsum"].cpu().double() - want).abs().max()) < 1e-3
            if epi == 3:
                used = tm * ((n + wide - 1) // wide)
                u = gm.arena.unwritten(gm.outs["sqsum"])
                assert not u[:used].any() and u[used:].all()
                sq2 = float((g["c"].cpu().double() ** 2).sum())
                assert abs(float(g["sqsum"].cpu().double().sum()) - sq2) <= 1e-5 * max(1.0, sq2)


def test_wide_tiles_in_a_child_process():
    """BRL_GEMM_TILE_N is read once per process: the 64 x 64 tiles of brl_mlp_gemm run the same cases in a child process."""
    if _tile_n() == 64:
        pytest.skip("this process already runs the 64-wide tiles")
    envv = dict(os.environ, BRL_GEMM_TILE_N="64", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", "-m", "gpu", os.path.abspath(__file__),
                        "-k", "test_mlp_gemm_guarded"], cwd=ROOT, env=envv, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "6 passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def _group_tables(ts):
    vp, i64 = C.c_void_p * len(ts), C.c_int64 * len(ts)
    return vp(*[t.data_ptr() for t in ts]), i64(*[t.stride(0) for t in ts])


@pytest.mark.parametrize("layout", [0, 1, 2])
def test_mlp_gemm_group_guarded(layout):
    """brl_mlp_gemm_group: the three shapes and (TN) the heads' 39 rows out of a [k, 40] array in ONE launch, every pointer at
    exactly 16 bytes, every leading dimension padded: column 39 of that operand is read (whole 16-byte pieces) and is NaN here —
    it may only reach output rows that are never stored."""
    L, check = _lib()
    shapes = GEMM_SHAPES + ([(39, 36, 52)] if layout == 2 else [])
    ops = [_gemm_operands(layout, m, n, k, 77 + layout + m) for m, n, k in shapes]
    nn = len(shapes)
    i64 = C.c_int64 * nn

    def run(mem):
        As = [mem.inp(f"a{i}", o[0], F32, 16, ld=round_up(o[0].shape[1], 4) + 4, plain_ld=round_up(o[0].shape[1], 4)) for i, o in enumerate(ops)]
        Bs = [mem.inp(f"b{i}", o[1], F32, 16, ld=o[1].shape[1] + 4) for i, o in enumerate(ops)]
        Cs = [mem.out(f"c{i}", (m, n), F32, 16, ld=n + 4) for i, (m, n, k) in enumerate(shapes)]
        pa, lda = _group_tables(As)
        pb, ldb = _group_tables(Bs)
        pc, ldc = _group_tables(Cs)
        check(L.brl_mlp_gemm_group(0, layout, nn, pa, lda, pb, ldb, pc, ldc, i64(*[s[0] for s in shapes]), i64(*[s[1] for s in shapes]),
                                   i64(*[s[2] for s in shapes]), _s()))
        return {f"c{i}": c for i, c in enumerate(Cs)}
    _, g, _ = both(run)
    for i, ((m, n, k), o) in enumerate(zip(shapes, ops)):
        ref = _gemm_ref64(layout, 0, 0, *o)
        assert float((g[f"c{i}"].cpu().double() - ref).abs().max()) < _gemm_bound(ref, k), (m, n, k)


@pytest.mark.parametrize("layout,epi", [(0, 0), (0, 1), (1, 0), (1, 2), (2, 0)])
def test_mlp_gemm_x3_guarded(layout, epi):
    """brl_mlp_gemm_x3 at exactly 16 bytes (colsum too: its header says every pointer), ld + 4, without and with the split-K
    workspace: that one at exactly 256 bytes and exactly *bytes long — the bytes behind it are guard bytes, and every ticket is
    zero again afterwards."""
    L, check = _lib()
    for (m, n, k) in X3_SHAPES:
        need = C.c_int64(-1)
        check(L.brl_mlp_gemm_x3_workspace(m, n, k, C.byref(need)))
        tiles = ((m + 127) // 128) * ((n + 127) // 128)
        assert (need.value > 0) == (tiles < 256 and k >= 128) and need.value % 4 == 0
        for ws in ([False, True] if need.value else [False]):
            act = (m + ws) % 2
            A, B, bias, gate = _gemm_operands(layout, m, n, k, 2000 * layout + 10 * epi + m + n + k)
            tm = (m + 63) // 64

            def run(mem):
                a = mem.inp("a", A, F32, 16, ld=A.shape[1] + 4)
                b = mem.inp("b", B, F32, 16, ld=B.shape[1] + 4)
                bi = mem.inp("bias", bias, F32, 16) if epi == 1 else None
                ga = mem.inp("gate", gate, F32, 16, ld=n + 4) if epi == 2 else None
                c = mem.out("c", (m, n), F32, 16, ld=n + 4)
                cs = mem.out("colsum", (tm, n), F32, 16) if epi == 2 else None
                work = mem.inp("workspace", torch.zeros(need.value, dtype=U8), U8, 256, inout=True) if ws else None
                check(L.brl_mlp_gemm_x3(0, layout, epi, _p(a), a.stride(0), _p(b), b.stride(0), _p(c), c.stride(0), m, n, k, act, _p(bi),
                                        _p(ga), ga.stride(0) if ga is not None else 0, _p(cs), _p(work), need.value if ws else 0, _s()))
                out = {"c": c}
                if cs is not None:
                    out["colsum"] = cs
                if ws:
                    out["tickets"] = work[:tiles * 4]
                return out
            _, g, _ = both(run, capacity=1 << 23)
            ref = _gemm_ref64(layout, epi, act, A, B, bias, gate)
            assert float((g["c"].cpu().double() - ref).abs().max()) < _gemm_bound(ref, k), (m, n, k, ws)
            if ws:
                assert int(g["tickets"].cpu().to(I64).sum()) == 0
            if epi == 2:
                want = torch.stack([g["c"].cpu()[64 * t:64 * t + 64].double().sum(0) for t in range(tm)])
                assert float((g["colsum"].cpu().double() - want).abs().max()) < 1e-3


@pytest.mark.parametrize("layout", [0, 1, 2])
def test_mlp_gemm_x3_group_guarded(layout):
    L, check = _lib()
    ops = [_gemm_operands(layout, m, n, k, 177 + layout + m) for m, n, k in X3_SHAPES]
    i64 = C.c_int64 * 3

    def run(mem):
        As = [mem.inp(f"a{i}", o[0], F32, 16, ld=o[0].shape[1] + 4) for i, o in enumerate(ops)]
        Bs = [mem.inp(f"b{i}", o[1], F32, 16, ld=o[1].shape[1] + 4) for i, o in enumerate(ops)]
        Cs = [mem.out(f"c{i}", (m, n), F32, 16, ld=n + 4) for i, (m, n, k) in enumerate(X3_SHAPES)]
        (pa, lda), (pb, ldb), (pc, ldc) = _group_tables(As), _group_tables(Bs), _group_tables(Cs)
        check(L.brl_mlp_gemm_x3_group(0, layout, 3, pa, lda, pb, ldb, pc, ldc, i64(*[s[0] for s in X3_SHAPES]),
                                      i64(*[s[1] for s in X3_SHAPES]), i64(*[s[2] for s in X3_SHAPES]), _s()))
        return {f"c{i}": c for i, c in enumerate(Cs)}
    _, g, _ = both(run, capacity=1 << 23)
    for i, ((m, n, k), o) in enumerate(zip(X3_SHAPES, ops)):
        ref = _gemm_ref64(layout, 0, 0, *o)
        assert float((g[f"c{i}"].cpu().double() - ref).abs().max()) < _gemm_bound(ref, k), (m, n, k)


# ---- brl_split_planes, brl_linear_x3p ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 36])
def test_split_planes_guarded(n):
    """x at 16 bytes, planes at 8 (what the entry point asks for), plane_stride = n + 8: the three planes add up to x exactly."""
    L, check = _lib()
    x = _rand(torch.Generator().manual_seed(n), n)

    def run(mem):
        xs = mem.inp("x", x, F32, 16)
        pl = mem.out("planes", (3, n), BF16, 8, ld=n + 8)
        check(L.brl_split_planes(0, _p(xs), n, _p(pl), pl.stride(0), _s()))
        return {"planes": pl}
    _, g, _ = both(run)
    pl = g["planes"].cpu().float()
    assert torch.equal((pl[0] + pl[1]) + pl[2], x)


def _planes_of(x):
    """the three bf16 planes of a float tensor, by the library on dense tensors (test_linear_x3p_... checks that split)"""
    L, check = _lib()
    xd = x.to(DEV).contiguous()
    out = torch.empty((3,) + tuple(x.shape), dtype=BF16, device=DEV)
    check(L.brl_split_planes(0, xd.data_ptr(), xd.numel(), out.data_ptr(), xd.numel(), _s()))
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("m", [1, 129])
@pytest.mark.parametrize("k,npx", [(32, 1), (32, 3), (96, 1), (96, 3)])
def test_linear_x3p_guarded(m, k, npx):
    """brl_linear_x3p at exactly 16 bytes with ldx / ldw / ldy / ldyp = dense + 8 and every plane stride 8 beyond its plane:
    y only, planes only, both — the same bits each way, the planes add up to y, y within the exact kernel's bound of float64."""
    L, check = _lib()
    n = 128
    gen = torch.Generator().manual_seed(m + k + npx)
    x = (torch.rand((m, k), generator=gen) < 0.2).float() if npx == 1 else _rand(gen, m, k)
    w = _rand(gen, n, k) * 0.2
    bias = _rand(gen, n) * 0.5
    xp = x.to(BF16)[None] if npx == 1 else _planes_of(x)
    wp = _planes_of(w)
    ref = (x.double() @ w.double().t() + bias.double()).clamp_min(0)
    results = {}
    for with_y, with_p in ((True, False), (False, True), (True, True)):
        def run(mem):
            xs = mem.inp("x_planes", xp, BF16, 16, strides=(m * (k + 8) + 8, k + 8, 1))
            ws = mem.inp("w_planes", wp, BF16, 16, strides=(n * (k + 8) + 8, k + 8, 1))
            bi = mem.inp("bias", bias, F32, 16)
            y = mem.out("y", (m, n), F32, 16, ld=n + 8) if with_y else None
            yp = mem.out("y_planes", (3, m, n), BF16, 16, strides=(m * (n + 8) + 8, n + 8, 1)) if with_p else None
            check(L.brl_linear_x3p(0, _p(xs), npx, xs.stride(1), xs.stride(0), _p(ws), ws.stride(1), ws.stride(0), _p(bi), 1, _p(y),
                                   y.stride(0) if with_y else 0, _p(yp), yp.stride(1) if with_p else 0, yp.stride(0) if with_p else 0,
                                   m, n, k, _s()))
            return {name: t for name, t in (("y", y), ("y_planes", yp)) if t is not None}
        _, g, _ = both(run)
        results[(with_y, with_p)] = {name: t.cpu() for name, t in g.items()}
    y, yp = results[(True, True)]["y"], results[(True, True)]["y_planes"]
    assert torch.equal(results[(True, False)]["y"], y) and torch.equal(_bits(results[(False, True)]["y_planes"]), _bits(yp))
    assert torch.equal((yp[0].float() + yp[1].float()) + yp[2].float(), y)
    assert float((y.double() - ref).abs().max()) < _gemm_bound(ref, k)


# ---- brl_linear_act, brl_linear_act_heads --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,fmt", [(BF16, 1), (F16, 2)])
@pytest.mark.parametrize("m", [1, 65])
@pytest.mark.parametrize("n_out,k,hp_ld", [(128, 8, 40), (128, 480, 44), (256, 8, 44), (256, 480, 40)])
def test_linear16_guarded(env, dt, fmt, m, n_out, k, hp_ld):
    """brl_linear_act and brl_linear_act_heads at exactly 16 bytes, ldx / ldw / ldy / ld_head_w = dense + 8, head_part_ld 40 / 44
    with head_part_stride 4 floats beyond a part; the heads call with y and with y = NULL.  "Nothing beyond column k of x or w is
    used": that padding is NaN here.  The head_part columns [n_heads, round_up(n_heads, 4)) may be written, with zeros; nothing
    else may.  y against test_linear16_matches_float64_product's bound; the parts' sum against the float64 product of the
    rounded layer output with the head weights: fp32 accumulation of <= 256 products of 16-bit values whose sum of magnitudes is
    a few units — 2e-4 * max(1, max|ref|), test_heads_inside_the_launches_match_given_logits' bound at four times the depth."""
    L, check = _lib()
    n_heads = 39
    gen = torch.Generator().manual_seed(m + n_out + k + fmt)
    x = ((torch.rand((m, k), generator=gen) < 0.2).float() if k == 480 else _rand(gen, m, k)).to(dt)
    w = (torch.randn((n_out, k), generator=gen) / k ** 0.5).to(dt)
    bias = (torch.randn(n_out, generator=gen) * 0.1).to(dt).float()
    hw = (torch.randn((n_heads, n_out), generator=gen) / n_out ** 0.5 * 3).to(dt)
    nparts = n_out // 128
    eps = 2.0 ** (-8 if fmt == 1 else -11)
    for relu in (1, 0):
        ref = x.double() @ w.double().t() + bias.double()
        ref = ref.clamp_min(0) if relu else ref
        ys = {}
        for how in ("layer", "heads", "heads_no_y"):
            def run(mem):
                xs = mem.inp("x", x, dt, 16, ld=k + 8)
                ws = mem.inp("w", w, dt, 16, ld=k + 8)
                bi = mem.inp("bias", bias, F32, 16)
                y = mem.out("y", (m, n_out), dt, 16, ld=n_out + 8) if how != "heads_no_y" else None
                if how == "layer":
                    check(L.brl_linear_act(env._h, _p(xs), xs.stride(0), _p(ws), ws.stride(0), _p(bi), _p(y), y.stride(0), m, n_out, k,
                                           relu, fmt, _s()))
                    return {"y": y}
                hws = mem.inp("head_w", hw, dt, 16, ld=n_out + 8)
                hp = mem.out("head_part", (nparts, m, n_heads), F32, 16, strides=(m * hp_ld + 4, hp_ld, 1), plain_ld=40)
                check(L.brl_linear_act_heads(env._h, _p(xs), xs.stride(0), _p(ws), ws.stride(0), _p(bi), _p(y),
                                             y.stride(0) if y is not None else 0, m, n_out, k, relu, fmt, _p(hws), hws.stride(0), n_heads,
                                             _p(hp), hp.stride(1), hp.stride(0), _s()))
                return {"head_part": hp, **({"y": y} if y is not None else {})}
            _, g, _ = both(run, allowed={} if how == "layer" else {"head_part": (n_heads, round_up(n_heads, 4))})
            ys[how] = {name: t.cpu() for name, t in g.items()}
        y = ys["layer"]["y"]
        err = (y.double() - ref).abs()
        assert int((err > ref.abs() * eps + 1e-3).sum()) == 0, (relu, float(err.max()))
        assert torch.equal(_bits(ys["heads"]["y"]), _bits(y))
        assert torch.equal(ys["heads"]["head_part"], ys["heads_no_y"]["head_part"])
        want = y.double() @ hw.double().t()
        got = ys["heads"]["head_part"].double().sum(0)
        assert float((got - want).abs().max()) < 2e-4 * max(1.0, float(want.abs().max()))


# ---- brl_obs_cast, brl_obs_cast_rows, brl_live_index ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 33])
def test_obs_cast_and_live_index_guarded(env, n):
    """brl_obs_cast / brl_obs_cast_rows (16-byte pieces in and out: obs and out at exactly 16, rows at 8) in the three formats, and
    brl_live_index with `terminated` at 1 byte (its byte-wise path) and at 8 (its 8-flags-per-load path), live / finished at 8:
    the entries of `live` behind n - finished are left untouched."""
    L, check = _lib()
    obs = env.init(100 + n, num_envs=n).observation.cpu().to(U8)
    rows = torch.arange(n - 1, -1, -2, dtype=I64)     # every other board, descending
    m = rows.numel()
    for fmt, dt in ((0, F32), (1, BF16), (2, F16)):
        def run(mem):
            o = mem.inp("obs", obs, U8, 16)
            r = mem.inp("rows", rows, I64, 8)
            out = mem.out("out", (n, 480), dt, 16)
            out_r = mem.out("out_rows", (m, 480), dt, 16)
            check(L.brl_obs_cast(env._h, _p(o), n, _p(out), fmt, _s()))
            check(L.brl_obs_cast_rows(env._h, _p(o), _p(r), m, _p(out_r), fmt, _s()))
            return {"out": out, "out_rows": out_r}
        _, g, _ = both(run)
        assert torch.equal(g["out"].cpu(), obs.to(dt)) and torch.equal(g["out_rows"].cpu(), obs[rows].to(dt))
    for k, term in enumerate([torch.zeros(n, dtype=U8), torch.ones(n, dtype=U8), (torch.arange(n) % 3 == 1).to(U8)]):
        alive = int((term == 0).sum())
        for align in (1, 8):
            def run(mem):
                t = mem.inp("terminated", term, U8, align)
                live = mem.out("live", (n,), I64, 8)
                fin = mem.out("finished", (1,), I64, 8)
                fin2 = mem.out("finished_only", (1,), I64, 8)
                check(L.brl_live_index(env._h, _p(t), n, _p(live), _p(fin), -1, _s()))
                check(L.brl_live_index(env._h, _p(t), n, None, _p(fin2), -1, _s()))      # count only: no list anywhere
                return {"live": live[:alive], "finished": fin, "finished_only": fin2}
            _, g, gm = both(run, partial=("live",))
            assert int(g["finished"]) == n - alive == int(g["finished_only"])
            assert torch.equal(g["live"].cpu(), (term == 0).nonzero().squeeze(1))
            u = gm.arena.unwritten(gm.outs["live"])
            assert not u[:alive].any() and u[alive:].all(), (n, k, align)


# ---- brl_init_random, brl_step, brl_observe, brl_gae ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 33, 65])
def test_env_steps_guarded(env, n):
    """brl_init_random, brl_step, brl_observe at exactly what include/brl_hip.h states: states and observation rows (8-byte pieces per lane) at 8, mask
    and terminated (byte stores) at 1, rewards (one 16-byte store per table) at 16, int32 / float columns at 4.  Once with every
    optional output, once with every one NULL: then only state_out is written."""
    L, check = _lib()
    st = env.init(500 + n, num_envs=n)            # (seeds the handle's generator: the direct calls below deal the same boards)
    state0, mask0 = st.packed.cpu(), st.legal_action_mask.cpu()
    action = mask0.to(torch.float32).argmax(1).to(I32)          # the first legal call
    action[::4] = mask0.to(torch.float32).flip(1).argmax(1)[::4].to(I32).neg() + 37   # ... the last legal one on every fourth table
    player = (torch.arange(n) % 4).to(I32)

    def run(mem):
        s0 = mem.out("state", (n, 16), I64, 8)
        check(L.brl_init_random(env._h, _p(s0), n, 0, _s()))
        act = mem.inp("action", action, I32, 4)
        s1 = mem.out("state_out", (n, 16), I64, 8)
        obs, mask = mem.out("obs", (n, 480), U8, 8), mem.out("mask", (n, 38), U8, 1)
        rew, term, cur = mem.out("rewards", (n, 4), F32, 16), mem.out("terminated", (n,), U8, 1), mem.out("current_player", (n,), I32, 4)
        check(L.brl_step(env._h, _p(s0), _p(s1), n, _p(act), 1, _p(obs), _p(mask), _p(rew), _p(term), _p(cur), _s()))
        s2 = mem.out("state_out_only", (n, 16), I64, 8)
        check(L.brl_step(env._h, _p(s0), _p(s2), n, _p(act), 1, None, None, None, None, None, _s()))
        pid = mem.inp("player_id", player, I32, 4)
        obs2, mask2 = mem.out("obs_of", (n, 480), U8, 8), mem.out("mask_of", (n, 38), U8, 1)
        check(L.brl_observe(env._h, _p(s1), n, _p(pid), _p(obs2), _p(mask2), _s()))
        obs3, mask3 = mem.out("obs_only", (n, 480), U8, 8), mem.out("mask_only", (n, 38), U8, 1)
        check(L.brl_observe(env._h, _p(s1), n, None, _p(obs3), None, _s()))
        check(L.brl_observe(env._h, _p(s1), n, None, None, _p(mask3), _s()))
        return {"state": s0, "state_out": s1, "obs": obs, "mask": mask, "rewards": rew, "terminated": term, "current_player": cur,
                "state_out_only": s2, "obs_of": obs2, "mask_of": mask2, "obs_only": obs3, "mask_only": mask3}
    _, g, _ = both(run)
    assert torch.equal(g["state"].cpu(), state0) and torch.equal(g["state_out"], g["state_out_only"])
    assert torch.equal(g["obs"], g["obs_only"]) and torch.equal(g["mask"], g["mask_only"])
    assert int(g["mask"].sum()) > 0 and bool((g["current_player"] >= 0).all())


@pytest.mark.parametrize("n", [1, 3, 33, 65])
@pytest.mark.parametrize("T", [1, 7])
def test_gae_guarded(env, oracle, n, T):
    """brl_gae: float columns at exactly 4 bytes, done at 1; against the oracle's scan, bit for bit."""
    L, check = _lib()
    rng = np.random.default_rng(n * 10 + T)
    done = (rng.random((T, n)) < 0.3).astype(np.uint8)
    value, reward = rng.standard_normal((T, n)).astype(np.float32), rng.standard_normal((T, n)).astype(np.float32)
    last = rng.standard_normal(n).astype(np.float32)
    gamma, lam = 0.99, 0.9
    gl = float(np.float32(gamma * lam))

    def run(mem):
        d, v, r, lv = mem.inp("done", done, U8, 1), mem.inp("value", value, F32, 4), mem.inp("reward", reward, F32, 4), mem.inp("last_val", last, F32, 4)
        adv, tgt = mem.out("advantages", (T, n), F32, 4), mem.out("targets", (T, n), F32, 4)
        check(L.brl_gae(env._h, _p(d), _p(v), _p(r), _p(lv), gamma, gl, T, n, _p(adv), _p(tgt), _s()))
        return {"advantages": adv, "targets": tgt}
    _, g, _ = both(run)
    want_adv, want_tgt = oracle.gae(done, value, reward, last, gamma, lam)
    assert np.array_equal(g["advantages"].cpu().numpy(), want_adv) and np.array_equal(g["targets"].cpu().numpy(), want_tgt)


# ---- brl_sl_sample, brl_sl_replay, brl_sl_loss ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sl_set():
    from brl_amd import sl_data
    return sl_data.parse_trajectories(sl_teacher.random_file(300, 11))


@pytest.mark.parametrize("batch", [1, 5, 257])
def test_sl_guarded(sl_set, batch):
    """The supervised pre-trainer's three entry points: int64 arrays at exactly 8 bytes, int32 / float at 4, bytes at 1, the
    replayed observation (16-byte pieces) at 16; logits with row stride 40 and NaN in columns 38, 39; dlogits given and NULL.
    The sampler against its numpy restatement, the loss against float64 with test_loss_matches_float64's bounds."""
    L, check = _lib()
    ts = sl_set
    hands, offsets, calls = ts.hands.view(np.int64), ts.offsets.astype(np.int64), ts.calls.astype(np.uint8)
    rng = np.random.default_rng(batch)
    z = rng.normal(0, 4, (batch, 38)).astype(np.float32)
    start, seed, ent = 7 * ts.n + 3, 42, 0.01

    def run(mem):
        ctr = mem.inp("counter", np.array([start], np.int64), I64, 8, inout=True)
        off = mem.inp("offsets", offsets, I64, 8)
        traj, pos = mem.out("traj", (batch,), I64, 8), mem.out("pos", (batch,), I32, 4)
        check(L.brl_sl_sample(0, _p(ctr), _p(off), ts.n, seed, batch, _p(traj), _p(pos), _s()))
        hd, cl = mem.inp("hands", hands, I64, 8), mem.inp("calls", calls, U8, 1)
        obs, mask, label = mem.out("obs", (batch, 480), F32, 16), mem.out("mask", (batch, 38), U8, 1), mem.out("label", (batch,), I32, 4)
        check(L.brl_sl_replay(0, _p(hd), _p(off), _p(cl), ts.n, _p(traj), _p(pos), batch, _p(obs), _p(mask), _p(label), _s()))
        lg = mem.inp("logits", z, F32, 4, ld=40)
        dl, out, out2 = mem.out("dlogits", (batch, 38), F32, 4), mem.out("out", (5,), F32, 4), mem.out("out_metrics_only", (5,), F32, 4)
        check(L.brl_sl_loss(0, _p(lg), lg.stride(0), _p(label), _p(mask), batch, ent, _p(dl), _p(out), _p(ctr), batch, _s()))
        check(L.brl_sl_loss(0, _p(lg), lg.stride(0), _p(label), _p(mask), batch, ent, None, _p(out2), None, 0, _s()))
        return {"traj": traj, "pos": pos, "obs": obs, "mask": mask, "label": label, "dlogits": dl, "out": out,
                "out_metrics_only": out2, "counter": ctr}
    _, g, _ = both(run, capacity=1 << 21)
    t, p = sl_teacher.sample(ts.offsets, seed, start, batch)
    assert np.array_equal(g["traj"].cpu().numpy(), t) and np.array_equal(g["pos"].cpu().numpy(), p)
    assert int(g["counter"]) == start + batch and torch.equal(g["out"], g["out_metrics_only"])
    label, mask = g["label"].cpu().numpy(), g["mask"].cpu().numpy().astype(bool)
    assert np.array_equal(label, calls[offsets[t] + p].astype(np.int32))
    want, dwant = sl_teacher.loss64(z.astype(np.float64), label, mask, ent)
    assert np.allclose(g["out"].cpu().double().numpy(), want, rtol=1e-6, atol=1e-7)
    assert np.abs(g["dlogits"].cpu().double().numpy() - dwant).max() <= 1e-6 * np.abs(dwant).max()


# ---- brl_distill_targets, brl_distill_loss -------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["stride40", "heads"])
@pytest.mark.parametrize("B", [1, 65])
def test_distill_guarded(B, layout):
    """Policy distillation's two entry points, K = 2: logits in rows of 40 floats (NaN in columns 38, 39) or as the [K, n, 39]
    heads stack; floats at exactly 4 bytes, `work` at 8 and exactly 8 doubles per block of 64 rows; dz / du given and NULL.
    Against the float64 restatement within ``distill_ref.tolerance`` (test_kernels_match_float64's bound)."""
    L, check = _lib()
    K, tau, c_pol, c_val = 2, 2.0, 1.0, 0.5
    z, u, t, v, w, mask = distill_ref.inputs(B, K, seed=100 + B + K)
    nblocks = (B + 63) // 64

    def run(mem):
        if layout == "heads":
            th = mem.inp("teacher_heads", np.concatenate([t, v[:, :, None]], 2), F32, 4)
            sh = mem.inp("student_heads", np.concatenate([z, u[:, None]], 1), F32, 4)
            tl, ks, rs, tv, vks, vs = th, th.stride(0), th.stride(1), th[:, :, 38], th.stride(0), th.stride(1)
            zz, zs, uu, us = sh, sh.stride(0), sh[:, 38], sh.stride(0)
        else:
            tl = mem.inp("t_logits", t, F32, 4, strides=(B * 40 + 4, 40, 1), plain_ld=40)
            tv = mem.inp("t_values", v, F32, 4, ld=B + 1)
            zz, uu = mem.inp("z", z, F32, 4, ld=40, plain_ld=40), mem.inp("u", u[:, None], F32, 4, ld=2)
            ks, rs, vks, vs, zs, us = tl.stride(0), tl.stride(1), tv.stride(0), 1, zz.stride(0), uu.stride(0)
        wt, mk = mem.inp("weights", w, F32, 4), mem.inp("mask", mask.astype(np.uint8), U8, 1)
        q, vstar, hq = mem.out("q", (B, 38), F32, 4), mem.out("vstar", (B,), F32, 4), mem.out("hq", (B,), F32, 4)
        check(L.brl_distill_targets(0, _p(tl), ks, rs, _p(tv), vks, vs, _p(wt), _p(mk), B, K, tau, _p(q), _p(vstar), _p(hq), _s()))
        dz, du, out, out2 = mem.out("dz", (B, 38), F32, 4), mem.out("du", (B,), F32, 4), mem.out("out", (8,), F32, 4), mem.out("out_only", (8,), F32, 4)
        work = mem.out("work", (nblocks * 8,), torch.float64, 8)
        check(L.brl_distill_loss(0, _p(zz), zs, _p(uu), us, _p(q), _p(vstar), _p(hq), _p(mk), B, tau, c_pol, c_val, _p(dz), _p(du),
                                 _p(out), _p(work), _s()))
        check(L.brl_distill_loss(0, _p(zz), zs, _p(uu), us, _p(q), _p(vstar), _p(hq), _p(mk), B, tau, c_pol, c_val, None, None,
                                 _p(out2), _p(work), _s()))
        return {"q": q, "vstar": vstar, "hq": hq, "dz": dz, "du": du, "out": out, "out_only": out2}
    _, g, _ = both(run, partial=("work",))
    got = {name: x.cpu().numpy() for name, x in g.items()}
    assert np.array_equal(got["out"], got["out_only"]) and (got["dz"][~mask] == 0.0).all()
    want64 = distill_ref.restate(z, u, t, v, w.astype(np.float64), mask, tau, c_pol, c_val, np.float64)
    want32 = distill_ref.restate(z, u, t, v, w, mask, tau, c_pol, c_val, np.float32)
    for name in ("q", "vstar", "hq", "dz", "du"):
        err = float(np.abs(got[name].astype(np.float64) - want64[name]).max())
        assert err <= distill_ref.tolerance(want64[name], want32[name]), (name, err)
    for i, name in enumerate(distill_ref.METRICS):
        assert abs(float(got["out"][i]) - want64["metrics"][i]) <= distill_ref.tolerance(want64["metrics"][i], want32["metrics"][i]), name


# ---- brl_policy_step_ex --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 33])
@pytest.mark.parametrize("stride,obs_fmt", [(39, 0), (40, 1), (39, 2)])
def test_policy_step_ex_guarded(env, n, stride, obs_fmt):
    """One sampled sub-step with the macro-step block: logits as the first 38 columns of a [n, 39] / [n, 40] matrix whose column
    38 is the value (value_in at that stride; with 40, column 39 is NaN padding), obs_cast in each format, done_out / reward_out /
    value_out / terminated_count — once with every optional output, once with every one NULL (then only state_out is written).
    States and observation rows at exactly 8 bytes, rewards_acc and obs_cast (16-byte pieces) at exactly 16: what the header states."""
    from brl_amd import _capi
    L, check = _lib()
    st = env.init(900 + n, num_envs=n)
    state0, actor = st.packed.cpu(), st.current_player.cpu().to(I32)
    heads = _rand(torch.Generator().manual_seed(n + stride), n, 39) * 3
    dt = (F32, BF16, F16)[obs_fmt]

    def run(mem):
        s0 = mem.inp("state_in", state0, I64, 8)
        hd = mem.inp("heads", heads, F32, 4, ld=stride, plain_ld=stride)
        s1, s2 = mem.out("state_out", (n, 16), I64, 8), mem.out("state_out_only", (n, 16), I64, 8)
        action, logp = mem.out("action", (n,), I32, 4), mem.out("log_prob", (n,), F32, 4)
        obs, mask = mem.out("obs", (n, 480), U8, 8), mem.out("mask", (n, 38), U8, 1)
        racc, tacc, cur = mem.out("rewards_acc", (n, 4), F32, 16), mem.out("terminated_acc", (n,), U8, 1), mem.out("current_player", (n,), I32, 4)
        vout, dout, rout = mem.out("value_out", (n,), F32, 4), mem.out("done_out", (n,), U8, 1), mem.out("reward_out", (n,), F32, 4)
        cast = mem.out("obs_cast", (n, 480), dt, 16)
        act = mem.inp("actor", actor, I32, 4)
        count = mem.inp("terminated_count", np.array([5], np.int64), I64, 8, inout=True)
        ext = _capi.MacroExt(first=1, last=1, value_in=hd.data_ptr() + 38 * 4, value_stride=hd.stride(0), value_out=_p(vout),
                             done_out=_p(dout), reward_out=_p(rout), actor=_p(act), reward_scale=7600.0, obs_fmt=obs_fmt,
                             terminated_count=_p(count), obs_cast=_p(cast))
        check(L.brl_policy_step_ex(env._h, _p(s0), _p(s1), n, _p(hd), hd.stride(0), 0, None, 7, 1, _p(action), _p(logp), _p(obs), _p(mask),
                                   _p(racc), _p(tacc), _p(cur), C.byref(ext), _s()))
        check(L.brl_policy_step_ex(env._h, _p(s0), _p(s2), n, _p(hd), hd.stride(0), 0, None, 7, 1, None, None, None, None, None, None, None,
                                   C.byref(_capi.MacroExt()), _s()))
        return {"state_out": s1, "state_out_only": s2, "action": action, "log_prob": logp, "obs": obs, "mask": mask, "rewards_acc": racc,
                "terminated_acc": tacc, "current_player": cur, "value_out": vout, "done_out": dout, "reward_out": rout, "obs_cast": cast,
                "terminated_count": count}
    _, g, _ = both(run)
    assert torch.equal(g["state_out"], g["state_out_only"]) and torch.equal(g["value_out"].cpu(), heads[:, 38])
    assert torch.equal(g["obs_cast"].cpu(), g["obs"].cpu().to(dt)) and torch.equal(g["done_out"], g["terminated_acc"])
    assert int(g["terminated_count"]) == 5 + int(g["terminated_acc"].sum())
    a = g["action"].cpu().long()
    assert bool(st.legal_action_mask.cpu()[torch.arange(n), a].all())     # a legal call of the state it was sampled in


# ---- brl_rollout_random, brl_rollout_random_gae --------------------------------------------------------------------------------
@pytest.mark.parametrize("ws", [None, "0"])
@pytest.mark.parametrize("n,T", [(1, 1), (33, 5), (96, 9)])
def test_fused_rollouts_guarded(dds, oracle, ws, n, T):
    """brl_rollout_random (substeps 1 and 4) and brl_rollout_random_gae with every Transition column a placement of its own: done
    at exactly 4 bytes, state, every other column, last_obs / last_mask, advantages / targets at exactly 16.  n * 38 and n * 480 are
    no multiples of 16 at n = 1 and 33 (the last row's tail store); n = 96 takes the flag-synchronised kernel and the one-launch
    GAE, the others the two-launch form.  The substeps-1 columns against the oracle's rollout."""
    from brl_amd import _capi
    L, check = _lib()
    e = make_env(dds, 4, ws)
    seed, draw_base, gamma = 11, 3, 0.99
    gl = float(np.float32(gamma * 0.9))
    state0 = e.init(seed, num_envs=n).packed.cpu()
    last_val = torch.from_numpy(np.random.default_rng(n).standard_normal(n).astype(np.float32))
    cols = (("done", (T, n), U8, 4), ("action", (T, n), I32, 16), ("value", (T, n), F32, 16), ("reward", (T, n), F32, 16),
            ("log_prob", (T, n), F32, 16), ("obs", (T, n, 480), U8, 16), ("legal_action_mask", (T, n, 38), U8, 16))
    for substeps, gae in ((1, False), (4, False), (1, True)):
        def run(mem):
            st = mem.inp("state", state0, I64, 16, inout=True)
            count = mem.inp("terminated_count", np.zeros(1, np.int64), I64, 8, inout=True)
            p, out = _capi.TransitionPtrs(), {}
            for name, shape, dt, align in cols:
                out[name] = mem.out(name, shape, dt, align)
                setattr(p, name, out[name].data_ptr())
            lo, lm = mem.out("last_obs", (n, 480), U8, 16), mem.out("last_mask", (n, 38), U8, 16)
            if gae:
                lv = mem.inp("last_val", last_val, F32, 4)
                adv, tgt = mem.out("advantages", (T, n), F32, 16), mem.out("targets", (T, n), F32, 16)
                check(L.brl_rollout_random_gae(e._h, _p(st), n, T, draw_base, 7600.0, C.byref(p), _p(lo), _p(lm), _p(count), _p(lv), gamma,
                                               gl, _p(adv), _p(tgt), _s()))
                out.update(advantages=adv, targets=tgt)
            else:
                check(L.brl_rollout_random(e._h, _p(st), n, T, substeps, draw_base, 7600.0, C.byref(p), _p(lo), _p(lm), _p(count), _s()))
            out.update(state=st, terminated_count=count, last_obs=lo, last_mask=lm)
            return out
        _, g, _ = both(run, capacity=1 << 22)
        if substeps == 1:
            ref = oracle.init_random(n, seed=seed)
            want = oracle.rollout_random(ref, T, seed=seed, draw_base=draw_base)
            for name in ("obs", "legal_action_mask", "action", "done", "reward", "log_prob", "value"):
                assert np.array_equal(g[name].cpu().numpy(), want[name]), (name, substeps, gae)
            assert int(g["terminated_count"]) == want["terminated_count"]
            assert np.array_equal(g["last_obs"].cpu().numpy(), ref["observation"])
            if gae:
                wa, wt = oracle.gae(want["done"], want["value"], want["reward"], last_val.numpy(), gamma, 0.9)
                assert np.array_equal(g["advantages"].cpu().numpy(), wa) and np.array_equal(g["targets"].cpu().numpy(), wt)


# ---- brl_mlp_forward_rows ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden,nlayers,ldo", [(64, 1, 40), (64, 3, 44), (260, 1, 44), (260, 3, 40)])
def test_mlp_forward_rows_guarded(hidden, nlayers, ldo):
    """The evaluators' one-call forward for m = 5 rows chosen out of 9: weights, hidden biases and scratch at exactly 16 bytes
    (they feed brl_mlp_gemm's tile code), head biases at 4, observation rows (4-byte pieces) at 4, rows at 8, scratch exactly
    m * (480 + 2 * hidden) floats; out [9, 39] with row pitch 40 / 44: the rows not chosen and the columns >= 39 stay untouched.
    Against the float64 forward within test_mlp_forward_rows_matches_float64's bound."""
    from brl_amd import _capi
    from tests.nets import observations
    L, check = _lib()
    n, m = 9, 5
    gen = torch.Generator().manual_seed(hidden + nlayers)
    dims = [480] + [hidden] * nlayers
    body = [(torch.randn((dims[i + 1], dims[i]), generator=gen) / dims[i] ** 0.5, torch.randn(dims[i + 1], generator=gen) * 0.1)
            for i in range(nlayers)]
    actor = (torch.randn((38, hidden), generator=gen) / hidden ** 0.5, torch.randn(38, generator=gen) * 0.1)
    critic = (torch.randn((1, hidden), generator=gen) / hidden ** 0.5, torch.randn(1, generator=gen) * 0.1)
    net = raw_net(body, actor, critic, torch.relu)
    obs = observations(n, 3).to(U8)
    rows = torch.tensor([7, 2, 8, 0, 4], dtype=I64)

    def run(mem):
        r, keep = _capi.MlpRef(), []          # (keep: the struct holds addresses only, the tensors must outlive the call)
        r.nlayers, r.act, r.in_features, r.hidden = nlayers, 0, 480, hidden

        def param(name, values, align):
            keep.append(mem.inp(name, values, F32, align))
            return keep[-1].data_ptr()
        for i, (W, b) in enumerate(body):
            r.w[i], r.b[i] = param(f"w{i}", W, 16), param(f"b{i}", b, 16)
        r.actor_w, r.actor_b = param("actor_w", actor[0], 16), param("actor_b", actor[1], 4)
        r.critic_w, r.critic_b = param("critic_w", critic[0], 16), param("critic_b", critic[1], 4)
        ob, rw = mem.inp("obs", obs, U8, 4), mem.inp("rows", rows, I64, 8)
        scratch = mem.out("scratch", (m * (480 + 2 * hidden),), F32, 16)
        out = mem.out("out", (n, 39), F32, 4, ld=ldo, plain_ld=ldo)
        check(L.brl_mlp_forward_rows(0, C.byref(r), _p(ob), _p(rw), m, _p(scratch), scratch.numel(), _p(out), out.stride(0), _s()))
        torch.cuda.synchronize()
        return {"out": out[rows.to(out.device)]}
    _, g, gm = both(run, partial=("out", "scratch"))
    u = gm.arena.unwritten(gm.outs["out"])
    chosen = np.zeros(n, bool)
    chosen[rows.numpy()] = True
    assert not u[chosen].any() and u[~chosen].all()
    want = forward64(net, obs[rows].float())
    assert float((g["out"].cpu().double() - want).abs().max()) < 2e-4 * max(1.0, float(want[:, :38].abs().max()))
