"""Guarded arrays for the memory-contract tests (DESIGN.md "Memory contract"): the part of a sanitizer's job that can be done
inside memory the process owns.

An ``Arena`` is ONE uint8 tensor.  Every array of a launch — inputs and outputs — is ``place``d inside it:
  * at EXACTLY the alignment asked for (``addr % (2 * align) == align``): a kernel that assumes more than its header states
    reads or writes the wrong bytes;
  * with the row pitch / strides asked for, so a leading dimension can be larger than dense;
  * with at least ``GUARD`` bytes of arena in front of and behind it, so a small overrun or a whole-piece over-read stays inside
    the allocation: nothing here depends on a fault.
Every byte that is not a logical element of a placed array is a GUARD byte: the gaps, and the padding columns between rows.
Guard bytes carry a position-dependent pattern (a kernel that stores the pattern's byte somewhere else is still seen); in the
padding of INPUT arrays they are 0xFF — NaN in fp32, bf16 and fp16 — so padding that is read into arithmetic poisons the result.
The logical elements of an OUTPUT start as a NaN / negative-integer variant of the pattern that no kernel result equals, so
``unwritten`` tells which elements a launch never stored.  ``check`` compares every guard byte with a host mirror and names the
nearest array, row, column and byte offset of the first difference.

Also here: ``Plain`` / ``Guarded`` / ``both`` — the two ways a GPU case gets its arrays, and the comparison of the two runs
(tests/test_gpu_memory_contract.py, tests/test_gpu_memory_contract_update.py and tests/test_gpu_memory_contract_match.py) — and the ledger of which C-ABI entry points run under these guards (``COVERED``) and which do not yet (``OPEN``);
tests/test_guarded_host.py holds every ``int brl_*(`` declaration of include/*.h against the two.
"""
from __future__ import annotations

import numpy as np
import torch

GUARD = 4096          # bytes of arena in front of and behind every placed array
_BASE_ALIGN = 512     # the arena's own base: every alignment up to 256 can be hit exactly


def pattern(lo: int, hi: int) -> np.ndarray:
    """the guard byte of arena offsets [lo, hi): position-dependent, never 0x00 (a stray zero store is seen everywhere)"""
    i = np.arange(lo, hi, dtype=np.int64)
    b = ((i * 37) ^ (i >> 8) * 101 ^ 0x5B) & 0xFF
    return np.where(b == 0, 0xA7, b).astype(np.uint8)


class GuardError(AssertionError):
    pass


class _Rec:
    __slots__ = ("name", "off", "shape", "strides", "itemsize", "dtype", "output", "extent", "view")


class Arena:
    def __init__(self, device="cpu", capacity=1 << 22):
        self.capacity = int(capacity)
        self._raw = torch.empty(self.capacity + _BASE_ALIGN, dtype=torch.uint8, device=device)
        skew = (-self._raw.data_ptr()) % _BASE_ALIGN
        self.buf = self._raw[skew:skew + self.capacity]
        self.base = self.buf.data_ptr()
        assert self.base % _BASE_ALIGN == 0
        self.expected = pattern(0, self.capacity)          # host mirror of every byte as placed
        self.logical = np.zeros(self.capacity, dtype=bool)  # bytes that belong to a logical element of a placed array
        self.readonly = np.zeros(self.capacity, dtype=bool)  # ... of an INPUT that no launch may change: checked like guard bytes
        self.buf.copy_(torch.from_numpy(self.expected))
        self.recs: list[_Rec] = []
        self._cursor = 0

    # ---- placing -------------------------------------------------------------------------------------------------------
    def place(self, shape, dtype, align, ld=None, fill=None, strides=None, name=None, inout=False):
        """A view of `shape` / `dtype` inside the arena whose address is `align`-byte aligned and NOT 2 * align aligned.
        ld: row pitch in elements (default dense); strides: all element strides (outer dimensions further apart than dense:
        plane strides, part strides).  fill: the values of an INPUT (anything torch.as_tensor takes; its padding becomes 0xFF);
        None: an OUTPUT (logical elements = the unwritten fill, padding = the position pattern).  An input's elements must still
        hold their values at `check` — unless it is `inout` (a state updated in place, a counter, a workspace)."""
        shape = tuple(int(s) for s in ((shape,) if isinstance(shape, int) else shape))
        assert len(shape) >= 1 and all(s > 0 for s in shape)
        itemsize = torch.empty((), dtype=dtype).element_size()
        assert align >= itemsize and align % itemsize == 0 and align & (align - 1) == 0 and 2 * align <= _BASE_ALIGN, align
        if strides is None:
            st = [1] * len(shape)
            for d in range(len(shape) - 2, -1, -1):
                st[d] = st[d + 1] * shape[d + 1]
                if d == len(shape) - 2 and ld is not None:
                    assert ld >= shape[-1]
                    st[d] = int(ld)
            strides = tuple(st)
        strides = tuple(int(s) for s in strides)
        assert len(strides) == len(shape) and strides[-1] == 1
        for d in range(len(shape) - 1):
            assert strides[d] >= strides[d + 1] * shape[d + 1], "strides must not overlap"
        extent = (shape[0] * strides[0] if len(shape) > 1 else shape[0]) * itemsize   # whole pitches: the last row's padding too
        off = self._cursor + GUARD
        off += (align - (self.base + off)) % (2 * align)
        assert (self.base + off) % (2 * align) == align
        assert off + extent + GUARD <= self.capacity, f"arena too small: {off + extent + GUARD} > {self.capacity}"
        self._cursor = off + extent

        r = _Rec()
        r.name, r.off, r.shape, r.strides, r.itemsize, r.dtype = name or f"array{len(self.recs)}", off, shape, strides, itemsize, dtype
        r.output, r.extent = fill is None, extent
        idx = self._byte_index(r)                       # [numel, itemsize] arena offsets of the logical elements' bytes
        if fill is None:
            b = self.expected[idx].copy()
            b[:, -1] = 0xFF                             # little-endian: the most significant byte
            if itemsize >= 2:
                b[:, -2] |= 0xC0                        # fp32 / bf16 / fp16: a NaN; integers: large and negative
            self.expected[idx] = b
        else:
            self.expected[off:off + extent] = 0xFF
            v = torch.empty(idx.shape[0], dtype=dtype)      # (a fresh dense copy: a one-element expand keeps stride 0)
            v.copy_(torch.as_tensor(fill).detach().to("cpu").to(dtype).expand(shape).reshape(-1))
            self.expected[idx] = v.view(torch.uint8).numpy().reshape(-1, itemsize)
        self.logical[idx] = True
        if fill is not None and not inout:
            self.readonly[idx] = True
        self.buf[off:off + extent].copy_(torch.from_numpy(self.expected[off:off + extent]))
        typed = self.buf[off:off + extent].view(dtype)
        r.view = torch.as_strided(typed, shape, strides)
        assert r.view.data_ptr() == self.base + off
        self.recs.append(r)
        return r.view

    @staticmethod
    def _elem_offsets(shape, strides):
        o = np.zeros((), dtype=np.int64)
        for n, s in zip(shape, strides):
            o = o[..., None] + np.arange(n, dtype=np.int64) * s
        return o

    def _byte_index(self, r, sel=None):
        e = self._elem_offsets(r.shape, r.strides)
        if sel is not None:
            e = e[sel]
        return r.off + e.reshape(-1, 1) * r.itemsize + np.arange(r.itemsize, dtype=np.int64)

    def rec(self, view) -> _Rec:
        p = view if isinstance(view, int) else view.data_ptr()
        for r in self.recs:
            if self.base + r.off == p:
                return r
        raise KeyError("not a placed array of this arena")

    def signalling_margins(self, view, nbytes=64):
        """The `nbytes` guard bytes in front of and behind a placed fp32 array become signalling NaNs (0x7FA0 over two pattern
        bytes).  For an accumulator updated in place: a read-modify-write that reaches one element too far and adds 0.0 stores the
        bytes it read — no guard byte changes — unless they are a signalling NaN, which the add returns quiet: other bits."""
        r = self.rec(view)
        assert r.itemsize == 4 and nbytes % 4 == 0 and 0 < nbytes <= GUARD // 2
        for lo in (r.off - nbytes, r.off + r.extent):
            w = self.expected[lo:lo + nbytes].reshape(-1, 4)
            w[:, 2], w[:, 3] = 0xA0, 0x7F
            self.buf[lo:lo + nbytes].copy_(torch.from_numpy(self.expected[lo:lo + nbytes]))

    # ---- checking ------------------------------------------------------------------------------------------------------
    def snapshot(self) -> np.ndarray:
        if self.buf.is_cuda:
            torch.cuda.synchronize(self.buf.device)
        return self.buf.cpu().numpy()

    def unwritten(self, view, cur=None) -> np.ndarray:
        """bool array of the view's logical shape: True where an element still holds the bytes it was placed with"""
        r = self.rec(view)
        cur = self.snapshot() if cur is None else cur
        idx = self._byte_index(r)
        return (cur[idx] == self.expected[idx]).all(axis=1).reshape(r.shape)

    def describe(self, i: int) -> str:
        """the placed array nearest to arena offset i, and where i lies relative to it"""
        def dist(r):
            return 0 if r.off <= i < r.off + r.extent else (r.off - i if i < r.off else i - (r.off + r.extent) + 1)
        r = min(self.recs, key=dist)
        rel = i - r.off
        if rel < 0:
            return f"{-rel} byte(s) BEFORE array '{r.name}' (byte offset {rel})"
        if rel >= r.extent:
            return f"{rel - r.extent + 1} byte(s) BEHIND array '{r.name}' (byte offset {rel} from its start, extent {r.extent})"
        e, pos = rel // r.itemsize, []
        for s in r.strides:
            pos.append(e // s)
            e -= pos[-1] * s
        outer = "".join(f"[{p}]" for p in pos[:-2])
        row, col = (pos[-2] if len(pos) > 1 else 0), pos[-1]
        return (f"array '{r.name}'{outer} row {row} column {col} (width {r.shape[-1]}, pitch "
                f"{r.strides[-2] if len(pos) > 1 else r.shape[-1]}; byte offset {rel} from its start)")

    def check(self, allowed=(), cur=None):
        """Every guard byte, and every element of an input that is not `inout`, is as placed.  allowed: (view, col_lo, col_hi) triples — columns [col_lo, col_hi) of every row of that
        array are padding the header lets the kernel write: each 4-byte word there holds exactly 0.0f or its pattern."""
        cur = self.snapshot() if cur is None else cur
        bad = (cur != self.expected) & (~self.logical | self.readonly)
        for view, lo, hi in allowed:
            r = self.rec(view)
            assert r.itemsize == 4 and r.shape[-1] <= lo <= hi <= r.strides[-2]
            if hi == lo:
                continue
            e = self._elem_offsets(r.shape[:-1], r.strides[:-1])[..., None] + np.arange(lo, hi, dtype=np.int64)
            idx = r.off + e.reshape(-1, 1) * 4 + np.arange(4, dtype=np.int64)
            ok = (cur[idx] == self.expected[idx]).all(axis=1) | (cur[idx] == 0).all(axis=1)
            bad[idx[ok]] = False
        if bad.any():
            i = int(np.argmax(bad))
            what = "input element" if self.readonly[i] else "guard byte"
            raise GuardError(f"{what} changed at arena offset {i}: {self.describe(i)}; placed 0x{self.expected[i]:02x}, "
                             f"found 0x{cur[i]:02x}; {int(bad.sum())} guarded byte(s) differ in all")
        return cur

    def assert_written(self, *views, cur=None):
        cur = self.snapshot() if cur is None else cur
        for v in views:
            u = self.unwritten(v, cur)
            if u.any():
                first = tuple(int(x) for x in np.argwhere(u)[0])
                raise GuardError(f"array '{self.rec(v).name}': {int(u.sum())} of {u.size} elements were never written, first {first}")


DEV = "cuda:0"     # the device of the GPU cases' Plain tensors and Guarded arenas


# ---- the two ways a case gets its arrays -------------------------------------------------------------------------------------
class Plain:
    """dense torch tensors: `ld` / `strides` are ignored, outputs start as zeros.  plain_ld: the row pitch where the dense one is not
    a legal leading dimension (39 columns of a [., 40] array)"""
    arena = None

    def inp(self, name, values, dtype, align, ld=None, strides=None, plain_ld=None, inout=False):
        v = torch.as_tensor(values).to(device=DEV, dtype=dtype).contiguous()
        if plain_ld is None:
            return v
        wide = torch.zeros(tuple(v.shape[:-1]) + (plain_ld,), dtype=dtype, device=DEV)
        wide[..., :v.shape[-1]] = v
        return wide[..., :v.shape[-1]]

    def out(self, name, shape, dtype, align, ld=None, strides=None, plain_ld=None):
        if plain_ld is None:
            return torch.zeros(shape, dtype=dtype, device=DEV)
        return torch.zeros(tuple(shape[:-1]) + (plain_ld,), dtype=dtype, device=DEV)[..., :shape[-1]]


class Guarded:
    def __init__(self, capacity=1 << 22):
        self.arena = Arena(DEV, capacity)
        self.outs = {}

    def inp(self, name, values, dtype, align, ld=None, strides=None, plain_ld=None, inout=False):
        """inout: the launch may change its elements (a state updated in place, a counter, a workspace); any other input must
        still hold its values afterwards"""
        v = torch.as_tensor(values)
        return self.arena.place(tuple(v.shape), dtype, align, ld=ld, strides=strides, fill=v, name=name, inout=inout)

    def out(self, name, shape, dtype, align, ld=None, strides=None, plain_ld=None):
        self.outs[name] = self.arena.place(shape, dtype, align, ld=ld, strides=strides, name=name)
        return self.outs[name]


def _bits(t):
    t = t.detach().contiguous().cpu()
    return t.reshape(-1).view(torch.uint8) if t.numel() else t.reshape(-1)


def both(run, capacity=1 << 22, allowed=(), partial=()):
    """run(mem) -> {name: tensor} on Plain and on Guarded memory: the same bits, no guard byte changed, every element of every
    output written (but those named in `partial`, which the caller checks itself).  allowed: names -> (col_lo, col_hi) of
    padding columns the header lets the kernel write.  -> (plain results, guarded results, Guarded)"""
    p = run(Plain())
    gm = Guarded(capacity)
    g = run(gm)
    cur = gm.arena.check(allowed=[(gm.outs[name], lo, hi) for name, (lo, hi) in dict(allowed).items()])
    assert set(p) == set(g)
    for name in p:
        assert p[name].shape == g[name].shape, name
        assert torch.equal(_bits(p[name]), _bits(g[name])), f"{name}: the guarded result differs from the plain one"
    gm.arena.assert_written(*[v for name, v in gm.outs.items() if name not in partial], cur=cur)
    return p, g, gm


def round_up(x: int, q: int) -> int:
    return (x + q - 1) // q * q


# ---- the ledger: every `int brl_*(` of include/*.h is in exactly one of the two ------------------------------------------------
# COVERED: entry point -> what tests/test_gpu_memory_contract.py (the PPO step's own entry points: tests/test_gpu_memory_contract_update.py;
# the entry points that play and record a match: tests/test_gpu_memory_contract_match.py) runs it on (alignments, strides, shapes)
COVERED = {
    "brl_mlp_gemm": "a / b / c / bias / gate at 16 bytes, colsum / sqsum at 4 and exactly sized; lda / ldb / ldc / ldg = dense + 4; NT, NN, TN x "
                    "every epilogue at (4,4,4), (68,36,52), (60,132,8); 64 x 32 tiles, and 64 x 64 in a child process (BRL_GEMM_TILE_N=64)",
    "brl_mlp_gemm_group": "the same three shapes + (TN) the 39-of-40 head product in one launch; 16 bytes, every ld + 4; 64 x 32 tiles only "
                          "(the 64 x 64 ones need > 256 tiles in one launch)",
    "brl_mlp_gemm_x3": "16 bytes (colsum too), ld + 4, (4,4,32), (132,132,160), (68,260,128), every layout and epilogue, without and with the "
                       "workspace (at 256 bytes, exactly *bytes long; tickets zero afterwards)",
    "brl_mlp_gemm_x3_workspace": "host only: its *bytes size the guarded workspace of brl_mlp_gemm_x3",
    "brl_mlp_gemm_x3_group": "the three x3 shapes in one launch per layout; 16 bytes, ld + 4",
    "brl_split_planes": "x at 16, planes at 8; n in {4, 36}; plane_stride = n + 8",
    "brl_linear_x3p": "16 bytes; m in {1, 129}, n = 128, k in {32, 96}, npx in {1, 3}; ldx / ldw / ldy / ldyp + 8, plane strides + 8; "
                      "y only, planes only, both",
    "brl_linear_act": "bf16 / fp16, 16 bytes, m in {1, 65}, n_out in {128, 256}, k in {8, 480}, ldx / ldw / ldy + 8, NaN beyond column k",
    "brl_linear_act_heads": "as brl_linear_act; ld_head_w + 8, head_part_ld in {40, 44}, head_part_stride + 4, y given and NULL; the columns "
                            "[39, 40) of head_part may hold 0.0",
    "brl_obs_cast": "n in {1, 3, 33}, three formats; obs and out at 16",
    "brl_obs_cast_rows": "every other row of n in {1, 3, 33}, three formats; obs and out at 16, rows at 8",
    "brl_live_index": "n in {1, 3, 33}; terminated at 1 and at 8 (its two load paths), live / finished at 8; entries behind n - finished untouched; "
                      "live = NULL",
    "brl_gae": "n in {1, 3, 33, 65} x T in {1, 7}; floats at 4, done at 1",
    "brl_init_random": "n in {1, 3, 33, 65}; state at 8",
    "brl_step": "n in {1, 3, 33, 65}; state at 8, obs at 8, mask / terminated at 1, rewards at 16, int32 columns at 4; every optional output "
                "given, and every one NULL",
    "brl_observe": "n in {1, 3, 33, 65}; player_id given and NULL; obs only, mask only, both",
    "brl_policy_step_ex": "n in {1, 3, 33}; state and obs at 8, rewards_acc at 16; logits_stride 39 / 40 (value_in at that stride, NaN in column 39), obs_cast in each format at 16, "
                          "done_out / reward_out / value_out / terminated_count; every optional output given, and every one NULL",
    "brl_rollout_random": "(n, T) in {(1,1), (33,5), (96,9)}, substeps 1 and 4, the default kernels and the K-tables-per-wave one; every "
                          "Transition column its own placement, done at 4, everything else at 16",
    "brl_rollout_random_gae": "the same shapes: one launch at (96,9), rollout + scan at the others; advantages / targets at 16, last_val at 4",
    "brl_mlp_forward_rows": "hidden in {64, 260}, nlayers in {1, 3}, 5 rows out of 9, ldo in {40, 44}; weights / hidden biases / scratch at 16, "
                            "head biases and obs at 4, rows at 8; scratch exactly m (480 + 2 hidden) floats",
    "brl_sl_sample": "batch in {1, 5, 257}; int64 at 8, pos at 4",
    "brl_sl_replay": "batch in {1, 5, 257}; obs at 16, mask at 1, label at 4",
    "brl_sl_loss": "batch in {1, 5, 257}; logits stride 40 with NaN padding; dlogits given and NULL; counter given and NULL",
    "brl_distill_targets": "B in {1, 65}, K = 2; rows of 40 floats (NaN padding, teachers 4 floats further apart than dense) and the [K, n, 39] "
                           "heads; floats at 4, mask at 1",
    "brl_distill_loss": "as brl_distill_targets; u at stride 2; work at 8, exactly 8 doubles per block of 64 rows; dz / du given and NULL",
    "brl_ppo_loss": "batch in {1, 5, 67}; logits_stride 38 / 40 (NaN in columns 38, 39); masked and unmasked; illegal_probs given and NULL; "
                    "partials exactly ceil(batch / 4) * 8 floats; floats / int32 at 4, mask at 1",
    "brl_ppo_stats": "on those partials; gram given and NULL; everything at 4",
    "brl_ppo_heads_loss_split": "hidden in {16, 272}, ldh = hidden + 4, batch in {1, 5, 67}, ksplit 1 and 8, head_parts exactly [ksplit, batch, 39]; "
                                "heads_out / gram_partials given and NULL; reward_scaling 0 and 1; h / head_w at 16, the rest at 4",
    "brl_ppo_stats_gram": "on the partials of brl_ppo_heads_loss_split; row_index NULL, and row 2 of 4 (the other rows untouched); vec_out given and NULL",
    "brl_ppo_stats_rows": "rows in {1, 3}; stat_sums / gram_sums / out_rows exactly sized, at 4",
    "brl_ppo_illegal_grad": "batch in {1, 5, 67}; dheads in/out, column 38 keeps its bits; everything at 4, mask at 1",
    "brl_ppo_heads_bwd": "hidden 256, ldh = 260, batch in {1, 17, 65}, nsplit = ceil(batch / 64) and one more; with the sums (row 2 of 4), without, "
                         "and dw_partials = db_partials = NULL; h / head_w / dh / tile_sums at 16, tile_sums exactly ceil(batch / 16) * 256",
    "brl_mb_gather_bind": "a trajectory of 12 rows, every brl_transition column its own placement (obs at 4), mbs in {1, 5}, *mb_index 0 and the "
                          "last; perm / args_dev (256 bytes) at 8, x0 at 16, the seven outputs exactly sized",
    "brl_mb_gather_dev": "as brl_mb_gather_bind: the launch that reads args_dev",
    "brl_act_bwd_colsum": "rows in {1, 17, 65} x cols in {4, 260}, ld = cols + 4 (NaN padding in dh and h), both activations; dh / h / scratch at 16, "
                          "scratch exactly ceil(rows / 16) * cols",
    "brl_act_bwd_colsum_heads_dw": "(rows, cols) in {(1,4), (17,260), (65,4), (65,260)} + the heads' dW role at hidden 256, batch in {17, 65}, nsplit "
                                   "ceil(batch / 64) and one more, with and without the sums; every output of the role exactly sized",
    "brl_bias_finalize_ex": "three segments in one launch, cols (39, 4, 260), tiles (1, 3, 5); partials exactly tiles * cols, at 4",
    "brl_bias_finalize_rows": "the same segments; first_row_seg in {0, 1, 3}, row_index = 2 of 4 rows (the other rows untouched)",
    "brl_adam_clip_fin_gather": "n in {8, 4100}; segments (4) and (4, 39 + 1 pad) tiling the end of g; scratch exactly 1024 + sum ceil(cols / 64); lr_dev / "
                                "norm_out / mb_index / gather_args (bound to the 12-row trajectory) given and NULL; max_norm 0.5 and 0; p / g / m / v at 16",
    "brl_adam_shard_norm": "world 2, two buckets 4 floats apart and 4 in front of the end, len in {4, 1028}, nsub in {1, 3}, ranks [0,1), [1,2), [0,2); "
                           "partials exactly world * nbuckets * nsub: only the range's rows written",
    "brl_adam_shard_apply": "the same geometry: gap, tail and the other ranks' slices keep their bits in p / m / v; g read only; p / g / m / v at 16",
    "brl_mlp_gemm_dh_heads_dw": "NN + GATE_COLSUM at (m, n, k) = (batch, 36, 52), every ld + 4, with the heads' dW role at hidden 256, batch in {17, 65}, "
                                "with and without the sums; dz / w / out / gate / h at 16",
    "brl_fair_forward": "rows in {1, 17}; x and the weights at 16, head_b / logits [rows, 38] / value [rows] at 4 and exactly sized",
    "brl_fair_chain": "batch in {16, 48}; every brl_fair_work array its own placement at 16, exactly the header's size; gram_partials given and NULL; "
                      "both activations",
    "brl_init_from_deals": "n in {1, 3, 33, 65}; int32 arrays at 4, uint8 at 1, state at 8; the deals of stepped env.init tables: the rebuilt state's "
                           "fields equal oracle.init_explicit's",
    "brl_get_fields": "n in {1, 3, 33, 65}; live, finished and illegally ended tables; state at 8, every brl_fields member its own placement: int32 at 4, "
                      "uint8 at 1, rewards at 16; every member given, and every one NULL but `turn`",
    "brl_imp_reward": "n in {1, 3, 33, 65}; a / b at 4, out at 16; scores with +-7600 and 0",
    "brl_duplicate_step": "n in {1, 3, 33}, eight scripted launches through both hand-overs; states at 8, both brl_table_info blocks in place with every member "
                          "its own placement (rewards at 16, int32 at 4, uint8 at 1), every launch's outputs placements of their own (obs at 8, rewards "
                          "at 16); every optional output given, and every one NULL",
    "brl_eval_step": "n in {1, 3, 33}, eight launches in place; logits at strides 38 and 40 (NaN in columns 38, 39); tables and brl_eval_stats members each "
                     "placed (rewards / rewards_sum at 16, the rest at 4 / 1); stats NULL, bid_count NULL, all given; bid_set 0 and 1; accumulators, "
                     "step outputs given and NULL; duplicate and single-table form",
    "brl_eval_step_team": "as brl_eval_step over eleven launches, acting_team alternating; obs_f32 at 16 and NULL; waiting boards keep the bits of state, "
                          "statistics and accumulators, action_out -1",
    "brl_eval_reduce": "n in {1, 3, 257}; tables read only (rewards at 16), bid_count at 8, state at 8, out int64 [231] at 8 and exactly sized; table_b, "
                       "bid_count and state each given and NULL",
    "brl_league_route": "(nmatch, n) in {(1,1), (3,5), (4,65)}, ngroups in {1, 3} (one group empty), team 0 and 1; terminated at 1, int32 at 4, rows at 8; "
                        "work exactly 2 nmatch, group_first exactly ngroups + 1; rows from R on untouched",
    "brl_xplay_route": "as brl_league_route; work exactly 4 nmatch (2 per slot)",
    "brl_league_forward": "hidden in {64, 260}, nlayers in {1, 3}, two networks (one with a single row), both activations; every weight / hidden bias at 16, "
                          "head biases at 4, the records at 8, obs at 4, rows at 8; scratch at 16, exactly rmax (480 + 2 hidden) floats, rmax = R and "
                          "R + 64; ldo in {40, 44}; unrouted rows of out untouched",
    "brl_board_records": "n in {1, 3, 65, 130}; state at 8, records at 16 and exactly n * 368 bytes; the 319-call auction, pass-outs, live, contract and "
                         "illegally ended tables",
    "brl_board_imp": "the same n; records at 16, out_imp at 4",
    "brl_board_keep_a": "n in {1, 3, 65}, behind five alternating launches of the scripted match; state / prev / final_a at 16, taken / a_done at 1, action at 4 "
                        "with -1 entries; final_a rows of boards whose table A has not ended untouched",
}

_NOT_YET = "not yet placed in an arena: "
# OPEN: entry point -> why it does not run under the guards (yet)
OPEN = {
    # host-only or no device arrays of the caller's
    "brl_version": "no pointer arguments",
    "brl_create": "host pointers only (the LUT is copied into memory the library owns)",
    "brl_set_lut": "host pointers only",
    "brl_destroy": "no arrays",
    "brl_set_rng": "no arrays",
}
for _n, _why in {
    "brl_policy_step": "brl_policy_step_ex with dense logits and no ext block (the same kernel, guarded there)",
    "brl_policy_step_at": "brl_policy_step_ex without the ext block (the same kernel, guarded there)",
    "brl_book_samples": "", "brl_book_reduce": "", "brl_par": "", "brl_par_imp": "", "brl_review_expand": "", "brl_review_reduce": "",
    "brl_belief_deal": "", "brl_belief_logp": "", "brl_belief_reduce": "", "brl_belief_resample": "", "brl_belief_propose": "",
    "brl_belief_accept": "", "brl_compare_tables": "", "brl_compare_rows": "", "brl_compare_reduce": "",
    "brl_lines_init": "", "brl_lines_expand": "", "brl_lines_finish": "", "brl_lines_imp": "",
}.items():
    OPEN[_n] = _NOT_YET + (_why or "compared with its reference on dense torch tensors only")
