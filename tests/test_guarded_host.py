"""tests/guarded.py on CPU tensors: plain numpy stores stand in for a kernel.  Each stray store — one byte in front of an output,
one behind it, one into a padding column — is caught with the array, row, column and byte offset named; a store into the padding
the header allows (brl_linear_act_heads' head_part columns [n_heads, round_up(n_heads, 4))) is accepted when it is 0.0f and caught
when it is anything else.  Also: `place` gives exactly the alignment asked for, input padding is NaN, and every `int brl_*(` of
include/*.h is in the ledger (COVERED or OPEN) — a new entry point cannot arrive without a decision."""
import glob
import os
import re

import numpy as np
import pytest
import torch

from tests import guarded
from tests.guarded import GUARD, Arena, GuardError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _raw(arena):
    """the arena's bytes as a writable numpy array (CPU arenas share memory with it)"""
    return arena.buf.numpy()


@pytest.mark.parametrize("align", [4, 8, 16, 256])
def test_place_gives_exactly_the_alignment_asked_for(align):
    a = Arena()
    dt = {4: torch.float32, 8: torch.int64, 16: torch.float32, 256: torch.uint8}[align]
    for shape in ((5,), (3, 7), (2, 3, 8)):
        v = a.place(shape, dt, align)
        assert v.data_ptr() % align == 0 and v.data_ptr() % (2 * align) == align
        assert v.shape == shape and v.is_contiguous()
    # at least GUARD bytes of arena in front of, between and behind the arrays
    ends = [0] + [r.off + r.extent for r in a.recs]
    for r, prev_end in zip(a.recs, ends):
        assert r.off - prev_end >= GUARD
    assert a.capacity - ends[-1] >= GUARD
    a.check()


def test_strides_padding_and_fills():
    a = Arena()
    x = a.place((3, 5), torch.float32, 16, ld=8, fill=np.arange(15, dtype=np.float32).reshape(3, 5), name="x")
    y = a.place((3, 5), torch.bfloat16, 16, ld=8, name="y")
    p = a.place((3, 2, 4), torch.int16, 8, strides=(24, 8, 1), name="planes")
    assert x.stride() == (8, 1) and y.stride() == (8, 1) and p.stride() == (24, 8, 1)
    assert torch.equal(x, torch.arange(15, dtype=torch.float32).reshape(3, 5))
    wide = torch.as_strided(x, (3, 8), (8, 1))
    assert bool(torch.isnan(wide[:, 5:]).all())               # an input's padding poisons arithmetic: fp32 ...
    xb = a.place((2, 3), torch.bfloat16, 16, ld=8, fill=torch.ones(2, 3), name="xb")
    xh = a.place((2, 3), torch.float16, 16, ld=8, fill=torch.ones(2, 3), name="xh")
    assert bool(torch.isnan(torch.as_strided(xb, (2, 8), (8, 1))[:, 3:].float()).all())    # ... bf16 ...
    assert bool(torch.isnan(torch.as_strided(xh, (2, 8), (8, 1))[:, 3:].float()).all())    # ... and fp16
    assert bool(torch.isnan(y.float()).all())                 # an output starts as NaNs no product of finite operands equals
    assert a.unwritten(y).all() and a.unwritten(p).all() and a.unwritten(p).shape == (3, 2, 4)
    i = a.place((4,), torch.int32, 4, name="i")
    assert bool((i < 0).all())                                # integers: negative (no action, index or count)
    y[1, 2] = 3.0
    u = a.unwritten(y)
    assert not u[1, 2] and u.sum() == 14
    with pytest.raises(GuardError, match=r"'y': 14 of 15 elements were never written, first \(0, 0\)"):
        a.assert_written(y)
    y.fill_(1.0)
    a.assert_written(y)
    a.check()
    # the pattern depends on the position: no single byte value fills a gap
    gap = a.expected[a.recs[0].off - 64:a.recs[0].off]
    assert len(set(gap.tolist())) > 16 and 0 not in gap


def test_stray_stores_are_caught_and_located():
    a = Arena()
    a.place((4, 4), torch.float32, 16, fill=torch.zeros(4, 4), name="a")
    c = a.place((3, 4), torch.float32, 16, ld=8, name="c")
    rc = a.rec(c)
    raw = _raw(a)
    c.copy_(torch.ones(3, 4))            # the kernel's legitimate stores
    a.check()

    def stray(off, match):
        old = raw[off]
        raw[off] ^= 0x10
        with pytest.raises(GuardError, match=match):
            a.check()
        raw[off] = old
        a.check()
    stray(rc.off - 1, r"1 byte\(s\) BEFORE array 'c' \(byte offset -1\)")
    stray(rc.off + rc.extent, r"1 byte\(s\) BEHIND array 'c'")
    # one element behind row 1's last column: what an edge tile that stores a full tile width does when ldc > n
    stray(rc.off + (1 * 8 + 4) * 4, r"array 'c' row 1 column 4 \(width 4, pitch 8; byte offset 48 from its start\)")
    stray(rc.off + (2 * 8 + 7) * 4 + 3, r"array 'c' row 2 column 7 .*byte offset 95")
    # a store of the very byte the pattern holds ELSEWHERE does not hide
    raw[rc.off - 2] = raw[rc.off - 3] if raw[rc.off - 3] != raw[rc.off - 2] else raw[rc.off - 4]
    with pytest.raises(GuardError, match=r"2 byte\(s\) BEFORE array 'c'"):
        a.check()


def test_a_store_into_an_input_is_caught_unless_it_is_inout():
    a = Arena()
    x = a.place((3, 4), torch.float32, 16, ld=8, fill=torch.ones(3, 4), name="x")
    st = a.place((2, 16), torch.int64, 8, fill=torch.zeros(2, 16, dtype=torch.int64), name="state", inout=True)
    st[1, 3] = 7                         # a state updated in place: its elements are the launch's to change
    a.check()
    x[2, 1] = 5.0
    with pytest.raises(GuardError, match=r"input element changed .*array 'x' row 2 column 1 \(width 4, pitch 8"):
        a.check()
    x[2, 1] = 1.0
    a.check()


def test_signalling_margins_show_an_add_of_zero():
    """an accumulator updated in place for one element too many: `x + 0.0` stores x's own bits on the pattern (nothing to see), and a
    quiet NaN on a signalling margin"""
    a = Arena()
    acc = a.place((3, 4), torch.float32, 16, fill=torch.zeros(3, 4), name="rewards_sum", inout=True)
    r = a.rec(acc)
    behind = a.buf[r.off + r.extent:r.off + r.extent + 16].view(torch.float32)      # "table 3" of a [3, 4] array
    behind += 0.0
    a.check()                                     # the pattern: the same bytes came back
    a.signalling_margins(acc)
    a.check()                                     # placing the margins changes nothing by itself
    assert bool(torch.isnan(behind).all())
    word = int(behind.view(torch.int32)[0]) | 0x00400000      # what an IEEE add returns for a signalling NaN: the same NaN, quiet
    behind.view(torch.int32)[0] = word
    with pytest.raises(GuardError, match=r"guard byte changed .*3 byte\(s\) BEHIND array 'rewards_sum'.*placed 0xa0, found 0xe0"):
        a.check()


def test_allowed_padding_takes_zeros_and_nothing_else():
    n_heads, ld = 39, 44
    a = Arena()
    hp = a.place((2, 5, n_heads), torch.float32, 16, strides=(5 * ld + 8, ld, 1), name="head_part")
    r = a.rec(hp)
    hp.fill_(0.5)
    wide = torch.as_strided(hp, (2, 5, ld), hp.stride())
    allowed = [(hp, n_heads, guarded.round_up(n_heads, 4))]
    a.check(allowed=allowed)                       # untouched padding passes
    wide[1, 3, 39] = 0.0                           # "the padding columns of a row may be written, with zeros"
    a.check(allowed=allowed)
    with pytest.raises(GuardError, match=r"array 'head_part'\[1\] row 3 column 39 \(width 39, pitch 44"):
        a.check()                                  # ... but only where the header says so
    wide[0, 0, 39] = 1.0                           # not a zero
    with pytest.raises(GuardError, match=r"array 'head_part'\[0\] row 0 column 39"):
        a.check(allowed=allowed)
    wide[0, 0, 39] = 0.0
    a.check(allowed=allowed)
    wide[0, 2, 40] = 0.0                           # column 40 is beyond round_up(n_heads, 4): not allowed, even as a zero
    with pytest.raises(GuardError, match=r"array 'head_part'\[0\] row 2 column 40 .*byte offset " + str((2 * ld + 40) * 4)):
        a.check(allowed=allowed)
    assert r.extent == 2 * (5 * ld + 8) * 4


def test_every_entry_point_is_in_the_ledger():
    names = []
    for path in sorted(glob.glob(os.path.join(ROOT, "include", "*.h"))):
        with open(path) as f:
            names += re.findall(r"^int (brl_\w+)\(", f.read(), flags=re.M)
    assert len(names) > 80 and len(set(names)) == len(names)
    both = set(guarded.COVERED) & set(guarded.OPEN)
    assert not both, f"in COVERED and in OPEN: {sorted(both)}"
    missing = [n for n in names if n not in guarded.COVERED and n not in guarded.OPEN]
    assert not missing, f"entry points without a memory-contract decision (tests/guarded.py COVERED / OPEN): {missing}"
    stale = [n for n in list(guarded.COVERED) + list(guarded.OPEN) if n not in names]
    assert not stale, f"ledger entries that are no entry points: {stale}"
    assert all(isinstance(v, str) and v for v in list(guarded.COVERED.values()) + list(guarded.OPEN.values()))
    # DESIGN.md's table names every one of them too
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        design = f.read()
    assert "## Memory contract" in design
    section = design[design.index("## Memory contract"):]
    absent = [n for n in names if f"`{n}`" not in section]
    assert not absent, f"DESIGN.md 'Memory contract' does not list: {absent}"
