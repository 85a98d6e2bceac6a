"""CPU-side checks of the drop-in boundary: the C-ABI library loads and exports every symbol
that include/brl_hip.h declares; the host mirror keeps the reference's names; there is no
fallback path when the extension or the GPU is missing.  No compute calls (no GPU here)."""
import ctypes
import glob
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built_lib():
    from brl_amd import build
    return build.build()


def header_symbols():
    text = open(os.path.join(ROOT, "include", "brl_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(brl_[a-z0-9_]+)\s*\(", text)))


def test_header_declares_the_expected_entry_points():
    syms = header_symbols()
    for s in ("brl_create", "brl_destroy", "brl_init_random", "brl_init_from_deals", "brl_step", "brl_observe",
              "brl_rollout_random", "brl_policy_step", "brl_gae", "brl_imp_reward", "brl_duplicate_step",
              "brl_get_fields", "brl_set_lut", "brl_set_rng", "brl_last_error"):
        assert s in syms


def test_library_exports_every_declared_symbol(built_lib):
    lib = ctypes.CDLL(built_lib)
    for s in header_symbols():
        assert hasattr(lib, s), f"{s} declared in include/brl_hip.h but not exported"


def test_binding_covers_every_declared_symbol(built_lib):
    from brl_amd import _capi
    assert sorted(_capi.EXPORTS) == header_symbols()
    L = _capi.lib()
    assert L.brl_version() == 6   # include/brl_hip.h: the round the exported set last changed in
    assert L.brl_last_error() is not None


HEADERS = sorted(glob.glob(os.path.join(ROOT, "include", "*.h")))

# every `int brl_*(` entry point of every header, spelled out: a new one cannot arrive unnoticed (brl_hip.h's are _capi.EXPORTS, held
# against the header above)
ENTRY_POINTS = {
    "brl_belief.h": ["brl_belief_deal", "brl_belief_logp", "brl_belief_reduce"],
    "brl_belief_smc.h": ["brl_belief_accept", "brl_belief_propose", "brl_belief_resample"],
    "brl_boards.h": ["brl_board_imp", "brl_board_keep_a", "brl_board_records"],
    "brl_book.h": ["brl_book_reduce", "brl_book_samples"],
    "brl_compare.h": ["brl_compare_reduce", "brl_compare_rows", "brl_compare_tables"],
    "brl_crossplay.h": ["brl_xplay_route"],
    "brl_distill.h": ["brl_distill_loss", "brl_distill_targets"],
    "brl_league.h": ["brl_league_forward", "brl_league_route"],
    "brl_lines.h": ["brl_lines_expand", "brl_lines_finish", "brl_lines_imp", "brl_lines_init"],
    "brl_par.h": ["brl_par", "brl_par_imp"],
    "brl_positions.h": ["brl_position_answers", "brl_position_rows"],
    "brl_review.h": ["brl_review_expand", "brl_review_reduce"],
    "brl_sl.h": ["brl_sl_loss", "brl_sl_replay", "brl_sl_sample"],
}


def prototypes(path):
    """[(return type, name, [kind of every parameter])] of every brl_* prototype of a header; kind: "ptr", 4 / 8 (bytes of an
    integer), "f", "d".  A parameter type it does not know is a KeyError, not a guess."""
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    scalar = {"int": 4, "int32_t": 4, "uint32_t": 4, "unsigned": 4, "int64_t": 8, "uint64_t": 8, "float": "f", "double": "d"}

    def kind(arg):
        if "*" in arg:
            return "ptr"
        words = arg.split()
        return scalar[" ".join(words[:-1]) if len(words) > 1 else words[0]]
    decls = re.findall(r"\b(int|const char \*|void)\s*(brl_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S)
    return [(ret, name, [] if args.strip() in ("", "void") else [kind(a.strip()) for a in args.split(",")]) for ret, name, args in decls]


def test_the_headers_are_the_ones_the_table_names():
    from brl_amd import _capi
    assert [os.path.basename(p) for p in HEADERS] == sorted(_capi.SIGNATURES) == sorted(["brl_hip.h", *ENTRY_POINTS])


@pytest.mark.parametrize("header", [os.path.basename(p) for p in HEADERS])
def test_binding_argument_types_match_header(built_lib, header):
    """Every argument of every declaration of every header of include/ against the ctypes argtypes of _capi.SIGNATURES[header]:
    beyond the sixth integer argument the x86-64 ABI passes on the stack, where an `int` bound to an `int64_t` parameter reads
    32 bits of garbage.  The header's `int brl_*(` prototypes are the table's entry, name for name, and no other header's."""
    from brl_amd import _capi
    table = _capi.SIGNATURES[header]
    decls = prototypes(os.path.join(ROOT, "include", header))
    if header == "brl_hip.h":
        assert sorted(n for _, n, _ in decls) == header_symbols() == sorted(_capi.EXPORTS)
        assert [d for d in decls if d[0] != "int"] == [("const char *", "brl_last_error", [])]
    else:
        assert sorted(n for _, n, _ in decls) == ENTRY_POINTS[header] and all(ret == "int" for ret, _, _ in decls)
    assert sorted(n for ret, n, _ in decls if ret == "int") == sorted(table)
    for other, sigs in _capi.SIGNATURES.items():
        assert other == header or not set(sigs) & set(table), f"{sorted(set(sigs) & set(table))} under {header} and {other}"

    def py_kind(t):
        if t in (ctypes.c_float,):
            return "f"
        if t in (ctypes.c_double,):
            return "d"
        if t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer):
            return "ptr"
        return ctypes.sizeof(t)

    L = _capi.lib()
    for ret, name, want in decls:
        if ret == "int":
            assert want == [py_kind(t) for t in table[name]], f"{name}: header {want} != table"
            assert getattr(L, name).argtypes == table[name] and getattr(L, name).restype is ctypes.c_int, name
        assert want == [py_kind(t) for t in (getattr(L, name).argtypes or [])], f"{name}: header {want} != ctypes"


def test_struct_layouts_match_header():
    from brl_amd import _capi
    text = open(os.path.join(ROOT, "include", "brl_hip.h")).read()
    for cls, name in ((_capi.Fields, "brl_fields"), (_capi.TransitionPtrs, "brl_transition"),
                      (_capi.TableInfoPtrs, "brl_table_info")):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        members = re.findall(r"\*\s*([a-z_]+)\s*;", body)
        assert members == cls._names, name


def test_macro_ext_layout_matches_header():
    """brl_macro_ext mixes ints, floats and pointers: member order and C types against the ctypes mirror."""
    from brl_amd import _capi
    text = open(os.path.join(ROOT, "include", "brl_hip.h")).read()
    body = re.search(r"typedef struct brl_macro_ext \{(.*?)\} brl_macro_ext;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decl = re.findall(r"([A-Za-z_0-9 ]+?[ \*]+)([a-z_]+)\s*;", body)
    want = [(n, "ptr" if "*" in t else t.split()[-1]) for t, n in decl]
    kinds = {ctypes.c_int32: "int32_t", ctypes.c_int64: "int64_t", ctypes.c_float: "float", ctypes.c_void_p: "ptr"}
    got = [(n, kinds[t]) for n, t in _capi.MacroExt._fields_]
    assert got == want
    assert ctypes.sizeof(_capi.MacroExt) == 152   # 88 + the in-kernel heads (3 pointers, ldh, hidden, fmt) + the partial-product heads (pointer, stride, ld, nparts)


def test_bad_arguments_are_reported_not_crashed(built_lib):
    from brl_amd import _capi
    L = _capi.lib()
    assert L.brl_set_rng(None, 0, 0) == -1  # BRL_E_ARG
    assert b"handle" in L.brl_last_error()
    assert L.brl_destroy(None) == 0


def test_fp32_gemm_entry_points_refuse_misaligned_pointers(built_lib):
    """include/brl_hip.h: a / b / c / bias / gate of brl_mlp_gemm, brl_mlp_gemm_group and brl_mlp_gemm_dh_heads_dw 16-byte
    aligned (the tile code moves 16-byte pieces), colsum / sqsum 4-byte.  The argument checks come before anything touches a
    device, so a refusal needs none: the addresses here are made up, nothing reads them and nothing is launched."""
    from brl_amd import _capi
    L = _capi.lib()
    P = 0x7F0000000000      # "a pointer": 16-byte aligned, never dereferenced
    DEV = 1 << 20           # no such device: were a check missing, hipSetDevice would fail (BRL_E_HIP) before any launch; a refusal
                            # returns before the runtime is touched at all (no sticky HIP error is left for the next caller)

    def gemm(layout=0, epi=0, a=P, b=P, c=P, bias=None, gate=None, colsum=None, sqsum=None):
        return L.brl_mlp_gemm(DEV, layout, epi, a, 8, b, 8, c, 8, 8, 8, 8, 0, bias, gate, 8, colsum, sqsum, None)
    for kw, what in ((dict(a=P + 4), b"a / b / c"), (dict(b=P + 8), b"a / b / c"), (dict(c=P + 12), b"a / b / c"),
                     (dict(epi=1, bias=P + 4), b"bias / gate"), (dict(layout=1, epi=2, gate=P + 8), b"bias / gate"),
                     (dict(layout=1, epi=2, gate=P, colsum=P + 2), b"colsum / sqsum"),
                     (dict(layout=2, epi=3, sqsum=P + 1), b"colsum / sqsum")):
        assert gemm(**kw) == -1 and what in L.brl_last_error() and b"aligned" in L.brl_last_error(), kw
    vp, i64 = ctypes.c_void_p * 2, ctypes.c_int64 * 2
    eight = i64(8, 8)
    for bad in range(3):
        ptrs = [vp(P, P + 4) if j == bad else vp(P, P) for j in range(3)]
        assert L.brl_mlp_gemm_group(DEV, 2, 2, ptrs[0], eight, ptrs[1], eight, ptrs[2], eight, eight, eight, eight, None) == -1
        assert b"16-byte aligned" in L.brl_last_error()
    for bad in range(5):
        dz, w, out, gate, colsum = [P + (2 if j == 4 else 4) if j == bad else P for j in range(5)]
        assert L.brl_mlp_gemm_dh_heads_dw(DEV, dz, 256, w, 256, out, 256, 64, 256, 256, 0, gate, 256, colsum, P, P, 256, 64, 256, 1,
                                          P, P, None, None, 0, None, None, None, None) == -1
        assert b"16-byte aligned" in L.brl_last_error()


def test_handle_entry_points_refuse_misaligned_pointers_before_anything_else(built_lib):
    """brl_mlp_forward_rows (w[l] / b[l] at 16 bytes: brl_mlp_gemm's operands, refused before its first launch; obs at 4, rows at
    8), brl_obs_cast / _rows (obs and out at 16, rows at 8), brl_step / brl_observe / brl_policy_step_ex (obs at 8, rewards at 16,
    brl_macro_ext.obs_cast at 16): the alignment checks stand in front of the handle and device checks, so made-up addresses and
    no handle are enough to ask for them — nothing is read, nothing is launched."""
    from brl_amd import _capi
    L = _capi.lib()
    P, DEV = 0x7F0000000000, 1 << 20

    def refused(rc, what):
        assert rc == -1 and what in L.brl_last_error(), (rc, L.brl_last_error())
    for field, off, what in (("w", 4, b"w[l] / b[l]"), ("b", 8, b"w[l] / b[l]"), ("obs", 2, b"obs /"), ("rows", 4, b"rows: 8-byte"),
                             ("critic_b", 2, b"critic_b")):
        r = _capi.MlpRef()
        r.nlayers, r.act, r.in_features, r.hidden = 2, 0, 480, 64
        for l in range(2):
            r.w[l], r.b[l] = P, P
        r.actor_w = r.actor_b = r.critic_w = r.critic_b = P
        if field in ("w", "b"):
            getattr(r, field)[1] = P + off          # the SECOND layer: refused before the first one is launched
        elif field == "critic_b":
            r.critic_b = P + off
        obs, rows = (P + off if field == "obs" else P), (P + off if field == "rows" else P)
        refused(L.brl_mlp_forward_rows(DEV, ctypes.byref(r), obs, rows, 1, P, 1 << 20, P, 40, None), what)
    refused(L.brl_obs_cast(None, P + 8, 4, P, 0, None), b"obs / out not 16-byte aligned")
    refused(L.brl_obs_cast(None, P, 4, P + 8, 0, None), b"obs / out not 16-byte aligned")
    refused(L.brl_obs_cast_rows(None, P + 8, P, 4, P, 0, None), b"obs / out not 16-byte aligned")
    refused(L.brl_obs_cast_rows(None, P, P + 4, 4, P, 0, None), b"rows: 8-byte")
    step = lambda **k: L.brl_step(None, k.get("si", P), k.get("so", P), 4, k.get("act", P), 0, k.get("obs", P), P + 1,   # noqa: E731
                                  k.get("rew", P), P + 1, k.get("cur", P), None)
    for kw in (dict(si=P + 4), dict(so=P + 4), dict(act=P + 2), dict(obs=P + 4), dict(rew=P + 8), dict(cur=P + 2)):
        refused(step(**kw), b"rewards not 16-byte")
    assert step() == -1 and b"handle" in L.brl_last_error()      # aligned (mask and terminated at an odd address): on to the handle
    refused(L.brl_observe(None, P, 4, P, P + 4, P + 1, None), b"obs not 8-byte")
    refused(L.brl_observe(None, P + 4, 4, None, P, None, None), b"obs not 8-byte")
    pol = lambda ext=None, **k: L.brl_policy_step_ex(None, P, P, 4, P, 38, 0, None, 0, 0, P, P, k.get("obs", P), P + 1,   # noqa: E731
                                                     k.get("rew", P), P + 1, P, ext, None)
    refused(pol(obs=P + 4), b"obs not 8-byte")
    refused(pol(rew=P + 8), b"rewards not 16-byte")
    refused(pol(ctypes.byref(_capi.MacroExt(obs_cast=P + 8))), b"obs_cast not 16-byte aligned")
    refused(pol(ctypes.byref(_capi.MacroExt(obs_cast=P, terminated_count=P + 4))), b"terminated_count: 8-byte")
    assert pol(ctypes.byref(_capi.MacroExt(obs_cast=P))) == -1 and b"handle" in L.brl_last_error()


def test_match_entry_points_refuse_misaligned_pointers_before_anything_else(built_lib):
    """The entry points that play and record a match (tests/test_gpu_memory_contract_match.py runs them under the guards): what
    their kernels move in pieces wider than the element type — brl_table_info.rewards, rewards, rewards_sum, brl_fields.rewards,
    brl_imp_reward's out, brl_board_keep_a's tables at 16 bytes, brl_eval_reduce's bid_count at 8, brl_league_forward's obs at 4 —
    and every array's own element type: asked for with made-up addresses and no handle, so nothing is read and nothing launched."""
    from brl_amd import _capi
    L = _capi.lib()
    P = 0x7F0000000000

    def refused(rc, what):
        assert rc == -1 and what in L.brl_last_error(), (rc, L.brl_last_error())

    def table(**k):
        t = _capi.TableInfoPtrs()
        for name in _capi.TableInfoPtrs._names:
            setattr(t, name, k.get(name, P + 1 if name in ("terminated", "call_x", "call_xx") else P))
        return ctypes.byref(t)
    bad_tables = (dict(rewards=P + 4), dict(rewards=P + 8), dict(last_bid=P + 2), dict(last_bidder=P + 2))
    dup = lambda ta=None, tb=None, **k: L.brl_duplicate_step(None, k.get("si", P), k.get("so", P), 4, k.get("act", P), ta or table(),   # noqa: E731
                                                             tb or table(), k.get("obs", P), P + 1, k.get("rew", P), P + 1, k.get("cur", P), None)
    for kw in (dict(si=P + 4), dict(so=P + 4), dict(act=P + 2), dict(obs=P + 4), dict(rew=P + 4), dict(rew=P + 8), dict(cur=P + 2)):
        refused(dup(**kw), b"rewards not 16-byte")
    for bad in bad_tables:
        refused(dup(ta=table(**bad)), b"table_a / table_b: rewards not 16-byte")
        refused(dup(tb=table(**bad)), b"table_a / table_b: rewards not 16-byte")
    assert dup() == -1 and b"handle" in L.brl_last_error()

    def stats(**k):
        s = _capi.EvalStatsPtrs()
        for name in _capi.EvalStatsPtrs._names:
            setattr(s, name, k.get(name, P))
        return ctypes.byref(s)

    def ev(team, ta=None, tb=None, st=None, **k):
        tail = (ta or table(), tb or table(), st, 0, k.get("cum", P), k.get("rsum", P), k.get("aout", P), k.get("obs", P), P + 1,
                k.get("rew", P), P + 1, k.get("cur", P))
        if team:
            return L.brl_eval_step_team(None, k.get("si", P), k.get("so", P), 4, k.get("lg", P), 38, 0, *tail, k.get("f32", P), None)
        return L.brl_eval_step(None, k.get("si", P), k.get("so", P), 4, k.get("lg", P), 38, k.get("lg2", P), 38, *tail, None)
    for team in (False, True):
        for kw in (dict(si=P + 4), dict(so=P + 4), dict(obs=P + 4), dict(rew=P + 4), dict(cur=P + 2)):
            refused(ev(team, **kw), b"rewards not 16-byte")
        for bad in bad_tables:
            refused(ev(team, tb=table(**bad)), b"table_a / table_b: rewards not 16-byte")
        for kw in (dict(rsum=P + 4), dict(rsum=P + 8), dict(cum=P + 2), dict(aout=P + 2), dict(lg=P + 2)):
            refused(ev(team, **kw), b"rewards_sum not 16-byte aligned")
        for name in _capi.EvalStatsPtrs._names:
            refused(ev(team, st=stats(**{name: P + 2})), b"rewards_sum not 16-byte aligned")
        assert ev(team, st=stats()) == -1 and b"handle" in L.brl_last_error()
    refused(ev(False, lg2=P + 2), b"rewards_sum not 16-byte aligned")
    refused(ev(True, f32=P + 4), b"obs_f32 not 16-byte aligned")
    red = lambda ta=None, tb=None, **k: L.brl_eval_reduce(None, 4, ta or table(), tb, k.get("bc", P), k.get("st", P), k.get("out", P), None)   # noqa: E731
    for kw in (dict(bc=P + 4), dict(st=P + 4), dict(out=P + 4)):
        refused(red(**kw), b"bid_count / state / out not 8-byte aligned")
    refused(red(ta=table(rewards=P + 4)), b"table_a / table_b: rewards not 16-byte")
    refused(red(tb=table(rewards=P + 4)), b"table_a / table_b: rewards not 16-byte")
    assert red() == -1 and b"handle" in L.brl_last_error()
    for out in (P + 4, P + 8):
        refused(L.brl_imp_reward(None, P, P, out, 4, None), b"out not 16-byte aligned")
    refused(L.brl_imp_reward(None, P + 2, P, P, 4, None), b"out not 16-byte aligned")
    assert L.brl_imp_reward(None, P + 4, P + 4, P, 4, None) == -1 and b"handle" in L.brl_last_error()
    for name, off in (("rewards", 4), ("rewards", 8), ("hand", 2), ("board_ctr", 2)):
        f = _capi.Fields()
        setattr(f, name, P + off)
        refused(L.brl_get_fields(None, P, 4, ctypes.byref(f), None), b"rewards not 16-byte")
    refused(L.brl_get_fields(None, P + 4, 4, ctypes.byref(_capi.Fields()), None), b"state not 8-byte aligned")
    refused(L.brl_init_from_deals(None, P + 4, 4, P, P, P + 1, P + 1, P, P + 1, None), b"state not 8-byte aligned")
    refused(L.brl_init_from_deals(None, P, 4, P + 2, P, P + 1, P + 1, P, P + 1, None), b"state not 8-byte aligned")
    assert L.brl_init_from_deals(None, P, 4, P, P, P + 1, P + 1, P, P + 1, None) == -1 and b"handle" in L.brl_last_error()
    DEV = 1 << 20     # (no such device: an aligned call fails at hipSetDevice, behind every argument check)
    keep = lambda **k: L.brl_board_keep_a(DEV, k.get("st", P), k.get("prev", P), k.get("act", P), P + 1, P + 1, k.get("fin", P), 4, None)   # noqa: E731
    for kw in (dict(st=P + 8), dict(prev=P + 8), dict(fin=P + 8), dict(fin=P + 4), dict(act=P + 2)):
        refused(keep(**kw), b"state / prev / final_a 16-byte aligned")
    assert keep() == -2
    refused(L.brl_board_imp(DEV, P + 4, P, 4, P, None), b"records 8-byte aligned")
    refused(L.brl_board_imp(DEV, P, P, 4, P + 2, None), b"records 8-byte aligned")
    fwd = lambda **k: L.brl_league_forward(DEV, k.get("nets", P), 1, 1, 64, 0, k.get("obs", P), k.get("rows", P), k.get("gf", P), 1, P, 608,   # noqa: E731
                                           k.get("out", P), 40, None)
    for kw in (dict(obs=P + 2), dict(obs=P + 1), dict(rows=P + 4), dict(nets=P + 4), dict(gf=P + 2), dict(out=P + 2)):
        refused(fwd(**kw), b"obs / group_first / out not 4-byte aligned")
    assert fwd(obs=P + 4) == -2
    for fn in (L.brl_league_route, L.brl_xplay_route):
        route = lambda **k: fn(DEV, P + 1, k.get("cur", P), 0, 4, k.get("order", P), P, 2, 1, k.get("work", P), k.get("rows", P), k.get("gf", P), None)   # noqa: E731
        for kw in (dict(cur=P + 2), dict(order=P + 2), dict(work=P + 2), dict(rows=P + 4), dict(gf=P + 2)):
            refused(route(**kw), b"rows not 8-byte")
        assert route() == -2


def test_update_entry_points_refuse_misaligned_pointers_before_anything_else(built_lib):
    """The PPO step's entry points (include/brl_hip.h states the alignment of every pointer argument): each pointer in turn is
    moved to half its alignment — 16-byte ones to P + 8, 8-byte ones to P + 4, 4-byte ones to P + 2 — and the call must come back
    with BRL_E_ARG and a message that names the argument; the pointers inside brl_transition, brl_fair_net, brl_fair_work and the
    finalize segments' partials[i] / out[i] too.  The checks stand in front of everything else, so made-up addresses and a
    device that does not exist are enough: nothing is read, nothing is launched.  With every pointer aligned the same call gets
    past them (whatever stops it then does not speak of alignment)."""
    from brl_amd import _capi
    L = _capi.lib()
    P, DEV = 0x7F0000000000, 1 << 20
    vp2, i64x2 = ctypes.c_void_p * 2, ctypes.c_int64 * 2

    def ask(fn, args, needs):
        """needs: {index in args: (alignment, words of the refusal)}"""
        rc = getattr(L, fn)(*args)
        assert rc != 0 and b"aligned" not in L.brl_last_error(), (fn, rc, L.brl_last_error())
        for i, (align, what) in needs.items():
            bad = list(args)
            bad[i] = P + align // 2
            assert getattr(L, fn)(*bad) == -1, (fn, i)
            err = L.brl_last_error()
            assert what in err and b"aligned" in err, (fn, i, err)

    f4 = lambda idx, what: {i: (4, what) for i in idx}          # noqa: E731
    f16 = lambda idx, what: {i: (16, what) for i in idx}        # noqa: E731
    ask("brl_ppo_loss", [DEV, P, 40, P, P + 1, P, P, P, P, P, 5, 0.2, 0.5, 0.01, 1, 1, P, P, P, P, None],
        f4((1, 3, 5, 6, 7, 8, 9, 16, 17, 18, 19), b"logits / value"))
    ask("brl_ppo_stats", [DEV, P, 5, P, 0.5, 0.01, P, None], f4((1, 3, 6), b"partials / gram / out"))
    ask("brl_ppo_heads_loss_split", [DEV, P, 20, P, P, 16, P + 1, P, P, P, P, P, 5, 0.2, 0.5, 0.01, 1, 1, 0, P, P, P, P, P, 1, None],
        {**f16((1, 3), b"h / head_w"), **f4((4, 7, 8, 9, 10, 11, 19, 20, 21, 22, 23), b"head_b / action")})
    ask("brl_ppo_heads_bwd", [DEV, P, P, 260, P, 5, 256, 0, 1, P, P, P, P, P, P, 2, P, P, P, None],
        {**f16((2, 4, 11, 12), b"h / head_w / dh / tile_sums"), **f4((1, 9, 10, 13, 14, 16, 17, 18), b"dheads / dw_partials")})
    ask("brl_ppo_stats_gram", [DEV, P, 2, 5, P, 2, 0.5, 0.01, 0.0, P, P, P, None], f4((1, 4, 9, 10, 11), b"partials / gram_partials / out_rows"))
    ask("brl_ppo_illegal_grad", [DEV, P, P + 1, P, 0.1, 5, P, None], f4((1, 3, 6), b"heads / vec / dheads"))
    ask("brl_ppo_stats_rows", [DEV, P, P, 3, 5, 0.5, 0.01, 0.0, P, None], f4((1, 2, 8), b"stat_sums / gram_sums / out_rows"))
    ask("brl_act_bwd_colsum", [DEV, P, P, 5, 8, 12, 0, P, None], f16((1, 2, 7), b"dh / h / scratch"))
    ask("brl_act_bwd_colsum_heads_dw", [DEV, P, P, 5, 256, 260, 0, P, P, P, 260, 5, 256, 1, P, P, P, P, 2, P, P, P, None],
        {**f16((1, 2, 7, 9), b"dz / hh / scratch / h"), **f4((8, 14, 15, 16, 17, 19, 20, 21), b"dheads / dw_partials")})
    ask("brl_mlp_gemm_dh_heads_dw", [DEV, P, 256, P, 256, P, 256, 64, 256, 256, 0, P, 256, P, P, P, 256, 64, 256, 1, P, P, P, P, 16, P, P, P,
                                     None],
        {15: (16, b"h not 16-byte"), **f4((14, 20, 21, 22, 23, 25, 26, 27), b"dheads / dw_partials")})
    ask("brl_mb_gather_dev", [DEV, P, 5, None], {1: (8, b"args_dev")})

    # brl_mb_gather_bind: the trajectory's columns, then its own arguments
    def bind(tp, *rest):
        return L.brl_mb_gather_bind(DEV, ctypes.byref(tp), *rest)
    rest = [P, P, P, P, 5, P, P + 1, P, P, P, P, P, 2, P, None]
    for name in _capi.TransitionPtrs._names:
        tp = _capi.TransitionPtrs(**{n: P for n in _capi.TransitionPtrs._names})
        setattr(tp, name, P + (1 if name in ("legal_action_mask", "done") else 2))
        rc = bind(tp, *rest)
        if name in ("legal_action_mask", "done", "reward"):      # bytes, and two columns the gather does not read
            assert b"aligned" not in L.brl_last_error(), name
        else:
            assert rc == -1 and b"trajectory" in L.brl_last_error() and b"aligned" in L.brl_last_error(), name
    tp = _capi.TransitionPtrs(**{n: P for n in _capi.TransitionPtrs._names})
    for i, (align, what) in {**f4((0, 1, 3, 7, 8, 9, 10, 11), b"adv / targets / mb_index"), 2: (8, b"perm, args_dev"), 5: (16, b"x0"),
                             13: (8, b"perm, args_dev")}.items():
        bad = list(rest)
        bad[i] = P + align // 2
        assert bind(tp, *bad) == -1 and what in L.brl_last_error() and b"aligned" in L.brl_last_error(), i
    assert bind(tp, *rest) != 0 and b"aligned" not in L.brl_last_error()

    # the finalize segments: partials[i] / out[i] of the SECOND segment
    cols, tiles = i64x2(4, 4), i64x2(1, 1)
    for which in (0, 1):
        ptrs = [vp2(P, P + 2) if j == which else vp2(P, P) for j in range(2)]
        assert L.brl_bias_finalize_ex(DEV, 2, ptrs[0], cols, tiles, ptrs[1], None) == -1 and b"partials[i] / out[i]" in L.brl_last_error()
        assert L.brl_bias_finalize_rows(DEV, 2, ptrs[0], cols, tiles, ptrs[1], 1, P, None) == -1 and b"partials[i] / out[i]" in L.brl_last_error()
        assert L.brl_adam_clip_fin_gather(DEV, P, P, P, P, 8, P, 1e-3, P, 0.9, 0.999, 1e-8, 0.5, P, 2048, P, P, P, 5, 2, ptrs[0], cols,
                                          tiles, ptrs[1], None) == -1 and b"partials[i] / out[i]" in L.brl_last_error()
    ok = vp2(P, P)
    assert L.brl_bias_finalize_rows(DEV, 2, ok, cols, tiles, ok, 1, P + 2, None) == -1 and b"row_index" in L.brl_last_error()
    assert L.brl_bias_finalize_ex(DEV, 2, ok, cols, tiles, ok, None) != 0 and b"aligned" not in L.brl_last_error()
    assert L.brl_bias_finalize_rows(DEV, 2, ok, cols, tiles, ok, 1, P, None) != 0 and b"aligned" not in L.brl_last_error()
    ask("brl_adam_clip_fin_gather", [DEV, P, P, P, P, 8, P, 1e-3, P, 0.9, 0.999, 1e-8, 0.5, P, 2048, P, P, P, 5, 2, ok, cols, tiles, ok, None],
        {**f16((1, 2, 3, 4), b"p / g / m / v"), 17: (8, b"gather_args"), **f4((6, 8, 13, 15, 16), b"step / lr_dev / scratch")})
    geom = _capi.ShardGeom()
    geom.nbuckets, geom.world, geom.nsub = 1, 1, 1
    geom.off[0], geom.len[0] = 0, 8
    ask("brl_adam_shard_norm", [DEV, P, ctypes.byref(geom), 0, 1, 1.0, P, P, P, None],
        {1: (16, b"g not 16-byte"), **f4((6, 7, 8), b"partials, step, mb_index")})
    ask("brl_adam_shard_apply", [DEV, P, P, P, P, ctypes.byref(geom), 0, 1, P, P, 1e-3, P, 0.9, 0.999, 1e-8, 0.5, 1.0, P, P, 5, None],
        {**f16((1, 2, 3, 4), b"p / g / m / v"), 18: (8, b"gather_args"), **f4((8, 9, 11, 17), b"partials / step / lr_dev / norm_out")})

    # the FAIR entry points: the structures' pointers, then their own
    def fair_net(**k):
        net = _capi.FairNet()
        for l in range(11):
            net.w[l], net.b[l] = P, P
        net.head_w, net.head_b = k.get("head_w", P), k.get("head_b", P)
        if "w" in k:
            net.w[10] = k["w"]
        if "b" in k:
            net.b[10] = k["b"]
        return ctypes.byref(net)

    def fair_work(**k):
        return ctypes.byref(_capi.FairWork(**{n: k.get(n, P) for n in _capi.FairWork._names}))
    chain = lambda net=None, work=None, x0=P, cols=(P,) * 5: L.brl_fair_chain(   # noqa: E731
        DEV, net or fair_net(), x0, P + 1, *cols, 16, 0.2, 0.5, 0.01, 1, 1, 0, 0, work or fair_work(), None)
    fwd = lambda net=None, x=P, logits=P, value=P: L.brl_fair_forward(DEV, net or fair_net(), x, 3, 0, logits, value, None)   # noqa: E731
    for call in (chain, fwd):
        for kw in (dict(w=P + 8), dict(b=P + 8), dict(head_w=P + 8), dict(head_b=P + 2)):
            assert call(net=fair_net(**kw)) == -1 and b"net" in L.brl_last_error() and b"align" in L.brl_last_error(), kw
        assert call() != 0 and b"aligned" not in L.brl_last_error()
    for name in _capi.FairWork._names:
        assert chain(work=fair_work(**{name: P + 8})) == -1 and b"16-byte align" in L.brl_last_error(), name
    assert chain(x0=P + 8) == -1 and b"16-byte align" in L.brl_last_error()
    for i in range(5):
        assert chain(cols=tuple(P + 2 if j == i else P for j in range(5))) == -1 and b"action / old_value" in L.brl_last_error(), i
    assert fwd(x=P + 8) == -1 and b"x: 16-byte" in L.brl_last_error()
    assert fwd(logits=P + 2) == -1 and b"logits / value" in L.brl_last_error()
    assert fwd(value=P + 2) == -1 and b"logits / value" in L.brl_last_error()


def test_no_cpu_fallback_without_gpu():
    import torch
    import brl_amd
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(brl_amd._capi.BrlError):
        brl_amd.BridgeBidding(lut=None)


def test_missing_extension_fails_loudly(monkeypatch, tmp_path):
    from brl_amd import _capi
    monkeypatch.setattr(_capi, "_lib", None)
    monkeypatch.setattr(_capi, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(_capi.BrlError, match="no CPU fallback"):
        _capi.lib()


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "brl_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".h")):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, re.M), f
                assert "liboracle" not in src and "bridge_oracle" not in src, f


def test_host_mirror_keeps_reference_names():
    import brl_amd
    from brl_amd import duplicate, gae, models, roll_out, utils
    assert brl_amd.BridgeBidding.observation_shape == (480,)  # ppo.py:241
    for mod, names in ((utils, ["auto_reset", "single_play_step_two_policy_commpetitive",
                                "single_play_step_two_policy_commpetitive_deterministic",
                                "single_play_step_free_run", "normal_step"]),
                       (roll_out, ["Transition", "make_roll_out"]), (gae, ["make_calc_gae"]),
                       (duplicate, ["_imp_reward", "duplicate_init", "duplicate_step", "Table_info"]),
                       (models, ["ActorCritic", "make_forward_pass"])):
        for n in names:
            assert hasattr(mod, n), n
    assert roll_out.Transition._fields == ("done", "action", "value", "reward", "log_prob", "obs", "legal_action_mask")
    assert duplicate.Table_info._fields == ("terminated", "rewards", "last_bid", "last_bidder", "call_x", "call_xx")


def test_mlp_shapes_match_reference_model():
    import torch
    from brl_amd.models import make_forward_pass
    for model, nparams in (("DeepMind", 480 * 1024 + 1024 + 3 * (1024 * 1024 + 1024) + 1024 * 38 + 38 + 1024 + 1),
                           ("FAIR", None)):
        fp = make_forward_pass("relu", model)
        net = fp.init(0)
        logits, value = fp.apply(net, torch.zeros(5, 480))
        assert logits.shape == (5, 38) and value.shape == (5,)
        if nparams:
            assert sum(p.numel() for p in net.parameters()) == nparams == 3681319
