"""CPU-side checks of the drop-in boundary: the C-ABI library loads and exports every symbol
that include/brl_hip.h declares; the host mirror keeps the reference's names; there is no
fallback path when the extension or the GPU is missing.  No compute calls (no GPU here)."""
import ctypes
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


def test_binding_argument_types_match_header(built_lib):
    """Every argument of every declaration in include/brl_hip.h against the ctypes argtypes: beyond the sixth integer argument
    the x86-64 ABI passes on the stack, where an `int` bound to an `int64_t` parameter reads 32 bits of garbage."""
    from brl_amd import _capi
    text = open(os.path.join(ROOT, "include", "brl_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    decls = re.findall(r"\b(?:int|const char \*|void)\s*(brl_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S)
    assert sorted(n for n, _ in decls) == header_symbols()
    scalar = {"int": 4, "int32_t": 4, "uint32_t": 4, "unsigned": 4, "int64_t": 8, "uint64_t": 8, "float": "f", "double": "d"}

    def c_kind(arg):
        if "*" in arg:
            return "ptr"
        words = arg.split()
        return scalar[" ".join(words[:-1]) if len(words) > 1 else words[0]]

    def py_kind(t):
        if t in (ctypes.c_float,):
            return "f"
        if t in (ctypes.c_double,):
            return "d"
        if t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer):
            return "ptr"
        return ctypes.sizeof(t)

    L = _capi.lib()
    for name, args in decls:
        want = [] if args.strip() in ("", "void") else [c_kind(a.strip()) for a in args.split(",")]
        got = [py_kind(t) for t in (getattr(L, name).argtypes or [])]
        assert want == got, f"{name}: header {want} != ctypes {got}"


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
