"""CPU-only checks: the C-ABI library builds, loads and exports every symbol the header declares;
host-side logic (parameter table, state_dict names, synthetic generators, sharding, error paths).
No compute call is made: there is no GPU here."""
import json
import os
import re

import numpy as np
import pytest
import torch

from mmdeer import _lib, build, synth
from mmdeer.model import CompleteDEERModel, ModelConfig, MultimodalDEER, loss_dict_from
from mmdeer.parallel import shard_rows
from mmdeer.spec import gate_param_table, n_live_params, param_offsets, param_table

from . import gemm_route_table as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions():
    src = open(os.path.join(ROOT, "include", "mmdeer.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(mmdeer_[a-z0-9_]+)\s*\(", src)))


def test_library_builds_and_exports_every_declared_symbol():
    path = build.build()
    assert os.path.exists(path)
    lib = _lib.load()
    declared = header_functions()
    assert len(declared) >= 20
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/mmdeer.h but not exported"
    bound = {n for n, _, _ in _lib.SYMBOLS}
    assert bound == set(declared), (bound ^ set(declared))
    assert lib.mmdeer_abi_version() == _lib.ABI_VERSION == header_abi_version()
    assert b"gfx950" in lib.mmdeer_version()


def test_ctypes_struct_layouts_match_the_library():
    """Every argument struct of include/mmdeer.h is mirrored in mmdeer/_lib.py: the sizes the compiler gave them (mmdeer_sizeof) are
    the sizes ctypes computes -- a field added on one side only fails here (and at load time) instead of shifting pointers."""
    import ctypes as C
    lib = _lib.load()
    assert len(_lib.STRUCTS) >= 13
    for name, cls in _lib.STRUCTS.items():
        assert lib.mmdeer_sizeof(name.encode()) == C.sizeof(cls), name
    assert lib.mmdeer_sizeof(b"no_such_struct") == -1


def test_derived_struct_layouts_match_the_compiler(tmp_path):
    """Size of every struct and offset, size and kind (floating point, signed or unsigned integer, pointer, struct) of every
    field, as ctypes lays the derived classes out, asserted by the compiler that builds the library against include/mmdeer.h
    itself: two same-sized fields in the wrong order show in their offsets, an int32_t bound as a float in its kind."""
    import ctypes as C
    import subprocess

    def kind(t):
        while issubclass(t, C.Array):
            t = t._type_
        if issubclass(t, C.Structure):
            return "std::is_class<T>::value"
        if t in (C.c_float, C.c_double):
            return "std::is_floating_point<T>::value"
        if t in (C.c_int32, C.c_longlong, C.c_int64):
            return "std::is_integral<T>::value && std::is_signed<T>::value"
        if t in (C.c_uint64, C.c_size_t):
            return "std::is_integral<T>::value && std::is_unsigned<T>::value"
        assert t is C.c_void_p or issubclass(t, C._Pointer), t
        return "std::is_pointer<T>::value"

    lines = ["#include <stddef.h>", "#include <type_traits>", '#include "mmdeer.h"',
             "template <class F> using elem = typename std::remove_all_extents<F>::type;"]
    for cname, cls in _lib._CLASSES.items():
        lines.append(f'static_assert(sizeof({cname}) == {C.sizeof(cls)}, "sizeof {cname}");')
        for field, ftype in cls._fields_:
            d = getattr(cls, field)
            lines.append(f'namespace {cname}_{field} {{ using T = elem<decltype({cname}::{field})>; '
                         f'static_assert({kind(ftype)}, "kind of {cname}.{field}"); }}')
            lines.append(f'static_assert(offsetof({cname}, {field}) == {d.offset}, "offsetof {cname}.{field}");')
            lines.append(f'static_assert(sizeof((({cname}*)0)->{field}) == {d.size}, "sizeof {cname}.{field}");')
    assert len(_lib._CLASSES) == 20 and len(lines) > 3 * 441
    tu = tmp_path / "layout.cpp"
    tu.write_text("\n".join(lines) + "\n")
    r = subprocess.run([build._hipcc(), "-x", "c++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(tu)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


@pytest.mark.parametrize("extra,named", [
    ("typedef struct mmdeer_bad_args { int32_t n; mmdeer_widget w; } mmdeer_bad_args;", "mmdeer_widget"),
    ("int mmdeer_bad_call(const void* x, uint16_t flags, void* stream);", "uint16_t"),
    ("typedef int (*mmdeer_callback)(void* user);", "mmdeer_callback"),
    ("typedef int32_t mmdeer_handle;", "mmdeer_handle"),
    ("typedef struct mmdeer_bad_args { int32_t n : 3; } mmdeer_bad_args;", "n : 3"),
    ("#define MMDEER_BAD_SIZE (3 + 4)", "3 + 4"),
    ("#define MMDEER_ROUND_UP(x) (((x) + 3) / 4 * 4)", "MMDEER_ROUND_UP"),
    ("#define OTHER_LIMIT 7", "OTHER_LIMIT"),
    ("#if MMDEER_ABI_VERSION > 14\nint mmdeer_either(void);\n#else\nlong long mmdeer_either(void);\n#endif", "#if MMDEER_ABI_VERSION"),
], ids=["struct_base_type", "parameter_type", "typedef_function_pointer", "typedef_scalar", "bit_field", "define_expression",
        "function_like_macro", "define_without_prefix", "conditional_branch"])
def test_header_parser_refuses_what_it_cannot_account_for(extra, named):
    from mmdeer import _header
    text = _header.read()
    end = text.rindex("#ifdef __cplusplus")                     # inside the extern "C" block, where declarations live
    _header.parse(text, _lib._NAMES, _lib._TYPED_POINTERS)      # the header itself parses
    with pytest.raises(_header.HeaderError) as e:
        _header.parse(text[:end] + extra + "\n" + text[end:], dict(_lib._NAMES, mmdeer_bad_args="BadArgs"), _lib._TYPED_POINTERS)
    assert named in str(e.value)


def test_header_parser_maps_a_void_return_to_none():
    from mmdeer import _header
    text = _header.read()
    end = text.rindex("#ifdef __cplusplus")
    symbols = _header.parse(text[:end] + "void mmdeer_reset(void);\n" + text[end:], _lib._NAMES, _lib._TYPED_POINTERS)[2]
    assert symbols[-1] == ("mmdeer_reset", None, [])


def header_declarations():
    """(struct names, {function: parameter count}, {MMDEER_ constant: text}) by regular expressions of this test's own."""
    src = open(os.path.join(ROOT, "include", "mmdeer.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    structs = re.findall(r"typedef\s+struct\s*\w*\s*\{[^}]*\}\s*(\w+)\s*;", src)
    protos = {n: 0 if p.strip() == "void" else p.count(",") + 1 for n, p in re.findall(r"\b(mmdeer_\w+)\s*\(([^)]*)\)\s*;", src)}
    defines = dict(re.findall(r"#define\s+MMDEER_(\w+)[ \t]+(\S[^\n]*?)\s*$", src, flags=re.M))
    return structs, protos, defines


def header_abi_version():
    return int(header_declarations()[2]["ABI_VERSION"])


def test_binding_covers_the_whole_header():
    import ctypes as C
    structs, protos, defines = header_declarations()
    assert len(structs) == 20 and "mmdeer_loss_cfg" in structs and len(protos) == 109
    assert set(_lib._CLASSES) == set(structs)
    for cname, cls in _lib._CLASSES.items():                   # every struct has a class, under its name as an attribute of _lib
        assert issubclass(cls, C.Structure) and getattr(_lib, cls.__name__) is cls and _lib._NAMES[cname] == cls.__name__
    assert set(_lib.STRUCTS) == {s[len("mmdeer_"):] for s in structs} - {"loss_cfg"}
    assert all(_lib.STRUCTS[s[len("mmdeer_"):]] is _lib._CLASSES[s] for s in structs if s != "mmdeer_loss_cfg")
    assert {n: len(args) for n, _, args in _lib.SYMBOLS} == protos and len(_lib.SYMBOLS) == len(protos)
    for (cname, field), elem in _lib._TYPED_POINTERS.items():  # every override names an existing pointer field
        assert dict(_lib._CLASSES[cname]._fields_)[field] is C.POINTER(elem), (cname, field)
    assert set(_lib.CONSTANTS) == set(defines)
    assert _lib.CONSTANTS["CHAIN_MAX_SEGS"] == 12 == C.sizeof(_lib.ChainArgs().seg) // C.sizeof(_lib.ChainSeg)
    assert (_lib.TEMPORAL_POOL_SCRATCH, _lib.TOKEN_POOL_SCRATCH, _lib.LOSS_OUT, _lib.UNC_TABLE, _lib.COMM_ID_BYTES) == \
        (256 * 256, 1024 * 384, 20, 40, 128)
    from mmdeer import _header
    with pytest.raises(_header.HeaderError, match="does not exist"):     # ... and an override of a field the header does not have is refused
        _header.parse(_header.read(), _lib._NAMES, {**_lib._TYPED_POINTERS, ("mmdeer_gemm_args", "nope"): C.c_float})
    with pytest.raises(_header.HeaderError, match="does not match"):     # as is one whose element type is not the header's
        _header.parse(_header.read(), _lib._NAMES, {**_lib._TYPED_POINTERS, ("mmdeer_adamw_args", "lr"): C.c_double})


def test_gemm_args_defaults():
    import ctypes as C
    a = _lib.gemm_args()
    assert isinstance(a, _lib.GemmArgs)
    neutral = {"tile": -1, "drop_site": -1, "regen_site": -1, "mask_scale": 1.0}
    for field, _ in _lib.GemmArgs._fields_:
        assert getattr(a, field) == neutral.get(field, 0) or (field not in neutral and getattr(a, field) is None), field
    b = _lib.gemm_args(A=4096, M=3, tile=2, mask_scale=0.5, drop_site=7, seed=2 ** 40, bias=None)
    assert (b.A, b.M, b.tile, b.mask_scale, b.drop_site, b.seed, b.bias, b.regen_site, b.N) == (4096, 3, 2, 0.5, 7, 2 ** 40, None, -1, 0)
    with pytest.raises(TypeError, match="no_such_field"):
        _lib.gemm_args(M=3, no_such_field=1)
    assert C.sizeof(a) == _lib.load().mmdeer_sizeof(b"gemm_args")


def _route_args(s):
    """The argument struct of a gemm_route_table spec over plausible, aligned buffer addresses: the dry run dereferences none."""
    mb = 1 << 24
    return G.Layout(s).args(s, A=1 * mb, W=2 * mb, C=3 * mb, bias=4 * mb, bias_grad=5 * mb, Y=6 * mb, slab=7 * mb)


def _route_of(s):
    rc, lines = G.dry_run(_route_args(s))
    return rc, [G.without_tiles(x) for x in lines], _lib.load().mmdeer_last_error().decode()


@pytest.mark.parametrize("route", sorted(G.ROUTES))
def test_gemm_route_names_the_kernel_of_every_route(route):
    """mmdeer_gemm_route (no GPU: everything mmdeer_gemm does before its first launch) answers, for every shape and epilogue of the
    route under the route's own options, the one line the table states by hand; M = 0 is no launch."""
    with _lib.options(**G.ROUTES[route].get("opts", {})):
        for s, i, ename in G.route_cases(route):
            assert _route_of(s)[:2] == (1, [G.route_line(route, i, ename)]), (route, s["M"], s["N"], s["K"], ename, _route_of(s))
            assert _route_of(dict(s, M=0))[:2] == (0, []), (route, ename)
    rc, lines = G.dry_run(_route_args(G.spec("glds_128x64_8w", 1031, 196, 64)))
    assert (rc, lines) == (1, ["nt_glds 128x64 w8 a=v16 b=v16 tiles=36"])         # tiles= counts the workgroups: 9 x 4


@pytest.mark.parametrize("plan", G.PLANS, ids=lambda d: "-".join(f"{k}{v}" for k, v in d.items()))
def test_gemm_route_under_every_launch_plan(plan):
    with _lib.options(**plan):
        for route in G.PLAN_ROUTES:
            for s, i, ename in G.plan_cases(route):
                assert _route_of(s)[:2] == (1, [G.plan_route_line(plan, route, i, s)]), (plan, route, s["M"], s["N"], s["K"], ename, _route_of(s))


def test_gemm_route_refuses_what_the_call_refuses():
    import ctypes as C
    for name in sorted(G.REFUSALS):
        s, post, words = G.refusal_spec(name)
        a = _route_args(s)
        if post:
            post(a)
        out = C.create_string_buffer(64)
        assert _lib.load().mmdeer_gemm_route(C.byref(a), out, len(out)) == -1, f"{name}: accepted"
        assert words in _lib.load().mmdeer_last_error().decode(), (name, _lib.load().mmdeer_last_error())
    for name, (route, kw) in sorted(G.UNSPLITTABLE.items()):      # a split request the fold cannot take: accepted, and runs unsplit
        for sk in (3, 8):
            s = G.spec(route, splitk=sk, bias_grad=1, **kw)
            rc, lines = G.dry_run(_route_args(s))
            assert rc == 1 and G.without_tiles(lines[0]) == G.route_line(route), (name, sk, lines)
            assert lines == G.dry_run(_route_args(dict(s, splitk=1)))[1], (name, sk, lines)
    assert _lib.load().mmdeer_gemm_route(None, None, 0) == -1 and b"NULL" in _lib.load().mmdeer_last_error()
    a = _route_args(G.spec("nt_f32_t0", 64, 68, 64))
    assert _lib.load().mmdeer_gemm_route(C.byref(a), None, 0) == 1               # the count alone
    out = C.create_string_buffer(8)
    assert _lib.load().mmdeer_gemm_route(C.byref(a), out, len(out)) == 1 and out.value == b"nt_reg "   # truncated, NUL-terminated


def test_layer_chain_operator_validates_its_table_on_the_host():
    """mmdeer_chain checks the whole segment table before it launches anything (no GPU is touched here: every case below is refused,
    or empty): unsupported widths, panels that do not fit, residual / stash options where they do not apply."""
    import ctypes as C
    lib = _lib.load()
    A = 1 << 20                                     # a plausible, aligned address: never dereferenced by the host checks
    a = _lib.ChainArgs()
    a.X, a.ldx, a.K0, a.rows, a.nseg = A, 256, 256, 0, 1
    assert lib.mmdeer_chain(C.byref(a)) == 0        # an empty batch is nothing to do
    a.rows, a.nseg = 64, 0
    assert lib.mmdeer_chain(C.byref(a)) != 0 and b"segments" in lib.mmdeer_last_error()
    a.nseg = 1
    s = a.seg[0]
    s.W, s.N, s.K, s.end_layer, s.nout, s.drop_site = A, 256, 320, 1, 256, -1
    assert lib.mmdeer_chain(C.byref(a)) != 0        # K = 320 reads past the 256-wide input panel
    s.K, s.N, s.nout = 256, 96, 96
    assert lib.mmdeer_chain(C.byref(a)) != 0        # N % 64
    s.N, s.nout, s.W = 256, 256, A + 2
    assert lib.mmdeer_chain(C.byref(a)) != 0        # misaligned weight image
    s.W, s.res_add = A, 1
    assert lib.mmdeer_chain(C.byref(a)) != 0 and b"bypass" in lib.mmdeer_last_error()
    s.res_add, s.stash, s.ld_stash, s.stash_split = 0, A, 256, 128
    assert lib.mmdeer_chain(C.byref(a)) != 0        # a split without the second tensor
    s.stash_split, a.samples_per_workgroup = 0, 24
    assert lib.mmdeer_chain(C.byref(a)) != 0 and b"samples_per_workgroup" in lib.mmdeer_last_error()
    a.samples_per_workgroup, a.K0 = 32, 768
    assert lib.mmdeer_chain(C.byref(a)) != 0        # a 768-wide input needs the 16-sample workgroups
    assert lib.mmdeer_chain_workgroups(4096, 0) == 256 and lib.mmdeer_chain_workgroups(4097, 0) == 129 and lib.mmdeer_chain_workgroups(100, 16) == 7
    j = (_lib.RepackJob * 1)()
    j[0].src, j[0].dst, j[0].ld_src, j[0].rows, j[0].cols, j[0].cols_valid, j[0].layout = A, A, 100, 100, 100, 100, 1
    assert lib.mmdeer_repack(j, 1, None) != 0       # a fragment-major image needs rows % 16 == 0 and columns % 64 == 0
    assert lib.mmdeer_repack(j, 0, None) == 0


def _chain_refusal(mutate):
    """A one-layer chain table (every pointer a plausible aligned address that the host checks never dereference) changed by
    `mutate`; returns mmdeer_chain's return code and message."""
    import ctypes as C
    lib = _lib.load()
    A = 1 << 20
    a = _lib.ChainArgs()
    a.X, a.ldx, a.K0, a.rows, a.nseg = A, 256, 256, 64, 1
    s = a.seg[0]
    s.W, s.N, s.K, s.end_layer, s.nout, s.drop_site, s.mask_scale = A, 256, 256, 1, 256, -1, 1.0
    mutate(a, A)
    rc = lib.mmdeer_chain(C.byref(a))
    return rc, lib.mmdeer_last_error().decode()


def _ln(s, A):
    s.gamma, s.beta, s.xln, s.mean, s.rstd = A, A, A, A, A


def _lnb(s, A):
    s.lnb_gamma, s.lnb_y, s.lnb_mean, s.lnb_rstd, s.lnb_dz, s.lnb_partial = A, A, A, A, A, A


def _layers(a, A, n, per_layer):
    """n single-segment 256-wide layers; per_layer(seg, i) adds vectors / LayerNorms."""
    a.nseg = n
    for i in range(n):
        s = a.seg[i]
        s.W, s.N, s.K, s.end_layer, s.nout, s.drop_site = A, 256, 256, 1, 256, -1
        per_layer(s, i)


def _segs(a, A, *spec):
    """Segments (N, K, kin_off, nout_off, end_layer, nout) of one chain."""
    a.nseg = len(spec)
    for i, (N, K, kin, nout_off, end, nout) in enumerate(spec):
        s = a.seg[i]
        s.W, s.N, s.K, s.kin_off, s.nout_off, s.end_layer, s.nout, s.drop_site = A, N, K, kin, nout_off, end, nout, -1


def _wide_ln_layers(a, A):
    """Three 512-wide Linear + LayerNorm layers (3 x 1536 vector floats) and a 256-wide Linear with a bias: 4864 floats."""
    _layers(a, A, 4, lambda s, i: None)
    for i in range(4):
        s = a.seg[i]
        s.K, s.bias = 256 if i == 0 else 512, A
        if i < 3:
            s.N, s.nout = 512, 512
            _ln(s, A)


CHAIN_REFUSALS = {
    # name: (mutation, a word of the message)
    "no_segments": (lambda a, A: setattr(a, "nseg", 0), "segments"),
    "13_segments": (lambda a, A: setattr(a, "nseg", 13), "segments"),
    "negative_rows": (lambda a, A: setattr(a, "rows", -1), "rows"),
    "samples_per_workgroup_24": (lambda a, A: setattr(a, "samples_per_workgroup", 24), "samples_per_workgroup"),
    "unaligned_X": (lambda a, A: setattr(a, "X", A + 8), "input rows"),
    "ldx_not_multiple_of_8": (lambda a, A: setattr(a, "ldx", 260), "input rows"),
    "ldx_below_K0": (lambda a, A: setattr(a, "ldx", 248), "ldx"),
    "K0_768_on_32_sample_workgroups": (lambda a, A: (setattr(a, "K0", 768), setattr(a, "ldx", 768), setattr(a, "samples_per_workgroup", 32)), "panel"),
    "unaligned_W": (lambda a, A: setattr(a.seg[0], "W", A + 2), "weights"),
    "N_96": (lambda a, A: (setattr(a.seg[0], "N", 96), setattr(a.seg[0], "nout", 128)), "unsupported"),
    "K_320_past_the_panel": (lambda a, A: setattr(a.seg[0], "K", 320), "reads columns"),
    "K_192_not_instantiated": (lambda a, A: setattr(a.seg[0], "K", 192), "not instantiated"),
    "K_768_on_32_sample_workgroups": (lambda a, A: (setattr(a, "K0", 512), setattr(a, "ldx", 512), setattr(a, "samples_per_workgroup", 32),
                                                    setattr(a.seg[0], "K", 768)), "reads columns"),
    "64_column_tiles_with_K_64": (lambda a, A: (setattr(a.seg[0], "N", 192), setattr(a.seg[0], "K", 64), setattr(a.seg[0], "nout", 192)), "unsupported"),
    "five_column_tiles": (lambda a, A: (setattr(a.seg[0], "N", 640), setattr(a.seg[0], "nout", 640)), "column tiles"),
    "negative_kin_off": (lambda a, A: (setattr(a.seg[0], "kin_off", -64), setattr(a.seg[0], "K", 64)), "reads columns"),
    "kin_off_window_past_the_panel": (lambda a, A: setattr(a.seg[0], "kin_off", 64), "reads columns"),
    "negative_nout_off": (lambda a, A: setattr(a.seg[0], "nout_off", -64), "output offset"),
    "nout_off_not_multiple_of_64": (lambda a, A: setattr(a.seg[0], "nout_off", 32), "output offset"),
    "segment_past_the_layer_width": (lambda a, A: _segs(a, A, (256, 256, 0, 0, 0, 0), (128, 256, 0, 256, 1, 256)), "writes columns"),
    "nout_past_the_panel": (lambda a, A: (setattr(a.seg[0], "nout_off", 576), setattr(a.seg[0], "nout", 832)), "does not fit"),
    "drop_shift_32": (lambda a, A: (setattr(a, "dropout_p", 0.1), setattr(a.seg[0], "drop_site", 1), setattr(a.seg[0], "drop_shift", 32)), "drop_shift"),
    "unaligned_bias": (lambda a, A: setattr(a.seg[0], "bias", A + 4), "bias"),
    "unaligned_mask": (lambda a, A: (setattr(a.seg[0], "mask_y", A + 2), setattr(a.seg[0], "ld_mask", 256)), "mask"),
    "mask_col0_not_multiple_of_4": (lambda a, A: (setattr(a.seg[0], "mask_y", A), setattr(a.seg[0], "ld_mask", 512), setattr(a.seg[0], "mask_col0", 2)), "mask"),
    "ld_mask_below_col0_plus_N": (lambda a, A: (setattr(a.seg[0], "mask_y", A), setattr(a.seg[0], "ld_mask", 256), setattr(a.seg[0], "mask_col0", 4)), "mask columns"),
    "negative_mask_col0": (lambda a, A: (setattr(a.seg[0], "mask_y", A), setattr(a.seg[0], "ld_mask", 512), setattr(a.seg[0], "mask_col0", -4)), "mask columns"),
    "unaligned_stash": (lambda a, A: (setattr(a.seg[0], "stash", A + 8), setattr(a.seg[0], "ld_stash", 256)), "stash"),
    "ld_stash_below_nout": (lambda a, A: (setattr(a.seg[0], "stash", A), setattr(a.seg[0], "ld_stash", 248)), "ld_stash"),
    "ld_stash_below_the_split_part": (lambda a, A: (setattr(a.seg[0], "stash", A), setattr(a.seg[0], "stash2", A), setattr(a.seg[0], "stash_split", 64),
                                                    setattr(a.seg[0], "ld_stash", 184)), "ld_stash"),
    "ld_stash_below_a_LayerNorm_width": (lambda a, A: (setattr(a.seg[0], "stash", A), setattr(a.seg[0], "ld_stash", 128), _ln(a.seg[0], A)), "ld_stash"),
    "split_without_stash2": (lambda a, A: (setattr(a.seg[0], "stash", A), setattr(a.seg[0], "ld_stash", 256), setattr(a.seg[0], "stash_split", 128)), "split"),
    "split_not_multiple_of_8": (lambda a, A: (setattr(a.seg[0], "stash", A), setattr(a.seg[0], "stash2", A), setattr(a.seg[0], "ld_stash", 256),
                                              setattr(a.seg[0], "stash_split", 100)), "split"),
    "split_at_nout": (lambda a, A: (setattr(a.seg[0], "stash", A), setattr(a.seg[0], "stash2", A), setattr(a.seg[0], "ld_stash", 256),
                                    setattr(a.seg[0], "stash_split", 256)), "split"),
    "split_with_a_LayerNorm": (lambda a, A: (setattr(a.seg[0], "stash", A), setattr(a.seg[0], "stash2", A), setattr(a.seg[0], "ld_stash", 256),
                                             setattr(a.seg[0], "stash_split", 128), _ln(a.seg[0], A)), "stash_split"),
    "LayerNorm_width_384": (lambda a, A: (_segs(a, A, (384, 256, 0, 0, 1, 384)), _ln(a.seg[0], A)), "LayerNorm width"),
    "LayerNorm_without_xln": (lambda a, A: (_ln(a.seg[0], A), setattr(a.seg[0], "xln", None)), "LayerNorm"),
    "LayerNorm_unaligned_gamma": (lambda a, A: (_ln(a.seg[0], A), setattr(a.seg[0], "gamma", A + 4)), "LayerNorm"),
    "residual_of_another_width": (lambda a, A: (_segs(a, A, (512, 256, 0, 0, 1, 512)), _ln(a.seg[0], A), setattr(a.seg[0], "residual", 1)), "residual"),
    "LayerNorm_backward_width_384": (lambda a, A: (_segs(a, A, (384, 256, 0, 0, 1, 384)), _lnb(a.seg[0], A)), "LayerNorm backward"),
    "LayerNorm_backward_without_partial": (lambda a, A: (_lnb(a.seg[0], A), setattr(a.seg[0], "lnb_partial", None)), "LayerNorm backward"),
    "LayerNorm_backward_unaligned_y": (lambda a, A: (_lnb(a.seg[0], A), setattr(a.seg[0], "lnb_y", A + 8)), "LayerNorm backward"),
    "res_add_without_a_bypass_copy": (lambda a, A: setattr(a.seg[0], "res_add", 1), "bypass"),
    "res_dup_on_a_128_wide_segment": (lambda a, A: (_segs(a, A, (128, 256, 0, 0, 1, 128)), setattr(a.seg[0], "res_dup", 1)), "residual epilogue"),
    "res_dup_in_a_512_wide_layer": (lambda a, A: (_segs(a, A, (256, 256, 0, 0, 1, 512)), setattr(a.seg[0], "res_dup", 1)), "that one segment"),
    "res_dup_beside_a_second_segment": (lambda a, A: (_segs(a, A, (256, 256, 0, 0, 0, 0), (128, 256, 0, 256, 1, 384)), setattr(a.seg[0], "res_dup", 1)),
                                        "that one segment"),
    "res_add_beside_a_second_segment": (lambda a, A: (_segs(a, A, (256, 256, 0, 0, 1, 256), (256, 256, 0, 0, 0, 0), (128, 256, 0, 256, 1, 384)),
                                                      setattr(a.seg[0], "res_dup", 1), setattr(a.seg[1], "res_add", 1)), "that one segment"),
    "last_segment_open": (lambda a, A: setattr(a.seg[0], "end_layer", 0), "last segment"),
    "17_vectors": (lambda a, A: _layers(a, A, 6, lambda s, i: (setattr(s, "bias", A), _ln(s, A) if i < 5 else _lnb(s, A))), "vectors"),
    "vector_floats_past_4864": (lambda a, A: (_wide_ln_layers(a, A), setattr(a.seg[3], "N", 512), setattr(a.seg[3], "nout", 512)), "floats"),
}


@pytest.mark.parametrize("name", list(CHAIN_REFUSALS))
def test_layer_chain_refuses_with_a_message(name):
    """Every documented limit of mmdeer_chain (include/mmdeer.h) is checked on the host before a launch: the call returns -1 and the
    message names what is wrong.  Every table here is refused by those checks, so no call reaches a device (the pointers are fake);
    tables at the limits that must be accepted run with real buffers in test_gpu_chain_routes.py."""
    mutate, word = CHAIN_REFUSALS[name]
    rc, msg = _chain_refusal(mutate)
    assert rc == -1 and word in msg, (name, rc, msg)


def test_repack_checks_every_job_before_it_launches():
    """mmdeer_repack splits more than 64 jobs over several launches; a bad job in a later launch is refused before the first launch
    (no GPU here: had the first 64 jobs launched, the message would be the launch's)."""
    lib = _lib.load()
    A = 1 << 20
    j = (_lib.RepackJob * 70)()
    for i in range(70):
        j[i].src, j[i].dst, j[i].ld_src, j[i].rows, j[i].cols, j[i].cols_valid, j[i].layout = A, A, 64, 16, 64, 64, 1
    j[66].rows = 8
    assert lib.mmdeer_repack(j, 70, None) == -1 and b"jobs 64" in lib.mmdeer_last_error()
    j[66].rows = 16
    for field, bad, word in (("ld_src", 32, b"ld_src"), ("cols_valid", -8, b"ld_src"), ("dst_col", 8, b"does not fit")):
        j[66].layout, j[66].ld_dst = 0, 64
        setattr(j[66], field, bad)
        assert lib.mmdeer_repack(j, 70, None) == -1 and word in lib.mmdeer_last_error(), field
        j[66].ld_src, j[66].cols_valid, j[66].dst_col, j[66].layout, j[66].ld_dst = 64, 64, 0, 1, 0


def test_frag_images_job_table_on_the_host():
    """mmdeer/chainops.py: FragImages lays its images out in one buffer and describes them to mmdeer_repack -- offsets, shapes, sub-images
    and the refusals are host logic (no launch here)."""
    from mmdeer.chainops import FragImages
    cpu = torch.device("cpu")
    W = torch.zeros(256, 84, dtype=torch.bfloat16)
    V = torch.zeros(512, 256, dtype=torch.bfloat16)
    F = FragImages(cpu)
    F.add("w", W, 256, 128, ld_src=84, cols_valid=84)            # zero-padded to K = 128
    F.add("v", V, 512, 256)
    F.add("v.T", V, 512, 256, transpose=1)
    F.area("bd", 24, 384)
    F.place("bd", V[:4], 4, 128, row0=8, col0=128)
    with pytest.raises(ValueError):
        F.add("bad", W, 256, 84)                                 # columns of a fragment-major image: multiples of 64
    with pytest.raises(ValueError):
        F.place("bd", V[:4], 4, 128, row0=22)                    # past the area
    F.finish()
    assert F.off["w"] == 0 and F.off["v"] == 256 * 128 and all(o % 64 == 0 for o in F.off.values())
    assert F.shape["v.T"] == (256, 512) and F("v.T").numel() == 256 * 512
    assert F("v", 64).numel() == (512 - 64) * 256 and F("v", 64).data_ptr() == F("v").data_ptr() + 2 * 64 * 256
    assert F.mat("bd").shape == (24, 384)
    jobs = {name: F.jobs[i] for i, (name, *_) in enumerate(F.specs)}
    assert (jobs["w"].ld_src, jobs["w"].cols, jobs["w"].cols_valid, jobs["w"].layout, jobs["w"].transpose) == (84, 128, 84, 1, 0)
    assert (jobs["v.T"].transpose, jobs["v.T"].layout) == (1, 1)
    assert (jobs["bd"].layout, jobs["bd"].ld_dst, jobs["bd"].dst_col) == (0, 384, 128) and jobs["bd"].dst == F.buf.data_ptr() + 2 * (F.off["bd"] + 8 * 384)


def test_parameter_table_matches_python_spec():
    lib = _lib.load()
    offs, total = param_offsets()
    table = param_table()
    assert lib.mmdeer_num_params() == len(table) == 50
    assert lib.mmdeer_flat_elems() == total
    for i, ((name, shape, _), off) in enumerate(zip(table, offs)):
        assert lib.mmdeer_param_name(i).decode() == name
        assert lib.mmdeer_param_rows(i) == shape[0]
        assert lib.mmdeer_param_cols(i) == (shape[1] if len(shape) == 2 else 1)
        assert lib.mmdeer_param_offset(i) == off and off % 64 == 0
    assert n_live_params() == 2907212                      # live gradient payload
    # the three heads' layers are contiguous in the flat buffer (stacked / batched GEMMs rely on it)
    names = [n for n, _, _ in table]
    i0 = names.index("head.deer_heads.0.evidence_net.0.weight")
    assert offs[i0 + 1] - offs[i0] == 128 * 256 and offs[i0 + 2] - offs[i0 + 1] == 128 * 256
    # buckets tile the flat buffer in reverse execution order
    assert lib.mmdeer_bucket_begin(2) == 0 and lib.mmdeer_bucket_end(0) == total
    assert lib.mmdeer_bucket_end(2) == lib.mmdeer_bucket_begin(1) and lib.mmdeer_bucket_end(1) == lib.mmdeer_bucket_begin(0)


def test_workspace_bytes_grow_with_batch():
    lib = _lib.load()
    w0, w1, w2 = (lib.mmdeer_workspace_bytes(b, 0) for b in (0, 1024, 4096))
    assert 0 < w0 < w1 < w2
    assert lib.mmdeer_workspace_bytes(4096, 1) > w2
    assert w2 < 1 << 30


def test_layout_lookups_answer_every_field_of_the_one_list():
    """csrc/layout.inc is the one list struct Layout, make_layout() and both name look-ups are made of: every field is answered, on a
    256-byte boundary, in list order (equal offsets only behind an empty field: wfpack, wtfpack and wa_frag with compute_f32, at the
    end of the buffer), inside the buffer; a name of the other buffer, or no field's name, is refused."""
    import re
    lib = _lib.load()
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "uncertainty-aware-multimodal-emotion-recognition_amd", "csrc")
    text = open(os.path.join(root, "layout.inc")).read()
    rows = re.findall(r"\bX\(([WS]),\s*(ACT|BF16|F32),\s*(\w+),\s*[^(),]+,\s*([01])\)", text)
    assert len(rows) == len(re.findall(r"\bX\([WS],", text)) and len({n for _, _, n, _ in rows}) == len(rows) >= 50
    for f32 in (0, 1):
        for batch in (0, 1, 7, 512, 4096, 4097, 8192, 16384):
            for buf in "WS":
                if buf == "W":
                    total, look = lib.mmdeer_weights_bytes(f32), lambda n: lib.mmdeer_weights_offset(f32, n.encode())
                else:
                    total, look = lib.mmdeer_workspace_bytes(batch, f32), lambda n: lib.mmdeer_workspace_offset(batch, f32, n.encode())
                prev, prev_empty = -1, False
                for b, _, name, bf16_only in rows:
                    if b != buf:
                        assert look(name) == -1, name
                        continue
                    off = look(name)
                    assert off >= 0 and off % 256 == 0 and off <= total, (name, off)
                    assert off > prev or (off == prev and prev_empty), (name, off, prev)
                    prev, prev_empty = off, bool(f32 and bf16_only == "1")
                    assert prev_empty or off < total, name
                assert look("no_such_field") == -1
    assert lib.mmdeer_workspace_offset(-1, 0, b"slab") == -1
    # the figures of the layout before the list existed
    assert (lib.mmdeer_weights_bytes(0), lib.mmdeer_weights_bytes(1)) == (36593664, 36528128)
    assert (lib.mmdeer_workspace_bytes(4096, 0), lib.mmdeer_workspace_bytes(4096, 1)) == (267252736, 436073472)
    assert (lib.mmdeer_workspace_offset(4096, 0, b"slab"), lib.mmdeer_workspace_offset(4096, 1, b"slab")) == (174216192, 343036928)


def test_state_dict_names_follow_the_reference(golden_dir):
    m = MultimodalDEER(ModelConfig())
    sd = m.state_dict()
    names = json.load(open(os.path.join(golden_dir, "state_dict_names.json")))
    # same key set (load_state_dict is keyed; the registration order of uncertainty_gate differs)
    assert sorted(k for k in sd if k.startswith("fusion.")) == sorted("fusion." + n for n in names["fusion"])
    assert sorted(k for k in sd if k.startswith("head.")) == sorted("head." + n for n in names["head"])
    for k, shape in names["shapes"].items():
        assert list(sd[k].shape) == shape, k
    assert sum(p.numel() for p in m.parameters()) == 3105711
    assert CompleteDEERModel is MultimodalDEER
    # reference init statistics: zero biases, unit LayerNorm, Xavier-bounded weights
    assert float(sd["fusion.output_projection.0.bias"].abs().max()) == 0.0
    assert torch.equal(sd["fusion.output_projection.3.weight"], torch.ones(512))
    w = sd["fusion.trimodal_fusion.text_projection.weight"]
    bound = (6.0 / (768 + 512)) ** 0.5
    assert float(w.abs().max()) <= bound and float(w.std()) == pytest.approx(bound / 3 ** 0.5, rel=0.02)
    fp = sd["head.feature_processor.0.weight"]                            # torch default init: U(+-1/sqrt(fan_in))
    assert float(fp.abs().max()) <= 1 / 512 ** 0.5 + 1e-7


def test_unsupported_geometry_and_cpu_inputs_fail_loudly():
    with pytest.raises(NotImplementedError):
        MultimodalDEER(ModelConfig(audio_dim=40))
    m = MultimodalDEER(ModelConfig()).eval()
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        m(torch.zeros(2, 84), torch.zeros(2, 256), torch.zeros(2, 768))
    with pytest.raises(ValueError):
        m({"audio": torch.zeros(2, 84)})


def test_loss_dict_layout():
    lo = torch.arange(20, dtype=torch.float32)
    d = loss_dict_from(lo, 5)
    assert float(d["total_loss"]) == 16 and float(d["cross_dim_loss"]) == 15
    assert float(d["arousal_kl_loss"]) == 8 and d["dominance_batch_size"] == 5
    for k in ("deer_loss", "nll_loss", "evidence_reg", "kl_reg"):       # keys training.py:187-190 accumulates
        assert k in d


def test_synth_is_counter_based_and_shardable():
    full = synth.make_batch(12, seed=3)
    a = synth.make_batch(5, seed=3, row_offset=0)
    b = synth.make_batch(7, seed=3, row_offset=5)
    for k in full:
        np.testing.assert_array_equal(full[k], np.concatenate([a[k], b[k]]))
    assert full["audio"].shape == (12, 84) and full["targets"].shape == (12, 3)
    assert np.abs(full["targets"]).max() < 1.0
    big = synth.make_batch(4096, seed=42)
    assert abs(float(big["text"].mean())) < 0.01 and abs(float(big["text"].std()) - 1.0) < 0.01
    s1, s2 = synth.closed_form_state(), synth.closed_form_state()
    for k in s1:
        np.testing.assert_array_equal(s1[k], s2[k])
    assert len(synth.closed_form_state(include_gate=True)) == len(param_table()) + len(gate_param_table())


def test_shard_rows_partitions_the_batch():
    for total, world in ((4096, 8), (10, 3), (7, 8)):
        spans = [shard_rows(total, r, world) for r in range(world)]
        assert spans[0][0] == 0 and spans[-1][1] == total
        for (b0, e0), (b1, e1) in zip(spans, spans[1:]):
            assert e0 == b1 and e0 >= b0


def test_fused_adamw_argument_checks_without_a_gpu():
    """optim.FusedAdamW validates its configuration on the host and refuses to step without gradients of a
    train_step (no silent torch fallback)."""
    import torch

    from mmdeer.model import ModelConfig, MultimodalDEER
    from mmdeer.optim import FusedAdamW

    m = MultimodalDEER(ModelConfig())
    with pytest.raises(ValueError):
        FusedAdamW(m, lr=-1.0)
    live = m.live_parameters()
    with pytest.raises(ValueError):
        FusedAdamW(m, [{"params": live[:3]}])                       # trainable parameters left out
    with pytest.raises(NotImplementedError):
        FusedAdamW(m, [{"params": live[:3], "weight_decay": 0.1}, {"params": live[3:]}])   # per-group decay
    opt = FusedAdamW(m, [{"params": live[:10], "lr": 5e-5}, {"params": live[10:]}], lr=1e-4)
    assert [g["lr"] for g in opt.param_groups] == [5e-5, 1e-4]
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.5)     # torch schedulers drive it unchanged
    with pytest.raises(RuntimeError):
        opt.step()
    sd = opt.state_dict()
    assert sd["step"] == 0 and sd["exp_avg"] is None
    del sched


def test_stackb_state_dict_matches_the_reference_names():
    """mmdeer.stackb.CompleteDEERModel exposes complete_project.CompleteDEERModel's state_dict keys and shapes
    (captured by tests/golden/make_golden.py), Xavier/zero/one initialisation, and has no CPU compute path."""
    import json
    import torch
    from mmdeer import stackb
    with open(os.path.join(os.path.dirname(__file__), "golden", "stackb_state_dict_names.json")) as fh:
        shapes = json.load(fh)
    m = stackb.create_complete_deer_model()
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == shapes
    sd = m.state_dict()
    assert float(sd["calibration_layer.temperature"].sum()) == 3.0
    assert float(sd["audio_encoder.input_projection.0.bias"].abs().sum()) == 0.0
    w = sd["fusion_module.av_fusion.0.weight"]
    assert float(w.abs().max()) <= (6.0 / (512 + 512)) ** 0.5 + 1e-6 and float(w.std()) > 0.02
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.eval()(torch.zeros(2, 84), torch.zeros(2, 256), torch.zeros(2, 768))


def test_loss_classes_keep_the_reference_protocol_and_refuse_cpu_tensors():
    """mmdeer.losses mirrors the constructor / call protocol of the reference's loss classes (deer.py:111-195,
    losses.py:40-601); without a GPU every numeric call fails loudly, the key-lookup fallbacks behave as in the reference."""
    import torch
    from mmdeer import losses
    assert isinstance(losses.create_deer_loss("basic", {"reg_weight": 0.2}), losses.DEERLoss)
    assert isinstance(losses.create_deer_loss("MultiTask"), losses.MultiTaskDEERLoss)
    comb = losses.create_deer_loss()
    assert isinstance(comb, losses.CombinedDEERLoss) and comb.use_calibration_loss and comb.calibration_loss.n_bins == 15
    with pytest.raises(ValueError, match="Unknown loss type"):
        losses.create_deer_loss("focal")
    with pytest.raises(NotImplementedError):
        losses.MultiTaskDEERLoss(emotion_dims=["valence"])
    pred = {k: torch.ones(4, 1) for k in ("mu", "nu", "alpha", "beta")}
    for fn in (losses.DEERLossV1(), losses.DEERLoss(), losses.UncertaintyRegularizationLoss(), losses.CalibrationLoss()):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(pred, torch.zeros(4))
    # flat keys absent: the two extra terms return 0 exactly as the reference does (losses.py:379-380, 447-448)
    per_dim = {"valence_alpha": torch.ones(4, 1)}
    assert float(losses.UncertaintyRegularizationLoss()(per_dim, torch.zeros(4))["reg_loss"]) == 0.0
    assert float(losses.CalibrationLoss()(per_dim, torch.zeros(4))) == 0.0


def test_host_metrics_match_the_reference_vectors():
    """mmdeer/metrics.py (the numpy mirror used by the CPU-side evaluators) against vectors captured from the imported
    reference's DEERMetrics / uncertainty_calibration_error (tests/golden/make_golden.py metrics): CCC, MAE, RMSE per
    dimension and the quantile-binned ECE, incl. NaN / inf rows, tied uncertainties and a too-small set."""
    import os

    import numpy as np
    import pytest

    from mmdeer.metrics import DEERMetrics, uncertainty_calibration_error, validation_metrics

    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metrics_cases.npz"))
    m = DEERMetrics()
    for tag in ("main", "nan", "small", "ties"):
        p, t, u = g[f"{tag}.predictions"], g[f"{tag}.targets"], g[f"{tag}.uncertainties"]
        for i, d in enumerate(("valence", "arousal", "dominance")):
            assert m.concordance_correlation_coefficient(t[:, i], p[:, i]) == pytest.approx(float(g[f"{tag}.ccc_{d}"]), rel=1e-6, abs=1e-9), (tag, d)
            assert m.mean_absolute_error(t[:, i], p[:, i]) == pytest.approx(float(g[f"{tag}.mae_{d}"]), rel=1e-5), (tag, d)
            assert m.root_mean_squared_error(t[:, i], p[:, i]) == pytest.approx(float(g[f"{tag}.rmse_{d}"]), rel=1e-5), (tag, d)
        assert uncertainty_calibration_error(p, t, u) == pytest.approx(float(g[f"{tag}.ece"]), rel=1e-5, abs=1e-8), tag
        assert uncertainty_calibration_error(p, t, u, n_bins=15) == pytest.approx(float(g[f"{tag}.ece_15"]), rel=1e-5, abs=1e-8), tag
    p, t, u = g["main.predictions"], g["main.targets"], g["main.uncertainties"]
    vm = validation_metrics(p, t, u)
    assert vm["ece"] == pytest.approx(float(g["main.ece"]), rel=1e-5)
    assert vm["ccc_overall"] == pytest.approx(np.mean([float(g[f"main.ccc_{d}"]) for d in ("valence", "arousal", "dominance")]), rel=1e-6)


def test_create_fusion_module_factory():
    """fusion.create_fusion_module (fusion.py:557-592): the 'hierarchical' branch with the reference's defaults and key
    names; the 'attention' and concatenation branches build the mirrors of mmdeer.fusions (same state_dict keys), CPU tensors raise."""
    import pytest

    from mmdeer.model import HierarchicalMultimodalFusion, create_fusion_module

    gen = create_fusion_module("hierarchical", {})                     # the reference's defaults are 256/256/256 inputs: the operator path
    assert isinstance(gen, HierarchicalMultimodalFusion) and gen.audio_visual_fusion.audio_projection.weight.shape == (256, 256)
    assert gen.uncertainty_gate.modality_encoders[2][0].weight.shape == (128, 256)
    with pytest.raises(NotImplementedError, match="fusion_dim = 512"):
        create_fusion_module("hierarchical", {"fusion_dim": 256})      # the attention operators are built for 64-wide heads
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gen(torch.zeros(2, 256), torch.zeros(2, 256), torch.zeros(2, 256))
    m = create_fusion_module("Hierarchical", {"audio_dim": 84, "video_dim": 256, "text_dim": 768, "dropout": 0.1})
    assert isinstance(m, HierarchicalMultimodalFusion)
    assert "trimodal_fusion.modality_attention.in_proj_weight" in m.state_dict()
    from mmdeer import fusions
    att = create_fusion_module("attention", {})                        # fusion.py:579-583
    assert isinstance(att, fusions.AttentionFusion) and att.attention.weight.shape == (1, 512) and len(att.projections) == 3
    seq = create_fusion_module("concatenation", {"input_dims": [84, 256, 768], "dropout": 0.2})     # fusion.py:584-592
    assert isinstance(seq, torch.nn.Sequential) and seq[0].weight.shape == (512, 1108) and seq[2].p == 0.2
    assert sorted(seq.state_dict()) == ["0.bias", "0.weight", "3.bias", "3.weight"]
    ada = fusions.AdaptiveFusionGating([84, 256, 768], ["attention", "bilinear"], 256)
    assert ada.fusion_modules["bilinear"].bilinear.weight.shape == (256, 84, 256) and ada.strategy_selector[0].out_features == 2
    with pytest.raises(RuntimeError, match="no CPU fallback"):         # product path: HIP or nothing
        att([torch.zeros(2, 256)] * 3)


def test_compat_modules_resolve_by_bare_name():
    """SURVEY 8b row 1 / VERDICT r2 missing #5: with compat/ on sys.path the bare-name imports of the reference's script
    (run_multimodal_deer.py:70-82) resolve to the HIP-backed classes.  A fresh interpreter: names like `metrics`, `losses`,
    `training` must not leak into this process's sys.modules."""
    import subprocess
    import sys
    code = (
        "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "from multi_dataset_framework import MultiDatasetDEERFramework\n"
        "from complete_project import CompleteDEERModel, ModelConfig\n"
        "from training import DEERTrainer, TrainingConfig\n"
        "from preprocessing import create_enhanced_dataloaders\n"
        "from deer import test_deer_implementation\n"
        "from encoders import AudioEncoder, VideoEncoder, TextEncoder\n"
        "from fusion import HierarchicalMultimodalFusion\n"
        "from evaluation import evaluate_deer_model\n"
        "from metrics import DEERMetrics\n"
        "from losses import DEERLoss\n"
        "from visualization import create_comprehensive_report, test_visualization_components\n"
        "import mmdeer.model as M, mmdeer.trainer as T, mmdeer.losses as L, mmdeer.metrics as X\n"
        "assert CompleteDEERModel is M.MultimodalDEER and ModelConfig is M.ModelConfig\n"
        "assert DEERTrainer is T.DEERTrainer and TrainingConfig is T.TrainingConfig and evaluate_deer_model is T.evaluate_deer_model\n"
        "assert HierarchicalMultimodalFusion is M.HierarchicalMultimodalFusion and DEERLoss is L.DEERLoss and DEERMetrics is X.DEERMetrics\n"
        "cfg = ModelConfig(audio_dim=84, video_dim=256, text_dim=768, fusion_dim=512, emotion_dims=3, dropout=0.3, attention_heads=8)\n"
        "m = CompleteDEERModel(cfg)                      # run_multimodal_deer.py:237-247\n"
        "assert sum(p.numel() for p in m.parameters()) == 3105711\n"
        "for stub, args in ((MultiDatasetDEERFramework, ()), (AudioEncoder, ()), (create_enhanced_dataloaders, ())):\n"
        "    try:\n"
        "        stub(*args)\n"
        "    except NotImplementedError as e:\n"
        "        assert 'SURVEY' in str(e)\n"
        "    else:\n"
        "        raise SystemExit('out-of-scope stub did not raise')\n"
        "print('ok')\n") % (ROOT, os.path.join(ROOT, "compat"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-2000:]
    env = dict(os.environ, MMDEER_STACK="b")
    r = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
                        "from complete_project import CompleteDEERModel\nimport mmdeer.stackb as S\nassert CompleteDEERModel is S.CompleteDEERModel"
                        % (ROOT, os.path.join(ROOT, "compat"))], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]


def test_option_table_matches_the_enum_order():
    """enum OptId and the table of names, defaults and ranges are generated from ONE list, csrc/options.inc, so their order cannot part
    (it happened once with two lists: dw_tile read chain_max).  What is left to hold: every row's name is its id without OPT_, in
    lower case, and the library enumerates exactly the rows of that list, in order, with NULL past the end."""
    import os
    import re
    from mmdeer import _lib
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "uncertainty-aware-multimodal-emotion-recognition_amd", "csrc")
    text = open(os.path.join(root, "options.inc")).read()
    rows = re.findall(r'^X\(OPT_([A-Z0-9_]+),\s*"([a-z0-9_]+)",\s*(-?\d+),', text, re.M)
    assert len(rows) == len(re.findall(r"^X\(", text, re.M)) >= 15          # every row is of that form
    assert [i.lower() for i, _, _ in rows] == [n for _, n, _ in rows]
    lib = _lib.load()
    assert [lib.mmdeer_option_name(i) for i in range(len(rows))] == [n.encode() for _, n, _ in rows]
    assert lib.mmdeer_option_name(len(rows)) is None and lib.mmdeer_option_name(-1) is None
    for text_of in ("options.h", "options.hip"):                              # no second list of ids or names anywhere
        src = open(os.path.join(root, text_of)).read()
        assert '#include "options.inc"' in src and not re.search(r"\bOPT_(?!COUNT\b)[A-Z0-9_]+\s*[,=]", src)


def test_set_option_refuses_values_outside_the_range():
    """several options index tables (dw_tile -> tile sizes of the weight-gradient launch); a value outside an option's
    range must be refused with a message, and the option must keep its value."""
    from mmdeer import _lib
    lib = _lib.load()
    for name, bad in (("dw_tile", 7), ("dw_tile", -1), ("dw_tile", 1), ("splitk_max", 0), ("splitk_max", 99), ("chain", 2),
                      ("chain_min", 0), ("dw_kg", 3), ("tile", 5), ("chain_depth", 3 * 100)):
        before = _lib.get_option(name)
        assert lib.mmdeer_set_option(name.encode(), bad) == -1
        assert name in lib.mmdeer_last_error().decode() and "outside" in lib.mmdeer_last_error().decode()
        assert _lib.get_option(name) == before
    assert lib.mmdeer_set_option(b"no_such_option", 1) == -1 and "unknown" in lib.mmdeer_last_error().decode()
    with _lib.options(dw_tile=3, chain_depth=2):
        assert _lib.get_option("dw_tile") == 3 and _lib.get_option("chain_depth") == 2


def test_chain_weight_ring_registers_are_never_touched_by_the_compiler():
    """csrc/chain.hip keeps its weight ring in v[224:255] / v[240:255] behind amdgpu_num_vgpr; tools/check_chain_ring.py reads the
    device ISA and fails when the register allocator uses one of them (or an accumulation register) outside the kernel's asm."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("check_chain_ring", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                                   "tools", "check_chain_ring.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    problems, seen = mod.check(mod.device_asm())
    assert not problems, "\n".join(problems[:20])
    assert all(n > 0 for n in seen.values()) and len(seen) >= 2


_FAKE = 0x7000          # a non-NULL, 16-byte aligned address that a refused call never dereferences


def _ln_fwd_args(**kw):
    a = dict(y=_FAKE, out=_FAKE, out32=None, mean=_FAKE, rstd=_FAKE, gamma=_FAKE, beta=_FAKE, M=4, N=256, act_f32=1)
    a.update(kw)
    return (a["y"], a["out"], a["out32"], a["mean"], a["rstd"], a["gamma"], a["beta"], a["M"], a["N"], a["act_f32"], None)


def _ln_bwd_args(**kw):
    a = dict(dout=_FAKE, y=_FAKE, mean=_FAKE, rstd=_FAKE, gamma=_FAKE, dz=_FAKE, dgamma=_FAKE, dbeta=_FAKE, partial=_FAKE, M=4, N=256,
             act_f32=1)
    a.update(kw)
    return (a["dout"], a["y"], a["mean"], a["rstd"], a["gamma"], a["dz"], a["dgamma"], a["dbeta"], a["partial"], a["M"], a["N"],
            a["act_f32"], 1.0, None)


@pytest.mark.parametrize("fn,args,words", [
    ("mmdeer_layernorm_fwd", _ln_fwd_args(N=0), "layernorm_fwd: N=0"),
    ("mmdeer_layernorm_fwd", _ln_fwd_args(N=-256), "layernorm_fwd: N=-256"),
    ("mmdeer_layernorm_fwd", _ln_fwd_args(N=1028), "layernorm_fwd: N=1028"),
    ("mmdeer_layernorm_fwd", _ln_fwd_args(N=6), "layernorm_fwd: N=6"),
    ("mmdeer_layernorm_fwd", _ln_fwd_args(M=-1), "layernorm_fwd: M must be >= 0"),
    ("mmdeer_layernorm_fwd", _ln_fwd_args(M=0, N=0), "layernorm_fwd: N=0"),
] + [("mmdeer_layernorm_fwd", _ln_fwd_args(**{k: None}), "layernorm_fwd: NULL") for k in ("y", "out", "mean", "rstd", "gamma", "beta")] + [
    ("mmdeer_layernorm_bwd", _ln_bwd_args(N=0), "layernorm_bwd: N=0"),
    ("mmdeer_layernorm_bwd", _ln_bwd_args(N=-4), "layernorm_bwd: N=-4"),
    ("mmdeer_layernorm_bwd", _ln_bwd_args(N=1028), "layernorm_bwd: N=1028"),
    ("mmdeer_layernorm_bwd", _ln_bwd_args(M=-16), "layernorm_bwd: M must be >= 0"),
    ("mmdeer_layernorm_bwd", _ln_bwd_args(partial=None), "layernorm_bwd: partial is NULL"),
    ("mmdeer_layernorm_bwd", _ln_bwd_args(M=0, partial=None), "layernorm_bwd: partial is NULL"),
    ("mmdeer_layernorm_bwd", _ln_bwd_args(dbeta=None), "layernorm_bwd: pass both dgamma and dbeta"),
    ("mmdeer_layernorm_bwd", _ln_bwd_args(dgamma=None), "layernorm_bwd: pass both dgamma and dbeta"),
] + [("mmdeer_layernorm_bwd", _ln_bwd_args(**{k: None}), "layernorm_bwd: NULL") for k in ("dout", "y", "mean", "rstd", "gamma", "dz")] + [
    ("mmdeer_trimodal_attn_fwd", (_FAKE, _FAKE, _FAKE, None, None, -1, 1, 0, 0.0, 0, 0, None), "trimodal_attn_fwd: batch must be >= 0"),
    ("mmdeer_trimodal_attn_fwd", (None, _FAKE, _FAKE, None, None, 4, 1, 0, 0.0, 0, 0, None), "trimodal_attn_fwd: NULL"),
    ("mmdeer_trimodal_attn_fwd", (_FAKE, None, _FAKE, None, None, 4, 1, 0, 0.0, 0, 0, None), "trimodal_attn_fwd: NULL"),
    ("mmdeer_trimodal_attn_fwd", (_FAKE, _FAKE, None, _FAKE, _FAKE, 4, 0, 1, 0.3, 0, 0, None), "trimodal_attn_fwd: NULL"),
    ("mmdeer_trimodal_attn_bwd", (_FAKE, _FAKE, _FAKE, _FAKE, -2147483648, 1, 0, 0.0, 0, 0, None), "trimodal_attn_bwd: batch must be >= 0"),
    ("mmdeer_trimodal_attn_bwd", (None, _FAKE, _FAKE, _FAKE, 4, 1, 0, 0.0, 0, 0, None), "trimodal_attn_bwd: NULL"),
    ("mmdeer_trimodal_attn_bwd", (_FAKE, None, _FAKE, _FAKE, 4, 1, 0, 0.0, 0, 0, None), "trimodal_attn_bwd: NULL"),
    ("mmdeer_trimodal_attn_bwd", (_FAKE, _FAKE, None, _FAKE, 4, 0, 1, 0.3, 0, 0, None), "trimodal_attn_bwd: NULL"),
    ("mmdeer_trimodal_attn_bwd", (_FAKE, _FAKE, _FAKE, None, 4, 0, 1, 0.3, 0, 0, None), "trimodal_attn_bwd: NULL"),
    ("mmdeer_dropout_mask", (1, -1, 8, 0.3, 0, 0, _FAKE, None), "dropout_mask: rows and cols must be >= 0"),
    ("mmdeer_dropout_mask", (1, 8, -1, 0.3, 0, 0, _FAKE, None), "dropout_mask: rows and cols must be >= 0"),
    ("mmdeer_dropout_mask", (1, -8, -8, 0.3, 0, 0, _FAKE, None), "dropout_mask: rows and cols must be >= 0"),     # a positive product
    ("mmdeer_dropout_mask", (1, -65536, -65536, 0.3, 0, 0, _FAKE, None), "dropout_mask: rows and cols must be >= 0"),   # ... of 2^32
    ("mmdeer_dropout_mask", (1, 8, 8, 0.3, 0, 0, None, None), "dropout_mask: out is NULL"),
    # the fused kernel stores obar through a 32-bit range of B * 1024 bytes, and offset 2^31 is its "do not store" marker: B <= 2^21 - 1
    ("mmdeer_trimodal_fused_fwd", (_FAKE, _FAKE, _FAKE, _FAKE, _FAKE, None, None, None, 2 ** 21, 0, 0.0, 0, 0, None),
     "tri_fused_fwd: batch 2097152 exceeds 2097151"),
    ("mmdeer_trimodal_fused_fwd", (_FAKE, _FAKE, _FAKE, _FAKE, _FAKE, _FAKE, _FAKE, _FAKE, 2 ** 31 - 1, 1, 0.3, 0, 0, None),
     "tri_fused_fwd: batch 2147483647 exceeds 2097151"),
    ("mmdeer_trimodal_fused_bwd", (_FAKE, _FAKE, _FAKE, _FAKE, _FAKE, _FAKE, 2 ** 21, 0, 0.0, 0, 0, None),
     "tri_fused_bwd: batch 2097152 exceeds 2097151"),
    ("mmdeer_trimodal_fused_fwd", (_FAKE, _FAKE, _FAKE, _FAKE, _FAKE, None, None, None, -1, 0, 0.0, 0, 0, None), "trimodal_fused_fwd: batch must be >= 0"),
    ("mmdeer_trimodal_fused_bwd", (_FAKE, _FAKE, _FAKE, _FAKE, None, _FAKE, 4, 0, 0.0, 0, 0, None), "trimodal_fused_bwd: NULL"),
])
def test_row_operators_refuse_before_any_launch(fn, args, words):
    """LayerNorm, the trimodal attention and the dropout mask check their shapes and pointers on the host: N = 0 would divide by zero in
    the kernel, a negative count gives a negative grid or -- two of them -- a positive product and stores out of range.  There is no GPU
    here and the pointers are fake: the message must be the operator's own refusal, not a HIP error from an attempted launch."""
    lib = _lib.load()
    assert getattr(lib, fn)(*args) == -1, f"{fn}{args}: accepted"
    msg = lib.mmdeer_last_error().decode()
    assert words in msg and "hip" not in msg.lower(), (fn, msg)


def test_row_operators_accept_empty_problems_without_a_launch():
    """M = 0, B = 0, rows * cols = 0: nothing to do, no pointer is looked at (LayerNorm backward still needs `partial`: it is zeroed --
    that one call needs a device and is made by tests/test_gpu_rowkernels.py)."""
    lib = _lib.load()
    assert lib.mmdeer_layernorm_fwd(None, None, None, None, None, None, None, 0, 256, 1, None) == 0
    assert lib.mmdeer_trimodal_attn_fwd(None, None, None, None, None, 0, 1, 1, 0.3, 0, 0, None) == 0
    assert lib.mmdeer_trimodal_attn_bwd(None, None, None, None, 0, 0, 1, 0.3, 0, 0, None) == 0
    assert lib.mmdeer_trimodal_fused_fwd(None, None, None, None, None, None, None, None, 0, 1, 0.3, 0, 0, None) == 0
    assert lib.mmdeer_trimodal_fused_bwd(None, None, None, None, None, None, 0, 1, 0.3, 0, 0, None) == 0
    assert lib.mmdeer_dropout_mask(1, 0, 8, 0.3, 0, 0, _FAKE, None) == 0 and lib.mmdeer_dropout_mask(1, 8, 0, 0.3, 0, 0, _FAKE, None) == 0


_F = _FAKE


@pytest.mark.parametrize("fn,args,words", [
    ("mmdeer_cross_modal_attn_fwd", (_F, _F, _F, _F, _F, 256, _F, _F, _F, -1, 1, None), "cross_modal_attn: batch must be >= 0"),
    ("mmdeer_cross_modal_attn_fwd", (_F, _F, None, _F, _F, 256, _F, _F, _F, 4, 1, None), "cross_modal_attn: NULL pointer"),
    ("mmdeer_cross_modal_attn_fwd", (_F, _F, _F, _F, _F, 256, None, _F, _F, 4, 0, None), "cross_modal_attn: NULL pointer"),
    ("mmdeer_cross_modal_attn_fwd", (_F, _F, _F, _F, _F, 252, _F, _F, _F, 4, 1, None), "cross_modal_attn: ld=252"),
    ("mmdeer_cross_modal_attn_fwd", (_F, _F, _F, _F, _F, 258, _F, _F, _F, 4, 0, None), "cross_modal_attn: ld=258"),
    ("mmdeer_cross_modal_attn_bwd", (_F, _F, _F, _F, _F, 256, _F, _F, _F, _F, _F, _F, _F, _F, _F, -3, 1, None), "cross_modal_attn_bwd: batch must be >= 0"),
    ("mmdeer_cross_modal_attn_bwd", (_F, _F, _F, _F, _F, 256, _F, _F, _F, _F, _F, _F, _F, _F, None, 4, 1, None), "cross_modal_attn_bwd: NULL pointer"),
    ("mmdeer_cross_modal_attn_bwd", (_F, _F, _F, _F, _F, 256, _F, None, _F, _F, _F, _F, _F, _F, _F, 4, 0, None), "cross_modal_attn_bwd: NULL pointer"),
    ("mmdeer_cross_modal_attn_bwd", (_F, _F, _F, _F, _F, 128, _F, _F, _F, _F, _F, _F, _F, _F, _F, 4, 1, None), "cross_modal_attn_bwd: ld=128"),
    ("mmdeer_lstm_cell_t1", (_F, 512, _F, 128, -1, 128, 1, 1, None), "lstm_cell_t1: bad shape"),
    ("mmdeer_lstm_cell_t1", (_F, 512, _F, 128, 4, 0, 1, 1, None), "lstm_cell_t1: bad shape"),
    ("mmdeer_lstm_cell_t1", (_F, 512, _F, 128, 4, 128, 3, 1, None), "lstm_cell_t1: bad shape"),
    ("mmdeer_lstm_cell_t1", (None, 512, _F, 128, 4, 128, 1, 1, None), "lstm_cell_t1: NULL pointer"),
    ("mmdeer_lstm_cell_t1", (_F, 511, _F, 128, 4, 128, 1, 0, None), "lstm_cell_t1: leading dimensions too small"),
    ("mmdeer_lstm_cell_t1", (_F, 1024, _F, 255, 4, 128, 2, 0, None), "lstm_cell_t1: leading dimensions too small"),
    ("mmdeer_lstm_cell_t1_bwd", (_F, 512, _F, 128, _F, 4, -128, 1, 1, None), "lstm_cell_t1_bwd: bad shape"),
    ("mmdeer_lstm_cell_t1_bwd", (_F, 512, _F, 128, None, 4, 128, 1, 1, None), "lstm_cell_t1_bwd: NULL pointer"),
    ("mmdeer_lstm_cell_t1_bwd", (_F, 1023, _F, 256, _F, 4, 128, 2, 0, None), "lstm_cell_t1_bwd: leading dimensions too small"),
])
def test_side_row_operators_refuse_before_any_launch(fn, args, words):
    """the side rows' own host checks (csrc/side.hip), by their messages: no launch is attempted (there is no GPU here)"""
    lib = _lib.load()
    assert getattr(lib, fn)(*args) == -1, f"{fn}{args}: accepted"
    msg = lib.mmdeer_last_error().decode()
    assert words in msg and "hip" not in msg.lower(), (fn, msg)
