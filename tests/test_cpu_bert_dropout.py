"""The BERT trunk's dropout without a GPU: the seventh companion header (include/mmdeer_bert_drop.h) through the strict parser, its
layout against the compiler, its symbols in the built library, every refusal of the five new operators and the two sizing entries
(all decided on the host), the constructor rules of BertEncoder(dropout=..., dropout_seed=...), and the float64 restatement
(tests/bert_drop_ref.py), which pins WHERE transformers.BertModel drops: its masks are fed to a live model in train() in call order."""
import ctypes as C
import glob
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from mmdeer import _header, _lib, bert, build

from . import bert_drop_ref as RD
from . import bert_ref as R
from .test_cpu_bert import TINY, golden
from .test_cpu_bert_backward import BERT_BWD_SYMBOLS, GRAD_TOL, upstream
from .test_cpu_bert import BERT_SYMBOLS

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BERT_DROP_SYMBOLS = {"mmdeer_bert_embed_drop_fwd": 1, "mmdeer_bert_attn_drop_fwd": 1, "mmdeer_bert_drop_add_ln_fwd": 1, "mmdeer_bert_attn_drop_bwd": 1,
                     "mmdeer_bert_attn_drop_bwd_workspace": 3, "mmdeer_bert_drop_add_ln_bwd": 1, "mmdeer_bert_drop_add_ln_bwd_scratch": 2}
BERT_DROP_STRUCTS = {"bert_embed_drop_args", "bert_attn_drop_args", "bert_drop_add_ln_args", "bert_attn_drop_bwd_args", "bert_drop_add_ln_bwd_args"}


# ------------------------------------------------------------------------------------------------ the C ABI additions
def test_new_symbols_are_declared_bound_and_exported():
    lib = _lib.load()
    assert {n: len(args) for n, _, args in _lib.BERT_DROP_SYMBOLS} == BERT_DROP_SYMBOLS
    for name, res, args in _lib.BERT_DROP_SYMBOLS:
        fn = getattr(lib, name)                                           # exported by the built library
        assert fn.restype is (C.c_longlong if name.endswith(("_workspace", "_scratch")) else C.c_int32) and fn.argtypes == args, name
    assert set(_lib.BERT_DROP_STRUCTS) == BERT_DROP_STRUCTS
    for name, cls in _lib.BERT_DROP_STRUCTS.items():                      # the ctypes mirrors against the library's own sizeof
        assert lib.mmdeer_sizeof(name.encode()) == C.sizeof(cls), name
    assert _lib.BERT_DROP_CONSTANTS == {"BERT_DROP_SITE_EMBED": 256, "BERT_DROP_SITE_LAYER0": 260}
    # the older tables are as they were: additions only, in a table of their own
    assert {n: len(args) for n, _, args in _lib.BERT_SYMBOLS} == BERT_SYMBOLS and {n: len(args) for n, _, args in _lib.BERT_BWD_SYMBOLS} == BERT_BWD_SYMBOLS
    new = {n for n, _, _ in _lib.BERT_DROP_SYMBOLS}
    for older in (_lib.SYMBOLS, _lib.VIDEO_SYMBOLS, _lib.FRAME_SYMBOLS, _lib.ROUTE_SYMBOLS, _lib.FRAME_BWD_SYMBOLS, _lib.BERT_SYMBOLS, _lib.BERT_BWD_SYMBOLS):
        assert not new & {n for n, _, _ in older}
    assert not set(_lib.BERT_DROP_STRUCTS) & (set(_lib.STRUCTS) | set(_lib.VIDEO_STRUCTS) | set(_lib.FRAME_STRUCTS) | set(_lib.FRAME_BWD_STRUCTS) |
                                              set(_lib.BERT_STRUCTS) | set(_lib.BERT_BWD_STRUCTS))
    assert "bert_drop.hip" in build.SOURCES
    assert _header.BERT_DROP_HEADER_PATH == build.BERT_DROP_HEADER_PATH
    assert os.path.samefile(build.BERT_DROP_HEADER_PATH, os.path.join(ROOT, "include", "mmdeer_bert_drop.h"))
    assert lib.mmdeer_abi_version() == _lib.ABI_VERSION == 16            # additions only


def test_each_struct_is_its_counterpart_plus_the_four_dropout_fields():
    plain = {"bert_embed_drop_args": _lib.BertEmbedArgs, "bert_attn_drop_args": _lib.BertAttnArgs, "bert_drop_add_ln_args": _lib.BertAddLnArgs,
             "bert_attn_drop_bwd_args": _lib.BertAttnBwdArgs, "bert_drop_add_ln_bwd_args": _lib.BertAddLnBwdArgs}
    extra = [("site", C.c_int32), ("dropout_p", C.c_float), ("seed", C.c_uint64), ("offset", C.c_uint64)]
    for name, cls in _lib.BERT_DROP_STRUCTS.items():
        mine, theirs = list(cls._fields_), list(plain[name]._fields_)
        added = [f for f in mine if f not in theirs]
        if name == "bert_drop_add_ln_bwd_args":       # and the second gradient with its leading dimension
            assert added[:2] == [("dy", C.c_void_p), ("ld_dy", C.c_int32)]
            added = added[2:]
        assert added == extra and [f for f in mine if f in theirs] == theirs, name


def test_header_layout_matches_the_compiler(tmp_path):
    """Offsets and sizes of every field of the five new structs, as ctypes lays them out, asserted by the compiler on the header."""
    lines = ["#include <stddef.h>", '#include "mmdeer_bert_drop.h"']
    for cname, cls in _lib._BERT_DROP_CLASSES.items():
        lines.append(f'static_assert(sizeof({cname}) == {C.sizeof(cls)}, "sizeof {cname}");')
        for field, _ in cls._fields_:
            d = getattr(cls, field)
            lines.append(f'static_assert(offsetof({cname}, {field}) == {d.offset}, "offsetof {cname}.{field}");')
            lines.append(f'static_assert(sizeof((({cname}*)0)->{field}) == {d.size}, "sizeof {cname}.{field}");')
    tu = tmp_path / "layout.cpp"
    tu.write_text("\n".join(lines) + "\n")
    r = subprocess.run([build._hipcc(), "-x", "c++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(tu)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    src = _header.read(_header.BERT_DROP_HEADER_PATH)
    for bad in (src.replace("int mmdeer_bert_attn_drop_fwd(", "int mmdeer_bert_attn_drop_fwd(uint16_t f, "),                  # the same strict parser
                src.replace("#define MMDEER_BERT_DROP_SITE_EMBED 256", "#define MMDEER_BERT_DROP_SITE_EMBED 256\n#if 0\n#endif"),
                src.replace("float* workspace;", "float* workspace; short s;")):
        assert bad != src
        with pytest.raises(_header.HeaderError):
            _header.parse(bad, _lib._BERT_DROP_NAMES, {})


def test_the_site_block_is_above_every_other_site_of_the_package():
    """every dropout site id the package states (``_SITE... = n, ...`` in its modules, the DropSite enum of csrc/common.h) is below 200"""
    pkg = os.path.dirname(os.path.realpath(bert.__file__))
    found = []
    for path in glob.glob(os.path.join(pkg, "*.py")):
        if os.path.basename(path) == "bert.py":
            continue
        with open(path) as f:
            for m in re.finditer(r"^_?SITE\w*(?:, _?SITE\w*)* = ([\d, ]+)", f.read(), flags=re.M):
                found += [int(v) for v in m.group(1).replace(" ", "").split(",") if v]
    with open(os.path.join(pkg, "csrc", "common.h")) as f:
        found += [int(v) for v in re.findall(r"^\s+SITE_\w+ = (\d+),", f.read(), flags=re.M)]
    assert len(found) >= 40 and {1, 71, 105, 138, 146} <= set(found) and max(found) < 200, sorted(found)[-5:]
    assert bert.SITE_EMBED == 256 and [bert.site(0, k) for k in range(3)] == [260, 261, 262] and bert.site(11, 2) == 306


A = 1 << 20     # a plausible, aligned address: never dereferenced by the host checks


def _set(a, kw):
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _drop(a):
    a.site, a.dropout_p, a.seed, a.offset = 260, 0.1, 5, 3
    return a


def _emb(**kw):
    a = _drop(_lib.BertEmbedDropArgs())
    a.ids, a.type_ids, a.word, a.pos, a.type, a.gamma, a.beta, a.x = (A,) * 8
    a.B, a.L, a.H, a.V, a.P, a.T, a.ld_x, a.act_f32, a.eps = 2, 37, 128, 64, 48, 2, 128, 0, 1e-12
    return _set(a, kw)


def _att(**kw):
    a = _drop(_lib.BertAttnDropArgs())
    a.qkv, a.mask, a.ctx = A, A, A
    a.B, a.L, a.H, a.ld_qkv, a.ld_ctx, a.act_f32 = 2, 37, 128, 384, 128, 0
    return _set(a, kw)


def _aln(**kw):
    a = _drop(_lib.BertDropAddLnArgs())
    a.y, a.x, a.gamma, a.beta, a.out = (A,) * 5
    a.M, a.N, a.ld_y, a.ld_x, a.ld_out, a.act_f32, a.eps = 5, 128, 128, 128, 128, 0, 1e-12
    return _set(a, kw)


def _atb(**kw):
    a = _drop(_lib.BertAttnDropBwdArgs())
    a.qkv, a.mask, a.dctx, a.dqkv, a.workspace = (A,) * 5
    a.B, a.L, a.H, a.ld_qkv, a.ld_dctx, a.ld_dqkv, a.act_f32 = 2, 37, 128, 384, 128, 384, 0
    a.workspace_bytes = 2 * 2 * 2 * 37 * 4
    return _set(a, kw)


def _alb(**kw):
    a = _drop(_lib.BertDropAddLnBwdArgs())
    a.y, a.x, a.g, a.g2, a.gamma, a.ds, a.dy, a.dgamma, a.dbeta, a.scratch = (A,) * 10
    a.M, a.N, a.ld_y, a.ld_x, a.ld_g, a.ld_g2, a.ld_ds, a.ld_dy, a.act_f32, a.eps = 5, 128, 128, 128, 128, 128, 128, 128, 0, 1e-12
    a.scratch_elems = 2 * 2 * 128
    return _set(a, kw)


def _refused(f, arg, msg):
    lib = _lib.load()
    assert f(arg) == -1, msg
    assert msg in lib.mmdeer_last_error(), (msg, lib.mmdeer_last_error())


# what every entry adds to its counterpart's refusals; p = 0 reaches the plain entry's own checks (the last two rows)
DROP_REFUSALS = [({"dropout_p": 1.0}, b"dropout_p"), ({"dropout_p": -0.1}, b"dropout_p"), ({"dropout_p": 1.5}, b"dropout_p"),
                 ({"dropout_p": float("nan")}, b"dropout_p"), ({"dropout_p": float("inf")}, b"dropout_p"), ({"site": -1}, b"site")]


def test_embed_drop_refuses_on_the_host():
    f = _lib.load().mmdeer_bert_embed_drop_fwd
    for p in (0.1, 0.0):
        for kw, msg in DROP_REFUSALS * (p > 0) + [
                ({"H": 96}, b"unsupported H"), ({"H": 1088, "ld_x": 1088}, b"unsupported H"), ({"B": -1}, b"bad shape"), ({"L": -1}, b"bad shape"),
                ({"V": 0}, b"bad shape"), ({"P": 0}, b"bad shape"), ({"T": 0}, b"bad shape"), ({"L": 49}, b"max_position_embeddings"),
                ({"ld_x": 124}, b"ld_x"), ({"ld_x": 130}, b"ld_x"), ({"eps": -1.0}, b"eps"), ({"eps": float("nan")}, b"eps"),
                ({"B": 1 << 17, "L": 32, "P": 32, "H": 1024, "ld_x": 1024}, b"2^31"),
                ({"ids": None}, b"NULL"), ({"word": None}, b"NULL"), ({"pos": None}, b"NULL"), ({"type": None}, b"NULL"), ({"gamma": None}, b"NULL"),
                ({"beta": None}, b"NULL"), ({"x": None}, b"NULL"),
                ({"ids": A + 4}, b"misaligned"), ({"type_ids": A + 4}, b"misaligned"), ({"word": A + 8}, b"misaligned"), ({"gamma": A + 4}, b"misaligned"),
                ({"x": A + 4}, b"misaligned"), ({"x": A + 8, "act_f32": 1}, b"misaligned")]:
            _refused(f, C.byref(_emb(**{"dropout_p": p, **kw})), msg)
        assert f(C.byref(_emb(dropout_p=p, B=0, ids=None, word=None, x=None))) == 0
    assert f(None) == -1


def test_attention_drop_forward_refuses_on_the_host():
    f = _lib.load().mmdeer_bert_attn_drop_fwd
    for p in (0.1, 0.0):
        for kw, msg in DROP_REFUSALS * (p > 0) + [
                ({"H": 96}, b"unsupported H"), ({"H": 32}, b"unsupported H"), ({"H": 1088, "ld_qkv": 3264, "ld_ctx": 1088}, b"unsupported H"),
                ({"B": -1}, b"bad shape"), ({"L": 0}, b"bad shape"), ({"L": 513}, b"tokens"),
                ({"ld_qkv": 376}, b"ld_qkv"), ({"ld_qkv": 388}, b"ld_qkv"), ({"ld_ctx": 124}, b"ld_ctx"), ({"ld_ctx": 130}, b"ld_ctx"),
                ({"B": 1 << 14, "L": 512, "H": 1024, "ld_qkv": 3072, "ld_ctx": 1024}, b"2^31"),
                ({"qkv": None}, b"NULL"), ({"mask": None}, b"NULL"), ({"ctx": None}, b"NULL"),
                ({"qkv": A + 8}, b"misaligned"), ({"mask": A + 2}, b"misaligned"), ({"ctx": A + 4}, b"misaligned"), ({"ctx": A + 8, "act_f32": 1}, b"misaligned")]:
            _refused(f, C.byref(_att(**{"dropout_p": p, **kw})), msg)
        assert f(C.byref(_att(dropout_p=p, B=0, qkv=None, mask=None, ctx=None))) == 0
    assert f(None) == -1


def test_drop_add_ln_forward_refuses_on_the_host():
    f = _lib.load().mmdeer_bert_drop_add_ln_fwd
    for p in (0.1, 0.0):
        for kw, msg in DROP_REFUSALS * (p > 0) + [
                ({"N": 126}, b"unsupported N"), ({"N": 0}, b"unsupported N"), ({"N": 1028, "ld_y": 1028, "ld_x": 1028, "ld_out": 1028}, b"unsupported N"),
                ({"M": -1}, b"bad shape"), ({"ld_y": 124}, b"leading dimension"), ({"ld_x": 130}, b"leading dimension"), ({"ld_out": 64}, b"leading dimension"),
                ({"eps": -1.0}, b"eps"), ({"eps": float("inf")}, b"eps"), ({"M": 1 << 21, "N": 1024, "ld_y": 1024, "ld_x": 1024, "ld_out": 1024}, b"2^31"),
                ({"y": None}, b"NULL"), ({"gamma": None}, b"NULL"), ({"beta": None}, b"NULL"), ({"out": None}, b"NULL"),
                ({"y": A + 4}, b"misaligned"), ({"x": A + 2}, b"misaligned"), ({"out": A + 4}, b"misaligned"), ({"gamma": A + 4}, b"misaligned"),
                ({"beta": A + 8}, b"misaligned"), ({"y": A + 8, "act_f32": 1}, b"misaligned")]:
            _refused(f, C.byref(_aln(**{"dropout_p": p, **kw})), msg)
        assert f(C.byref(_aln(dropout_p=p, M=0, y=None, out=None))) == 0
        assert f(C.byref(_aln(dropout_p=p, M=0, x=None, ld_x=0))) == 0      # no residual: its leading dimension is not looked at
    assert f(None) == -1


def test_attention_drop_backward_refuses_on_the_host():
    lib = _lib.load()
    f = lib.mmdeer_bert_attn_drop_bwd
    for p in (0.1, 0.0):
        for kw, msg in DROP_REFUSALS * (p > 0) + [
                ({"H": 96}, b"unsupported H"), ({"H": 1088, "ld_qkv": 3264, "ld_dqkv": 3264, "ld_dctx": 1088}, b"unsupported H"),
                ({"B": -1}, b"bad shape"), ({"L": 0}, b"bad shape"), ({"L": 513}, b"tokens"),
                ({"ld_qkv": 376}, b"ld_qkv"), ({"ld_dqkv": 388}, b"ld_dqkv"), ({"ld_dctx": 120}, b"ld_dctx"), ({"ld_dctx": 132}, b"ld_dctx"),
                ({"B": 1 << 13, "L": 512, "ld_dctx": 512}, b"2^31"),
                ({"qkv": None}, b"NULL"), ({"mask": None}, b"NULL"), ({"dctx": None}, b"NULL"), ({"dqkv": None}, b"NULL"), ({"workspace": None}, b"NULL"),
                ({"workspace_bytes": 2 * 2 * 2 * 37 * 4 - 4}, b"workspace too small"), ({"workspace_bytes": 0}, b"workspace too small"),
                ({"qkv": A + 8}, b"misaligned"), ({"dctx": A + 8}, b"misaligned"), ({"dqkv": A + 8}, b"misaligned"), ({"workspace": A + 4}, b"misaligned"),
                ({"mask": A + 2}, b"misaligned")]:
            _refused(f, C.byref(_atb(**{"dropout_p": p, **kw})), msg)
        assert f(C.byref(_atb(dropout_p=p, B=0, qkv=None, mask=None, dctx=None, dqkv=None, workspace=None, workspace_bytes=0))) == 0
    assert f(None) == -1
    q, plain = lib.mmdeer_bert_attn_drop_bwd_workspace, lib.mmdeer_bert_attn_bwd_workspace
    for shape in ((2, 37, 128), (32, 128, 768), (0, 37, 128), (1, 512, 1024), (2, 37, 96), (2, 37, 1088), (-1, 37, 128), (2, 0, 128), (2, 513, 128)):
        assert q(*shape) == plain(*shape), shape
    assert q(2, 37, 128) == 2 * 2 * 2 * 37 * 4 and q(2, 37, 96) == -1


def test_drop_add_ln_backward_refuses_on_the_host():
    lib = _lib.load()
    f = lib.mmdeer_bert_drop_add_ln_bwd
    lds = {"ld_y": 1028, "ld_x": 1028, "ld_g": 1028, "ld_g2": 1028, "ld_ds": 1028, "ld_dy": 1028}
    for p in (0.1, 0.0):
        for kw, msg in DROP_REFUSALS * (p > 0) + [
                ({"N": 126}, b"unsupported N"), ({"N": 0}, b"unsupported N"), ({"N": 1028, **lds}, b"unsupported N"), ({"M": -1}, b"bad shape"),
                ({"ld_y": 124}, b"leading dimension"), ({"ld_x": 130}, b"leading dimension"), ({"ld_g": 64}, b"leading dimension"),
                ({"ld_g2": 126}, b"leading dimension"), ({"ld_ds": 124}, b"leading dimension"), ({"ld_dy": 124}, b"leading dimension"),
                ({"ld_dy": 130}, b"leading dimension"),
                ({"eps": -1.0}, b"eps"), ({"eps": float("nan")}, b"eps"), ({"M": 1 << 21, "ld_g2": 1024}, b"2^31"), ({"M": 1 << 21, "ld_dy": 1024}, b"2^31"),
                ({"dgamma": None}, b"go together"), ({"dbeta": None}, b"go together"),
                ({"y": None}, b"NULL"), ({"g": None}, b"NULL"), ({"gamma": None}, b"NULL"), ({"ds": None}, b"NULL"), ({"dy": None}, b"NULL"),
                ({"scratch": None}, b"NULL"), ({"scratch_elems": 2 * 2 * 128 - 1}, b"scratch too small"), ({"M": 4099, "scratch_elems": 1023 * 2 * 128}, b"scratch too small"),
                ({"y": A + 4}, b"misaligned"), ({"x": A + 2}, b"misaligned"), ({"g": A + 4}, b"misaligned"), ({"g2": A + 4}, b"misaligned"),
                ({"ds": A + 4}, b"misaligned"), ({"dy": A + 4}, b"misaligned"), ({"gamma": A + 4}, b"misaligned"), ({"dgamma": A + 8}, b"misaligned"),
                ({"scratch": A + 8}, b"misaligned"), ({"dy": A + 8, "act_f32": 1}, b"misaligned")]:
            _refused(f, C.byref(_alb(**{"dropout_p": p, **kw})), msg)
        assert f(C.byref(_alb(dropout_p=p, M=0, y=None, g=None, ds=None, dy=None, gamma=None, scratch=None, scratch_elems=0))) == 0
    assert f(None) == -1
    q, plain = lib.mmdeer_bert_drop_add_ln_bwd_scratch, lib.mmdeer_bert_add_ln_bwd_scratch
    for shape in ((5, 128), (1, 4), (0, 128), (4096, 768), (4099, 1024), (5, 126), (5, 0), (5, 1028), (-1, 128)):
        assert q(*shape) == plain(*shape), shape
    assert q(5, 128) == 2 * 2 * 128 and q(5, 126) == -1


# ------------------------------------------------------------------------------------------------ BertEncoder(dropout=..., dropout_seed=...)
def test_constructor_rules():
    enc = bert.BertEncoder(TINY)
    assert enc.dropout is False and enc.dropout_seed == 0 and enc._train_step == 0 and enc.p_hidden == enc.p_attn == 0.0
    assert enc.config["hidden_dropout_prob"] == enc.config["attention_probs_dropout_prob"] == 0.1         # BertConfig's defaults
    on = bert.BertEncoder(TINY, dropout=True, dropout_seed=7)
    assert on.dropout is True and on.dropout_seed == 7 and on.p_hidden == on.p_attn == 0.1
    both = bert.BertEncoder({**TINY, "hidden_dropout_prob": 0.3, "attention_probs_dropout_prob": 0.0}, dropout=True, finetune_layers=1)
    assert both.p_hidden == 0.3 and both.p_attn == 0.0
    assert list(on.state_dict()) == list(enc.state_dict())                # no parameter, no buffer
    for bad in (1, 0, "yes", None, 0.5):
        with pytest.raises(ValueError, match="dropout must be a bool"):
            bert.BertEncoder(TINY, dropout=bad)
    for bad in (-1, 2 ** 64, 1.0, "3", True, None):
        with pytest.raises(ValueError, match="dropout_seed"):
            bert.BertEncoder(TINY, dropout=True, dropout_seed=bad)
    for key in ("hidden_dropout_prob", "attention_probs_dropout_prob"):
        for bad in (1.0, -0.1, 1.5, float("nan"), float("inf"), "0.1", True):
            with pytest.raises(ValueError, match=key):
                bert.BertEncoder({**TINY, key: bad}, dropout=True)
            assert bert.BertEncoder({**TINY, key: bad}).p_hidden == 0.0   # read only with dropout=True
    with pytest.raises(ValueError, match="unknown config keys"):
        bert.BertEncoder({**TINY, "hidden_dropout": 0.1}, dropout=True)


def test_the_counter_and_the_switch_before_any_launch():
    """_drop() is what forward() asks: live only in training mode with the switch on and a nonzero probability"""
    on = bert.BertEncoder(TINY, dropout=True, dropout_seed=9)
    assert on._drop() == (9, 0) and on._drop() == (9, 1) and on._train_step == 2
    on.eval()
    assert on._drop() is None and on._train_step == 2
    on.train()
    assert on._drop() == (9, 2)
    off = bert.BertEncoder(TINY)
    assert off._drop() is None and off._train_step == 0
    zero = bert.BertEncoder({**TINY, "hidden_dropout_prob": 0.0, "attention_probs_dropout_prob": 0.0}, dropout=True)
    assert zero._drop() is None and zero._train_step == 0
    with pytest.raises(RuntimeError, match="no CPU fallback"):           # and a CPU call still goes to the device check
        with torch.no_grad():
            on(torch.zeros(2, 5, dtype=torch.int64))


def test_a_transformers_config_object_gives_the_default_module():
    transformers = pytest.importorskip("transformers")
    cfg = transformers.BertConfig(**TINY)
    enc = bert.BertEncoder(cfg)
    assert enc.dropout is False and enc.p_hidden == 0.0 and enc.train()._drop() is None
    assert bert.BertEncoder(cfg, dropout=True).p_hidden == cfg.hidden_dropout_prob == 0.1


# ------------------------------------------------------------------------------------------------ the restatement
def test_the_draw_is_the_librarys_hash_on_the_stated_rows_and_columns():
    B, L, H, heads = 2, 5, 128, 2
    s = RD.sites(B, L, H, heads, 2, 0.3, 0.5)
    assert [(n, i, r, c, p) for n, i, r, c, p in s] == [
        ("embed", 256, 10, 128, 0.3), ("attn.0", 260, 20, 5, 0.5), ("self_out.0", 261, 10, 128, 0.3), ("out.0", 262, 10, 128, 0.3),
        ("attn.1", 264, 20, 5, 0.5), ("self_out.1", 265, 10, 128, 0.3), ("out.1", 266, 10, 128, 0.3)]
    assert [n for n, *_ in RD.sites(B, L, H, heads, 1, 0.0, 0.5)] == ["attn.0"] and RD.sites(B, L, H, heads, 1, 0.0, 0.0) == []
    m = RD.draw(s, seed=11, step=4)
    assert set(m) == {n for n, *_ in s} and m["attn.1"].shape == (20, 5) and m["embed"].shape == (10, 128)
    assert set(m["attn.0"].unique().tolist()) == {0.0, 2.0}
    scale = float(np.float32(1.0 / (1.0 - float(np.float32(0.3)))))
    assert set(m["out.1"].unique().tolist()) == {0.0, scale} and 0.6 < float((m["out.1"] != 0).double().mean()) < 0.8
    assert not torch.equal(m["self_out.0"], m["out.0"]) and not torch.equal(m["out.0"], RD.draw(s, 11, 5)["out.0"])
    # the hash by hand for one element of the attention site: row = (b * heads + h) * L + i, col = j
    from .rowkernel_ref import drop_key, drop_threshold, mix32
    b, h, i, j = 1, 1, 3, 2
    row = (b * heads + h) * L + i
    draw = int(mix32(((row * 0x9E3779B1) & 0xFFFFFFFF) ^ ((j * 0x85EBCA77) & 0xFFFFFFFF) ^ drop_key(264, 11, 4)))
    assert (draw < drop_threshold(0.5)[0]) == bool(m["attn.1"][row, j] != 0)


def test_restatement_without_masks_is_the_plain_one():
    sd, ids, mask, typ, hidden = golden()
    up = upstream(mask, 128)
    from . import bert_bwd_ref as RB
    for rnd in (R.ident, R.bf16_round):
        states, grads = RD.trunk_grads(sd, ids, mask, typ, up, None, rnd=rnd)
        want_out, want = RB.trunk_grads(sd, ids, mask, typ, up, rnd=rnd)
        assert torch.equal(states[-1], want_out) and all(torch.equal(grads[k], want[k]) for k in want) and set(grads) == set(want)
        assert all(torch.equal(a, b) for a, b in zip(RD.trunk(sd, ids, mask, typ, None, rnd=rnd), R.trunk(sd, ids, mask, typ, rnd=rnd)))


def test_restatement_operators_with_masks():
    torch.manual_seed(4)
    B, L, H = 2, 7, 128
    qkv = torch.randn(B * L, 3 * H, dtype=torch.float64)
    mask = torch.cat([torch.zeros(7), torch.tensor([1., 0, 1, 1, 0, 0, 1])]).double()
    dctx = torch.randn(B * L, H, dtype=torch.float64)
    m = RD.drop_mask(260, B * 2 * L, L, 0.5, 3, 0)
    ctx = RD.attention(qkv, mask, B, L, H, m)
    # by hand, head 1 of sample 1: the softmax over the undropped probabilities, the mask on the operand of the second product only
    q, k, v = (qkv[L:, i * H + 64:i * H + 128] for i in range(3))
    keep = mask[L:] != 0
    P = torch.softmax((q @ k.T / 8).masked_fill(~keep, float("-inf")), -1)
    mm = m[(1 * 2 + 1) * L:(1 * 2 + 2) * L]
    torch.testing.assert_close(ctx[L:, 64:], (P * mm) @ v, rtol=1e-12, atol=1e-13)
    assert torch.equal(ctx[:L], torch.zeros(L, H, dtype=torch.float64))
    d = RD.attention_bwd(qkv, mask, dctx, B, L, H, m)
    do = dctx[L:, 64:]
    dPd = (do @ v.T) * mm
    dS = P * (dPd - (P * dPd).sum(-1, keepdim=True))
    for got, want in ((d[L:, 64:128], dS @ k / 8), (d[L:, H + 64:H + 128], dS.T @ q / 8), (d[L:, 2 * H + 64:], (P * mm).T @ do)):
        torch.testing.assert_close(got, want, rtol=1e-11, atol=1e-12)
    y, x, g, g2 = (torch.randn(5, 64, dtype=torch.float64) for _ in range(4))
    gamma, beta = torch.rand(64, dtype=torch.float64) + 0.5, torch.randn(64, dtype=torch.float64)
    mh = RD.drop_mask(261, 5, 64, 0.3, 3, 0)
    ds, dy, dgamma, dbeta = RD.add_ln_bwd(y, x, g, g2, gamma, beta, 1e-12, mh)
    from . import bert_bwd_ref as RB
    want = RB.add_ln_bwd(y * mh, x, g, g2, gamma, beta, 1e-12)
    assert torch.equal(dy, ds * mh) and all(torch.allclose(a, b, rtol=1e-12, atol=1e-13) for a, b in zip((ds, dgamma, dbeta), want))
    assert bool((dy[mh == 0] == 0).all()) and int((mh == 0).sum()) > 50
    assert torch.equal(RD.add_ln(y, x, gamma, beta, 1e-12, mh), R.add_ln(y * mh, x, gamma, beta, 1e-12))


def test_restatement_equals_a_live_bert_model_in_train_mode():
    """transformers.BertModel in train(), float64, eager attention, both probabilities 0.3, with torch.nn.functional.dropout replaced for
    the call by a multiplication with the restatement's masks in call order (embeddings; per layer attention, self-output, output):
    all hidden states and the 36 gradient tensors of the no-dropout comparison, to its bound (1e-9 of each tensor's largest element).
    The golden masks leave every sample a valid key, where the additive-mask and exact-exclusion forms agree."""
    transformers = pytest.importorskip("transformers")
    sd, ids, mask, typ, hidden = golden()
    assert bool((mask.sum(1) > 0).all())
    B, L = ids.shape
    p = 0.3
    s = RD.sites(B, L, 128, 2, 2, p, p)
    masks = RD.draw(s, seed=21, step=6)
    cfg = transformers.BertConfig(**TINY, attn_implementation="eager", hidden_dropout_prob=p, attention_probs_dropout_prob=p)
    model = transformers.BertModel(cfg).double().train()
    model.load_state_dict(sd, strict=True)
    up = upstream(mask, 128)
    order, calls = [n for n, *_ in s], []

    def fed(x, p=0.5, training=True, inplace=False):
        name = order[len(calls)]
        calls.append((name, p, training))
        return x * masks[name].reshape(x.shape)

    real = torch.nn.functional.dropout
    torch.nn.functional.dropout = fed
    try:
        out = model(input_ids=ids, attention_mask=mask, token_type_ids=typ, output_hidden_states=True)
    finally:
        torch.nn.functional.dropout = real
    assert [c[0] for c in calls] == order and len(calls) == 1 + 3 * 2 and all(c[1] == p and c[2] for c in calls)
    (out.last_hidden_state * up).sum().backward()
    states, grads = RD.trunk_grads(sd, ids, mask, typ, up, masks)
    assert len(out.hidden_states) == len(states) == 3
    for i, (a, b) in enumerate(zip(states, out.hidden_states)):
        d = float((a - b.detach()).abs().max())
        print(f"hidden state {i}: max |restatement - transformers| = {d:.3g}")
        assert d <= GRAD_TOL * float(b.detach().abs().max()), (i, d)
    assert all(torch.equal(a, b) for a, b in zip(states, RD.trunk(sd, ids, mask, typ, masks)))
    assert float((states[-1] - R.trunk(sd, ids, mask, typ)[-1]).abs().max()) > 0.5        # the masks did something
    live = {n: q.grad for n, q in model.named_parameters() if q.grad is not None}
    compared = [n for n in live if n != "embeddings.word_embeddings.weight" and not n.startswith("pooler.")]
    assert len(compared) == 2 * 16 + 4
    worst = 0.0
    for n in compared:
        scale = float(live[n.replace(".key.bias", ".query.bias")].abs().max())          # key.bias: analytically zero, held to query.bias's scale
        rel = float((grads[n] - live[n]).abs().max()) / scale
        worst = max(worst, rel)
        assert rel <= GRAD_TOL, (n, rel)
    print(f"largest |restatement - transformers| / max |gradient| over {len(compared)} tensors: {worst:.3g}")
    assert max(float(g.abs().max()) for g in live.values()) > 1.0
