"""The BERT trunk's backward without a GPU: the sixth companion header (include/mmdeer_bert_bwd.h) through the strict parser, its
layout against the compiler, its symbols in the built library, every refusal of the three new operators and the two sizing entries
(all decided on the host), the float64 restatement of the backward (tests/bert_bwd_ref.py) against autograd through a live
transformers.BertModel, and what BertEncoder(finetune_layers=k) promises before any launch."""
import ctypes as C
import os
import subprocess

import pytest
import torch

from mmdeer import _header, _lib, bert, build

from . import bert_bwd_ref as RB
from . import bert_ref as R
from .test_cpu_bert import BERT_SYMBOLS, TINY, golden
from .test_cpu_frame_backward import BWD_SYMBOLS

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BERT_BWD_SYMBOLS = {"mmdeer_bert_attn_bwd": 1, "mmdeer_bert_attn_bwd_workspace": 3, "mmdeer_bert_add_ln_bwd": 1, "mmdeer_bert_add_ln_bwd_scratch": 2,
                    "mmdeer_bert_gelu_bwd": 1}
BERT_BWD_STRUCTS = {"bert_attn_bwd_args", "bert_add_ln_bwd_args", "bert_gelu_bwd_args"}
# float64 against float64, relative to the largest element of the gradient tensor: the issue's bound (measured: below 1e-10)
GRAD_TOL = 1e-9


# ------------------------------------------------------------------------------------------------ the C ABI additions
def test_new_symbols_are_declared_bound_and_exported():
    lib = _lib.load()
    assert {n: len(args) for n, _, args in _lib.BERT_BWD_SYMBOLS} == BERT_BWD_SYMBOLS
    for name, res, args in _lib.BERT_BWD_SYMBOLS:
        fn = getattr(lib, name)                                           # exported by the built library
        assert fn.restype is (C.c_longlong if name.endswith(("_workspace", "_scratch")) else C.c_int32) and fn.argtypes == args, name
    assert set(_lib.BERT_BWD_STRUCTS) == BERT_BWD_STRUCTS
    for name, cls in _lib.BERT_BWD_STRUCTS.items():                       # the ctypes mirrors against the library's own sizeof
        assert lib.mmdeer_sizeof(name.encode()) == C.sizeof(cls), name
    assert _lib.BERT_BWD_CONSTANTS == {"BERT_LN_BWD_PARTS": 1024}
    # the older tables are as they were: additions only, in a table of their own
    assert {n: len(args) for n, _, args in _lib.BERT_SYMBOLS} == BERT_SYMBOLS and {n: len(args) for n, _, args in _lib.FRAME_BWD_SYMBOLS} == BWD_SYMBOLS
    assert set(_lib.BERT_STRUCTS) == {"bert_embed_args", "bert_attn_args", "bert_add_ln_args", "bert_gelu_args"}
    assert _lib.BERT_CONSTANTS == {"BERT_HEAD_DIM": 64, "BERT_MAX_HIDDEN": 1024, "BERT_MAX_TOKENS": 512}
    new = {n for n, _, _ in _lib.BERT_BWD_SYMBOLS}
    for older in (_lib.SYMBOLS, _lib.VIDEO_SYMBOLS, _lib.FRAME_SYMBOLS, _lib.ROUTE_SYMBOLS, _lib.FRAME_BWD_SYMBOLS, _lib.BERT_SYMBOLS):
        assert not new & {n for n, _, _ in older}
    assert not set(_lib.BERT_BWD_STRUCTS) & (set(_lib.STRUCTS) | set(_lib.VIDEO_STRUCTS) | set(_lib.FRAME_STRUCTS) | set(_lib.FRAME_BWD_STRUCTS) | set(_lib.BERT_STRUCTS))
    assert not any(k.startswith("BERT") for k in _lib.CONSTANTS)
    assert "bert_bwd.hip" in build.SOURCES and "bert.hip" in build.SOURCES
    assert _header.BERT_BWD_HEADER_PATH == build.BERT_BWD_HEADER_PATH
    assert os.path.samefile(build.BERT_BWD_HEADER_PATH, os.path.join(ROOT, "include", "mmdeer_bert_bwd.h"))
    assert lib.mmdeer_abi_version() == _lib.ABI_VERSION == 16            # additions only


def test_header_layout_matches_the_compiler(tmp_path):
    """Offsets and sizes of every field of the three new structs, as ctypes lays them out, asserted by the compiler on the header."""
    lines = ["#include <stddef.h>", '#include "mmdeer_bert_bwd.h"']
    for cname, cls in _lib._BERT_BWD_CLASSES.items():
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
    src = _header.read(_header.BERT_BWD_HEADER_PATH)
    for bad in (src.replace("int mmdeer_bert_gelu_bwd(", "int mmdeer_bert_gelu_bwd(uint16_t f, "),                  # the same strict parser
                src.replace("#define MMDEER_BERT_LN_BWD_PARTS 1024", "#define MMDEER_BERT_LN_BWD_PARTS 1024\n#if 0\n#endif"),
                src.replace("float* workspace;", "float* workspace; short s;")):
        assert bad != src
        with pytest.raises(_header.HeaderError):
            _header.parse(bad, _lib._BERT_BWD_NAMES, {})


A = 1 << 20     # a plausible, aligned address: never dereferenced by the host checks


def _set(a, kw):
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _att(**kw):
    a = _lib.BertAttnBwdArgs()
    a.qkv, a.mask, a.dctx, a.dqkv, a.workspace = (A,) * 5
    a.B, a.L, a.H, a.ld_qkv, a.ld_dctx, a.ld_dqkv, a.act_f32 = 2, 37, 128, 384, 128, 384, 0
    a.workspace_bytes = 2 * 2 * 2 * 37 * 4
    return _set(a, kw)


def _aln(**kw):
    a = _lib.BertAddLnBwdArgs()
    a.y, a.x, a.g, a.g2, a.gamma, a.ds, a.dgamma, a.dbeta, a.scratch = (A,) * 9
    a.M, a.N, a.ld_y, a.ld_x, a.ld_g, a.ld_g2, a.ld_ds, a.act_f32, a.eps = 5, 128, 128, 128, 128, 128, 128, 0, 1e-12
    a.scratch_elems = 2 * 2 * 128
    return _set(a, kw)


def _gel(**kw):
    a = _lib.BertGeluBwdArgs()
    a.x, a.g, a.dx = A, A, A
    a.M, a.N, a.ld_x, a.ld_g, a.ld_dx, a.act_f32 = 5, 256, 256, 256, 256, 0
    return _set(a, kw)


def _refused(f, arg, msg):
    lib = _lib.load()
    assert f(arg) == -1, msg
    assert msg in lib.mmdeer_last_error(), (msg, lib.mmdeer_last_error())


def test_attention_backward_refuses_on_the_host():
    lib = _lib.load()
    f = lib.mmdeer_bert_attn_bwd
    wide = {"H": 1088, "ld_qkv": 3264, "ld_dqkv": 3264, "ld_dctx": 1088}
    for kw, msg in [({"H": 96}, b"unsupported H"), ({"H": 32}, b"unsupported H"), (wide, b"unsupported H"), ({"H": 96, "B": 0}, b"unsupported H"),
                    ({"B": -1}, b"bad shape"), ({"L": 0}, b"bad shape"), ({"L": -1, "B": 0}, b"bad shape"),
                    ({"L": 513}, b"tokens"), ({"L": 513, "B": 0}, b"tokens"),
                    ({"ld_qkv": 376}, b"ld_qkv"), ({"ld_qkv": 388}, b"ld_qkv"), ({"ld_dqkv": 376}, b"ld_dqkv"), ({"ld_dqkv": 388}, b"ld_dqkv"),
                    ({"ld_dctx": 120}, b"ld_dctx"), ({"ld_dctx": 132}, b"ld_dctx"),
                    ({"B": 1 << 14, "L": 512, "H": 1024, "ld_qkv": 3072, "ld_dqkv": 3072, "ld_dctx": 1024}, b"2^31"),
                    ({"B": 1 << 13, "L": 512, "ld_dctx": 512}, b"2^31"),
                    ({"qkv": None}, b"NULL"), ({"mask": None}, b"NULL"), ({"dctx": None}, b"NULL"), ({"dqkv": None}, b"NULL"),
                    ({"workspace": None}, b"NULL"), ({"workspace_bytes": 2 * 2 * 2 * 37 * 4 - 4}, b"workspace too small"), ({"workspace_bytes": 0}, b"workspace too small"),
                    ({"qkv": A + 8}, b"misaligned"), ({"dctx": A + 8}, b"misaligned"), ({"dqkv": A + 8}, b"misaligned"),
                    ({"workspace": A + 4}, b"misaligned"), ({"mask": A + 2}, b"misaligned"), ({"dqkv": A + 8, "act_f32": 1}, b"misaligned")]:
        _refused(f, C.byref(_att(**kw)), msg)
    assert f(C.byref(_att(B=0, qkv=None, mask=None, dctx=None, dqkv=None, workspace=None, workspace_bytes=0))) == 0
    assert f(C.byref(_att(B=0, L=0, qkv=None))) == 0
    assert f(None) == -1
    q = lib.mmdeer_bert_attn_bwd_workspace
    assert q(2, 37, 128) == 2 * 2 * 2 * 37 * 4 and q(32, 128, 768) == 2 * 32 * 12 * 128 * 4 and q(0, 37, 128) == 0 and q(0, 0, 64) == 0
    assert q(1, 512, 1024) == 2 * 16 * 512 * 4
    for bad in ((2, 37, 96), (2, 37, 1088), (-1, 37, 128), (2, 0, 128), (2, 513, 128), (0, -1, 128)):
        assert q(*bad) == -1, bad


def test_add_ln_backward_refuses_on_the_host():
    lib = _lib.load()
    f = lib.mmdeer_bert_add_ln_bwd
    lds = {"ld_y": 1028, "ld_x": 1028, "ld_g": 1028, "ld_g2": 1028, "ld_ds": 1028}
    big = {"ld_y": 1024, "ld_x": 1024, "ld_g": 1024, "ld_g2": 1024, "ld_ds": 1024}
    for kw, msg in [({"N": 126}, b"unsupported N"), ({"N": 0}, b"unsupported N"), ({"N": 1028, **lds}, b"unsupported N"), ({"N": 126, "M": 0}, b"unsupported N"),
                    ({"M": -1}, b"bad shape"),
                    ({"ld_y": 124}, b"leading dimension"), ({"ld_x": 130}, b"leading dimension"), ({"ld_g": 64}, b"leading dimension"),
                    ({"ld_g2": 126}, b"leading dimension"), ({"ld_ds": 124}, b"leading dimension"),
                    ({"eps": -1.0}, b"eps"), ({"eps": float("nan")}, b"eps"), ({"eps": float("inf")}, b"eps"),
                    ({"M": 1 << 21, "N": 1024, **big}, b"2^31"), ({"M": 1 << 21, "ld_g2": 1024}, b"2^31"),
                    ({"dgamma": None}, b"go together"), ({"dbeta": None}, b"go together"), ({"dbeta": None, "M": 0}, b"go together"),
                    ({"y": None}, b"NULL"), ({"g": None}, b"NULL"), ({"gamma": None}, b"NULL"), ({"ds": None}, b"NULL"), ({"scratch": None}, b"NULL"),
                    ({"scratch_elems": 2 * 2 * 128 - 1}, b"scratch too small"), ({"scratch_elems": 0}, b"scratch too small"),
                    ({"M": 4099, "scratch_elems": 1023 * 2 * 128}, b"scratch too small"),
                    ({"y": A + 4}, b"misaligned"), ({"x": A + 2}, b"misaligned"), ({"g": A + 4}, b"misaligned"), ({"g2": A + 4}, b"misaligned"),
                    ({"ds": A + 4}, b"misaligned"), ({"gamma": A + 4}, b"misaligned"), ({"dgamma": A + 8}, b"misaligned"), ({"dbeta": A + 4}, b"misaligned"),
                    ({"scratch": A + 8}, b"misaligned"), ({"y": A + 8, "act_f32": 1}, b"misaligned")]:
        _refused(f, C.byref(_aln(**kw)), msg)
    assert f(C.byref(_aln(M=0, y=None, g=None, ds=None, gamma=None, scratch=None, scratch_elems=0))) == 0
    assert f(C.byref(_aln(x=None, ld_x=0, g2=None, ld_g2=0, M=0))) == 0        # no residual, no second gradient: their leading dimensions are not looked at
    assert f(None) == -1
    q = lib.mmdeer_bert_add_ln_bwd_scratch
    assert q(5, 128) == 2 * 2 * 128 and q(1, 4) == 8 and q(0, 128) == 0 and q(4096, 768) == 1024 * 2 * 768 and q(4099, 1024) == 1024 * 2 * 1024 and q(4093, 64) == 1024 * 2 * 64 and q(4092, 64) == 1023 * 2 * 64
    assert q(1023, 64) == 256 * 2 * 64 and q(1021, 64) == 256 * 2 * 64 and q(1020, 64) == 255 * 2 * 64
    for bad in ((5, 126), (5, 0), (5, 1028), (-1, 128)):
        assert q(*bad) == -1, bad


def test_gelu_backward_refuses_on_the_host():
    f = _lib.load().mmdeer_bert_gelu_bwd
    for kw, msg in [({"N": 254}, b"unsupported N"), ({"N": 0}, b"unsupported N"), ({"N": 254, "M": 0}, b"unsupported N"), ({"M": -1}, b"bad shape"),
                    ({"ld_x": 252}, b"leading dimension"), ({"ld_g": 258}, b"leading dimension"), ({"ld_dx": 128}, b"leading dimension"),
                    ({"M": 1 << 20, "N": 2048, "ld_x": 2048, "ld_g": 2048, "ld_dx": 2048}, b"2^31"), ({"M": 1 << 23, "ld_g": 512}, b"2^31"),
                    ({"x": None}, b"NULL"), ({"g": None}, b"NULL"), ({"dx": None}, b"NULL"),
                    ({"x": A + 4}, b"misaligned"), ({"g": A + 2}, b"misaligned"), ({"dx": A + 4}, b"misaligned"), ({"dx": A + 8, "act_f32": 1}, b"misaligned")]:
        _refused(f, C.byref(_gel(**kw)), msg)
    assert f(C.byref(_gel(M=0, x=None, g=None, dx=None))) == 0
    assert f(None) == -1


# ------------------------------------------------------------------------------------------------ the restatement
def upstream(mask, H, seed=11):
    """(B, L, H) float64, exact in bf16, zero on masked tokens: what everything downstream of the trunk hands back"""
    gen = torch.Generator().manual_seed(seed)
    up = torch.randn(*mask.shape, H, generator=gen).bfloat16().double()
    return up * (mask != 0).double().unsqueeze(-1)


def test_restatement_forward_is_bert_refs():
    sd, ids, mask, typ, hidden = golden()
    up = upstream(mask, 128)
    for rnd in (R.ident, R.bf16_round):
        out, grads = RB.trunk_grads(sd, ids, mask, typ, up, rnd=rnd)
        assert torch.equal(out, R.trunk(sd, ids, mask, typ, rnd=rnd)[-1])
        assert set(grads) == {k for k in sd if not k.startswith("pooler.")} and all(bool(torch.isfinite(g).all()) for g in grads.values())
    # the hook rounds in the backward: the gradient of an identity under it is the rounded upstream, its forward is untouched
    t = torch.tensor([1.0 + 2.0 ** -10, 3.0], dtype=torch.float64, requires_grad=True)
    y = RB._grad_round(R.bf16_round)(t)
    assert torch.equal(y, t)
    (g,) = torch.autograd.grad((y * t.detach()).sum(), [t])
    assert torch.equal(g, torch.tensor([1.0, 3.0], dtype=torch.float64))
    z = RB._straight(R.bf16_round)(t)
    (g,) = torch.autograd.grad((z * t.detach()).sum(), [t])
    assert torch.equal(z, torch.tensor([1.0, 3.0], dtype=torch.float64)) and torch.equal(g, t.detach())


def test_restatement_operator_gradients():
    torch.manual_seed(4)
    B, L, H = 2, 7, 128
    qkv = torch.randn(B * L, 3 * H + 8, dtype=torch.float64)
    mask = torch.cat([torch.zeros(7), torch.tensor([1., 0, 1, 1, 0, 0, 1])]).double()
    dctx = torch.randn(B * L, H, dtype=torch.float64)
    d = RB.attention_bwd(qkv, mask, dctx, B, L, H)
    assert d.shape == (B * L, 3 * H) and torch.equal(d[:L], torch.zeros(L, 3 * H, dtype=torch.float64))     # the dead sample
    dead_keys = (mask[L:] == 0).nonzero().flatten() + L
    assert torch.equal(d[dead_keys, H:], torch.zeros(len(dead_keys), 2 * H, dtype=torch.float64))           # masked keys: dK = dV = 0 exactly
    assert float(d[dead_keys, :H].abs().min()) > 0                                                          # masked queries attend
    # by hand: P, dV = P^T dO, dP = dO V^T, dS = P o (dP - delta), dQ = dS K / 8, dK = dS^T Q / 8 on head 1 of sample 1
    q, k, v = (qkv[L:, i * H + 64:i * H + 128] for i in range(3))
    do, keep = dctx[L:, 64:128], mask[L:] != 0
    P = torch.softmax((q @ k.T / 8).masked_fill(~keep, float("-inf")), -1)
    dP = do @ v.T
    dS = P * (dP - (P * dP).sum(-1, keepdim=True))
    for got, want in ((d[L:, 64:128], dS @ k / 8), (d[L:, H + 64:H + 128], dS.T @ q / 8), (d[L:, 2 * H + 64:], P.T @ do)):
        torch.testing.assert_close(got, want, rtol=1e-11, atol=1e-12)
    y, x, g, g2 = (torch.randn(5, 64, dtype=torch.float64) for _ in range(4))
    gamma, beta = torch.rand(64, dtype=torch.float64) + 0.5, torch.randn(64, dtype=torch.float64)
    gamma[3] = 0.0
    ds, dgamma, dbeta = RB.add_ln_bwd(y, x, g, g2, gamma, beta, 1e-12)
    s, G = y + x, g + g2
    xhat = (s - s.mean(-1, keepdim=True)) / torch.sqrt(s.var(-1, unbiased=False, keepdim=True) + 1e-12)
    torch.testing.assert_close(dgamma, (G * xhat).sum(0), rtol=1e-11, atol=1e-12)
    torch.testing.assert_close(dbeta, G.sum(0), rtol=1e-11, atol=1e-12)
    assert float(dgamma[3]) != 0.0 and float(ds[:, 3].abs().max()) > 0        # xhat is there where gamma = 0; ds there through the row means alone
    grid = torch.tensor([0.0, 0.75, -0.75, 3.0, -3.0, 10.0, -10.0], dtype=torch.float64)
    want = 0.5 * (1 + torch.erf(grid / 2 ** 0.5)) + grid * torch.exp(-grid ** 2 / 2) / (2 * torch.pi) ** 0.5
    torch.testing.assert_close(RB.gelu_bwd(grid, torch.ones(7)), want, rtol=1e-13, atol=1e-14)
    assert 1e-4 < float((RB.gelu_tanh_bwd(grid, torch.ones(7)) - want).abs().max()) < 1e-2


def test_restatement_gradients_equal_a_live_bert_model():
    """autograd through transformers.BertModel in float64 (train mode, eager attention, both dropout probabilities 0) on the golden
    model, ids and masks (every sample there has a valid key), under an upstream gradient that is zero on masked tokens"""
    transformers = pytest.importorskip("transformers")
    sd, ids, mask, typ, hidden = golden()
    cfg = transformers.BertConfig(**TINY, attn_implementation="eager", hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    model = transformers.BertModel(cfg).double().train()
    model.load_state_dict(sd, strict=True)
    up = upstream(mask, 128)
    out = model(input_ids=ids, attention_mask=mask, token_type_ids=typ).last_hidden_state
    (out * up).sum().backward()
    got_out, grads = RB.trunk_grads(sd, ids, mask, typ, up)
    assert float((got_out - out.detach()).abs().max()) <= 2e-13
    live = {n: p.grad for n, p in model.named_parameters() if p.grad is not None}
    compared = [n for n in live if n != "embeddings.word_embeddings.weight" and not n.startswith("pooler.")]     # padding_idx differs; never trained
    assert len(compared) == 2 * 16 + 4 and {n for n in compared if n.startswith("encoder.layer.")} == {k for k in sd if k.startswith("encoder.layer.")}
    worst = 0.0
    for n in compared:
        # key.bias: analytically zero (a shift of every score of a row leaves the softmax alone), about 1e-14 in float64: held to query.bias's scale
        scale = float(live[n.replace(".key.bias", ".query.bias")].abs().max())
        rel = float((grads[n] - live[n]).abs().max()) / scale
        worst = max(worst, rel)
        assert rel <= GRAD_TOL, (n, rel)
        if n.endswith(".key.bias"):
            assert float(live[n].abs().max()) < 1e-12 * scale and float(grads[n].abs().max()) < 1e-12 * scale
    print(f"largest |restatement - transformers| / max |gradient| over {len(compared)} tensors: {worst:.3g}")
    assert max(float(g.abs().max()) for g in live.values()) > 1.0          # gradients of a size worth comparing


# ------------------------------------------------------------------------------------------------ BertEncoder(finetune_layers=k)
def test_finetune_layers_selects_the_trainable_parameters():
    assert bert.BertEncoder(TINY).finetune_layers == 0
    for k in (0, 1, 2):
        enc = bert.BertEncoder(TINY, finetune_layers=k)
        want = {n for n, _ in enc.named_parameters() if n.startswith("encoder.layer.") and int(n.split(".")[2]) >= 2 - k}
        assert {n for n, p in enc.named_parameters() if p.requires_grad} == want and len(want) == 16 * k and enc.finetune_layers == k
    for bad in (-1, 3, 1.0, "1", None, True):
        with pytest.raises(ValueError, match="finetune_layers"):
            bert.BertEncoder(TINY, finetune_layers=bad)
    six = bert.BertEncoder({**TINY, "num_hidden_layers": 12}, finetune_layers=6)         # the reference's _setup_bert_fine_tuning
    assert {int(n.split(".")[2]) for n, p in six.named_parameters() if p.requires_grad} == set(range(6, 12))
    assert not any(p.requires_grad for n, p in six.named_parameters() if not n.startswith("encoder.layer."))
    assert list(six.state_dict()) == list(bert.BertEncoder({**TINY, "num_hidden_layers": 12}).state_dict())


def test_the_default_module_is_as_before():
    enc = bert.BertEncoder(TINY)
    ids = torch.zeros(2, 5, dtype=torch.int64)
    assert not any(p.requires_grad for p in enc.parameters())
    enc.encoder.layer[1].output.dense.weight.requires_grad_(True)
    with pytest.raises(ValueError, match="forward only"):
        enc(ids)
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        enc(ids)


def test_a_parameter_outside_the_tail_that_requires_grad_is_named():
    ids = torch.zeros(2, 5, dtype=torch.int64)
    for name in ("encoder.layer.0.intermediate.dense.weight", "encoder.layer.0.attention.self.key.bias", "embeddings.position_embeddings.weight",
                 "embeddings.LayerNorm.bias", "pooler.dense.weight"):
        enc = bert.BertEncoder(TINY, finetune_layers=1)
        enc.get_parameter(name).requires_grad_(True)
        with pytest.raises(ValueError, match=name.replace(".", r"\.")):
            enc(ids)
        with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):      # without grad the call goes on to the device check
            enc(ids)
    enc = bert.BertEncoder(TINY, finetune_layers=1)
    enc.embeddings.word_embeddings.weight.requires_grad_(True)
    with pytest.raises(ValueError, match="an embedding parameter"):
        enc(ids)
    with pytest.raises(RuntimeError, match="no CPU fallback"):                            # a well-formed tail goes on to the device check
        bert.BertEncoder(TINY, finetune_layers=2)(ids)


def test_packed_operands_are_cached_per_layer():
    """an in-place step on one layer's parameter repacks that layer alone; any changed parameter is noticed"""
    enc = bert.BertEncoder({**TINY, "num_hidden_layers": 3}, compute_dtype="fp32", finetune_layers=1)
    first = enc._operands()
    assert enc._operands() is first                                       # built once
    with torch.no_grad():
        enc.encoder.layer[2].intermediate.dense.bias.add_(1.0)
    second = enc._operands()
    assert second is not first and second["emb"] is first["emb"]
    assert second["layers"][0] is first["layers"][0] and second["layers"][1] is first["layers"][1] and second["layers"][2] is not first["layers"][2]
    assert torch.equal(second["layers"][2]["bi"], first["layers"][2]["bi"] + 1.0) and second["layers"][2]["wi"].data_ptr() != first["layers"][2]["wi"].data_ptr()
    before = second["emb"][3].clone()                                     # (an fp32 table is packed as the parameter itself, not a copy)
    with torch.no_grad():
        enc.embeddings.LayerNorm.weight.mul_(2.0)
    third = enc._operands()
    assert third["emb"] is not second["emb"] and all(a is b for a, b in zip(third["layers"], second["layers"]))
    assert torch.equal(third["emb"][3], 2.0 * before)
    enc.encoder.layer[0].attention.output.dense.weight.data = enc.encoder.layer[0].attention.output.dense.weight.data.clone()       # a replaced storage
    fourth = enc._operands()
    assert fourth["layers"][0] is not third["layers"][0] and fourth["layers"][1] is third["layers"][1] and fourth["emb"] is third["emb"]
    assert enc._operands() is fourth
