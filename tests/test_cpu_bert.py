"""The BERT trunk without a GPU: the fifth companion header (include/mmdeer_bert.h) through the strict parser, its layout against
the compiler, its symbols in the built library, every refusal of the four new C entry points (all decided on the host), the float64
restatement (tests/bert_ref.py) against the capture from transformers.BertModel (tests/golden/bert_tiny.npz) and against a live
BertModel, and what BertEncoder / TemporalTextEncoder(bert=...) promise before any launch."""
import ctypes as C
import functools
import json
import os
import subprocess
import types

import numpy as np
import pytest
import torch

from mmdeer import _header, _lib, bert, build, text

from . import bert_ref as R
from .test_cpu_frame_backward import BWD_SYMBOLS
from .test_cpu_frame_encoder import NEW_SYMBOLS as FRAME_SYMBOLS

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "bert_tiny.npz")
NAMES = os.path.join(HERE, "golden", "bert_state_dict_names.json")
TINY = dict(vocab_size=64, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, max_position_embeddings=48,
            type_vocab_size=2)
BERT_SYMBOLS = {"mmdeer_bert_embed_fwd": 1, "mmdeer_bert_attn_fwd": 1, "mmdeer_bert_add_ln_fwd": 1, "mmdeer_bert_gelu_fwd": 1}
# float64 against float64: the largest difference measured between the restatement and the capture is 1.1e-14 (layer 1's output,
# values of rms 1.05), and 1.3e-14 against the live model below; the bound is ten times the larger, rounded up
F64_TOL = 2e-13


@functools.lru_cache(maxsize=None)
def golden():
    """(state dict in float64 with a zero pooler, ids, mask, types, [hidden states]) of the capture: loaded once, shared, left unchanged"""
    g = np.load(GOLDEN)
    sd = {k[2:]: torch.from_numpy(g[k].view(np.int16).copy()).view(torch.bfloat16).double() for k in g.files if k.startswith("w.")}
    sd["pooler.dense.weight"], sd["pooler.dense.bias"] = torch.zeros(128, 128, dtype=torch.float64), torch.zeros(128, dtype=torch.float64)
    ids, mask, typ = (torch.from_numpy(g[k].astype(np.int64)) for k in ("ids", "mask", "types"))
    return sd, ids, mask, typ, [torch.from_numpy(g[f"hidden.{i}"]) for i in range(3)]


def names():
    with open(NAMES) as f:
        return json.load(f)


# ------------------------------------------------------------------------------------------------ the fixture and the restatement
def test_fixture_is_small_and_complete():
    assert os.path.getsize(GOLDEN) < 688 * 1024
    sd, ids, mask, typ, hidden = golden()
    assert set(sd) == set(names()) and len(names()) == 5 + 16 * 2 + 2
    assert ids.shape == mask.shape == typ.shape == (4, 37) and all(h.shape == (4, 37, 128) and h.dtype == torch.float64 for h in hidden)
    assert mask[0].all() and mask[1, :23].all() and not mask[1, 23:].any() and int(mask[2].sum()) == 1 and not mask[3, 2::3].any() and mask[3, 0::3].all()
    assert int(ids.min()) == 0 and int(ids.max()) == 63 and set(typ.unique().tolist()) == {0, 1}
    for k, v in sd.items():                                   # every weight exact in bf16; LayerNorms non-trivial
        assert torch.equal(v.float().bfloat16().double(), v), k
    assert float(sd["encoder.layer.1.output.LayerNorm.weight"].std()) > 0.2 and float(sd["embeddings.LayerNorm.bias"].abs().max()) > 0.2


def test_restatement_reproduces_the_capture_layer_by_layer():
    sd, ids, mask, typ, hidden = golden()
    got = R.trunk(sd, ids, mask, typ)
    assert len(got) == len(hidden)
    for i, (a, b) in enumerate(zip(got, hidden)):
        d = float((a - b).abs().max())
        print(f"hidden state {i}: max |restatement - capture| = {d:.3g}")
        assert d <= F64_TOL, (i, d)
    # attention in the fixture is far from uniform: the mean largest probability of layer 0, head 0, sample 0 is above 1/2 (37 keys)
    x = hidden[0][0]
    q, k = (x @ sd[f"encoder.layer.0.attention.self.{n}.weight"].T + sd[f"encoder.layer.0.attention.self.{n}.bias"] for n in ("query", "key"))
    assert float(torch.softmax(q[:, :64] @ k[:, :64].T / 8, -1).max(-1).values.mean()) > 0.5


def test_restatement_equals_a_live_bert_model():
    """a second geometry (one head, three layers, an intermediate size that is no multiple of 64, three token types) at
    L = max_position_embeddings, arbitrary binary masks; every sample has a valid key, where the two agree"""
    transformers = pytest.importorskip("transformers")
    cfg = transformers.BertConfig(vocab_size=50, hidden_size=64, num_hidden_layers=3, num_attention_heads=1, intermediate_size=72,
                                  max_position_embeddings=16, type_vocab_size=3, attn_implementation="eager")
    model = transformers.BertModel(cfg).double().eval()
    gen = torch.Generator().manual_seed(5)
    sd = {k: (0.5 + torch.rand(v.shape, generator=gen, dtype=torch.float64) if k.endswith("LayerNorm.weight")
              else torch.randn(v.shape, generator=gen, dtype=torch.float64) * (0.3 if v.dim() == 1 or "embeddings" in k else 0.25))
          for k, v in model.state_dict().items()}
    model.load_state_dict(sd, strict=True)
    ids = torch.randint(0, 50, (3, 16), generator=gen)
    typ = torch.randint(0, 3, (3, 16), generator=gen)
    mask = torch.ones(3, 16, dtype=torch.int64)
    mask[1, 9:] = 0
    mask[2, ::2] = 0
    with torch.no_grad():
        out = model(input_ids=ids, attention_mask=mask, token_type_ids=typ, output_hidden_states=True)
        plain = model(input_ids=ids[:1], attention_mask=mask[:1])              # the reference's call: no token types
    got = R.trunk(sd, ids, mask, typ)
    for i, (a, b) in enumerate(zip(got, out.hidden_states)):
        assert float((a - b).abs().max()) <= F64_TOL, i
    assert float((R.trunk(sd, ids[:1], mask[:1])[-1] - plain.last_hidden_state).abs().max()) <= F64_TOL
    assert list(sd) == list(bert.BertEncoder(cfg).state_dict())                   # a BertConfig object is a config too


def test_restatement_operators():
    torch.manual_seed(2)
    x, y = torch.randn(5, 128, dtype=torch.float64), torch.randn(5, 128, dtype=torch.float64)
    g, b = torch.rand(128, dtype=torch.float64) + 0.5, torch.randn(128, dtype=torch.float64)
    torch.testing.assert_close(R.add_ln(y, x, g, b, 1e-12), torch.nn.functional.layer_norm(x + y, (128,), g, b, 1e-12), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(R.gelu(x), torch.nn.functional.gelu(x), rtol=1e-13, atol=1e-13)
    grid = torch.tensor([0.75, -0.75, 3.0], dtype=torch.float64)
    assert 1e-4 < float((R.gelu(grid) - R.gelu_tanh(grid)).abs().max()) < 1e-3      # the distance a 1e-6 bound must tell apart
    # a row of variance 1e-6: eps = 1e-5 instead of 1e-12 changes it by a factor of about 3.3
    row = 2.0 + 1e-3 * torch.randn(1, 128, dtype=torch.float64)
    a12, a5 = R.layer_norm(row, g, torch.zeros_like(b), 1e-12), R.layer_norm(row, g, torch.zeros_like(b), 1e-5)
    assert 2.5 < float(a12.abs().max() / a5.abs().max()) < 4.0
    # the fully masked sample: zeros, and its neighbour as if alone; clamped ids
    qkv = torch.randn(2 * 7, 3 * 128, dtype=torch.float64)
    mask = torch.cat([torch.zeros(7), torch.tensor([1., 0, 1, 1, 0, 0, 1])]).double()
    ctx = R.attention(qkv, mask, 2, 7, 128)
    assert torch.equal(ctx[:7], torch.zeros(7, 128, dtype=torch.float64)) and torch.isfinite(ctx).all()
    torch.testing.assert_close(ctx[7:], R.attention(qkv[7:], mask[7:], 1, 7, 128), rtol=1e-13, atol=1e-13)   # (batched and single matmuls round apart)
    word, pos, typ = torch.randn(9, 64, dtype=torch.float64), torch.randn(4, 64, dtype=torch.float64), torch.randn(2, 64, dtype=torch.float64)
    e = R.embed_ln(word, pos, typ, g[:64], b[:64], 1e-12, torch.tensor([[-3, 0, 8, 99]]))
    assert torch.equal(e[0, 0], R.embed_ln(word, pos, typ, g[:64], b[:64], 1e-12, torch.tensor([[0]]))[0, 0])
    assert torch.equal(e[0, 3], R.layer_norm(word[8] + typ[0] + pos[3], g[:64], b[:64], 1e-12))


# ------------------------------------------------------------------------------------------------ the C ABI additions
def test_new_symbols_are_declared_bound_and_exported():
    lib = _lib.load()
    assert {n: len(args) for n, _, args in _lib.BERT_SYMBOLS} == BERT_SYMBOLS
    for name, res, args in _lib.BERT_SYMBOLS:
        fn = getattr(lib, name)                                           # exported by the built library
        assert fn.restype is C.c_int32 and fn.argtypes == args, name
    assert set(_lib.BERT_STRUCTS) == {"bert_embed_args", "bert_attn_args", "bert_add_ln_args", "bert_gelu_args"}
    for name, cls in _lib.BERT_STRUCTS.items():                           # the ctypes mirrors against the compiler's layout
        assert lib.mmdeer_sizeof(name.encode()) == C.sizeof(cls), name
    assert _lib.BERT_CONSTANTS == {"BERT_HEAD_DIM": 64, "BERT_MAX_HIDDEN": 1024, "BERT_MAX_TOKENS": 512}
    # the four older companion tables and mmdeer.h's are as they were: additions only, in a table of their own
    assert {n: len(args) for n, _, args in _lib.FRAME_BWD_SYMBOLS} == BWD_SYMBOLS and {n: len(args) for n, _, args in _lib.FRAME_SYMBOLS} == FRAME_SYMBOLS
    assert set(_lib.FRAME_BWD_STRUCTS) == {"bn2d_bwd_args", "conv2d_wgrad_args", "conv2d_dgrad_args"} and set(_lib.FRAME_STRUCTS) == {"conv2d_args", "bn2d_args"}
    assert set(_lib.VIDEO_STRUCTS) == {"conv3_time_args", "bn_time_args"}
    new = {n for n, _, _ in _lib.BERT_SYMBOLS}
    for older in (_lib.SYMBOLS, _lib.VIDEO_SYMBOLS, _lib.FRAME_SYMBOLS, _lib.ROUTE_SYMBOLS, _lib.FRAME_BWD_SYMBOLS):
        assert not new & {n for n, _, _ in older}
    assert not set(_lib.BERT_STRUCTS) & (set(_lib.STRUCTS) | set(_lib.VIDEO_STRUCTS) | set(_lib.FRAME_STRUCTS) | set(_lib.FRAME_BWD_STRUCTS))
    assert not any(k.startswith("BERT") for k in _lib.CONSTANTS) and "gemm_args" in _lib.STRUCTS
    assert "bert.hip" in build.SOURCES
    assert _header.BERT_HEADER_PATH == build.BERT_HEADER_PATH
    assert os.path.samefile(build.BERT_HEADER_PATH, os.path.join(ROOT, "include", "mmdeer_bert.h"))
    assert lib.mmdeer_abi_version() == _lib.ABI_VERSION == 16            # additions only


def test_header_layout_matches_the_compiler(tmp_path):
    """Offsets and sizes of every field of the four new structs, as ctypes lays them out, asserted by the compiler on the header."""
    lines = ["#include <stddef.h>", '#include "mmdeer_bert.h"']
    for cname, cls in _lib._BERT_CLASSES.items():
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
    src = _header.read(_header.BERT_HEADER_PATH)
    for bad in (src.replace("int mmdeer_bert_attn_fwd(", "int mmdeer_bert_attn_fwd(uint16_t f, "),                  # the same strict parser
                src.replace("#define MMDEER_BERT_MAX_TOKENS 512", "#define MMDEER_BERT_MAX_TOKENS 512\n#if 0\n#endif"),
                src.replace("const float* mask;", "const float* mask; short s;")):
        assert bad != src
        with pytest.raises(_header.HeaderError):
            _header.parse(bad, _lib._BERT_NAMES, {})


A = 1 << 20     # a plausible, aligned address: never dereferenced by the host checks


def _set(a, kw):
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _emb(**kw):
    a = _lib.BertEmbedArgs()
    a.ids, a.type_ids, a.word, a.pos, a.type, a.gamma, a.beta, a.x = (A,) * 8
    a.B, a.L, a.H, a.V, a.P, a.T, a.ld_x, a.act_f32, a.eps = 2, 37, 128, 64, 48, 2, 128, 0, 1e-12
    return _set(a, kw)


def _att(**kw):
    a = _lib.BertAttnArgs()
    a.qkv, a.mask, a.ctx = A, A, A
    a.B, a.L, a.H, a.ld_qkv, a.ld_ctx, a.act_f32 = 2, 37, 128, 384, 128, 0
    return _set(a, kw)


def _aln(**kw):
    a = _lib.BertAddLnArgs()
    a.y, a.x, a.gamma, a.beta, a.out = (A,) * 5
    a.M, a.N, a.ld_y, a.ld_x, a.ld_out, a.act_f32, a.eps = 5, 128, 128, 128, 128, 0, 1e-12
    return _set(a, kw)


def _gel(**kw):
    a = _lib.BertGeluArgs()
    a.x, a.out = A, A
    a.M, a.N, a.ld_x, a.ld_out, a.act_f32 = 5, 256, 256, 256, 0
    return _set(a, kw)


def _refused(f, arg, msg):
    lib = _lib.load()
    assert f(arg) == -1, msg
    assert msg in lib.mmdeer_last_error(), (msg, lib.mmdeer_last_error())


def test_embed_refuses_on_the_host():
    f = _lib.load().mmdeer_bert_embed_fwd
    for kw, msg in [({"H": 96}, b"unsupported H"), ({"H": 0}, b"unsupported H"), ({"H": 1088, "ld_x": 1088}, b"unsupported H"), ({"H": 96, "B": 0}, b"unsupported H"),
                    ({"B": -1}, b"bad shape"), ({"L": -1}, b"bad shape"), ({"V": 0}, b"bad shape"), ({"P": 0}, b"bad shape"), ({"T": 0}, b"bad shape"),
                    ({"L": 49}, b"max_position_embeddings"), ({"L": 49, "B": 0}, b"max_position_embeddings"),
                    ({"ld_x": 124}, b"leading dimension"), ({"ld_x": 130}, b"leading dimension"),
                    ({"eps": -1e-12}, b"eps"), ({"eps": float("nan")}, b"eps"), ({"eps": float("inf")}, b"eps"),
                    ({"B": 1 << 16, "L": 512, "P": 512, "H": 1024, "ld_x": 1024}, b"2^31"),
                    ({"ids": None}, b"NULL"), ({"word": None}, b"NULL"), ({"pos": None}, b"NULL"), ({"type": None}, b"NULL"), ({"gamma": None}, b"NULL"),
                    ({"beta": None}, b"NULL"), ({"x": None}, b"NULL"),
                    ({"ids": A + 4}, b"misaligned"), ({"type_ids": A + 4}, b"misaligned"), ({"word": A + 8}, b"misaligned"), ({"pos": A + 4}, b"misaligned"),
                    ({"type": A + 8}, b"misaligned"), ({"gamma": A + 4}, b"misaligned"), ({"beta": A + 8}, b"misaligned"), ({"x": A + 4}, b"misaligned"),
                    ({"x": A + 8, "act_f32": 1}, b"misaligned")]:
        _refused(f, C.byref(_emb(**kw)), msg)
    assert f(C.byref(_emb(B=0, ids=None, word=None, x=None))) == 0 and f(C.byref(_emb(L=0, ids=None, x=None))) == 0
    assert f(None) == -1


def test_attention_refuses_on_the_host():
    f = _lib.load().mmdeer_bert_attn_fwd
    for kw, msg in [({"H": 96}, b"unsupported H"), ({"H": 32}, b"unsupported H"), ({"H": 1088, "ld_qkv": 3264, "ld_ctx": 1088}, b"unsupported H"),
                    ({"H": 96, "B": 0}, b"unsupported H"), ({"B": -1}, b"bad shape"), ({"L": 0}, b"bad shape"), ({"L": -1, "B": 0}, b"bad shape"),
                    ({"L": 513}, b"tokens"), ({"L": 513, "B": 0}, b"tokens"),
                    ({"ld_qkv": 376}, b"ld_qkv"), ({"ld_qkv": 388}, b"ld_qkv"), ({"ld_ctx": 124}, b"ld_ctx"), ({"ld_ctx": 130}, b"ld_ctx"),
                    ({"B": 1 << 14, "L": 512, "H": 1024, "ld_qkv": 3072, "ld_ctx": 1024}, b"2^31"),
                    ({"qkv": None}, b"NULL"), ({"mask": None}, b"NULL"), ({"ctx": None}, b"NULL"),
                    ({"qkv": A + 8}, b"misaligned"), ({"mask": A + 2}, b"misaligned"), ({"ctx": A + 4}, b"misaligned"), ({"ctx": A + 8, "act_f32": 1}, b"misaligned")]:
        _refused(f, C.byref(_att(**kw)), msg)
    assert f(C.byref(_att(B=0, qkv=None, mask=None, ctx=None))) == 0 and f(C.byref(_att(B=0, L=0, qkv=None))) == 0
    assert f(None) == -1


def test_add_ln_and_gelu_refuse_on_the_host():
    lib = _lib.load()
    f = lib.mmdeer_bert_add_ln_fwd
    for kw, msg in [({"N": 126}, b"unsupported N"), ({"N": 0}, b"unsupported N"), ({"N": 1028, "ld_y": 1028, "ld_x": 1028, "ld_out": 1028}, b"unsupported N"),
                    ({"N": 126, "M": 0}, b"unsupported N"), ({"M": -1}, b"bad shape"),
                    ({"ld_y": 124}, b"leading dimension"), ({"ld_x": 130}, b"leading dimension"), ({"ld_out": 64}, b"leading dimension"),
                    ({"eps": -1.0}, b"eps"), ({"eps": float("nan")}, b"eps"),
                    ({"M": 1 << 21, "N": 1024, "ld_y": 1024, "ld_x": 1024, "ld_out": 1024}, b"2^31"),
                    ({"y": None}, b"NULL"), ({"gamma": None}, b"NULL"), ({"beta": None}, b"NULL"), ({"out": None}, b"NULL"),
                    ({"y": A + 4}, b"misaligned"), ({"x": A + 2}, b"misaligned"), ({"out": A + 4}, b"misaligned"), ({"gamma": A + 4}, b"misaligned"),
                    ({"beta": A + 8}, b"misaligned"), ({"y": A + 8, "act_f32": 1}, b"misaligned")]:
        _refused(f, C.byref(_aln(**kw)), msg)
    assert f(C.byref(_aln(M=0, y=None, out=None, gamma=None))) == 0
    assert f(C.byref(_aln(x=None, ld_x=0, M=0))) == 0                      # no residual: its leading dimension is not looked at
    assert f(None) == -1
    f = lib.mmdeer_bert_gelu_fwd
    for kw, msg in [({"N": 254}, b"unsupported N"), ({"N": 0}, b"unsupported N"), ({"N": 254, "M": 0}, b"unsupported N"), ({"M": -1}, b"bad shape"),
                    ({"ld_x": 252}, b"leading dimension"), ({"ld_out": 258}, b"leading dimension"),
                    ({"M": 1 << 20, "N": 2048, "ld_x": 2048, "ld_out": 2048}, b"2^31"),
                    ({"x": None}, b"NULL"), ({"out": None}, b"NULL"), ({"x": A + 4}, b"misaligned"), ({"out": A + 2}, b"misaligned"),
                    ({"out": A + 8, "act_f32": 1}, b"misaligned")]:
        _refused(f, C.byref(_gel(**kw)), msg)
    assert f(C.byref(_gel(M=0, x=None, out=None))) == 0
    assert f(None) == -1


# ------------------------------------------------------------------------------------------------ BertEncoder before any launch
def test_bert_encoder_state_dict_is_bert_models():
    enc = bert.BertEncoder(TINY)
    assert list(enc.state_dict()) == names()
    sd = golden()[0]
    assert {k: tuple(v.shape) for k, v in enc.state_dict().items()} == {k: tuple(v.shape) for k, v in sd.items()}
    enc.load_state_dict({k: v.float() for k, v in sd.items()}, strict=True)
    assert not any(p.requires_grad for p in enc.parameters()) and enc.compute_dtype == "bf16"
    nopool = bert.BertEncoder({**TINY, "add_pooling_layer": False})
    assert list(nopool.state_dict()) == [k for k in names() if not k.startswith("pooler.")]
    d = bert.BertEncoder({"num_hidden_layers": 1}).config                 # the defaults are bert-base-uncased's
    assert (d["vocab_size"], d["hidden_size"], d["num_attention_heads"], d["intermediate_size"], d["max_position_embeddings"], d["type_vocab_size"],
            d["layer_norm_eps"], d["hidden_act"]) == (30522, 768, 12, 3072, 512, 2, 1e-12, "gelu")
    obj = types.SimpleNamespace(**TINY, layer_norm_eps=1e-7, hidden_act="gelu")                     # any object with the attribute names
    assert bert.BertEncoder(obj).eps == 1e-7 and list(bert.BertEncoder(obj).state_dict()) == names()


def test_bert_encoder_initialisation_is_transformers():
    torch.manual_seed(0)
    enc = bert.BertEncoder({**TINY, "vocab_size": 2000})
    sd = enc.state_dict()
    for k, v in sd.items():
        if "LayerNorm.weight" in k:
            assert torch.equal(v, torch.ones_like(v)), k
        elif k.endswith(".bias"):
            assert torch.equal(v, torch.zeros_like(v)), k
        else:
            assert 0.018 < float(v.std()) < 0.022 and abs(float(v.mean())) < 2e-3, k      # normal(0, initializer_range = 0.02)
    assert torch.equal(sd["embeddings.word_embeddings.weight"][0], torch.zeros(128))     # the padding row


def test_bert_encoder_refuses_what_is_not_built():
    for cfg, msg in [({"hidden_size": 128, "num_attention_heads": 4}, "64 \\* num_attention_heads"), ({"hidden_size": 96, "num_attention_heads": 2}, "64 \\* num_attention_heads"),
                     ({"hidden_size": 1088, "num_attention_heads": 17}, "outside 64 .. 1024"), ({"hidden_act": "gelu_new"}, "hidden_act"), ({"hidden_act": "relu"}, "hidden_act"),
                     ({"position_embedding_type": "relative_key"}, "position_embedding_type"), ({"intermediate_size": 100}, "multiple of 8")]:
        with pytest.raises(NotImplementedError, match=msg):
            bert.BertEncoder({**TINY, **cfg})
    with pytest.raises(ValueError, match="unknown config keys"):
        bert.BertEncoder({**TINY, "hidden": 128})
    with pytest.raises(ValueError, match="compute must be"):
        bert.BertEncoder(TINY, compute_dtype="fp16")


def test_bert_encoder_is_forward_only_and_has_no_cpu_path():
    enc = bert.BertEncoder(TINY)
    ids = torch.zeros(2, 5, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        enc(ids)
    with pytest.raises(ValueError, match="max_position_embeddings"):
        enc(torch.zeros(2, 49, dtype=torch.int64))
    with pytest.raises(ValueError, match="integer"):
        enc(torch.zeros(2, 5))
    with pytest.raises(ValueError, match="shape"):
        enc(ids, torch.ones(2, 4))
    enc.encoder.layer[1].output.dense.weight.requires_grad_(True)
    with pytest.raises(ValueError, match="forward only"):
        enc(ids)
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):      # without grad the call goes on to the device check
        enc(ids)


# ------------------------------------------------------------------------------------------------ TemporalTextEncoder with a trunk
def test_text_encoder_with_a_trunk_has_the_references_keys():
    with open(os.path.join(HERE, "golden", "text_state_dict_names.json")) as f:
        plain_shapes = json.load(f)                                        # name -> shape, of the reference's no-BERT configuration
    plain = text.TemporalTextEncoder()
    assert {k: list(v.shape) for k, v in plain.state_dict().items()} == plain_shapes and len(plain_shapes) == 14 and plain.bert is None   # unchanged
    plain_names = list(plain.state_dict())
    trunk = bert.BertEncoder({"num_hidden_layers": 1, "vocab_size": 100, "max_position_embeddings": 32})
    enc = text.TemporalTextEncoder({"hidden_dim": 512}, "bf16", bert=trunk)
    tail = [k for k in plain_names if not k.startswith(("embedding.", "positional_encoding."))]
    assert len(tail) == 12
    assert list(enc.state_dict()) == ["bert." + k for k in trunk.state_dict()] + tail
    assert enc.bert is trunk and not hasattr(enc, "embedding") and not hasattr(enc, "positional_encoding")
    assert {n for n, p in enc.named_parameters() if p.requires_grad} == set(tail)
    with pytest.raises(ValueError, match="hidden_size 768"):
        text.TemporalTextEncoder(bert=bert.BertEncoder(TINY))
    with pytest.raises(TypeError):
        text.TemporalTextEncoder(bert=torch.nn.Linear(2, 2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        enc(torch.zeros(2, 5, dtype=torch.int64), torch.ones(2, 5))
