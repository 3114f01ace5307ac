"""The temporal text encoder without a GPU: the float64 restatement (tests/text_ref.py) against the vectors captured from the
reference (tests/golden/text_seq.npz), the state_dict contract, and every refusal of the new C entry points and of the module
that is decided on the host."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from mmdeer import _lib, synth, text

from . import text_ref as R
from .test_oracle_golden import check_side_grads

HERE = os.path.dirname(__file__)
GOLDEN = os.path.join(HERE, "golden", "text_seq.npz")
NAMES = json.load(open(os.path.join(HERE, "golden", "text_state_dict_names.json")))
CASES = [(9, 2), (5, 7), (3, 130)]


def _state(tag):
    return {k: torch.from_numpy(v).double() for k, v in synth.module_fill(tag, {k: tuple(s) for k, s in NAMES.items()}).items()}


def embeddings(i, B, L):
    """The closed-form contextual embeddings of case i (tests/golden/make_golden_text.py: embeddings)."""
    return synth.normal(760 + i, B * L * 768).reshape(B, L, 768).astype(np.float32)


def check_embedding_rows(g, tag, grad):
    """embedding.weight's gradient against the capture: the touched rows (whole or by their l2 norms), the norm of all of it,
    and exact zeros everywhere else (row 0, the padding row, among them)."""
    grad = grad.detach().double().cpu()
    idx = torch.from_numpy(g[f"{tag}.emb_ids"])
    assert 0 not in idx.tolist()
    if f"{tag}.emb_rows" in g:
        ref = g[f"{tag}.emb_rows"]
        np.testing.assert_allclose(grad[idx].numpy(), ref, rtol=3e-3, atol=3e-3 * float(np.abs(ref).max()))
    else:
        np.testing.assert_allclose(grad[idx].norm(dim=1).numpy(), g[f"{tag}.emb_rownorm"], rtol=3e-3)
    assert float(grad.norm()) == pytest.approx(float(g[f"{tag}.embnorm"]), rel=3e-3)
    rest = torch.ones(grad.shape[0], dtype=torch.bool)
    rest[idx] = False
    assert not bool(grad[rest].any())


@pytest.mark.parametrize("i", range(len(CASES)))
def test_restatement_reproduces_the_reference_capture(i):
    B, L = CASES[i]
    g = np.load(GOLDEN)
    tag = f"txt{B}x{L}"
    mask = torch.from_numpy(g[f"{tag}.mask"])
    w = torch.from_numpy(g[f"{tag}.loss_w"]).double()
    # forward(ids, mask)
    P = {k: v.requires_grad_(True) for k, v in _state(tag).items()}
    y, a, f = R.encoder(P, torch.from_numpy(g[f"{tag}.ids"]), mask)
    np.testing.assert_allclose(y.detach().numpy(), g[f"{tag}.out"], rtol=1e-4, atol=5e-6)
    np.testing.assert_allclose(a.detach().numpy(), g[f"{tag}.attn"], rtol=1e-4, atol=5e-6)
    np.testing.assert_allclose(f.numpy(), g[f"{tag}.ling"], rtol=1e-6, atol=0)
    (y * w).sum().backward()
    check_side_grads(g, tag, {k: v.grad for k, v in P.items()}, {}, rtol=3e-4, atol_frac=3e-5)
    check_embedding_rows(g, tag, P["embedding.weight"].grad)
    # b2 shifts every score equally: its exact gradient is zero, the reference's value is rounding noise
    assert abs(float(P["token_attention.2.bias"].grad)) <= 1e-12
    assert abs(float(g[f"{tag}.gradnoise.token_attention.2.bias"].reshape(-1)[0])) <= 1e-4 * float(np.abs(g[f"{tag}.grad.token_attention.2.weight"]).max())
    # forward_embeddings(E, ids, mask)
    te = tag + "e"
    P = {k: v.requires_grad_(True) for k, v in _state(tag).items()}
    E = torch.from_numpy(embeddings(i, B, L)).double().requires_grad_(True)
    y, a, f = R.encoder_embeddings(P, E, torch.from_numpy(g[f"{te}.ids"]), mask)
    np.testing.assert_allclose(y.detach().numpy(), g[f"{te}.out"], rtol=1e-4, atol=5e-6)
    np.testing.assert_allclose(a.detach().numpy(), g[f"{te}.attn"], rtol=1e-4, atol=5e-6)
    np.testing.assert_allclose(f.numpy(), g[f"{te}.ling"], rtol=1e-6, atol=0)
    (y * w).sum().backward()
    check_side_grads(g, te, {k: v.grad for k, v in P.items()}, {}, rtol=3e-4, atol_frac=3e-5)
    check_dE(g, te, E.grad, rtol=3e-4, atol_frac=3e-5)


def check_dE(g, te, dE, rtol, atol_frac):
    v = dE.detach().double().cpu()
    if f"{te}.dE" in g:
        ref = g[f"{te}.dE"]
        np.testing.assert_allclose(v.numpy(), ref, rtol=rtol, atol=atol_frac * float(np.abs(ref).max()))
    else:
        v = v.reshape(-1)
        assert float(v.norm()) == pytest.approx(float(g[f"{te}.dEnorm"]), rel=rtol)
        ref = g[f"{te}.dEsample"]
        idx = torch.linspace(0, v.numel() - 1, 1024).round().long()
        np.testing.assert_allclose(v[idx].numpy(), ref, rtol=rtol, atol=atol_frac * float(np.abs(ref).max()))


def test_restatement_table_gradients_equal_autograd():
    torch.manual_seed(0)
    ids = torch.randint(-3, 60, (4, 9))
    mask = (torch.rand(4, 9) < 0.7).long()
    emb, pos = torch.randn(50, 8, dtype=torch.float64, requires_grad=True), torch.randn(5, 8, dtype=torch.float64, requires_grad=True)
    dx = torch.randn(4, 9, 8, dtype=torch.float64)
    (R.gather(ids, mask, emb, pos) * dx).sum().backward()
    d_emb, d_pos = R.table_grads(ids, mask, dx, 50, 5)
    torch.testing.assert_close(emb.grad, d_emb, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(pos.grad, d_pos, rtol=1e-12, atol=1e-12)


def test_state_dict_matches_the_reference():
    m = text.TemporalTextEncoder()
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == NAMES
    assert list(m.state_dict().keys()) == list(NAMES.keys())
    m.load_state_dict({k: torch.zeros(s) for k, s in NAMES.items()}, strict=True)
    from compat import encoders
    assert encoders.EnhancedTextEncoder is text.TemporalTextEncoder


A = 1 << 20     # a plausible, aligned address: never dereferenced by the host checks


def _embed(tables=True, **kw):
    a = _lib.TokenEmbedArgs()
    a.mask, a.x, a.ld_x, a.dx, a.ld_dx = A, A, 768, A, 768
    if tables:
        a.ids, a.emb, a.pos, a.V, a.P, a.ids32, a.d_emb, a.d_pos, a.scratch, a.scratch_bytes = A, A, A, 30000, 128, A, A, A, A, 1 << 30
    else:
        a.src, a.ld_src, a.d_src, a.ld_dsrc = A, 768, A, 768
    a.B, a.L, a.width, a.act_f32 = 8, 4, 768, 0
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _pool(**kw):
    a = _lib.TokenPoolArgs()
    a.x, a.ld_x, a.z, a.ld_z, a.mask, a.w2, a.b2, a.attended, a.ld_att, a.weights, a.probs = A, 768, A, 384, A, A, A, A, 768, A, A
    a.dout, a.ld_dout, a.dx, a.ld_dx, a.dz, a.ld_dz, a.dw2, a.db2, a.scratch = A, 768, A, 768, A, 384, A, A, A
    a.B, a.L, a.width, a.att_width, a.act_f32 = 8, 4, 768, 384, 0
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _stats(**kw):
    a = _lib.TokenStatsArgs()
    a.ids, a.mask, a.out, a.ld_out, a.B, a.L, a.max_length = A, A, A, 16, 8, 4, 128
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _refuses(f, args, msg):
    lib = _lib.load()
    assert f(C.byref(args)) != 0, msg
    assert msg in lib.mmdeer_last_error(), (msg, lib.mmdeer_last_error())


@pytest.mark.parametrize("op", ["mmdeer_token_embed_fwd", "mmdeer_token_embed_bwd"])
def test_gather_operators_refuse_on_the_host(op):
    f = getattr(_lib.load(), op)
    bwd = op.endswith("bwd")
    act, ld = ("dx", "ld_dx") if bwd else ("x", "ld_x")
    for tables in (True, False):
        _refuses(f, _embed(tables, width=512), b"width")
        _refuses(f, _embed(tables, mask=None), b"NULL")
        _refuses(f, _embed(tables, **{act: None}), b"NULL")
        _refuses(f, _embed(tables, **{act: A + 8}), b"misaligned")
        _refuses(f, _embed(tables, **{ld: 772}), b"misaligned")
        _refuses(f, _embed(tables, **{ld: 760}), b"leading")
        _refuses(f, _embed(tables, B=-1), b"bad shape")
        _refuses(f, _embed(tables, L=-1), b"bad shape")
        for kw in ({"B": 0}, {"L": 0}):
            assert f(C.byref(_embed(tables, mask=None, x=None, dx=None, **kw))) == 0
    _refuses(f, _embed(True, **{"d_pos" if bwd else "pos": None}), b"NULL")
    _refuses(f, _embed(True, **{"d_emb" if bwd else "emb": A + 4}), b"misaligned")
    _refuses(f, _embed(True, V=1 << 24), b"V")
    _refuses(f, _embed(True, **{"d_src" if bwd else "src": A}), b"not both")
    _refuses(f, _embed(False, **{"d_src" if bwd else "src": A + 4}), b"misaligned")
    _refuses(f, _embed(False, **{"ld_dsrc" if bwd else "ld_src": 512}), b"leading")
    if bwd:
        _refuses(f, _embed(True, B=8193, L=128), b"above the limit")             # B * L > 2^20
        _refuses(f, _embed(True, scratch_bytes=64), b"scratch")
        _refuses(f, _embed(True, B=8192, L=128, scratch_bytes=64), b"scratch")   # 2^20 rows pass that check and fail the next
    assert f(None) != 0
    assert _lib.load().mmdeer_token_embed_bwd_scratch(1 << 20) == 2 * 4 * (1 << 20) + _lib.load().mmdeer_sort_pairs_scratch(1 << 20)
    assert _lib.load().mmdeer_token_embed_bwd_scratch((1 << 20) + 1) == 0


@pytest.mark.parametrize("op", ["mmdeer_token_pool_fwd", "mmdeer_token_pool_bwd"])
def test_pool_operators_refuse_on_the_host(op):
    f = getattr(_lib.load(), op)
    bwd = op.endswith("bwd")
    for kw, msg in [({"width": 512}, b"widths"), ({"att_width": 256}, b"widths"), ({"x": None}, b"NULL"), ({"mask": None}, b"NULL"),
                    ({"probs" if bwd else "attended": None}, b"NULL"), ({"dz" if bwd else "b2": None}, b"NULL"),
                    ({"ld_x": 512}, b"leading"), ({"ld_z": 256}, b"leading"), ({"ld_dz" if bwd else "ld_att": 128}, b"leading"),
                    ({"z": A + 8}, b"misaligned"), ({"dx" if bwd else "attended": A + 2}, b"misaligned"), ({"ld_x": 772}, b"misaligned"),
                    ({"weights": A + 1}, b"misaligned"), ({"B": -1}, b"bad shape"), ({"L": -2}, b"bad shape")]:
        _refuses(f, _pool(**kw), msg)
    for kw in ({"B": 0}, {"L": 0}):
        assert f(C.byref(_pool(x=None, z=None, attended=None, dz=None, **kw))) == 0
    assert f(None) != 0


def test_statistics_operator_refuses_on_the_host():
    f = _lib.load().mmdeer_token_stats
    for kw, msg in [({"ids": None}, b"NULL"), ({"out": None}, b"NULL"), ({"mask": A + 2}, b"misaligned"), ({"ld_out": 10}, b"leading"),
                    ({"L": 2049}, b"above the limit"), ({"max_length": 0}, b"max_length"), ({"B": -1}, b"bad shape")]:
        _refuses(f, _stats(**kw), msg)
    for kw in ({"B": 0}, {"L": 0}):
        assert f(C.byref(_stats(ids=None, mask=None, out=None, **kw))) == 0
    assert f(None) != 0


def test_sizeof_of_the_new_structs():
    lib = _lib.load()
    for name, cls in (("token_embed_args", _lib.TokenEmbedArgs), ("token_pool_args", _lib.TokenPoolArgs), ("token_stats_args", _lib.TokenStatsArgs)):
        assert lib.mmdeer_sizeof(name.encode()) == C.sizeof(cls), name
        assert _lib.STRUCTS[name] is cls


def test_module_input_errors():
    m = text.TemporalTextEncoder()
    ids, mask = torch.zeros(2, 5, dtype=torch.long), torch.ones(2, 5, dtype=torch.long)
    with pytest.raises(ValueError):
        m(torch.zeros(2, 0, dtype=torch.long), torch.ones(2, 0, dtype=torch.long))          # L == 0
    with pytest.raises(ValueError):
        m(ids, torch.ones(2, 4, dtype=torch.long))                                          # mismatched shapes
    with pytest.raises(ValueError):
        m(torch.zeros(2, 5, 1, dtype=torch.long), torch.ones(2, 5, 1, dtype=torch.long))
    with pytest.raises(ValueError):
        m(torch.zeros(2, 5), mask)                                                          # floating-point ids
    with pytest.raises(ValueError):
        m.forward_embeddings(torch.zeros(2, 5, 512), ids, mask)                             # wrong last dimension
    with pytest.raises(ValueError):
        m.forward_embeddings(torch.zeros(2, 4, 768), ids, mask)
    with pytest.raises(ValueError):
        m.forward_embeddings(torch.zeros(2, 5, 768, dtype=torch.float16), ids, mask)
    with pytest.raises(RuntimeError):
        m(ids, mask)                                                                        # no CPU fallback
    with pytest.raises(RuntimeError):
        m.forward_embeddings(torch.zeros(2, 5, 768), ids, mask)
    with pytest.raises(NotImplementedError):
        text.TemporalTextEncoder({"hidden_dim": 100})
    with pytest.raises(ValueError):
        text.TemporalTextEncoder(compute_dtype="fp16")
