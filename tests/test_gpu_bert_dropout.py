"""The BERT trunk's dropout (include/mmdeer_bert_drop.h, mmdeer.bert.BertEncoder(dropout=True)) on the GPU: the five new operators
at their edges against float64 with masks drawn on the CPU (tests/bert_drop_ref.py), their exact zeros, canaries, determinism and
p = 0 against the plain entries bit for bit; the module's hidden states and tail gradients against the restatement at a fixed
dropout step; and TemporalTextEncoder(bert=trunk) training with the trunk's dropout on.

Bounds: those of the no-dropout tests of the same operators, imported.  fp32: rtol 1e-3, atol 2e-5 of the float64 tensor's largest
element.  bf16: BF16_RMS / BF16_MAX times the distance from float64 of the restatement with storage rounding only -- for a single
operator the rounded output (test_gpu_bert.check), for the module the restatement run with rnd = bf16_round on the same case and
masks (computed here, once per model).  One bound is reasoned here and not imported: dy = ds o m of the add + LN backward is held on
ds's scale (check_dy has the reasoning)."""
import ctypes as C
import functools
import math

import pytest
import torch

from mmdeer import _lib, bert, text

from . import bert_drop_ref as RD
from . import bert_ref as R
from .test_cpu_bert import TINY, golden
from .test_cpu_bert_backward import upstream
from .test_gpu_bert import BF16_MAX, BF16_RMS, BIG, FP32, big_model, check, dist, dtype_of, ln_params, masks_for
from .test_gpu_bert_backward import attention_bwd_case, check_grad, close_fp32, key_bias_fp32

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED, STEP = 2 ** 40 + 7, 2 ** 33 + 1            # both halves of the 64-bit seed and offset take part in the key
SITE = bert.site(3, 0)


def drop(a, site, p, step=STEP, seed=SEED):
    a.site, a.dropout_p, a.seed, a.offset = site, p, seed, step
    return a


# ------------------------------------------------------------------------------------------------ attention
def run_attention_drop(qkv, mask, B, L, H, compute, p, site=SITE, step=STEP, pad=8, extra_rows=3):
    """qkv (B * L, ld) on the device -> ctx (B * L, H) of a padded, canaried destination; two runs, bit-equal"""
    ld_ctx = H + pad
    runs = []
    for _ in range(2):
        buf = torch.full((B * L + extra_rows, ld_ctx), 777.0, dtype=qkv.dtype, device=DEV)
        a = drop(_lib.BertAttnDropArgs(), site, p, step)
        a.qkv, a.mask, a.ctx = qkv.data_ptr(), mask.data_ptr(), buf.data_ptr()
        a.B, a.L, a.H, a.ld_qkv, a.ld_ctx, a.act_f32, a.stream = B, L, H, qkv.stride(0), ld_ctx, int(compute == "fp32"), _lib.current_stream()
        _lib.check(_lib.load().mmdeer_bert_attn_drop_fwd(C.byref(a)))
        torch.cuda.synchronize()
        assert bool((buf[B * L:] == 777.0).all()) and bool((buf[:, H:] == 777.0).all()), "the canary behind ctx was written"
        runs.append(buf)
    assert torch.equal(runs[0], runs[1]), "two runs of mmdeer_bert_attn_drop_fwd differ"
    return runs[0][:B * L, :H]


def run_attention_drop_bwd(qkv, mask, dctx, B, L, H, compute, p, site=SITE, step=STEP, pad=8, extra_rows=3):
    """operands on the device -> dqkv (B * L, 3 H) of a padded, canaried destination; two runs, bit-equal"""
    lib = _lib.load()
    ld = 3 * H + pad
    nbytes = lib.mmdeer_bert_attn_drop_bwd_workspace(B, L, H)
    assert nbytes == 2 * B * (H // 64) * L * 4
    ws = torch.full((nbytes // 4 + 8,), 555.0, device=DEV)
    runs = []
    for _ in range(2):
        buf = torch.full((B * L + extra_rows, ld), 777.0, dtype=qkv.dtype, device=DEV)
        a = drop(_lib.BertAttnDropBwdArgs(), site, p, step)
        a.qkv, a.mask, a.dctx, a.dqkv = qkv.data_ptr(), mask.data_ptr(), dctx.data_ptr(), buf.data_ptr()
        a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
        a.B, a.L, a.H, a.ld_qkv, a.ld_dctx, a.ld_dqkv = B, L, H, qkv.stride(0), dctx.stride(0), ld
        a.act_f32, a.stream = int(compute == "fp32"), _lib.current_stream()
        _lib.check(lib.mmdeer_bert_attn_drop_bwd(C.byref(a)))
        torch.cuda.synchronize()
        assert bool((buf[B * L:] == 777.0).all()) and bool((buf[:, 3 * H:] == 777.0).all()), "the canary behind dqkv was written"
        assert bool((ws[nbytes // 4:] == 555.0).all()), "the canary behind the workspace was written"
        runs.append(buf)
    assert torch.equal(runs[0], runs[1]), "two runs of mmdeer_bert_attn_drop_bwd differ"
    return runs[0][:B * L, :3 * H]


def attention_drop_check(name, qkv, dctx, mask, B, L, H, compute, p, dead=(), single_key=False):
    """one mask: forward and backward against float64 under the CPU-drawn keep mask, and the zeros that must be exact"""
    heads = H // 64
    m = RD.drop_mask(SITE, B * heads * L, L, p, SEED, STEP)
    m64 = mask.reshape(-1).double()
    dq, dm, dd = qkv.to(DEV), m64.float().to(DEV), dctx.to(DEV)
    ref = RD.attention(qkv.double(), m64, B, L, H, m)
    got = run_attention_drop(dq, dm, B, L, H, compute, p)
    ref_b = RD.attention_bwd(qkv.double(), m64, dctx[:, :H], B, L, H, m)
    got_b = run_attention_drop_bwd(dq, dm, dd, B, L, H, compute, p)
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(got_b).all())
    # a query all of whose valid keys were dropped: ctx = 0 exactly, per (sample, head)
    none_kept = ((m.reshape(B, heads, L, L) != 0) & (mask.reshape(B, 1, 1, L) != 0)).sum(-1) == 0          # (B, heads, L)
    rows = none_kept.permute(0, 2, 1).reshape(B * L, heads, 1).expand(B * L, heads, 64).reshape(B * L, H)
    assert bool((got[rows.to(DEV)] == 0).all()) and bool((ref[rows] == 0).all())
    masked = (m64 == 0).nonzero().flatten()
    assert bool((got_b[masked.to(DEV)][:, H:] == 0).all()) and bool((ref_b[masked][:, H:] == 0).all()), "dK / dV of a masked key must be exact zeros"
    if single_key:                                    # one valid key per live sample: dQ = dK = 0 exactly, kept or dropped
        assert bool((got_b[:, :2 * H] == 0).all()) and float(ref_b[:, :2 * H].abs().max()) < 1e-12
        if not dead and (p == 0.5 or none_kept.numel() >= 100):
            assert 0 < int(none_kept.sum()) < none_kept.numel(), "the case must hold rows of both kinds"
    live = torch.ones(B * L, dtype=torch.bool)
    for b in dead:                                    # a sample without a valid key: exact zeros everywhere
        for g, r in ((got, ref), (got_b, ref_b)):
            assert bool((g[b * L:(b + 1) * L] == 0).all()) and bool((r[b * L:(b + 1) * L] == 0).all())
        live[b * L:(b + 1) * L] = False
    check(f"{name} p={p} ctx", compute, got[live.to(DEV)], ref[live])
    for i, part in enumerate(("dQ", "dK", "dV")):     # each on its own scale
        r = ref_b[live][:, i * H:(i + 1) * H]
        if float(r.abs().max()) > 1e-12:
            check_grad(f"{name} p={p} {part}", compute, got_b[live.to(DEV)][:, i * H:(i + 1) * H], r)
    return none_kept


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("L,heads", [(1, 2), (37, 2), (64, 2), (65, 2), (129, 2), (37, 12)])
def test_attention_dropout_against_float64(L, heads, p, compute):
    B = 2
    H, gen, qkv, dctx = attention_bwd_case(B, L, heads, compute, scale=1.5)
    for name, mask in masks_for(L, gen).items():      # at L = 1 every live sample has one valid key, under 'last' at every L
        attention_drop_check(f"attn_drop L={L} heads={heads} {name}", qkv, dctx, mask, B, L, H, compute, p,
                             dead=(0,) if name == "dead" else (), single_key=name == "last" or L == 1)


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_attention_dropout_at_512_tokens(compute):
    B, L, heads = 1, 512, 2
    H, gen, qkv, dctx = attention_bwd_case(B, L, heads, compute, scale=1.5)
    mask = (torch.rand(1, L, generator=gen) < 0.6).float()
    mask[0, 128:256] = 0                              # a whole key tile (and two whole 64-key workgroups) without a valid key
    mask[0, 500:] = 0
    attention_drop_check("attn_drop L=512", qkv, dctx, mask, B, L, H, compute, 0.1)


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_attention_dropout_p0_is_the_plain_entry_and_steps_differ(compute):
    from .test_gpu_bert import run_attention
    from .test_gpu_bert_backward import run_attention_bwd
    B, L, heads = 2, 65, 2
    H, gen, qkv, dctx = attention_bwd_case(B, L, heads, compute, scale=1.5)
    mask = masks_for(L, gen)["holes"].reshape(-1).to(DEV)
    dq, dd = qkv.to(DEV), dctx.to(DEV)
    assert torch.equal(run_attention_drop(dq, mask, B, L, H, compute, 0.0), run_attention(dq, mask, B, L, H, compute))
    assert torch.equal(run_attention_drop_bwd(dq, mask, dd, B, L, H, compute, 0.0), run_attention_bwd(dq, mask, dd, B, L, H, compute))
    a, b = (run_attention_drop(dq, mask, B, L, H, compute, 0.1, step=s) for s in (4, 5))
    assert not torch.equal(a, b)
    a, b = (run_attention_drop_bwd(dq, mask, dd, B, L, H, compute, 0.1, step=s) for s in (4, 5))
    assert not torch.equal(a, b)
    a, b = (run_attention_drop(dq, mask, B, L, H, compute, 0.1, site=s) for s in (SITE, SITE + 4))
    assert not torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ drop + add + LN
LN_SITE = bert.site(2, 1)


def run_drop_add_ln(y, x, gamma, beta, M, N, compute, p, out=None, ld_out=None, step=STEP):
    dt = y.dtype
    buf = torch.full((M + 2, N + 12), 777.0, dtype=dt, device=DEV) if out is None else out
    a = drop(_lib.BertDropAddLnArgs(), LN_SITE, p, step)
    a.y, a.x, a.gamma, a.beta, a.out, a.eps = y.data_ptr(), _lib.ptr(x), gamma.data_ptr(), beta.data_ptr(), buf.data_ptr(), 1e-12
    a.M, a.N, a.ld_y, a.ld_x, a.ld_out = M, N, y.stride(0), (x.stride(0) if x is not None else 0), (N + 12 if out is None else ld_out)
    a.act_f32, a.stream = int(compute == "fp32"), _lib.current_stream()
    _lib.check(_lib.load().mmdeer_bert_drop_add_ln_fwd(C.byref(a)))
    torch.cuda.synchronize()
    if out is None:
        assert bool((buf[M:] == 777.0).all()) and bool((buf[:, N:] == 777.0).all())
    return buf[:M, :N]


def run_drop_add_ln_bwd(y, x, g, g2, gamma, M, N, compute, sums, p, step=STEP):
    """device operands (padded) -> (ds, dy (M, N), dgamma, dbeta); canaries behind every output, two runs bit-equal"""
    lib = _lib.load()
    runs = []
    for _ in range(2):
        ds = torch.full((M + 2, N + 12), 777.0, dtype=y.dtype, device=DEV)
        dy = torch.full((M + 2, N + 4), 777.0, dtype=y.dtype, device=DEV)
        dgb = torch.full((2, N + 4), 777.0, device=DEV)
        need = lib.mmdeer_bert_drop_add_ln_bwd_scratch(M, N)
        scratch = torch.full((need + 4,), 555.0, device=DEV)
        a = drop(_lib.BertDropAddLnBwdArgs(), LN_SITE, p, step)
        a.y, a.x, a.g, a.g2, a.gamma = y.data_ptr(), _lib.ptr(x), g.data_ptr(), _lib.ptr(g2), gamma.data_ptr()
        a.ds, a.dy, a.ld_ds, a.ld_dy = ds.data_ptr(), dy.data_ptr(), N + 12, N + 4
        if sums:
            a.dgamma, a.dbeta, a.scratch, a.scratch_elems = dgb[0].data_ptr(), dgb[1].data_ptr(), scratch.data_ptr(), need
        a.eps, a.M, a.N, a.ld_y, a.ld_g = 1e-12, M, N, y.stride(0), g.stride(0)
        a.ld_x, a.ld_g2 = (x.stride(0) if x is not None else 0), (g2.stride(0) if g2 is not None else 0)
        a.act_f32, a.stream = int(compute == "fp32"), _lib.current_stream()
        _lib.check(lib.mmdeer_bert_drop_add_ln_bwd(C.byref(a)))
        torch.cuda.synchronize()
        for buf in (ds, dy, dgb):
            assert bool((buf[:, N:] == 777.0).all())
        assert bool((ds[M:] == 777.0).all()) and bool((dy[M:] == 777.0).all()) and bool((scratch[need:] == 555.0).all())
        if not sums:
            assert bool((dgb == 777.0).all()) and bool((scratch == 555.0).all())
        runs.append((ds, dy, dgb))
    assert all(torch.equal(a, b) for a, b in zip(*runs)), "two runs of mmdeer_bert_drop_add_ln_bwd differ"
    return runs[0][0][:M, :N], runs[0][1][:M, :N], runs[0][2][0, :N], runs[0][2][1, :N]


def check_dy(name, compute, dy, ref_dy, ref_ds, mscale):
    """dy = ds o m is a SELECTION of ds's elements, so its error is ds's at those elements times m, and ds's error goes with the
    largest element of its row (a difference of sums over the row), not with the selected element: a row of N = 4 with one kept y and
    no residual has ds = 0 analytically at the kept element (the gradient is orthogonal to xhat and to the constant), and dy is then
    fp32 rounding noise of sums of order max |ds| around a float64 value of 1e-11.  Hence the fp32 bound's atol is taken at
    max |ds| * max m, and the bf16 bound is the usual multiples of dy's own storage-rounding distance plus that fp32 term."""
    top = float(ref_ds.abs().max()) * mscale
    rms, mx = dist(dy, ref_dy)
    if compute == "fp32":
        print(f"{name} fp32: max |hip - float64| = {mx:.3g} at max |ds| max m = {top:.3g}")
        torch.testing.assert_close(dy.double().cpu(), ref_dy.double(), rtol=FP32["rtol"], atol=FP32["atol"] * top)
    else:
        rrms, rmx = dist(R.bf16_round(ref_dy), ref_dy)
        print(f"{name} bf16: hip rms {rms:.3g} max {mx:.3g}; bf16 storage alone rms {rrms:.3g} max {rmx:.3g}; fp32 term {FP32['atol'] * top:.3g}")
        assert rms <= BF16_RMS * rrms + FP32["atol"] * top and mx <= BF16_MAX * rmx + FP32["atol"] * top, (name, rms, rrms, mx, rmx)


def ln_case(M, N, compute):
    gen = torch.Generator().manual_seed(5 * M + N)
    dt = dtype_of(compute)
    y, x = torch.randn(M, N + 4, generator=gen), torch.randn(M, N + 8, generator=gen)
    g, g2 = torch.randn(M, N + 8, generator=gen), torch.randn(M, N + 4, generator=gen)
    gamma, beta = ln_params(N, gen)
    gamma[N // 2] = 0.0
    return tuple(t.to(dt) for t in (y, x, g, g2)) + (gamma, beta)


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("N", [4, 64, 768, 1024])
@pytest.mark.parametrize("M", [1, 5, 67])
def test_drop_add_ln_against_float64(M, N, p, compute):
    y, x, g, g2, gamma, beta = ln_case(M, N, compute)
    m = RD.drop_mask(LN_SITE, M, N, p, SEED, STEP)
    dev = {k: v.to(DEV) for k, v in dict(y=y, x=x, g=g, g2=g2, gamma=gamma, beta=beta).items()}
    g64, b64 = gamma.double(), beta.double()
    for use_x, use_g2, sums in ((True, True, True), (False, False, False), (True, False, True), (False, True, False)):
        name = f"drop_add_ln M={M} N={N} p={p} x={use_x} g2={use_g2}"
        xr, g2r = (x[:, :N].double() if use_x else None), (g2[:, :N].double() if use_g2 else None)
        ref = RD.add_ln(y[:, :N].double(), xr, g64, b64, 1e-12, m)
        out = run_drop_add_ln(dev["y"], dev["x"] if use_x else None, dev["gamma"], dev["beta"], M, N, compute, p)
        check(name, compute, out, ref)
        ref_ds, ref_dy, ref_dg, ref_db = RD.add_ln_bwd(y[:, :N].double(), xr, g[:, :N].double(), g2r, g64, b64, 1e-12, m)
        ds, dy, dg, db = run_drop_add_ln_bwd(dev["y"], dev["x"] if use_x else None, dev["g"], dev["g2"] if use_g2 else None, dev["gamma"], M, N,
                                             compute, sums, p)
        assert bool(torch.isfinite(ds).all()) and bool(torch.isfinite(dy).all())
        check_grad(name + " ds", compute, ds, ref_ds)
        check_dy(name + " dy", compute, dy, ref_dy, ref_ds, float(m.max()))
        dropped = (m == 0).to(DEV)
        assert bool((dy[dropped] == 0).all()) and bool(((dy != 0) | dropped | (ds == 0)).all()), "dy = ds o m: exact zeros where m = 0, and only there"
        if sums:                                      # fp32 sums of fp32 products in both compute dtypes: the fp32 bound
            close_fp32(name + " dgamma", dg, ref_dg)
            close_fp32(name + " dbeta", db, ref_db)
            assert float(ref_dg[N // 2].abs()) > 0 and float(dg[N // 2].abs()) > 0         # xhat is there where gamma = 0
    # out aliasing y: the row is read whole before it is written
    ya = dev["y"].clone()
    got = run_drop_add_ln(ya, dev["x"], dev["gamma"], dev["beta"], M, N, compute, p, out=ya, ld_out=ya.stride(0))
    assert torch.equal(got, run_drop_add_ln(dev["y"], dev["x"], dev["gamma"], dev["beta"], M, N, compute, p)) and torch.equal(ya[:, N:], dev["y"][:, N:])


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_drop_add_ln_p0_is_the_plain_entry_and_steps_differ(compute):
    from .test_gpu_bert_backward import run_add_ln_bwd
    M, N = 67, 768
    y, x, g, g2, gamma, beta = (t.to(DEV) for t in ln_case(M, N, compute))
    plain = torch.full((M + 2, N + 12), 777.0, dtype=y.dtype, device=DEV)
    a = _lib.BertAddLnArgs()
    a.y, a.x, a.gamma, a.beta, a.out, a.eps = y.data_ptr(), x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), plain.data_ptr(), 1e-12
    a.M, a.N, a.ld_y, a.ld_x, a.ld_out, a.act_f32, a.stream = M, N, y.stride(0), x.stride(0), N + 12, int(compute == "fp32"), _lib.current_stream()
    _lib.check(_lib.load().mmdeer_bert_add_ln_fwd(C.byref(a)))
    assert torch.equal(run_drop_add_ln(y, x, gamma, beta, M, N, compute, 0.0), plain[:M, :N])
    ds, dy, dg, db = run_drop_add_ln_bwd(y, x, g, g2, gamma, M, N, compute, True, 0.0)
    pds, pdg, pdb = run_add_ln_bwd(y, x, g, g2, gamma, M, N, compute, True)
    assert torch.equal(ds, pds) and torch.equal(dy, pds) and torch.equal(dg, pdg) and torch.equal(db, pdb)
    a, b = (run_drop_add_ln(y, x, gamma, beta, M, N, compute, 0.1, step=s) for s in (4, 5))
    assert not torch.equal(a, b)
    a, b = (run_drop_add_ln_bwd(y, x, g, g2, gamma, M, N, compute, True, 0.1, step=s) for s in (4, 5))
    assert not torch.equal(a[1], b[1])


# ------------------------------------------------------------------------------------------------ embeddings
@pytest.mark.parametrize("compute", ["fp32", "bf16"])
@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("L", [1, 37])
def test_embed_dropout_on_the_golden_tables(L, p, compute):
    sd, ids, mask, typ, _ = golden()
    ids, typ = ids[:, :L].contiguous(), typ[:, :L].contiguous()
    B, H = ids.shape[0], 128
    e = "embeddings."
    tabs = [sd[e + k] for k in ("word_embeddings.weight", "position_embeddings.weight", "token_type_embeddings.weight", "LayerNorm.weight", "LayerNorm.bias")]
    m = RD.drop_mask(bert.SITE_EMBED, B * L, H, p, SEED, STEP) if p > 0 else None
    ref = RD.embed_ln(*tabs, 1e-12, ids, typ, m).reshape(B * L, H)
    outs = []
    for _ in range(2):
        out = torch.full((B * L + 2, H + 4), 777.0, dtype=dtype_of(compute), device=DEV)
        dev = [t.to(DEV) for t in (ids.reshape(-1), typ.reshape(-1))] + [t.float().to(DEV) for t in tabs]
        a = drop(_lib.BertEmbedDropArgs(), bert.SITE_EMBED, p)
        a.ids, a.type_ids, a.word, a.pos, a.type, a.gamma, a.beta = [t.data_ptr() for t in dev]
        a.x, a.eps, a.B, a.L, a.H, a.V, a.P, a.T, a.ld_x = out.data_ptr(), 1e-12, B, L, H, 64, 48, 2, H + 4
        a.act_f32, a.stream = int(compute == "fp32"), _lib.current_stream()
        _lib.check(_lib.load().mmdeer_bert_embed_drop_fwd(C.byref(a)))
        torch.cuda.synchronize()
        assert bool((out[B * L:] == 777.0).all()) and bool((out[:, H:] == 777.0).all())
        outs.append(out)
    assert torch.equal(outs[0], outs[1])
    got = outs[0][:B * L, :H]
    check(f"embed_drop L={L} p={p}", compute, got, ref)
    if p > 0:
        assert bool((got[(m == 0).to(DEV)] == 0).all()) and 0 < int((m == 0).sum()) < m.numel()
    else:                                             # the plain entry's bits
        plain = torch.full((B * L + 2, H + 4), 777.0, dtype=dtype_of(compute), device=DEV)
        b = _lib.BertEmbedArgs()
        for f, _ in b._fields_:
            setattr(b, f, getattr(a, f))
        b.x = plain.data_ptr()
        _lib.check(_lib.load().mmdeer_bert_embed_fwd(C.byref(b)))
        assert torch.equal(plain, outs[0])


# ------------------------------------------------------------------------------------------------ the module
P_H, P_A, MOD_SEED, MOD_STEP = 0.1, 0.1, 91, 5


def encoder(config, sd, compute, k, dropout=True):
    enc = bert.BertEncoder({**config, "hidden_dropout_prob": P_H, "attention_probs_dropout_prob": P_A}, compute_dtype=compute, finetune_layers=k,
                           dropout=dropout, dropout_seed=MOD_SEED)
    enc.load_state_dict({n: v.float() for n, v in sd.items()}, strict=True)
    return enc.to(DEV)


@functools.lru_cache(maxsize=None)
def module_case(which):
    """(config, state dict, ids, mask, types, upstream, masks, float64 (states, grads), bf16-storage (states, grads)) at B = 2, L = 37:
    computed once per model, shared, left unchanged"""
    if which == "tiny":
        sd, ids, mask, typ, _ = golden()
        config, ids, mask, typ = TINY, ids[:2], mask[:2], typ[:2]
    else:
        sd, ids, mask, _ = big_model()
        config, ids, mask, typ = BIG, ids[:2], mask[:2], None
    H, heads, layers = config["hidden_size"], config["num_attention_heads"], config["num_hidden_layers"]
    masks = RD.draw(RD.sites(2, 37, H, heads, layers, P_H, P_A), MOD_SEED, MOD_STEP)
    up = upstream(mask, H)
    f64 = RD.trunk_grads(sd, ids, mask, typ, up, masks)
    b16 = RD.trunk_grads(sd, ids, mask, typ, up, masks, rnd=R.bf16_round)
    return config, sd, ids, mask, typ, up, masks, f64, b16


def forward_at(enc, step, ids, mask, typ, **kw):
    enc._train_step = step
    return enc(ids.to(DEV), mask.to(DEV), None if typ is None else typ.to(DEV), **kw)


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
@pytest.mark.parametrize("k", [0, 1, 2])
@pytest.mark.parametrize("which", ["tiny", "big"])
def test_module_with_dropout_against_the_restatement(which, k, compute):
    config, sd, ids, mask, typ, up, masks, (states, ref), (states16, ref16) = module_case(which)
    enc = encoder(config, sd, compute, k).train()
    first_tail = config["num_hidden_layers"] - k
    out = forward_at(enc, MOD_STEP, ids, mask, typ, output_hidden_states=True)
    assert enc._train_step == MOD_STEP + 1 and out.last_hidden_state.requires_grad == (k > 0)
    for i, (s, r) in enumerate(zip(out.hidden_states, states)):
        rms, mx = dist(s, r)
        print(f"{which} k={k} {compute} hidden state {i}: rms {rms:.3g} max {mx:.3g}")
        if compute == "fp32":
            torch.testing.assert_close(s.double().cpu(), r, **FP32, msg=lambda msg, i=i: f"hidden state {i}: {msg}")
    if compute == "bf16":
        rms, mx = dist(out.last_hidden_state, states[-1])
        rrms, rmx = dist(states16[-1], states[-1])
        print(f"{which} k={k} bf16 last hidden state: hip rms {rms:.3g} max {mx:.3g}; bf16 storage alone rms {rrms:.3g} max {rmx:.3g}")
        assert rms <= BF16_RMS * rrms and mx <= BF16_MAX * rmx
    with torch.no_grad():                             # the frozen path under no_grad runs the same sites: the same bits
        assert torch.equal(forward_at(enc, MOD_STEP, ids, mask, typ).last_hidden_state, out.last_hidden_state)
    if k == 0:
        return
    (out.last_hidden_state.float() * up.float().to(DEV)).sum().backward()
    torch.cuda.synchronize()
    failures = []
    for n, p in enc.named_parameters():
        in_tail = n.startswith("encoder.layer.") and int(n.split(".")[2]) >= first_tail
        assert p.requires_grad == in_tail
        if not in_tail:
            assert p.grad is None, n
            continue
        g = p.grad
        assert g is not None and g.dtype == p.dtype and g.shape == p.shape and bool(torch.isfinite(g).all()), n
        nq = n.replace(".key.bias", ".query.bias")    # key.bias: analytically zero, held to query.bias's scale and distance
        rrms, rmx = dist(ref16[nq], ref[nq])
        if compute == "fp32" and n.endswith(".key.bias"):
            key_bias_fp32(n, g, ref)
        elif compute == "fp32" or rrms == 0:          # (the top layer's output.LayerNorm.bias: an fp32 sum of bf16-exact terms)
            close_fp32(f"{which} k={k} {compute} {n}", g, ref[n])
        else:
            rms, mx = dist(g, ref[n])
            print(f"{which} k={k} bf16 {n}: rms {rms:.3g} max {mx:.3g}; bf16 storage alone rms {rrms:.3g} max {rmx:.3g}")
            if not (rms <= BF16_RMS * rrms and mx <= BF16_MAX * rmx):
                failures.append((n, rms, mx, rrms, rmx))
    assert not failures, failures


def test_module_switch_counter_and_the_step_of_a_backward():
    config, sd, ids, mask, typ, up, *_ = module_case("tiny")
    enc, plain = encoder(config, sd, "bf16", 1), encoder(config, sd, "bf16", 1, dropout=False)
    args = (ids.to(DEV), mask.to(DEV), typ.to(DEV))
    enc.eval()
    assert torch.equal(enc(*args).last_hidden_state, plain(*args).last_hidden_state) and enc._train_step == 0       # eval(): today's bits, no tick
    plain.train()
    assert torch.equal(plain(*args).last_hidden_state, enc(*args).last_hidden_state) and plain._train_step == 0     # dropout=False: train() changes nothing
    enc.train()

    def grads_of(out):
        for p in enc.parameters():
            p.grad = None
        (out.last_hidden_state.float() * up.float().to(DEV)).sum().backward()
        torch.cuda.synchronize()
        return {n: p.grad.clone() for n, p in enc.named_parameters() if p.grad is not None}

    first = enc(*args)
    assert enc._train_step == 1
    with torch.no_grad():
        second = enc(*args)                           # live under no_grad too: one tick
    assert enc._train_step == 2 and not torch.equal(first.last_hidden_state, second.last_hidden_state)
    assert not torch.equal(first.last_hidden_state, plain(*args).last_hidden_state)
    late = grads_of(first)                            # the backward of step 0 after step 1 has run
    again = forward_at(enc, 0, *[t.cpu() for t in args])
    assert torch.equal(again.last_hidden_state, first.last_hidden_state)
    alone = grads_of(again)
    assert len(late) == 16 and all(torch.equal(late[n], alone[n]) for n in late), "the backward must use its own forward's step"
    other = grads_of(forward_at(enc, 1, *[t.cpu() for t in args]))
    assert any(not torch.equal(late[n], other[n]) for n in late)


# ------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_text_encoder_trains_the_tail_with_the_trunks_dropout(compute):
    """test_gpu_bert_backward's end-to-end case (width 768, one layer, B = 3, L = 9) with the trunk built with dropout=True and the
    encoder in train(): everything finite, gradients on the encoder's 12 parameters and the tail, and -- with both step counters
    pinned, so that every forward draws the same masks -- four SGD steps on the trunk's tail lower the loss every time (with fresh
    masks the loss is another function each step and not monotone by construction)."""
    torch.manual_seed(5)
    cfg = dict(vocab_size=97, hidden_size=768, num_hidden_layers=1, num_attention_heads=12, intermediate_size=3072, max_position_embeddings=16)
    trunk = bert.BertEncoder(cfg, compute_dtype=compute, finetune_layers=1, dropout=True, dropout_seed=3)
    with torch.no_grad():
        for n, p in trunk.named_parameters():
            if "LayerNorm.weight" in n:
                p.copy_(0.5 + torch.rand_like(p))
            elif n.startswith("embeddings.") and n.endswith("weight"):
                p.copy_(0.5 * torch.randn_like(p))
            elif n.endswith("weight"):
                p.copy_(torch.randn_like(p) / p.shape[1] ** 0.5)
    enc = text.TemporalTextEncoder({"hidden_dim": 512}, compute, bert=trunk).to(DEV).train()
    assert trunk.training
    gen = torch.Generator().manual_seed(6)
    ids = torch.randint(1, 97, (3, 9), generator=gen).to(DEV)
    mask = torch.ones(3, 9)
    mask[1, 5:] = 0
    mask[2, 1::2] = 0
    mask = mask.to(DEV)
    target = torch.randn(3, 512, generator=gen).to(DEV)
    tail = [p for n, p in enc.named_parameters() if n.startswith("bert.encoder.layer.0.")]
    assert len(tail) == 16 and all(p.requires_grad for p in tail)

    def pinned():
        enc._train_step, trunk._train_step = 7, 7
        return enc(ids, mask)

    a, b = pinned(), pinned()
    assert torch.equal(a, b) and trunk._train_step == 8 and bool(torch.isfinite(a).all())
    assert not torch.equal(a, enc(ids, mask))         # the next step: other masks
    enc.eval()
    quiet = enc(ids, mask)
    enc.train()
    assert trunk._train_step == 9 and not torch.equal(quiet, a)
    losses, lr = [], None
    for step in range(5):
        for p in enc.parameters():
            p.grad = None
        loss = (pinned() - target).square().mean()
        losses.append(float(loss))
        if step == 4:
            break
        loss.backward()
        if step == 0:
            own = {n: p for n, p in enc.named_parameters() if not n.startswith("bert.")}
            assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in own.values()) and len(own) == 12
            assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0 for p in tail[:3] + tail[4:])          # (key.bias: analytically zero)
            assert all(p.grad is None for n, p in enc.named_parameters() if n.startswith("bert.") and not n.startswith("bert.encoder.layer.0."))
            lr = 0.2 * losses[0] / float(sum(p.grad.double().square().sum() for p in tail))
        with torch.no_grad():
            for p in tail:
                p.sub_(lr * p.grad)
    print(f"text encoder + trunk tail with dropout, {compute}: loss before and after each of four SGD steps: " + ", ".join(f"{v:.6g}" for v in losses))
    assert all(math.isfinite(v) for v in losses) and all(b < a for a, b in zip(losses, losses[1:])), losses

