"""The BERT trunk (mmdeer.bert, include/mmdeer_bert.h) on the GPU: the four new operators at their edges and the whole trunk against
the float64 restatement (tests/bert_ref.py) and the capture from transformers.BertModel (tests/golden/bert_tiny.npz), the
packed-operand cache, HIP-graph capture, and the text encoder with the trunk in front.

Tolerances.  fp32: the text encoder's fp32 bounds against float64 (rtol 1e-3, atol 2e-5); each test prints its largest absolute
difference (transformers' own float32 CPU run of the 768-wide two-layer model sits 6.3e-6 from float64 at outputs of rms 1).
bf16: the yardstick is what bf16 STORAGE alone costs -- the restatement run with every tensor the HIP path stores in bf16 rounded
at that point (bert_ref's ``rnd``), and its distance to float64.  The HIP result may be BF16_RMS times that distance in rms and
BF16_MAX times in max abs: a reordered fp32 sum moves a bf16 rounding by one ulp (twice the largest rounding error) and no more.
For a single operator the distance is computed per case (its inputs are bf16 already, so only the output is rounded); for the whole
trunk it is the measured constants below, which test_bf16_reference_distances_are_the_recorded_ones recomputes."""
import ctypes as C
import functools

import pytest
import torch

from mmdeer import _lib, bert, text

from . import bert_ref as R
from .test_cpu_bert import TINY, golden

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FP32 = dict(rtol=1e-3, atol=2e-5)
BF16_RMS, BF16_MAX = 2.0, 4.0
# distance of the bf16-storage restatement from float64 at the last hidden state (rms, max abs); outputs of rms 1.05 / 1.0.
# For orientation: torch's own bf16 CPU run of the 768-wide model is 0.011 rms / 0.061 max from float64.
REF_BF16_TINY = (0.00837, 0.0761)      # the golden model, B = 4, L = 37
REF_BF16_BIG = (0.00811, 0.0626)       # 768 / 12 heads / 3072, 2 layers, B = 3, L = 37 (big_model below)
BIG = dict(vocab_size=97, hidden_size=768, num_hidden_layers=2, num_attention_heads=12, intermediate_size=3072, max_position_embeddings=40,
           type_vocab_size=2)


def dtype_of(compute):
    return torch.float32 if compute == "fp32" else torch.bfloat16


def dist(got, ref):
    d = got.detach().double().cpu() - ref.double()
    return float(d.pow(2).mean().sqrt()), float(d.abs().max())


def check(name, compute, got, ref64):
    """fp32: assert_close against float64.  bf16: against the distance of the bf16-rounded float64 result, times BF16_RMS / BF16_MAX."""
    rms, mx = dist(got, ref64)
    if compute == "fp32":
        print(f"{name} fp32: max |hip - float64| = {mx:.3g}")
        torch.testing.assert_close(got.detach().double().cpu(), ref64.double(), **FP32)
    else:
        rrms, rmx = dist(R.bf16_round(ref64), ref64)
        print(f"{name} bf16: hip rms {rms:.3g} max {mx:.3g}; bf16 storage alone rms {rrms:.3g} max {rmx:.3g}")
        assert rms <= BF16_RMS * rrms and mx <= BF16_MAX * rmx, (name, rms, rrms, mx, rmx)


# ------------------------------------------------------------------------------------------------ attention
def masks_for(L, gen):
    """name -> (2, L) 0 / 1; every sample has a valid key except sample 0 of 'dead'"""
    tail = torch.ones(2, L)
    tail[0, max(1, L - max(1, L // 3)):] = 0          # ends inside a key tile (and inside a block of 32) for every L > 1 here
    tail[1, max(1, L // 2 + 1):] = 0
    last = torch.zeros(2, L)
    last[:, L - 1] = 1
    holes = torch.ones(2, L)
    holes[0, 2::3] = 0
    holes[1] = (torch.rand(L, generator=gen) < 0.5).float()
    holes[1, L // 2] = 1
    if L > 40:
        holes[1, 32:64] = 0                           # a whole block of 32 keys without a valid one: the skipped path
    dead = holes.clone()
    dead[0] = 0
    return {"all": torch.ones(2, L), "tail": tail, "last": last, "holes": holes, "dead": dead}


def run_attention(qkv, mask, B, L, H, compute, pad=8, extra_rows=3):
    """qkv (B * L, ld) on the device -> (ctx (B * L, H), the whole destination buffer, its sentinel)"""
    ld_ctx = H + pad
    buf = torch.full((B * L + extra_rows, ld_ctx), 777.0, dtype=qkv.dtype, device=DEV)
    a = _lib.BertAttnArgs()
    a.qkv, a.mask, a.ctx = qkv.data_ptr(), mask.data_ptr(), buf.data_ptr()
    a.B, a.L, a.H, a.ld_qkv, a.ld_ctx, a.act_f32, a.stream = B, L, H, qkv.stride(0), ld_ctx, int(compute == "fp32"), _lib.current_stream()
    _lib.check(_lib.load().mmdeer_bert_attn_fwd(C.byref(a)))
    torch.cuda.synchronize()
    assert bool((buf[B * L:] == 777.0).all()) and bool((buf[:, H:] == 777.0).all()), "the canary behind ctx was written"
    return buf[:B * L, :H]


def attention_case(B, L, heads, compute, scale=1.0, seed=0):
    H = 64 * heads
    gen = torch.Generator().manual_seed(1000 * L + heads + seed)
    qkv = torch.randn(B * L, 3 * H + 8, generator=gen)
    qkv[:, :2 * H] *= scale
    return H, gen, qkv.to(dtype_of(compute))          # the operator's input IS the stored tensor: the reference reads the same values


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
@pytest.mark.parametrize("heads", [2, 12])
@pytest.mark.parametrize("L", [1, 37, 64, 65, 129])
def test_attention_against_float64(L, heads, compute):
    B = 2
    H, gen, qkv = attention_case(B, L, heads, compute, scale=1.5)
    q64, dq = qkv.double(), qkv.to(DEV)
    for name, mask in masks_for(L, gen).items():
        ref = R.attention(q64, mask.reshape(-1).double(), B, L, H)
        got = run_attention(dq, mask.reshape(-1).to(DEV), B, L, H, compute)
        assert bool(torch.isfinite(got).all())
        if name == "dead":                            # the fully masked sample: exact zeros; its neighbour as ever
            assert bool((got[:L] == 0).all()) and bool((ref[:L] == 0).all())
            check(f"attention L={L} heads={heads} {name}", compute, got[L:], ref[L:])
        else:                                         # all rows, masked query rows included
            check(f"attention L={L} heads={heads} {name}", compute, got, ref)


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_attention_at_512_tokens(compute):
    B, L, heads = 1, 512, 2
    H, gen, qkv = attention_case(B, L, heads, compute, scale=1.5)
    mask = (torch.rand(1, L, generator=gen) < 0.6).float()
    mask[0, 128:256] = 0                              # a whole key tile without a valid key
    mask[0, 500:] = 0
    ref = R.attention(qkv.double(), mask.reshape(-1).double(), B, L, H)
    check("attention L=512", compute, run_attention(qkv.to(DEV), mask.reshape(-1).to(DEV), B, L, H, compute), ref)


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_attention_with_large_scores(compute):
    """raw scores q . k up to +-80: the running maximum keeps every exponent at or below zero"""
    B, L, heads = 2, 129, 2
    H, gen, qkv = attention_case(B, L, heads, compute, seed=7)
    q, k = (qkv[:, i * H:(i + 1) * H].double().reshape(B, L, heads, 64).permute(0, 2, 1, 3) for i in range(2))
    top = float((q @ k.transpose(-1, -2)).abs().max())
    qkv[:, :H] = (qkv[:, :H].double() * (82.0 / top)).to(qkv.dtype)
    q = qkv[:, :H].double().reshape(B, L, heads, 64).permute(0, 2, 1, 3)
    raw = q @ k.transpose(-1, -2)
    assert float(raw.abs().max()) > 79 and float(raw.max()) > 60 and float(raw.min()) < -60
    mask = masks_for(L, gen)["holes"]
    ref = R.attention(qkv.double(), mask.reshape(-1).double(), B, L, H)
    got = run_attention(qkv.to(DEV), mask.reshape(-1).to(DEV), B, L, H, compute)
    assert bool(torch.isfinite(got).all())
    check("attention, scores to +-80", compute, got, ref)


# ------------------------------------------------------------------------------------------------ add + LN, embed + LN, GELU
def ln_params(N, gen):
    return torch.rand(N, generator=gen) + 0.5, 0.6 * torch.rand(N, generator=gen) - 0.3


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
@pytest.mark.parametrize("N", [128, 768, 1024])
@pytest.mark.parametrize("M", [1, 5, 67])
def test_add_ln_against_float64(M, N, compute):
    gen = torch.Generator().manual_seed(M + N)
    dt = dtype_of(compute)
    y, x = torch.randn(M, N + 4, generator=gen), torch.randn(M, N + 8, generator=gen)
    y[0], x[0] = 7e-4 * y[0], 7e-4 * x[0]             # a row of variance about 1e-6: eps = 1e-5 would shrink it by a factor of 3.3
    y, x = y.to(dt), x.to(dt)
    assert 3e-7 < float((y[0, :N].double() + x[0, :N].double()).var()) < 3e-6
    gamma, beta = ln_params(N, gen)
    ref = R.add_ln(y[:, :N].double(), x[:, :N].double(), gamma.double(), beta.double(), 1e-12)
    wrong_eps = R.add_ln(y[:1, :N].double(), x[:1, :N].double(), gamma.double(), torch.zeros(N, dtype=torch.float64), 1e-5)
    assert float((ref[0] - beta.double()).abs().max() / wrong_eps.abs().max()) > 2.5
    out = torch.full((M + 2, N + 12), 777.0, dtype=dt, device=DEV)
    dy, dx, dg, db = y.to(DEV), x.to(DEV), gamma.to(DEV), beta.to(DEV)
    a = _lib.BertAddLnArgs()
    a.y, a.x, a.gamma, a.beta, a.out, a.eps = dy.data_ptr(), dx.data_ptr(), dg.data_ptr(), db.data_ptr(), out.data_ptr(), 1e-12
    a.M, a.N, a.ld_y, a.ld_x, a.ld_out, a.act_f32, a.stream = M, N, N + 4, N + 8, N + 12, int(compute == "fp32"), _lib.current_stream()
    _lib.check(_lib.load().mmdeer_bert_add_ln_fwd(C.byref(a)))
    torch.cuda.synchronize()
    assert bool((out[M:] == 777.0).all()) and bool((out[:, N:] == 777.0).all())
    check(f"add_ln M={M} N={N}", compute, out[:M, :N], ref)
    check(f"add_ln M={M} N={N}, the small-variance row", compute, out[:1, :N], ref[:1])
    a.x, a.out, a.ld_out = None, dy.data_ptr(), N + 4  # no residual, in place over y
    _lib.check(_lib.load().mmdeer_bert_add_ln_fwd(C.byref(a)))
    check(f"ln in place M={M} N={N}", compute, dy[:, :N], R.layer_norm(y[:, :N].double(), gamma.double(), beta.double(), 1e-12))


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
@pytest.mark.parametrize("typed", [False, True])
@pytest.mark.parametrize("H", [128, 768, 1024])
@pytest.mark.parametrize("BL", [(1, 1), (1, 5), (2, 67)])
def test_embed_ln_against_float64(BL, H, typed, compute):
    (B, L), V, P, T = BL, 31, BL[1], 3                # t reaches P - 1
    gen = torch.Generator().manual_seed(B * L + H)
    word, pos, typ = torch.randn(V, H, generator=gen), torch.randn(P, H, generator=gen), torch.randn(T, H, generator=gen)
    ids = torch.randint(0, V, (B, L), generator=gen)
    ids.reshape(-1)[0] = 1
    pos[0], typ[0], word[1] = 0.0, 0.0, 1e-3 * torch.randn(H, generator=gen)     # row 0 of the output: a sum of variance about 1e-6
    if L >= 5:
        ids[0, 1], ids[0, 2], ids[0, 3], ids[0, 4] = 0, V - 1, V + 5, -2  # the ends of the table, and out of range (clamped)
    types = torch.randint(0, T, (B, L), generator=gen) if typed else None
    if typed:
        types.reshape(-1)[0] = 0
        if L >= 5:
            types[0, 1], types[0, 2] = T - 1, T + 3                       # clamped too
    gamma, beta = ln_params(H, gen)
    ref = R.embed_ln(word.double(), pos.double(), typ.double(), gamma.double(), beta.double(), 1e-12, ids, types).reshape(B * L, H)
    assert 3e-7 < float((word[1] + typ[0] + pos[0]).double().var()) < 3e-6
    out = torch.full((B * L + 2, H + 4), 777.0, dtype=dtype_of(compute), device=DEV)
    dev = [t.to(DEV) for t in (ids.reshape(-1), word, pos, typ, gamma, beta)] + [types.reshape(-1).to(DEV) if typed else None]
    a = _lib.BertEmbedArgs()
    a.ids, a.word, a.pos, a.type, a.gamma, a.beta, a.type_ids = [_lib.ptr(t) for t in dev]
    a.x, a.eps, a.B, a.L, a.H, a.V, a.P, a.T, a.ld_x = out.data_ptr(), 1e-12, B, L, H, V, P, T, H + 4
    a.act_f32, a.stream = int(compute == "fp32"), _lib.current_stream()
    _lib.check(_lib.load().mmdeer_bert_embed_fwd(C.byref(a)))
    torch.cuda.synchronize()
    assert bool((out[B * L:] == 777.0).all()) and bool((out[:, H:] == 777.0).all())
    if B * L > 1:
        check(f"embed B={B} L={L} H={H} typed={typed}", compute, out[1:B * L, :H], ref[1:])
    check(f"embed B={B} L={L} H={H} typed={typed}, the small-variance row", compute, out[:1, :H], ref[:1])


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_gelu_is_the_erf_form(compute):
    grid = torch.cat([torch.tensor([0.0, 0.75, -0.75, 3.0, -3.0, 10.0, -10.0, 1e-4, -1e-4, 0.5, -0.5, 6.0]), torch.linspace(-9.0, 9.0, 1200 - 12)])
    M, N = 5, 240
    x = grid.reshape(M, N).to(dtype_of(compute))
    ref = R.gelu(x.double())
    buf = torch.full((M + 1, N + 4), 777.0, dtype=x.dtype, device=DEV)
    buf[:M, :N] = x.to(DEV)
    out = torch.full((M + 1, N + 8), 777.0, dtype=x.dtype, device=DEV)
    a = _lib.BertGeluArgs()
    a.x, a.out, a.M, a.N, a.ld_x, a.ld_out, a.act_f32, a.stream = buf.data_ptr(), out.data_ptr(), M, N, N + 4, N + 8, int(compute == "fp32"), _lib.current_stream()
    _lib.check(_lib.load().mmdeer_bert_gelu_fwd(C.byref(a)))
    a.out, a.ld_out = buf.data_ptr(), N + 4           # and in place
    _lib.check(_lib.load().mmdeer_bert_gelu_fwd(C.byref(a)))
    torch.cuda.synchronize()
    assert torch.equal(out[:M, :N], buf[:M, :N])
    assert bool((out[M:] == 777.0).all()) and bool((out[:, N:] == 777.0).all()) and bool((buf[M:] == 777.0).all()) and bool((buf[:, N:] == 777.0).all())
    if compute == "fp32":
        err = float((out[:M, :N].double().cpu() - ref).abs().max())
        print(f"gelu fp32: max |hip - erf form| = {err:.3g}; the tanh form is {float((R.gelu_tanh(x.double()) - ref).abs().max()):.3g} away")
        assert err <= 1e-6                            # 400 times tighter than the tanh approximation's distance (about 4e-4)
        assert float((R.gelu_tanh(x.double()) - ref).abs().max()) > 1e-4
    else:
        check("gelu", compute, out[:M, :N], ref)


# ------------------------------------------------------------------------------------------------ the whole trunk
def encoder(config, sd, compute):
    enc = bert.BertEncoder(config, compute_dtype=compute)
    enc.load_state_dict({k: v.float() for k, v in sd.items()}, strict=True)
    return enc.to(DEV)


@functools.lru_cache(maxsize=None)
def big_model(seed=0):
    """(state dict, ids, mask, [float64 hidden states]) of the 768 / 12 / 3072 two-layer model at B = 3, L = 37: weights drawn as the
    golden model's (scores with a spread of a few units, non-trivial LayerNorms) and rounded to bf16, so that both compute dtypes
    read the same model.  Computed once, shared, left unchanged."""
    gen = torch.Generator().manual_seed(31 + seed)
    sd = {}
    for k, v in bert.BertEncoder(BIG).state_dict().items():
        n, u = torch.randn(v.shape, generator=gen), torch.rand(v.shape, generator=gen)
        w = (0.5 + u if k.endswith("LayerNorm.weight") else 0.6 * u - 0.3 if k.endswith("LayerNorm.bias") else 0.1 * n if k.endswith(".bias")
             else 0.5 * n if "embeddings" in k else 0.08 * n if (".query." in k or ".key." in k) else n / v.shape[1] ** 0.5)
        sd[k] = w.bfloat16().double()
    ids = torch.randint(0, BIG["vocab_size"], (3, 37), generator=gen)
    mask = torch.ones(3, 37, dtype=torch.int64)
    mask[1, 20:] = 0
    mask[2, 1::4] = 0
    return sd, ids, mask, R.trunk(sd, ids, mask)


def test_bf16_reference_distances_are_the_recorded_ones():
    """the constants the bf16 trunk tests are held to, recomputed on the CPU (no launch).  Another BLAS rounds a float64 sum in another
    order, which can flip single bf16 roundings of the emulation: the rms then moves in its third digit (bound 5 %), the max, one
    element, by more (bound 25 %)"""
    sd, ids, mask, typ, hidden = golden()
    tiny = dist(R.trunk(sd, ids, mask, typ, rnd=R.bf16_round)[-1], hidden[-1])
    sd, ids, mask, states = big_model()
    big = dist(R.trunk(sd, ids, mask, rnd=R.bf16_round)[-1], states[-1])
    print(f"bf16 storage alone: tiny rms {tiny[0]:.4g} max {tiny[1]:.4g}; big rms {big[0]:.4g} max {big[1]:.4g}")
    for got, want in ((tiny, REF_BF16_TINY), (big, REF_BF16_BIG)):
        assert got[0] == pytest.approx(want[0], rel=0.05) and got[1] == pytest.approx(want[1], rel=0.25)


def check_trunk(name, compute, states, refs, recorded):
    for i, (s, r) in enumerate(zip(states, refs)):
        rms, mx = dist(s.reshape(r.shape), r)
        print(f"{name} {compute} hidden state {i}: rms {rms:.3g} max {mx:.3g}")
    if compute == "fp32":
        for i, (s, r) in enumerate(zip(states, refs)):
            torch.testing.assert_close(s.double().cpu().reshape(r.shape), r, **FP32, msg=lambda m, i=i: f"hidden state {i}: {m}")
    else:
        rms, mx = dist(states[-1].reshape(refs[-1].shape), refs[-1])
        assert rms <= BF16_RMS * recorded[0] and mx <= BF16_MAX * recorded[1], (name, rms, mx, recorded)


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_trunk_reproduces_the_capture_layer_by_layer(compute):
    sd, ids, mask, typ, hidden = golden()
    enc = encoder(TINY, sd, compute)
    out = enc(ids.to(DEV), mask.to(DEV), typ.to(DEV), output_hidden_states=True)
    assert out.last_hidden_state.shape == (4, 37, 128) and out.last_hidden_state.dtype == dtype_of(compute) and not out.last_hidden_state.requires_grad
    assert torch.equal(out.last_hidden_state, out.hidden_states[-1]) and len(out.hidden_states) == 3
    check_trunk("tiny", compute, out.hidden_states, hidden, REF_BF16_TINY)


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_trunk_at_bert_base_width(compute):
    sd, ids, mask, states = big_model()
    enc = encoder(BIG, sd, compute)
    out = enc(ids.to(DEV), mask.to(DEV), output_hidden_states=True)
    check_trunk("768 / 12 / 3072", compute, out.hidden_states, states, REF_BF16_BIG)
    plain = enc(ids.to(DEV)).last_hidden_state                        # no mask: all valid
    ref = R.trunk(sd, ids)[-1]
    if compute == "fp32":
        torch.testing.assert_close(plain.double().cpu(), ref, **FP32)
    assert enc(ids[:0].to(DEV)).last_hidden_state.shape == (0, 37, 768)


def test_load_state_dict_invalidates_the_packed_operands():
    sd, ids, mask, typ, hidden = golden()
    enc = encoder(TINY, sd, "fp32")
    first = enc(ids.to(DEV), mask.to(DEV), typ.to(DEV)).last_hidden_state.clone()
    packed = enc._packed
    assert enc(ids.to(DEV), mask.to(DEV), typ.to(DEV)).last_hidden_state.equal(first) and enc._packed is packed      # built once
    other = {k: (v.flip(0) if k.endswith("query.weight") or k.endswith("output.dense.weight") else v).float() for k, v in sd.items()}
    enc.load_state_dict(other, strict=True)
    second = enc(ids.to(DEV), mask.to(DEV), typ.to(DEV)).last_hidden_state
    assert enc._packed is not packed
    torch.testing.assert_close(second.double().cpu(), R.trunk(other, ids, mask, typ)[-1], **FP32)
    assert float((second - first).abs().max()) > 0.1
    with torch.no_grad():                                             # an in-place edit of one parameter counts as well
        enc.encoder.layer[0].intermediate.dense.bias.add_(1.0)
    assert float((enc(ids.to(DEV), mask.to(DEV), typ.to(DEV)).last_hidden_state - second).abs().max()) > 1e-3


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_graph_capture_replays_eager_bit_for_bit(compute):
    sd, ids, mask, typ, hidden = golden()
    enc = encoder(TINY, sd, compute)
    dids, dmask, dtyp = ids.to(DEV), mask.to(DEV), typ.to(DEV)
    eager = enc(dids, dmask, dtyp).last_hidden_state.clone()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        enc(dids, dmask, dtyp)                                        # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = enc(dids, dmask, dtyp).last_hidden_state
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    dids.copy_(dids.flip(1))                                          # new inputs in the captured buffers
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, enc(dids, dmask, dtyp).last_hidden_state) and not torch.equal(out, eager)


# ------------------------------------------------------------------------------------------------ the text encoder with the trunk
@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_text_encoder_runs_the_trunk_then_its_own_path(compute):
    sd, ids, mask, _ = big_model()
    trunk = encoder(BIG, sd, compute)
    torch.manual_seed(3)
    enc = text.TemporalTextEncoder({"hidden_dim": 512}, compute, bert=trunk).to(DEV).eval()
    dids, dmask = ids.to(DEV), mask.to(DEV)
    y = enc(dids, dmask)
    assert y.shape == (3, 512) and y.dtype == torch.float32 and bool(torch.isfinite(y).all())
    hidden = trunk(dids, dmask).last_hidden_state
    assert hidden.dtype == dtype_of(compute)
    assert torch.equal(y, enc.forward_embeddings(hidden, dids, dmask))
    enc.train()                                                       # a training step on the tail: gradients there, none in the trunk
    loss = enc(dids, dmask).square().sum()
    loss.backward()
    tail = {n: p for n, p in enc.named_parameters() if not n.startswith("bert.")}
    assert len(tail) == 12 and all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in tail.values())
    assert sum(float(p.grad.abs().sum()) > 0 for p in tail.values()) >= 10          # (token_attention.2.bias is analytically zero)
    assert all(p.grad is None and not p.requires_grad for n, p in enc.named_parameters() if n.startswith("bert."))
