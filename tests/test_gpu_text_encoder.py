"""The temporal text encoder (mmdeer.text) on the GPU: the whole encoder against the vectors captured from the reference
(tests/golden/text_seq.npz), the pool, gather and statistics operators against the float64 restatement (tests/text_ref.py),
edges, training and HIP-graph capture."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from mmdeer import _lib, synth, text

from . import text_ref as R
from .test_cpu_text_encoder import CASES, check_dE, check_embedding_rows, embeddings
from .test_oracle_golden import check_side_grads

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "text_seq.npz")
E, A = 768, 384


def _fill(module, tag):
    """The closed-form parameter fill of tests/golden/make_golden.py, keyed by state_dict name."""
    sd = synth.module_fill(tag, {k: tuple(v.shape) for k, v in module.state_dict().items()})
    module.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return module


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _case(g, i):
    B, L = CASES[i]
    tag = f"txt{B}x{L}"
    return (tag, torch.from_numpy(g[f"{tag}.ids"]).to(DEV), torch.from_numpy(g[f"{tag}.ids"].clip(min=0)).to(DEV),
            torch.from_numpy(g[f"{tag}.mask"]).to(DEV), torch.from_numpy(g[f"{tag}.loss_w"]).to(DEV))


# ------------------------------------------------------------------------------------------------ golden (reference capture)
@pytest.mark.parametrize("i", range(len(CASES)))
def test_golden_fp32_ids_path(i):
    g = np.load(GOLDEN)
    tag, ids, _, mask, w = _case(g, i)
    m = _fill(text.TemporalTextEncoder(compute_dtype="fp32"), tag).to(DEV).eval()
    y = m(ids, mask)
    np.testing.assert_allclose(y.detach().cpu().numpy(), g[f"{tag}.out"], rtol=1e-3, atol=2e-5)
    np.testing.assert_allclose(m.last_attention_weights.cpu().numpy(), g[f"{tag}.attn"], rtol=1e-3, atol=2e-5)
    (y * w).sum().backward()
    grads = {n: p.grad for n, p in m.named_parameters()}
    check_side_grads(g, tag, grads, {}, rtol=3e-3, atol_frac=3e-3)
    check_embedding_rows(g, tag, grads["embedding.weight"])         # touched rows; row 0 and untouched rows exactly zero
    assert float(grads["token_attention.2.bias"].abs().max()) == 0.0


@pytest.mark.parametrize("i", range(len(CASES)))
def test_golden_fp32_embeddings_path(i):
    g = np.load(GOLDEN)
    tag, _, ide, mask, w = _case(g, i)
    te = tag + "e"
    assert np.array_equal(ide.cpu().numpy(), g[f"{te}.ids"])
    m = _fill(text.TemporalTextEncoder(compute_dtype="fp32"), tag).to(DEV).eval()
    Em = torch.from_numpy(embeddings(i, *CASES[i])).to(DEV).requires_grad_(True)
    y = m.forward_embeddings(Em, ide, mask)
    np.testing.assert_allclose(y.detach().cpu().numpy(), g[f"{te}.out"], rtol=1e-3, atol=2e-5)
    np.testing.assert_allclose(m.last_attention_weights.cpu().numpy(), g[f"{te}.attn"], rtol=1e-3, atol=2e-5)
    (y * w).sum().backward()
    grads = {n: p.grad for n, p in m.named_parameters()}
    check_side_grads(g, te, grads, {}, rtol=3e-3, atol_frac=3e-3)
    check_dE(g, te, Em.grad, rtol=3e-3, atol_frac=3e-3)
    assert float(grads["token_attention.2.bias"].abs().max()) == 0.0
    assert not bool(Em.grad[mask == 0].any())                        # masked positions get exact zeros


@pytest.mark.parametrize("path", ["ids", "embeddings"])
@pytest.mark.parametrize("i", range(len(CASES)))
def test_golden_bf16_gradients_track_fp32(i, path):
    g = np.load(GOLDEN)
    tag, ids, ide, mask, w = _case(g, i)
    Em = torch.from_numpy(embeddings(i, *CASES[i])).to(DEV)
    res = {}
    for compute in ("fp32", "bf16"):
        m = _fill(text.TemporalTextEncoder(compute_dtype=compute), tag).to(DEV).eval()
        y = m(ids, mask) if path == "ids" else m.forward_embeddings(Em, ide, mask)
        (y * w).sum().backward()
        res[compute] = {n: p.grad.double().flatten() for n, p in m.named_parameters() if p.grad is not None}
    assert len(res["fp32"]) == (14 if path == "ids" else 12)
    for n, a in res["fp32"].items():
        # token_attention.2.bias: analytically zero in both.  token_attention.0.bias: the sum over tokens of dz, whose terms cancel
        # (the softmax gradient sums to zero over the positions of a sample); the fp32 golden tests pin it against the reference.
        if n in ("token_attention.2.bias", "token_attention.0.bias"):
            continue
        b = res["bf16"][n]
        cos = float((a @ b) / (a.norm() * b.norm()))
        print(f"{path} case {i} {n}: cosine {cos:.5f}")
        assert cos > 0.97, (n, cos)


# ------------------------------------------------------------------------------------------------ the pool operators
def _pool_inputs(B, L, dt):
    gen = torch.Generator().manual_seed(B + 100 * L)
    mask = (torch.rand(B, L, generator=gen) < 0.7).float()
    mask[0, 0] = 1.0
    if B > 1:
        mask[1] = 0.0                                  # a fully masked sample
    if B > 2:
        mask[2] = 0.0
        mask[2, L - 1] = 1.0                           # only the last token valid
    x = (torch.randn(B, L, E, generator=gen) * mask.unsqueeze(-1)).to(dt)
    z = torch.randn(B, L, A, generator=gen)
    w2 = torch.randn(1, A, generator=gen) * 0.27        # sum |w2| is about 80
    b2 = torch.randn(1, generator=gen)
    if L > 1:    # sample 0: scores +-sum|w2|, alternating between positions (the softmax must subtract the max)
        sign = torch.tensor([1.0 if t % 2 else -1.0 for t in range(L)])
        z[0] = 20.0 * sign[:, None] * torch.sign(w2)
        mask[0] = 1.0
        x[0] = torch.randn(L, E, generator=gen).to(dt)
    gout = torch.randn(B, E, generator=gen).to(dt)
    return [t.to(DEV) for t in (x, z.to(dt), mask, w2, b2, gout)]


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
@pytest.mark.parametrize("L", [1, 2, 33, 130])
@pytest.mark.parametrize("B", [1, 5, 37])
def test_pool_operators_match_float64(B, L, compute):
    dt = torch.float32 if compute == "fp32" else torch.bfloat16
    x, z, mask, w2, b2, gout = _pool_inputs(B, L, dt)
    xr, zr = x.reshape(B * L, E).clone().requires_grad_(True), z.reshape(B * L, A).clone().requires_grad_(True)
    w2r, b2r = w2.clone().requires_grad_(True), b2.clone().requires_grad_(True)
    att, wts = text._TokenPoolFn.apply(xr, zr, mask.reshape(-1).contiguous(), w2r, b2r, B, L, compute)
    (att * gout.float()).sum().backward()
    # float64 on the values the kernel read; only the direct term a_t dout reaches x (the score path is the caller's GEMM)
    x64, z64 = x.double(), z.double().requires_grad_(True)
    w64, b64 = w2.double().requires_grad_(True), b2.double().requires_grad_(True)
    att64, a64, _ = R.masked_pool(x64, z64, mask, w64, b64)
    (att64 * gout.double()).sum().backward()
    dx64 = a64.detach().unsqueeze(-1) * gout.double().unsqueeze(1)
    hip = {"att": att, "wts": wts, "dx": xr.grad.float().reshape(B, L, E), "dz": zr.grad.float().reshape(B, L, A), "dw2": w2r.grad}
    r64 = {"att": att64, "wts": a64, "dx": dx64, "dz": z64.grad, "dw2": w64.grad}
    for v in hip.values():
        assert torch.isfinite(v).all()
    # dz and dw2 are sums of terms that cancel: ds_t = p_t (m_t (da_t - c) - c eps) / (S + eps) is analytically zero for a sample
    # with one valid token, and sample 0's saturated tanh makes its dz zero and its dw2 the sum of ds_t over the positions that
    # hold the probability mass, which is zero too.  Where such samples are the whole batch (B = 1, L = 1, ...) the exact value
    # is a rounding residue and an error relative to it has no meaning.  So: where the exact gradient is at least 1e-2 of the
    # terms summed into it (`scale`, their absolute values summed), the error is relative to the exact gradient, as the bound
    # is stated; otherwise it is relative to `scale`, which is what fp32 arithmetic can answer for.
    with torch.no_grad():
        da = (gout.double().unsqueeze(1) * x64).sum(-1)
        p64 = torch.softmax(torch.tanh(z64) @ w64.reshape(-1) + b64, dim=1)
        S, c = (p64 * mask).sum(1, keepdim=True), (a64 * da).sum(1, keepdim=True)
        gabs = p64 * (mask * (da.abs() + c.abs()) + c.abs() * R.EPS) / (S + R.EPS)
        tz = torch.tanh(z64)
        scale = {"dz": float((gabs.unsqueeze(-1) * w64.abs().reshape(1, 1, A) * (1 - tz * tz)).norm()),
                 "dw2": float((gabs.unsqueeze(-1) * tz.abs()).sum((0, 1)).norm())}
    fp32_bound = {"att": 1e-5, "wts": 1e-5, "dx": 1e-5, "dz": 1e-4, "dw2": 1e-4}
    for k in hip:
        ref = r64[k].detach()
        den = float(ref.norm())
        if k in scale and den < 1e-2 * scale[k]:
            den = scale[k]
        err = float((hip[k].double() - ref).norm())
        if den == 0.0:
            assert err == 0.0, k
            continue
        d = err / den
        if compute == "fp32" or k in ("wts", "dw2"):     # fp32 arithmetic on fp32 storage in both modes
            bound = fp32_bound[k]
        else:                                            # stored as bf16: judged against the rounding of the exact value
            bound = 2 * float((R.bf16(ref) - ref).norm()) / den + 1e-6
        print(f"B={B} L={L} {compute} {k}: {d:.3e} (bound {bound:.3e})")
        assert d <= bound, (k, d, bound)
    assert float(b2r.grad.abs().max()) == 0.0           # written as an exact zero
    if B > 1:                                            # fully masked: outputs exactly zero, nothing reaches x
        assert float(att[1].abs().max()) == 0.0 and float(wts[1].abs().max()) == 0.0
        assert float(hip["dx"][1].abs().max()) == 0.0 and torch.isfinite(hip["dz"][1]).all()
    if B > 2:
        # only the last token valid: all the weight is there, short of 1 by 1e-10 / p (p may be small: the padded positions
        # take part in the softmax), and exact zeros before it
        assert float(wts[2, L - 1]) == pytest.approx(float(a64[2, L - 1]), rel=1e-5) and float(wts[2, :L - 1].abs().sum()) == 0.0


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
@pytest.mark.parametrize("B", [1024, 1027])
def test_pool_backward_past_its_grid_cap_and_the_fold(B, compute):
    """The backward runs at most `cap` workgroups of one sample each and strides over the batch beyond them: at B = 1027 three
    workgroups take a second sample and cross the barrier between samples.  L = 2 with the masks of _pool_inputs (some samples
    have one position masked, some both).  dx, dz and dw2 against text_ref.masked_pool in float64 with the bounds of
    test_pool_operators_match_float64; and dw2 must be the workgroups' partials, read back from the caller's scratch buffer,
    added in index order in fp32 -- bit for bit -- with db2 = +0.0."""
    L = 2
    cap = _lib.TOKEN_POOL_SCRATCH // A
    nparts = min(B, cap)
    dt = torch.float32 if compute == "fp32" else torch.bfloat16
    x, z, mask, w2, b2, gout = _pool_inputs(B, L, dt)
    assert bool(((mask.sum(1) == 1).sum() > 0) & ((mask.sum(1) == 2).sum() > 0))
    xa, za, m = x.reshape(B * L, E).contiguous(), z.reshape(B * L, A).contiguous(), mask.reshape(-1).contiguous()
    w2f = w2.reshape(-1).contiguous()
    att = torch.empty(B, E, dtype=dt, device=DEV)
    wts, probs = torch.empty(B, L, device=DEV), torch.empty(B, L, device=DEV)
    dx, dz = torch.full_like(xa, float("nan")), torch.full_like(za, float("nan"))
    dw2, db2 = torch.full((A,), float("nan"), device=DEV), torch.full((1,), -1.0, device=DEV)
    scratch = torch.full((_lib.TOKEN_POOL_SCRATCH,), float("nan"), device=DEV)
    a = text._pool_args(compute, B, L)
    a.x, a.ld_x, a.z, a.ld_z, a.mask, a.w2, a.b2 = xa.data_ptr(), E, za.data_ptr(), A, m.data_ptr(), w2f.data_ptr(), b2.data_ptr()
    a.attended, a.ld_att, a.weights, a.probs = att.data_ptr(), E, wts.data_ptr(), probs.data_ptr()
    _lib.check(_lib.load().mmdeer_token_pool_fwd(C.byref(a)))
    a.dout, a.ld_dout, a.dx, a.ld_dx, a.dz, a.ld_dz = gout.data_ptr(), E, dx.data_ptr(), E, dz.data_ptr(), A
    a.dw2, a.db2, a.scratch = dw2.data_ptr(), db2.data_ptr(), scratch.data_ptr()
    _lib.check(_lib.load().mmdeer_token_pool_bwd(C.byref(a)))
    # float64 on the values the kernel read, and the scale of the terms summed into dz and dw2 (see the test above)
    x64, z64, w64 = x.double(), z.double().requires_grad_(True), w2.double().requires_grad_(True)
    att64, a64, p64 = R.masked_pool(x64, z64, mask, w64, b2.double())
    (att64 * gout.double()).sum().backward()
    with torch.no_grad():
        da = (gout.double().unsqueeze(1) * x64).sum(-1)
        S, c = (p64 * mask).sum(1, keepdim=True), (a64 * da).sum(1, keepdim=True)
        gabs = p64 * (mask * (da.abs() + c.abs()) + c.abs() * R.EPS) / (S + R.EPS)
        tz = torch.tanh(z64)
        scale = {"dz": float((gabs.unsqueeze(-1) * w64.abs().reshape(1, 1, A) * (1 - tz * tz)).norm()),
                 "dw2": float((gabs.unsqueeze(-1) * tz.abs()).sum((0, 1)).norm())}
    hip = {"dx": dx.float().reshape(B, L, E), "dz": dz.float().reshape(B, L, A), "dw2": dw2.reshape(1, A)}
    r64 = {"dx": a64.detach().unsqueeze(-1) * gout.double().unsqueeze(1), "dz": z64.grad, "dw2": w64.grad}
    fp32_bound = {"dx": 1e-5, "dz": 1e-4, "dw2": 1e-4}
    for k in hip:
        ref = r64[k].detach()
        assert torch.isfinite(ref).all() and torch.isfinite(hip[k]).all(), k
        den = float(ref.norm())
        if k in scale and den < 1e-2 * scale[k]:
            den = scale[k]
        d = float((hip[k].double() - ref).norm()) / den
        if compute == "fp32" or k == "dw2":
            bound = fp32_bound[k]
        else:
            bound = 2 * float((R.bf16(ref) - ref).norm()) / den + 1e-6
        print(f"B={B} L={L} {compute} nparts={nparts} {k}: {d:.3e} (bound {bound:.3e})")
        assert d <= bound, (k, d, bound)
    # the fold: the partials in index order from zero, one column per thread
    parts = scratch.cpu().numpy().reshape(cap, A)
    assert np.isfinite(parts[:nparts]).all() and np.isnan(parts[nparts:]).all()
    acc = np.zeros(A, np.float32)
    for p in range(nparts):
        acc = acc + parts[p]
    assert acc.dtype == np.float32 and np.array_equal(acc.view(np.uint32), dw2.cpu().numpy().view(np.uint32))
    assert db2.cpu().numpy().view(np.uint32)[0] == 0                                 # +0.0


# ------------------------------------------------------------------------------------------------ gather and table gradients
V, P = 1000, 20


def _gather_inputs(B, L, kind):
    gen = torch.Generator().manual_seed(7 * B + L)
    if kind == "same":
        ids = torch.full((B, L), 7, dtype=torch.long)
    else:
        ids = torch.randint(-50, V + 50, (B, L), generator=gen)            # out of range on both sides
        ids[0, 0] = 0
    mask = (torch.rand(B, L, generator=gen) < 0.7).long()
    mask[0, 0] = 1
    emb, pos = torch.randn(V, E, generator=gen), torch.randn(P, E, generator=gen)
    dx = torch.randn(B, L, E, generator=gen)
    return [t.to(DEV) for t in (ids, mask, emb, pos, dx)]


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["random", "same"])
@pytest.mark.parametrize("B,L", [(1, 1), (37, 33), (3, 130)])
def test_gather_and_table_gradients(B, L, kind, compute):
    dt = torch.float32 if compute == "fp32" else torch.bfloat16
    ids, mask, emb, pos, dx = _gather_inputs(B, L, kind)
    dx = dx.to(dt)
    m = (mask != 0).float().reshape(-1).contiguous()
    x_ref = R.gather(ids, mask, emb.double(), pos.double())
    d_emb_ref, d_pos_ref = R.table_grads(ids, mask, dx.double(), V, P)
    runs = []
    for _ in range(2):
        e, p = emb.clone().requires_grad_(True), pos.clone().requires_grad_(True)
        x, ids32 = text._TokenEmbedFn.apply(e, p, ids.reshape(-1).contiguous(), m, B, L, compute)
        (x.float() * dx.float().reshape(B * L, E)).sum().backward()
        runs.append((x.detach(), e.grad, p.grad))
    x, d_emb, d_pos = runs[0]
    assert torch.equal(ids32.reshape(B, L).long(), ids.clamp(0, V - 1))
    assert torch.equal(x.reshape(B, L, E), x_ref.float().to(dt))     # one add and a 0 / 1 factor: correctly rounded, so equal
    for got, ref, name in ((d_emb, d_emb_ref, "d_emb"), (d_pos, d_pos_ref, "d_pos")):
        if float(ref.abs().max()) == 0.0:
            assert float(got.abs().max()) == 0.0, name
        else:
            assert _rel(got, ref) <= 1e-4, (name, _rel(got, ref))
    assert not bool(d_emb[0].any())                                   # padding row
    assert not bool(d_emb[(d_emb_ref.abs().sum(1) == 0)].any())      # rows no valid token names: exact zeros
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)                                      # deterministic: no floating-point atomics
    # precomputed embeddings: x = src * m, d_src = dx * m
    src = emb[ids.clamp(0, V - 1)].reshape(B * L, E).clone().requires_grad_(True)
    xs = text._TokenSrcFn.apply(src, m, B, L, compute)
    (xs.float() * dx.float().reshape(B * L, E)).sum().backward()
    assert torch.equal(xs, (src.detach() * m[:, None]).to(dt))
    assert torch.equal(src.grad, dx.float().reshape(B * L, E) * m[:, None])


# ------------------------------------------------------------------------------------------------ statistics
def _check_stats(ids, mask, max_length=128):
    B, L = ids.shape
    m = (mask != 0).float().reshape(-1).contiguous().to(DEV)
    out = text.token_stats(ids.to(torch.int32).reshape(-1).contiguous().to(DEV), m, B, L, max_length).cpu()
    ref, counts = R.stats(ids.cpu(), mask.cpu(), max_length)
    assert not bool(out[:, 10:].any()) and not bool(out[:, 6:10].any())
    assert torch.equal(out[:, 3].long(), counts[:, 2])                                  # c_max: exact
    assert torch.equal((out[:, 0] * max_length).round().long(), counts[:, 0])           # n: exact
    np.testing.assert_allclose(out[:, :10].numpy(), ref.numpy(), rtol=1e-6, atol=0)
    return out


def test_statistics_match_the_restatement_and_the_capture():
    g = np.load(GOLDEN)
    for B, L in CASES:
        tag = f"txt{B}x{L}"
        mask = torch.from_numpy(g[f"{tag}.mask"])
        out = _check_stats(torch.from_numpy(g[f"{tag}.ids"]).clamp(0, 29999), mask)
        np.testing.assert_allclose(out[:, :10].numpy(), g[f"{tag}.ling"], rtol=1e-6, atol=0)
        out = _check_stats(torch.from_numpy(g[f"{tag}e.ids"]), mask)                    # unclamped above
        np.testing.assert_allclose(out[:, :10].numpy(), g[f"{tag}e.ling"], rtol=1e-6, atol=0)
    gen = torch.Generator().manual_seed(3)
    ids = torch.randint(90, 1100, (64, 128), generator=gen)
    ids[5] = torch.randint(0, 30000, (128,), generator=gen)
    ids[6] = 1005
    mask = (torch.rand(64, 128, generator=gen) < 0.6).long()
    mask[7] = 0
    _check_stats(ids, mask)
    _check_stats(torch.randint(0, 40, (3, 700), generator=gen), torch.ones(3, 700, dtype=torch.long), max_length=512)   # L > 512


# ------------------------------------------------------------------------------------------------ edges
def test_empty_batch_eval_determinism_and_cpu_input():
    lib = _lib.load()
    for args, fns in ((_lib.TokenEmbedArgs(), (lib.mmdeer_token_embed_fwd, lib.mmdeer_token_embed_bwd)),
                      (_lib.TokenPoolArgs(), (lib.mmdeer_token_pool_fwd, lib.mmdeer_token_pool_bwd))):
        args.B, args.L, args.width, args.act_f32, args.stream = 0, 4, E, 1, _lib.current_stream()
        if hasattr(args, "att_width"):
            args.att_width = A
        for f in fns:
            assert f(C.byref(args)) == 0
    torch.manual_seed(3)
    m = text.TemporalTextEncoder().to(DEV).eval()
    ids0, mask0 = torch.zeros(0, 6, dtype=torch.long, device=DEV), torch.zeros(0, 6, dtype=torch.long, device=DEV)
    assert tuple(m(ids0, mask0).shape) == (0, 512)
    assert tuple(m.forward_embeddings(torch.zeros(0, 6, E, device=DEV), ids0, mask0).shape) == (0, 512)
    ids = torch.randint(0, 30000, (17, 9), device=DEV)
    mask = (torch.rand(17, 9, device=DEV) < 0.7).long()
    Em = torch.randn(17, 9, E, device=DEV)
    with torch.no_grad():
        assert torch.equal(m(ids, mask), m(ids, mask))
        assert torch.equal(m.forward_embeddings(Em, ids, mask), m.forward_embeddings(Em, ids, mask))
        yb = m.forward_embeddings(Em.bfloat16(), ids, mask)                 # bf16 embeddings are accepted
        assert yb.dtype == torch.float32 and _rel(yb, m.forward_embeddings(Em, ids, mask)) < 2e-2
    with pytest.raises(RuntimeError):
        m(ids.cpu(), mask.cpu())
    with pytest.raises(RuntimeError):
        m.forward_embeddings(Em.cpu(), ids, mask)


# ------------------------------------------------------------------------------------------------ training
def test_training_dropout_gradients_and_sgd():
    torch.manual_seed(5)
    m = text.TemporalTextEncoder({"dropout_seed": 11}, compute_dtype="fp32").to(DEV).train()
    ids = torch.randint(0, 2000, (64, 16), device=DEV)
    mask = (torch.rand(64, 16, device=DEV) < 0.8).long()
    mask[:, 0] = 1
    with torch.no_grad():
        assert not torch.equal(m(ids, mask), m(ids, mask))          # the step counter moves the masks
    target = torch.randn(64, 512, device=DEV) * 0.5
    losses = []
    opt = torch.optim.SGD(m.parameters(), lr=0.05)
    for it in range(10):
        opt.zero_grad()
        loss = (m(ids, mask) - target).square().mean()
        loss.backward()
        losses.append(float(loss))
        for n, p in m.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all(), n
            if it == 0 and n != "token_attention.2.bias":
                assert float(p.grad.abs().max()) > 0, n
        assert float(m.token_attention[2].bias.grad.abs().max()) == 0.0
        opt.step()
    assert losses[-1] < losses[0], losses


# ------------------------------------------------------------------------------------------------ HIP graph capture
@pytest.mark.parametrize("path", ["embeddings", "ids"])
@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_graph_capture_replays_eager(compute, path):
    torch.manual_seed(9)
    m = text.TemporalTextEncoder(compute_dtype=compute).to(DEV).eval()
    ids = torch.randint(0, 30000, (256, 16), device=DEV)
    mask = (torch.rand(256, 16, device=DEV) < 0.8).long()
    Em = torch.randn(256, 16, E, device=DEV, requires_grad=True)
    w = torch.randn(256, 512, device=DEV)
    leaves = list(m.parameters()) + [Em]

    def fwd_bwd():
        y = m(ids, mask) if path == "ids" else m.forward_embeddings(Em, ids, mask)
        (y * w).sum().backward()
        return y

    def step():
        for p in leaves:
            p.grad = None
        y = fwd_bwd()
        return y.detach().clone(), [None if p.grad is None else p.grad.detach().clone() for p in leaves]

    y0, g0 = step()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()                                        # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    for p in leaves:
        p.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = fwd_bwd()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, y0)
    assert sum(g is not None for g in g0) >= 12
    for p, g in zip(leaves, g0):
        assert (p.grad is None) == (g is None)
        if g is not None:
            assert torch.equal(p.grad, g)
