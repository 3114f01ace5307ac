"""The BERT trunk's backward (include/mmdeer_bert_bwd.h, mmdeer.bert.BertEncoder(finetune_layers=k)) on the GPU: the three new
operators at their edges against float64 autograd (tests/bert_bwd_ref.py), the fine-tuned trunk's parameter gradients against the
restatement, bit-equality of its forward with the frozen trunk's, determinism, the per-layer operand cache, and a few SGD steps
through TemporalTextEncoder(bert=trunk).

Bounds.  fp32: the project's FP32 bounds against float64 (rtol 1e-3, atol 2e-5), atol multiplied by the float64 tensor's largest
absolute element -- gradients here reach 40 where the forward's outputs have rms 1; each test prints its largest difference.
bf16: test_gpu_bert's yardstick, unchanged -- the HIP result may be BF16_RMS times in rms and BF16_MAX times in max abs the
distance from float64 of the restatement with STORAGE rounding only (bert_bwd_ref with rnd = bf16_round).  For a single operator
that distance is computed per case (the inputs are bf16 already, so only the output is rounded: test_gpu_bert.check).  For the
module's parameter gradients it is the recorded constants below, which test_bf16_gradient_distances_are_the_recorded_ones
recomputes on the CPU.  Two entries of those tables are zero or noise by construction and are held otherwise (grad_bound)."""
import ctypes as C
import functools

import pytest
import torch

from mmdeer import _lib, bert, text

from . import bert_bwd_ref as RB
from . import bert_ref as R
from .test_cpu_bert import TINY, golden
from .test_cpu_bert_backward import upstream
from .test_gpu_bert import BF16_MAX, BF16_RMS, BIG, FP32, big_model, check, dist, dtype_of, masks_for

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

# distance from float64 of the restatement with bf16 storage rounding only, per tail parameter's gradient: (rms, max abs, the
# float64 gradient's largest element for orientation).  Keys: the name behind "encoder.layer.".
REF_BF16_GRAD_TINY = {     # the golden model, B = 4, L = 37, upstream(mask, 128); layer 1 alone is finetune_layers = 1
    "0.attention.self.query.weight": (0.206, 1.4, 29.6),
    "0.attention.self.query.bias": (0.15, 0.371, 15),
    "0.attention.self.key.weight": (0.213, 1.69, 37.5),
    "0.attention.self.key.bias": (0.0104, 0.0456, 1.08e-14),
    "0.attention.self.value.weight": (0.2, 1.16, 62.6),
    "0.attention.self.value.bias": (0.162, 0.471, 31.7),
    "0.attention.output.dense.weight": (0.197, 1.33, 70.4),
    "0.attention.output.dense.bias": (0.166, 0.512, 35),
    "0.attention.output.LayerNorm.weight": (0.297, 0.988, 59.7),
    "0.attention.output.LayerNorm.bias": (0.227, 0.71, 37),
    "0.intermediate.dense.weight": (0.136, 0.958, 41.6),
    "0.intermediate.dense.bias": (0.113, 0.453, 16.9),
    "0.output.dense.weight": (0.167, 1.39, 67.6),
    "0.output.dense.bias": (0.174, 0.527, 35.8),
    "0.output.LayerNorm.weight": (0.288, 0.846, 51.7),
    "0.output.LayerNorm.bias": (0.193, 0.55, 36.6),
    "1.attention.self.query.weight": (0.0896, 0.619, 31.5),
    "1.attention.self.query.bias": (0.0806, 0.284, 13.8),
    "1.attention.self.key.weight": (0.0938, 0.727, 27.3),
    "1.attention.self.key.bias": (0.00669, 0.0271, 6.05e-15),
    "1.attention.self.value.weight": (0.0832, 0.584, 43.6),
    "1.attention.self.value.bias": (0.0443, 0.15, 18.9),
    "1.attention.output.dense.weight": (0.0825, 0.669, 58.7),
    "1.attention.output.dense.bias": (0.0363, 0.16, 31.6),
    "1.attention.output.LayerNorm.weight": (0.0971, 0.315, 38.3),
    "1.attention.output.LayerNorm.bias": (0.0458, 0.116, 32.4),
    "1.intermediate.dense.weight": (0.046, 0.38, 29.9),
    "1.intermediate.dense.bias": (0.0274, 0.0868, 13.8),
    "1.output.dense.weight": (0.0518, 0.37, 57.6),
    "1.output.dense.bias": (0.0183, 0.0569, 26.1),
    "1.output.LayerNorm.weight": (0.0849, 0.315, 28),
    "1.output.LayerNorm.bias": (0, 0, 22.1),
}
REF_BF16_GRAD_BIG = {      # 768 / 12 heads / 3072, 2 layers, B = 3, L = 37 (test_gpu_bert.big_model), upstream(mask, 768)
    "1.attention.self.query.weight": (0.0667, 0.93, 30.9),
    "1.attention.self.query.bias": (0.0618, 0.242, 8.74),
    "1.attention.self.key.weight": (0.0665, 1.09, 36.7),
    "1.attention.self.key.bias": (0.00586, 0.0259, 1.02e-14),
    "1.attention.self.value.weight": (0.0661, 0.665, 89.6),
    "1.attention.self.value.bias": (0.0326, 0.1, 22.4),
    "1.attention.output.dense.weight": (0.0665, 0.598, 53.4),
    "1.attention.output.dense.bias": (0.0296, 0.108, 23.9),
    "1.attention.output.LayerNorm.weight": (0.0777, 0.253, 38.8),
    "1.attention.output.LayerNorm.bias": (0.0371, 0.112, 28),
    "1.intermediate.dense.weight": (0.027, 0.285, 36.8),
    "1.intermediate.dense.bias": (0.0166, 0.0647, 12.3),
    "1.output.dense.weight": (0.044, 0.469, 90),
    "1.output.dense.bias": (0.0129, 0.0518, 31.9),
    "1.output.LayerNorm.weight": (0.0718, 0.304, 33.6),
    "1.output.LayerNorm.bias": (0, 0, 27.9),
}


def close_fp32(name, got, ref64):
    """the project's FP32 bounds with atol scaled by the float64 tensor's largest element"""
    ref64 = ref64.double()
    top = float(ref64.abs().max())
    print(f"{name} fp32: max |hip - float64| = {dist(got, ref64)[1]:.3g} at max |float64| = {top:.3g}")
    torch.testing.assert_close(got.detach().double().cpu(), ref64, rtol=FP32["rtol"], atol=FP32["atol"] * top)


def check_grad(name, compute, got, ref64):
    if compute == "fp32":
        close_fp32(name, got, ref64)
    else:
        check(name, compute, got, ref64)


# ------------------------------------------------------------------------------------------------ attention backward
def run_attention_bwd(qkv, mask, dctx, B, L, H, compute, pad=8, extra_rows=3):
    """operands on the device -> dqkv (B * L, 3 H) of a padded, canaried destination; two runs, bit-equal"""
    lib = _lib.load()
    ld = 3 * H + pad
    nbytes = lib.mmdeer_bert_attn_bwd_workspace(B, L, H)
    assert nbytes == 2 * B * (H // 64) * L * 4
    ws = torch.full((nbytes // 4 + 8,), 555.0, device=DEV)
    runs = []
    for _ in range(2):
        buf = torch.full((B * L + extra_rows, ld), 777.0, dtype=qkv.dtype, device=DEV)
        a = _lib.BertAttnBwdArgs()
        a.qkv, a.mask, a.dctx, a.dqkv = qkv.data_ptr(), mask.data_ptr(), dctx.data_ptr(), buf.data_ptr()
        a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
        a.B, a.L, a.H, a.ld_qkv, a.ld_dctx, a.ld_dqkv = B, L, H, qkv.stride(0), dctx.stride(0), ld
        a.act_f32, a.stream = int(compute == "fp32"), _lib.current_stream()
        _lib.check(lib.mmdeer_bert_attn_bwd(C.byref(a)))
        torch.cuda.synchronize()
        assert bool((buf[B * L:] == 777.0).all()) and bool((buf[:, 3 * H:] == 777.0).all()), "the canary behind dqkv was written"
        assert bool((ws[nbytes // 4:] == 555.0).all()), "the canary behind the workspace was written"
        runs.append(buf)
    assert torch.equal(runs[0], runs[1]), "two runs of mmdeer_bert_attn_bwd differ"
    return runs[0][:B * L, :3 * H]


def attention_bwd_case(B, L, heads, compute, scale=1.0, seed=0):
    H = 64 * heads
    gen = torch.Generator().manual_seed(2000 * L + heads + seed)
    qkv = torch.randn(B * L, 3 * H + 8, generator=gen)
    qkv[:, :2 * H] *= scale
    dctx = torch.randn(B * L, H + 8, generator=gen)
    return H, gen, qkv.to(dtype_of(compute)), dctx.to(dtype_of(compute))     # the operator's inputs ARE the stored tensors


def attention_bwd_check(name, qkv, dctx, mask, B, L, H, compute, dead=()):
    """one mask: the reference, the run, zeros where they must be exact, the bound on the rest"""
    m64 = mask.reshape(-1).double()
    ref = RB.attention_bwd(qkv.double(), m64, dctx[:, :H], B, L, H)
    got = run_attention_bwd(qkv.to(DEV), m64.float().to(DEV), dctx.to(DEV), B, L, H, compute)
    assert bool(torch.isfinite(got).all())
    masked = (m64 == 0).nonzero().flatten().to(DEV)
    assert bool((got[masked][:, H:] == 0).all()) and bool((ref[masked.cpu()][:, H:] == 0).all()), "dK / dV of a masked key must be exact zeros"
    live = torch.ones(B * L, dtype=torch.bool)
    for b in dead:                                    # a sample without a valid key: exact zeros everywhere
        assert bool((got[b * L:(b + 1) * L] == 0).all()) and bool((ref[b * L:(b + 1) * L] == 0).all())
        live[b * L:(b + 1) * L] = False
    check_grad(name, compute, got[live.to(DEV)], ref[live])
    for i, part in enumerate(("dQ", "dK", "dV")):     # and each on its own scale: dV is the largest of the three
        if float(ref[live][:, i * H:(i + 1) * H].abs().max()) > 0:
            check_grad(f"{name} {part}", compute, got[live.to(DEV)][:, i * H:(i + 1) * H], ref[live][:, i * H:(i + 1) * H])


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
@pytest.mark.parametrize("L,heads", [(1, 2), (37, 2), (64, 2), (65, 2), (129, 2), (37, 12)])
def test_attention_backward_against_float64(L, heads, compute):
    B = 2
    H, gen, qkv, dctx = attention_bwd_case(B, L, heads, compute, scale=1.5)
    for name, mask in masks_for(L, gen).items():
        attention_bwd_check(f"attn_bwd L={L} heads={heads} {name}", qkv, dctx, mask, B, L, H, compute, dead=(0,) if name == "dead" else ())


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_attention_backward_at_512_tokens(compute):
    B, L, heads = 1, 512, 2
    H, gen, qkv, dctx = attention_bwd_case(B, L, heads, compute, scale=1.5)
    mask = (torch.rand(1, L, generator=gen) < 0.6).float()
    mask[0, 128:256] = 0                              # a whole key tile (and two whole 64-key workgroups) without a valid key
    mask[0, 500:] = 0
    attention_bwd_check("attn_bwd L=512", qkv, dctx, mask, B, L, H, compute)


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_attention_backward_with_large_scores(compute):
    """raw scores q . k up to +-80: every exponent stays at or below zero"""
    B, L, heads = 2, 129, 2
    H, gen, qkv, dctx = attention_bwd_case(B, L, heads, compute, seed=7)
    q, k = (qkv[:, i * H:(i + 1) * H].double().reshape(B, L, heads, 64).permute(0, 2, 1, 3) for i in range(2))
    top = float((q @ k.transpose(-1, -2)).abs().max())
    qkv[:, :H] = (qkv[:, :H].double() * (82.0 / top)).to(qkv.dtype)
    q = qkv[:, :H].double().reshape(B, L, heads, 64).permute(0, 2, 1, 3)
    raw = q @ k.transpose(-1, -2)
    assert float(raw.abs().max()) > 79 and float(raw.max()) > 60 and float(raw.min()) < -60
    attention_bwd_check("attn_bwd, scores to +-80", qkv, dctx, masks_for(L, gen)["holes"], B, L, H, compute)


# ------------------------------------------------------------------------------------------------ add + LN backward
def run_add_ln_bwd(y, x, g, g2, gamma, M, N, compute, sums, eps=1e-12):
    """device operands (padded) -> (ds (M, N), dgamma, dbeta); canaries behind every output, two runs bit-equal"""
    lib = _lib.load()
    runs = []
    for _ in range(2):
        ds = torch.full((M + 2, N + 12), 777.0, dtype=y.dtype, device=DEV)
        dgb = torch.full((2, N + 4), 777.0, device=DEV)
        need = lib.mmdeer_bert_add_ln_bwd_scratch(M, N)
        scratch = torch.full((need + 4,), 555.0, device=DEV)
        a = _lib.BertAddLnBwdArgs()
        a.y, a.x, a.g, a.g2, a.gamma, a.ds = y.data_ptr(), _lib.ptr(x), g.data_ptr(), _lib.ptr(g2), gamma.data_ptr(), ds.data_ptr()
        if sums:
            a.dgamma, a.dbeta, a.scratch, a.scratch_elems = dgb[0].data_ptr(), dgb[1].data_ptr(), scratch.data_ptr(), need
        a.eps, a.M, a.N, a.ld_y, a.ld_g, a.ld_ds = eps, M, N, y.stride(0), g.stride(0), N + 12
        a.ld_x, a.ld_g2 = (x.stride(0) if x is not None else 0), (g2.stride(0) if g2 is not None else 0)
        a.act_f32, a.stream = int(compute == "fp32"), _lib.current_stream()
        _lib.check(lib.mmdeer_bert_add_ln_bwd(C.byref(a)))
        torch.cuda.synchronize()
        assert bool((ds[M:] == 777.0).all()) and bool((ds[:, N:] == 777.0).all()) and bool((dgb[:, N:] == 777.0).all()) and bool((scratch[need:] == 555.0).all())
        if not sums:
            assert bool((dgb == 777.0).all()) and bool((scratch == 555.0).all())
        runs.append((ds, dgb))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "two runs of mmdeer_bert_add_ln_bwd differ"
    return runs[0][0][:M, :N], runs[0][1][0, :N], runs[0][1][1, :N]


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
@pytest.mark.parametrize("N", [4, 64, 128, 768, 1024])
@pytest.mark.parametrize("M", [1, 5, 67, 4099])
def test_add_ln_backward_against_float64(M, N, compute):
    """M = 4099 is past the 1024 workgroups x 4 waves of the column sums: a wave then owns several rows.  Row 0 has variance about
    1e-6 (eps = 1e-5 would shrink its rstd by a factor of 3.3); no row is constant; gamma has an exact zero."""
    gen = torch.Generator().manual_seed(3 * M + N)
    dt = dtype_of(compute)
    y, x = torch.randn(M, N + 4, generator=gen), torch.randn(M, N + 8, generator=gen)
    y[0], x[0] = 7e-4 * y[0], 7e-4 * x[0]
    g, g2 = torch.randn(M, N + 8, generator=gen), torch.randn(M, N + 4, generator=gen)
    y, x, g, g2 = (t.to(dt) for t in (y, x, g, g2))
    gamma, beta = torch.rand(N, generator=gen) + 0.5, torch.zeros(N)
    gamma[N // 2] = 0.0
    if N > 4:
        assert 2e-7 < float((y[0, :N].double() + x[0, :N].double()).var()) < 4e-6
    dev = {k: v.to(DEV) for k, v in dict(y=y, x=x, g=g, g2=g2, gamma=gamma).items()}
    for use_x, use_g2, sums in ((True, True, True), (False, False, False), (True, False, True), (False, True, False)):
        name = f"add_ln_bwd M={M} N={N} x={use_x} g2={use_g2} sums={sums}"
        ref_ds, ref_dg, ref_db = RB.add_ln_bwd(y[:, :N], x[:, :N] if use_x else None, g[:, :N], g2[:, :N] if use_g2 else None, gamma, beta, 1e-12)
        ds, dg, db = run_add_ln_bwd(dev["y"], dev["x"] if use_x else None, dev["g"], dev["g2"] if use_g2 else None, dev["gamma"], M, N, compute, sums)
        assert bool(torch.isfinite(ds).all())
        check_grad(name + ", the small-variance row", compute, ds[:1], ref_ds[:1])
        if M > 1:
            check_grad(name, compute, ds[1:], ref_ds[1:])
        if sums:                                      # fp32 sums of fp32 products in both compute dtypes: the fp32 bound
            close_fp32(name + " dgamma", dg, ref_dg)
            close_fp32(name + " dbeta", db, ref_db)
            assert float(ref_dg[N // 2].abs()) > 0 and float(dg[N // 2].abs()) > 0         # xhat is not taken from an output that gamma = 0 wiped


# ------------------------------------------------------------------------------------------------ GELU backward
GELU_BWD_TOL = 4e-6     # fp32 erff and expf are good to a few ulp at values below 1.13, three more roundings, times |g| <= 2


def test_gelu_backward_is_the_erf_forms():
    gen = torch.Generator().manual_seed(9)
    M, N = 5, 244                                     # ragged: no multiple of a workgroup's 1024 elements, padded rows
    grid = torch.cat([torch.tensor([0.0, 0.75, -0.75, 3.0, -3.0, 10.0, -10.0]), 3.0 * torch.randn(M * N - 7, generator=gen)])
    for compute in ("fp32", "bf16"):
        dt = dtype_of(compute)
        x = grid.reshape(M, N).to(dt)
        g = (4.0 * torch.rand(M, N, generator=gen) - 2.0).to(dt)
        ref = RB.gelu_bwd(x.double(), g.double())
        other = float((RB.gelu_tanh_bwd(x.double(), g.double()) - ref).abs().max())
        if compute == "fp32":
            assert other > 10 * GELU_BWD_TOL, other   # the bound tells the two derivative forms apart
        xb, gb = torch.full((M + 1, N + 4), 777.0, dtype=dt, device=DEV), torch.full((M + 1, N + 8), 777.0, dtype=dt, device=DEV)
        xb[:M, :N], gb[:M, :N] = x.to(DEV), g.to(DEV)
        out = torch.full((M + 1, N + 12), 777.0, dtype=dt, device=DEV)
        a = _lib.BertGeluBwdArgs()
        a.x, a.g, a.dx, a.M, a.N, a.ld_x, a.ld_g, a.ld_dx = xb.data_ptr(), gb.data_ptr(), out.data_ptr(), M, N, N + 4, N + 8, N + 12
        a.act_f32, a.stream = int(compute == "fp32"), _lib.current_stream()
        _lib.check(_lib.load().mmdeer_bert_gelu_bwd(C.byref(a)))
        a.dx, a.ld_dx = gb.data_ptr(), N + 8          # and in place over g
        _lib.check(_lib.load().mmdeer_bert_gelu_bwd(C.byref(a)))
        torch.cuda.synchronize()
        assert torch.equal(out[:M, :N], gb[:M, :N])
        for buf in (out, gb, xb):
            assert bool((buf[M:] == 777.0).all()) and bool((buf[:, N:] == 777.0).all())
        assert torch.equal(xb[:M, :N], x.to(DEV))
        if compute == "fp32":
            err = float((out[:M, :N].double().cpu() - ref).abs().max())
            print(f"gelu_bwd fp32: max |hip - erf form| = {err:.3g}; the tanh form's derivative is {other:.3g} away")
            assert err <= GELU_BWD_TOL
        else:
            check("gelu_bwd", compute, out[:M, :N], ref)


# ------------------------------------------------------------------------------------------------ the module
def encoder(config, sd, compute, k):
    enc = bert.BertEncoder(config, compute_dtype=compute, finetune_layers=k)
    enc.load_state_dict({n: v.float() for n, v in sd.items()}, strict=True)
    return enc.to(DEV)


@functools.lru_cache(maxsize=None)
def tiny_grads(rounded=False):
    sd, ids, mask, typ, _ = golden()
    return RB.trunk_grads(sd, ids, mask, typ, upstream(mask, 128), rnd=R.bf16_round if rounded else R.ident)[1]


@functools.lru_cache(maxsize=None)
def big_grads(rounded=False):
    sd, ids, mask, _ = big_model()
    return RB.trunk_grads(sd, ids, mask, None, upstream(mask, 768), rnd=R.bf16_round if rounded else R.ident)[1]


def grad_bound(recorded, key):
    """(rms, max) that a bf16 gradient may be from float64, or None where the storage-only distance says nothing:
    - output.LayerNorm.bias of the TOP layer: its gradient is the column sum of the upstream gradient itself, no stored bf16 tensor in
      between, so the restatement's distance is exactly 0; the HIP value is an fp32 sum of bf16-exact terms and is held to the fp32 bound.
    - key.bias: analytically zero (a shift of all scores of a row leaves the softmax alone), about 1e-14 in float64; what the
      table holds for it is rounding noise of the same sums that form query.bias, so it is held to query.bias's distance."""
    rms, mx, _ = recorded[key.replace(".key.bias", ".query.bias")]
    return None if rms == 0 else (BF16_RMS * rms, BF16_MAX * mx)


def test_bf16_gradient_distances_are_the_recorded_ones():
    """the constants the bf16 module tests are held to, recomputed on the CPU (no launch); tolerances as in
    test_gpu_bert.test_bf16_reference_distances_are_the_recorded_ones (rms 5 %, max, one element, 25 %)"""
    for recorded, g64, g16 in ((REF_BF16_GRAD_TINY, tiny_grads(), tiny_grads(True)), (REF_BF16_GRAD_BIG, big_grads(), big_grads(True))):
        for key, (rms, mx, top) in recorded.items():
            got = dist(g16["encoder.layer." + key], g64["encoder.layer." + key])
            if key.endswith(".key.bias"):             # noise around zero: its order of magnitude only
                assert float(g64["encoder.layer." + key].abs().max()) < 1e-12 and 0.2 * rms < got[0] < 5 * rms, (key, got)
                continue
            assert got[0] == pytest.approx(rms, rel=0.05, abs=1e-12) and got[1] == pytest.approx(mx, rel=0.25, abs=1e-12), (key, got, rms, mx)
            assert float(g64["encoder.layer." + key].abs().max()) == pytest.approx(top, rel=0.01)


def module_case(which, compute, k):
    if which == "tiny":
        sd, ids, mask, typ, _ = golden()
        return TINY, sd, ids, mask, typ, 128, tiny_grads(), REF_BF16_GRAD_TINY
    sd, ids, mask, _ = big_model()
    return BIG, sd, ids, mask, None, 768, big_grads(), REF_BF16_GRAD_BIG


def backward_once(enc, ids, mask, typ, up):
    for p in enc.parameters():
        p.grad = None
    out = enc(ids.to(DEV), mask.to(DEV), None if typ is None else typ.to(DEV), output_hidden_states=True)
    (out.last_hidden_state.float() * up.float().to(DEV)).sum().backward()
    torch.cuda.synchronize()
    return out, {n: (None if p.grad is None else p.grad.clone()) for n, p in enc.named_parameters()}


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
@pytest.mark.parametrize("which,k", [("tiny", 1), ("tiny", 2), ("big", 1)])
def test_finetuned_trunk_gradients(which, k, compute):
    config, sd, ids, mask, typ, H, ref, recorded = module_case(which, compute, k)
    up = upstream(mask, H)
    enc, frozen = encoder(config, sd, compute, k), encoder(config, sd, compute, 0)
    first_tail = config["num_hidden_layers"] - k
    out, grads = backward_once(enc, ids, mask, typ, up)
    plain = frozen(ids.to(DEV), mask.to(DEV), None if typ is None else typ.to(DEV), output_hidden_states=True)
    assert out.last_hidden_state.requires_grad and not plain.last_hidden_state.requires_grad
    assert torch.equal(out.last_hidden_state, plain.last_hidden_state), "the tail's forward must store the frozen trunk's bits"
    assert len(out.hidden_states) == len(plain.hidden_states) == config["num_hidden_layers"] + 1
    assert all(torch.equal(a, b) and not a.requires_grad for a, b in zip(out.hidden_states, plain.hidden_states))
    with torch.no_grad():                             # and without grad the fine-tuned module runs the frozen path
        assert torch.equal(enc(ids.to(DEV), mask.to(DEV), None if typ is None else typ.to(DEV)).last_hidden_state, plain.last_hidden_state)
    failures = []
    for n, p in enc.named_parameters():
        in_tail = n.startswith("encoder.layer.") and int(n.split(".")[2]) >= first_tail
        assert p.requires_grad == in_tail
        if not in_tail:
            assert grads[n] is None, n
            continue
        g = grads[n]
        assert g is not None and g.dtype == p.dtype and g.shape == p.shape and bool(torch.isfinite(g).all()), n
        bound = grad_bound(recorded, n[len("encoder.layer."):]) if compute == "bf16" else None
        if compute == "fp32" and n.endswith(".key.bias"):
            key_bias_fp32(n, g, ref)
        elif bound is None:
            close_fp32(f"{which} k={k} {compute} {n}", g, ref[n])
        else:
            rms, mx = dist(g, ref[n])
            print(f"{which} k={k} bf16 {n}: rms {rms:.3g} max {mx:.3g}; allowed {bound[0]:.3g} / {bound[1]:.3g}")
            if not (rms <= bound[0] and mx <= bound[1]):
                failures.append((n, rms, mx, bound))
    assert not failures, failures
    _, again = backward_once(enc, ids, mask, typ, up)
    assert all((grads[n] is None and again[n] is None) or torch.equal(grads[n], again[n]) for n in grads), "two backward runs differ"


def key_bias_fp32(n, g, ref):
    """fp32: key.bias's gradient is analytically zero, so the bound's atol is scaled by query.bias's largest element"""
    top = float(ref[n.replace(".key.bias", ".query.bias")].abs().max())
    print(f"{n} fp32: max |hip| = {float(g.abs().max()):.3g} (analytically zero) at max |query.bias gradient| = {top:.3g}")
    assert float(g.abs().max()) <= FP32["atol"] * top


def test_a_frozen_tail_parameter_gets_no_gradient_and_the_lowest_layer_moves_up():
    sd, ids, mask, typ, _ = golden()
    enc = encoder(TINY, sd, "fp32", 2)
    full = backward_once(enc, ids, mask, typ, upstream(mask, 128))[1]
    off = ["encoder.layer.1.intermediate.dense.weight", "encoder.layer.1.output.LayerNorm.bias"] + [n for n, _ in enc.named_parameters() if n.startswith("encoder.layer.0.")]
    for n in off:
        enc.get_parameter(n).requires_grad_(False)
    part = backward_once(enc, ids, mask, typ, upstream(mask, 128))[1]
    for n in full:
        if n in off or not n.startswith("encoder.layer."):
            assert part[n] is None, n
        else:                                         # the others are the same sums, bit for bit
            assert torch.equal(part[n], full[n]), n


def test_a_step_on_the_tail_repacks_the_tail_only():
    sd, ids, mask, typ, _ = golden()
    enc = encoder(TINY, sd, "bf16", 1)
    dids, dmask, dtyp = ids.to(DEV), mask.to(DEV), typ.to(DEV)
    first_out = enc(dids, dmask, dtyp).last_hidden_state.detach().clone()
    first = enc._packed
    enc(dids, dmask, dtyp)
    assert enc._packed is first
    with torch.no_grad():
        enc.encoder.layer[1].output.dense.weight.mul_(0.5)
    second_out = enc(dids, dmask, dtyp).last_hidden_state.detach()
    second = enc._packed
    assert second is not first and second["emb"] is first["emb"] and second["layers"][0] is first["layers"][0]
    assert second["layers"][1] is not first["layers"][1] and not torch.equal(second["layers"][1]["wo2"], first["layers"][1]["wo2"])
    assert float((second_out - first_out).abs().max()) > 1e-2


# ------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_text_encoder_trains_the_trunks_tail(compute):
    """TemporalTextEncoder(bert=trunk) with finetune_layers = 1 at width 768 (1 layer, B = 3, L = 9): the gradient reaches the trunk's
    tail through forward_embeddings, and four plain SGD steps on the trunk's tail alone lower the loss every time.  The step is
    fixed once from the first gradient so that a first-order model lowers the loss by a fifth per step; the encoder is in eval mode
    (its own dropout masks would change the loss from step to step; the trunk has none)."""
    torch.manual_seed(5)
    cfg = dict(vocab_size=97, hidden_size=768, num_hidden_layers=1, num_attention_heads=12, intermediate_size=3072, max_position_embeddings=16)
    trunk = bert.BertEncoder(cfg, compute_dtype=compute, finetune_layers=1)
    with torch.no_grad():
        for n, p in trunk.named_parameters():         # livelier than initializer_range = 0.02: scores with a spread, non-trivial LayerNorms
            if "LayerNorm.weight" in n:
                p.copy_(0.5 + torch.rand_like(p))
            elif n.startswith("embeddings.") and n.endswith("weight"):
                p.copy_(0.5 * torch.randn_like(p))
            elif n.endswith("weight"):
                p.copy_(torch.randn_like(p) / p.shape[1] ** 0.5)
    enc = text.TemporalTextEncoder({"hidden_dim": 512}, compute, bert=trunk).to(DEV).eval()
    gen = torch.Generator().manual_seed(6)
    ids = torch.randint(1, 97, (3, 9), generator=gen).to(DEV)
    mask = torch.ones(3, 9)
    mask[1, 5:] = 0
    mask[2, 1::2] = 0
    mask = mask.to(DEV)
    target = torch.randn(3, 512, generator=gen).to(DEV)
    tail = [p for n, p in enc.named_parameters() if n.startswith("bert.encoder.layer.0.")]
    assert len(tail) == 16 and all(p.requires_grad for p in tail)
    assert list(enc.state_dict()) == ["bert." + k for k in trunk.state_dict()] + [k for k in text.TemporalTextEncoder().state_dict()
                                                                                   if not k.startswith(("embedding.", "positional_encoding."))]
    with torch.no_grad():                             # grad disabled: the frozen path, no graph
        assert not enc(ids, mask).requires_grad
    losses, lr = [], None
    for step in range(5):
        for p in enc.parameters():
            p.grad = None
        loss = (enc(ids, mask) - target).square().mean()
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
    print(f"text encoder + trunk tail, {compute}: loss before and after each of four SGD steps on the trunk's tail: " + ", ".join(f"{v:.6g}" for v in losses))
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
