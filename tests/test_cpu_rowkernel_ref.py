"""The float64 restatements of tests/rowkernel_ref.py are right, and the comparison the GPU tests make with them has teeth.

 * they agree with oracle.deer_oracle (k_ln_fwd, k_ln_bwd, k_tri_fwd, k_tri_bwd, cross_modal_attention, lstm_t1_bidir) where it has the
   same operation, and every hand-written backward agrees with autograd of its forward;
 * the same formulas in float32 on the CPU pass the comparison at half the constants K of rowkernel_ref.K over all cases of
   tests/test_gpu_rowkernels.py (the worst ratios are printed: pytest -s), and eleven seeded errors are rejected;
 * the staged statement of the fused in_proj + attention kernel (csrc/tri_fused.hip) agrees with k_tri_fwd / k_tri_bwd behind a float64
   in_proj, its float32 evaluation passes at K / 2 over all cases of tests/test_gpu_fused_attention.py, and twelve seeded errors are rejected;
 * the dropout draw, restated in uint32 arithmetic, is statistically a Bernoulli(thresh / 2^32) field without row, column, site, seed
   or offset structure (|z| < 6), and its threshold has the stated edges;
 * convert() is round-to-nearest-even.
"""
import math

import numpy as np
import pytest
import torch

from oracle import deer_oracle as O

from . import rowkernel_ref as R

F32, F64 = torch.float32, torch.float64
WORST = {}


def _measure(family, pairs):
    """pairs: (name, float32 value, float64 SV, bf16-stored).  Half of K must hold for the float32 CPU evaluation."""
    log = []
    for name, v32, ref, bf in pairs:
        R.assert_close(name, bf16(v32) if bf else v32, ref, R.K[family] / 2, bf16=bf, log=log)
    w = max(r for _, r in log)
    WORST[family] = max(WORST.get(family, 0.0), w)
    return w


def bf16(x):
    return R.bf16_round(x.float())


# =========================================================================== K: the float32 CPU evaluation over the GPU tests' cases
@pytest.mark.parametrize("bf", [False, True], ids=["fp32", "bf16"])
def test_float32_layernorm_is_within_half_of_K(bf):
    for M, N in R.ln_shapes():
        y, dout, gamma, beta = R.ln_inputs(M, N, bf)
        f, f32 = R.ln_fwd(y, gamma, beta), R.ln_fwd(y, gamma, beta, F32)
        _measure("ln_fwd", [("out", f32["out"].v, f["out"], bf), ("mean", f32["mean"].v, f["mean"], False),
                            ("rstd", f32["rstd"].v, f["rstd"], False)])
        mean, rstd = f["mean"].v.float(), f["rstd"].v.float()
        b, b32 = R.ln_bwd(dout, y, mean, rstd, gamma, 0.0), R.ln_bwd(dout, y, mean, rstd, gamma, 0.0, F32)
        pairs = [(k, b32[k].v, b[k], False) for k in ("dgamma", "dbeta", "slab")]
        for ms in R.LN_MASK_SCALES:
            pairs.append((f"dz[{ms:.3g}]", R.ln_mask(b32["_dy"], y, ms).v, R.ln_mask(b["_dy"], y, ms), bf))
        _measure("ln_bwd", pairs)
    print(f"\nfloat32 CPU worst ratios ({'bf16' if bf else 'fp32'} storage): ln_fwd {WORST['ln_fwd']:.2f}  ln_bwd {WORST['ln_bwd']:.2f}")


@pytest.mark.parametrize("bf", [False, True], ids=["fp32", "bf16"])
def test_float32_trimodal_attention_is_within_half_of_K(bf):
    for B in R.TRI_B:
        for cls in R.TRI_CLASSES:
            qkv, dobar = R.tri_inputs(B, cls, bf)
            for p in R.TRI_P:
                keep, av = R.tri_keep(B, p, R.TRI_SEED, R.TRI_OFFSET) if p > 0 else (None, None)
                f, f32 = R.tri_attn(qkv, keep, p, av), R.tri_attn(qkv, keep, p, av, F32)
                _measure("tri_fwd", [("obar", f32["obar"].v, f["obar"], bf)] + [(k, f32[k].v, f[k], False) for k in ("probs", "attn_w", "av_w")])
                probs = f["probs"].v.float()
                _measure("tri_bwd", [("dqkv", R.tri_attn_bwd(qkv, dobar, probs, keep, p, F32).v, R.tri_attn_bwd(qkv, dobar, probs, keep, p), bf)])
    print(f"\nfloat32 CPU worst ratios ({'bf16' if bf else 'fp32'} storage): tri_fwd {WORST['tri_fwd']:.2f}  tri_bwd {WORST['tri_bwd']:.2f}")


@pytest.mark.parametrize("bf", [False, True], ids=["fp32", "bf16"])
def test_float32_side_rows_are_within_half_of_K(bf):
    for B in R.CROSS_B:
        for cls in R.CROSS_CLASSES:
            a = R.cross_inputs(B, cls, bf)
            f, f32 = R.cross_modal_attn(*a[:6]), R.cross_modal_attn(*a[:6], dt=F32)
            _measure("cross_fwd", [(k, f32[k].v, f[k], False) for k in ("out_a", "out_v")])
            b, b32 = R.cross_modal_attn_bwd(*a), R.cross_modal_attn_bwd(*a, dt=F32)
            _measure("cross_bwd", [(k, b32[k].v, b[k], bf and k != "dgl") for k in b])
    for B, H, nd, cls in R.lstm_cases():
        gates, dout = R.lstm_inputs(B, H, nd, cls, bf)
        _measure("lstm", [("h", R.lstm_cell_t1(gates, H, nd, F32).v, R.lstm_cell_t1(gates, H, nd), bf),
                          ("dgates", R.lstm_cell_t1_bwd(gates, dout, H, nd, F32).v, R.lstm_cell_t1_bwd(gates, dout, H, nd), bf)])
    print(f"\nfloat32 CPU worst ratios ({'bf16' if bf else 'fp32'} storage): cross_fwd {WORST['cross_fwd']:.2f}  "
          f"cross_bwd {WORST['cross_bwd']:.2f}  lstm {WORST['lstm']:.2f}")


# =========================================================================== the fused in_proj + attention kernel (csrc/tri_fused.hip)
def _fused_stages(B, cls, p, seed, offset, dt=F64, tile=None, variant=None):
    """the staged statement of rowkernel_ref for one case -> dict of SV (tile, probs, obar, attn_w, av_w, dqkv) and the largest score
    gap.  `tile`: the stored q|k|v the probabilities are formed from (the GPU test passes the kernel's; here the float32 evaluation's);
    the backward takes the float32 probabilities formed from that tile as its saved ones."""
    x, bias, dobar = R.fused_inputs(B, cls)
    keep, av = R.tri_keep(B, p, seed, offset) if p > 0 else (None, None)
    proj = R.fused_proj_of(B, cls, dt) if variant is None else R.fused_proj(x, R.fused_weights()[0], bias, dt, variant)
    if tile is None:
        tile = bf16(R.fused_proj_of(B, cls, F32).v)
    saved = R.fused_probs(tile, keep, p, F32)[0].v
    if variant == "unrounded_qk":
        probs, gap = R.fused_probs(proj.v, keep, p, dt)
    else:
        probs, gap = R.fused_probs(tile, keep, p, dt, variant)
    f = R.tri_attn(proj, keep, p, av, dt, variant, probs=probs)
    out = {"tile": proj, "probs": probs, "obar": f["obar"], "attn_w": f["attn_w"], "av_w": f["av_w"],
           "dqkv": R.tri_attn_bwd(proj, dobar, saved, keep, p, dt, variant)}
    return out, gap


_FUSED_FAMILY = {"tile": ("fused_tile", True), "probs": ("fused_probs", False), "obar": ("fused_ctx", True), "attn_w": ("fused_ctx", False),
                 "av_w": ("fused_ctx", False), "dqkv": ("fused_bwd", True)}


def test_float32_fused_attention_is_within_half_of_K():
    """every case of tests/test_gpu_fused_attention.py: the float32 evaluation of the kernel's formula (the accumulator starts at the
    bias and takes 16 steps of 32 exact products; q and k rounded to bf16 in front of the scores) passes at K / 2; the classes reach the
    score gaps they are there for."""
    gaps, floor = {}, {}
    for B in R.FUSED_B:
        for cls, p, seed, offset in R.fused_cases(B):
            ref, gap = _fused_stages(B, cls, p, seed, offset)
            f32, _ = _fused_stages(B, cls, p, seed, offset, F32)
            gaps[cls] = max(gaps.get(cls, 0.0), gap)
            for key, (family, bf) in _FUSED_FAMILY.items():
                floor[family] = max(floor.get(family, 0.0), _measure(family, [(f"B={B} {cls} p={p} {key}", f32[key].v, ref[key], bf)]))
            if cls in ("identical_tokens", "x_zero"):
                assert bool((f32["probs"].v == 0.5).all())
    print("\nfloat32 CPU worst ratios: " + "  ".join(f"{k} {v:.2f}" for k, v in floor.items()))
    print("largest score gap after the 1/8: " + "  ".join(f"{k} {v:.1f}" for k, v in gaps.items()))
    clamp_at = R.EXP2_CLAMP / R.LOG2E                                                            # 79.7
    assert 60 < gaps["saturated"] < clamp_at - 1 and gaps["normal"] < 20 and gaps["bias_zero"] < 20
    assert gaps["clamp_x4"] > 160 and gaps["clamp_qbias40"] > 160
    # K: twice the float32 figure rounded up to the next half, at least 8 for the families that contain the projection
    for family, at_least in (("fused_tile", 8.0), ("fused_probs", 0.0), ("fused_ctx", 8.0), ("fused_bwd", 8.0)):
        assert R.K[family] == max(at_least, math.ceil(4 * floor[family]) / 2), (family, floor[family])


FUSED_VARIANTS = [  # variant, the output that shows it, a case of the GPU file: (B, class, p)
    ("no_bias", "tile", (2, "normal", 0.0)), ("bias_qk_swap", "tile", (2, "normal", 0.0)), ("wn_swap", "tile", (2, "normal", 0.0)),
    ("unrounded_qk", "probs", (129, "normal", 0.0)), ("no_scale", "probs", (2, "normal", 0.0)), ("drop_before", "probs", (2, "normal", 0.3)),
    ("keep_swap", "obar", (129, "normal", 0.3)), ("no_half", "obar", (2, "normal", 0.0)), ("no_clamp", "probs", (2, "clamp_x4", 0.0)),
    ("dk_transposed", "dqkv", (2, "normal", 0.3)), ("dv_no_keep", "dqkv", (2, "normal", 0.3)), ("ds_no_scale", "dqkv", (2, "normal", 0.0))]


@pytest.mark.parametrize("variant,key,case", FUSED_VARIANTS, ids=[v[0] for v in FUSED_VARIANTS])
def test_seeded_fused_attention_errors_are_rejected(variant, key, case):
    """twelve errors the kernel could hold, each shown by one output on a case of the GPU file, at the K the GPU test uses; the float32
    evaluation of the right formula passes there.  `unrounded_qk` proves that the comparison pins the rounding point in front of the
    scores.  (v rounded to bf16 in front of P V is NOT on the list: it moves obar by less than obar's own bf16 cell.)"""
    B, cls, p = case
    seed, offset = next((s, o) for c, pp, s, o in R.fused_cases(B) if c == cls and pp == p)
    family, bf = _FUSED_FAMILY[key]
    ref, _ = _fused_stages(B, cls, p, seed, offset)
    f32, _ = _fused_stages(B, cls, p, seed, offset, F32)
    bad, _ = _fused_stages(B, cls, p, seed, offset, variant=variant)
    store = (lambda t: bf16(t)) if bf else (lambda t: t.float())
    assert not R.rejects(key, store(f32[key].v), ref[key], R.K[family], bf)
    assert R.rejects(key, store(bad[key].v), ref[key], R.K[family], bf)


@pytest.mark.parametrize("p", [0.0, 0.3])
def test_fused_attention_stages_agree_with_the_oracle_and_with_autograd(p):
    """the staged statement against oracle.deer_oracle: k_tri_fwd / k_tri_bwd behind their float64 in_proj (the oracle rounds q and k
    to bf16 itself: the tile handed to fused_probs is that rounding); the restated backward on an SV is autograd of the forward."""
    B, cls = 5, "normal"
    g = R._gen("oracle tie", 17)
    x, dobar = R.bf16_round(torch.randn(2 * B, 512, generator=g)).double(), R.bf16_round(torch.randn(B, 512, generator=g)).double()
    w, bias = R.fused_weights()
    keep, av = R.tri_keep(B, p, 1234, 5) if p > 0 else (None, None)
    proj = R.fused_proj(x, w, bias)
    assert _rel(proj.v, x @ R.bf16_round(w).double().t() + bias.double()) < 1e-14
    assert bool((proj.s >= (x.abs() @ R.bf16_round(w).double().abs().t() + bias.double().abs())).all())
    probs, gap = R.fused_probs(bf16(proj.v))
    prob_o, obar_o = O.k_tri_fwd(x.view(B, 2, 512), w.double(), bias.double(), mask=keep, p=p)
    assert gap < 20 and _rel(probs.v, prob_o) < 1e-12
    f = R.tri_attn(proj, keep, p, av, probs=probs)
    assert float(((f["obar"].v - obar_o).abs() - 2.0 ** -8 * f["obar"].v.abs()).max()) <= 0          # the oracle's obar is bf16-rounded
    dq_o = O.k_tri_bwd(x.view(B, 2, 512), w.double(), bias.double(), dobar, prob_o, mask=keep, p=p).reshape(2 * B, 1536)
    mine = R.tri_attn_bwd(proj, dobar, prob_o, keep, p)
    assert float(((mine.v - dq_o).abs() - 2.0 ** -8 * mine.v.abs()).max()) <= 0
    # autograd through the SV path (the unstaged forward: its own softmax of the unrounded q, k, whose probabilities are the saved ones)
    leaf = proj.v.clone().requires_grad_(True)
    ff = R.tri_attn(R.SV(leaf, proj.s), keep, p, av)
    (ff["obar"].v * dobar).sum().backward()
    assert _rel(R.tri_attn_bwd(proj, dobar, ff["probs"].v.detach(), keep, p).v, leaf.grad) < 1e-12
    # the clamp: a losing key keeps 2^-115, the winner 1; without it the true probability is far below
    t = torch.zeros(2, 1536)
    t[0, 0], t[1, 0], t[0, 512], t[1, 512] = 32.0, -32.0, -32.0, 32.0                             # head 0: q_t . k_t = -1024, gap 256
    pc = R.fused_probs(t)[0].v[0, 0]
    assert pc[0, 1] == 1.0 and pc[1, 0] == 1.0 and pc[0, 0] == 2.0 ** -115 and pc[1, 1] == 2.0 ** -115
    assert R.fused_probs(t, variant="no_clamp")[0].v[0, 0, 0, 0] < 1e-100
    t[0, 512], t[1, 512] = 32.0, -32.0                                                            # q_t . k_t = +1024
    pw = R.fused_probs(t)[0].v[0, 0]                                                              # the winner's side is not clamped
    assert pw[0, 0] == 1.0 and 0 < pw[0, 1] < 1e-100


def test_fused_weight_image_restatement_is_the_documented_permutation():
    """row 192 h + 96 wn + 32 part + dd <- row 512 part + 64 h + 32 wn + dd, a bijection on the 1536 rows, values through convert()."""
    w = torch.arange(1536 * 512, dtype=torch.float32).reshape(1536, 512) * 0.5 + 1.0
    bits = w.view(torch.int32).numpy().view(np.uint32)
    img = torch.from_numpy(R.fused_weight_image(bits).view(np.int16)).view(torch.bfloat16)
    want = w.bfloat16().view(3, 8, 2, 32, 512).permute(1, 2, 0, 3, 4).reshape(1536, 512)
    assert torch.equal(img.view(torch.int16), want.view(torch.int16))


# =========================================================================== seeded errors
def _ln_case():
    M, N = 17, 1020
    y, dout, gamma, beta = R.ln_inputs(M, N, False)
    classes = {R.ln_row_class(i, M, N) for i in range(M)}
    assert classes == set(range(len(R.LN_CLASSES)))                     # every row class is in this case
    return y, dout, gamma, beta


@pytest.mark.parametrize("variant,key", [("unbiased", "rstd"), ("unbiased", "out"), ("no_eps", "rstd"), ("no_eps", "out")])
def test_seeded_layernorm_forward_errors_are_rejected(variant, key):
    y, dout, gamma, beta = _ln_case()
    f = R.ln_fwd(y, gamma, beta)
    assert not R.rejects(key, R.ln_fwd(y, gamma, beta, F32)[key].v, f[key], R.K["ln_fwd"])
    assert R.rejects(key, R.ln_fwd(y, gamma, beta, variant=variant)[key].v, f[key], R.K["ln_fwd"])


@pytest.mark.parametrize("variant,key", [("mask_ge", "dz"), ("no_xhat_term", "dz"), ("slab15", "slab")])
def test_seeded_layernorm_backward_errors_are_rejected(variant, key):
    y, dout, gamma, beta = _ln_case()
    f = R.ln_fwd(y, gamma, beta)
    args = (dout, y, f["mean"].v.float(), f["rstd"].v.float(), gamma, 1.0)
    b = R.ln_bwd(*args)
    assert not R.rejects(key, R.ln_bwd(*args, dt=F32)[key].v, b[key], R.K["ln_bwd"])
    assert R.rejects(key, R.ln_bwd(*args, variant=variant)[key].v, b[key], R.K["ln_bwd"])


@pytest.mark.parametrize("variant,key,p", [("no_scale", "probs", 0.0), ("no_scale", "obar", 0.0), ("drop_before", "obar", 0.3),
                                           ("drop_before", "attn_w", 0.3), ("av_swap", "av_w", 0.3)])
def test_seeded_trimodal_attention_errors_are_rejected(variant, key, p):
    B = 5
    qkv, _ = R.tri_inputs(B, "normal", False)
    keep, av = R.tri_keep(B, p, R.TRI_SEED, R.TRI_OFFSET) if p > 0 else (None, None)
    f = R.tri_attn(qkv, keep, p, av)
    assert not R.rejects(key, R.tri_attn(qkv, keep, p, av, F32)[key].v, f[key], R.K["tri_fwd"])
    assert R.rejects(key, R.tri_attn(qkv, keep, p, av, variant=variant)[key].v, f[key], R.K["tri_fwd"])


@pytest.mark.parametrize("variant", ["softmax_dims", "gate_swap"])
def test_seeded_cross_modal_attention_errors_are_rejected(variant):
    a = R.cross_inputs(5, "normal", False)
    f = R.cross_modal_attn(*a[:6])
    for key in ("out_a", "out_v"):
        assert not R.rejects(key, R.cross_modal_attn(*a[:6], dt=F32)[key].v, f[key], R.K["cross_fwd"])
        assert R.rejects(key, R.cross_modal_attn(*a[:6], variant=variant)[key].v, f[key], R.K["cross_fwd"])


def test_seeded_lstm_cell_without_tanh_c_is_rejected():
    gates, _ = R.lstm_inputs(37, 3, 2, "normal_x3", False)
    ref = R.lstm_cell_t1(gates, 3, 2)
    assert not R.rejects("h", R.lstm_cell_t1(gates, 3, 2, F32).v, ref, R.K["lstm"])
    assert R.rejects("h", R.lstm_cell_t1(gates, 3, 2, variant="no_tanh_c").v, ref, R.K["lstm"])


def test_exact_zeros_must_be_matched_exactly():
    """a value of scale 0 (a masked dz, the forget block) admits no error at all, however large K is."""
    gates, dout = R.lstm_inputs(3, 3, 1, "normal_x3", False)
    ref = R.lstm_cell_t1_bwd(gates, dout, 3, 1)
    got = ref.v.clone()
    assert not R.rejects("dgates", got, ref, 8.0)
    got.view(3, 4, 3)[1, 1, 2] = 1e-30
    assert R.rejects("dgates", got, ref, 1e30)


# =========================================================================== tie to the oracle, and to autograd
def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("M,N", [(17, 256), (33, 1020)])
def test_layernorm_agrees_with_the_oracle_and_with_autograd(M, N):
    y, dout, gamma, beta = (t.double() for t in R.ln_inputs(M, N, False))
    f = R.ln_fwd(y, gamma, beta)
    out, mean, rstd = O.k_ln_fwd(y, gamma, beta)
    assert _rel(f["mean"].v, mean) < 1e-13 and _rel(f["rstd"].v, rstd) < 1e-13
    assert float(((f["out"].v - out).abs() - 2.0 ** -8 * f["out"].v.abs()).max()) <= 0          # the oracle's out is bf16-rounded
    for p in (0.0, 0.3):
        ms = O.drop_scale(p) if p > 0 else 1.0
        b = R.ln_bwd(dout, y, mean, rstd, gamma, ms)
        dz, dgam, dbet = O.k_ln_bwd(dout, y, mean, rstd, gamma, p)
        assert float(((b["dz"].v - dz).abs() - 2.0 ** -8 * b["dz"].v.abs()).max()) <= 0
        assert _rel(b["dgamma"].v, dgam.double()) < 1e-6 and _rel(b["dbeta"].v, dbet.double()) < 1e-6       # the oracle returns float32
    # autograd of the forward restatement: dz without a mask, dgamma, dbeta; the slab sums to them
    leaves = [t.clone().requires_grad_(True) for t in (y, gamma, beta)]
    (R.ln_fwd(*leaves)["out"].v * dout).sum().backward()
    b = R.ln_bwd(dout, y, f["mean"].v, f["rstd"].v, gamma, 0.0)
    assert _rel(b["dz"].v, leaves[0].grad) < 1e-11 and _rel(b["dgamma"].v, leaves[1].grad) < 1e-12 and _rel(b["dbeta"].v, leaves[2].grad) < 1e-12
    assert b["slab"].v.shape == ((M + 15) // 16, 2, N)
    assert _rel(b["slab"].v[:, 0].sum(0), b["dgamma"].v) < 1e-12 and _rel(b["slab"].v[:, 1].sum(0), b["dbeta"].v) < 1e-12
    assert _rel(b["slab"].v[1, 1], dout[16:32].sum(0)) < 1e-12
    ref = torch.nn.functional.layer_norm(y, (N,), gamma, beta, 1e-5)
    assert _rel(f["out"].v, ref) < 1e-12


@pytest.mark.parametrize("p", [0.0, 0.3])
def test_trimodal_attention_agrees_with_the_oracle_and_with_autograd(p):
    B = 5
    qkv, dobar = (t.double() for t in R.tri_inputs(B, "normal", True))
    keep, av = R.tri_keep(B, p, 1234, 5) if p > 0 else (None, None)
    f = R.tri_attn(qkv, keep, p, av)
    # the oracle's operation contains the in_proj: with three permutation matrices as the weight, q | k | v are the columns of xtok
    g = torch.Generator().manual_seed(3)
    perm = [torch.randperm(512, generator=g) for _ in range(3)]
    w_in = torch.zeros(1536, 512, dtype=F64)
    for i in range(3):
        w_in[512 * i + torch.arange(512), perm[i]] = 1.0
    xtok = qkv[:, :512].reshape(B, 2, 512)
    mine_qkv = torch.cat([xtok[..., perm[i]] for i in range(3)], -1).reshape(2 * B, 1536)
    f = R.tri_attn(mine_qkv, keep, p, av)
    prob, obar = O.k_tri_fwd(xtok, w_in, torch.zeros(1536, dtype=F64), mask=keep, p=p)
    assert _rel(f["probs"].v, prob) < 1e-13
    assert float(((f["obar"].v - obar).abs() - 2.0 ** -8 * f["obar"].v.abs()).max()) <= 0
    dq = O.k_tri_bwd(xtok, w_in, torch.zeros(1536, dtype=F64), dobar, prob, mask=keep, p=p).reshape(2 * B, 1536)
    mine = R.tri_attn_bwd(mine_qkv, dobar, prob, keep, p)
    assert float(((mine.v - dq).abs() - 2.0 ** -8 * mine.v.abs()).max()) <= 0
    # autograd of the forward restatement, the keep mask fixed
    x = mine_qkv.clone().requires_grad_(True)
    (R.tri_attn(x, keep, p, av)["obar"].v * dobar).sum().backward()
    assert _rel(mine.v, x.grad) < 1e-12
    # the returned weights: head mean of the dropped probabilities; one key's softmax is 1, so av_w shows only the dropout
    d = f["probs"].v * (1.0 if keep is None else keep.double() * R.drop_threshold(p)[1])
    assert _rel(f["attn_w"].v, d.mean(1)) < 1e-13
    if keep is None:
        assert bool((f["av_w"].v == 1).all())
    else:
        a_rows = torch.from_numpy(R.drop_keep(1, 2 * B, 8, p, 1234, 5)).double()
        assert _rel(f["av_w"].v[:, 0], a_rows[:B].mean(1) * R.drop_threshold(p)[1]) < 1e-13
        assert _rel(f["av_w"].v[:, 1], a_rows[B:].mean(1) * R.drop_threshold(p)[1]) < 1e-13


def test_cross_modal_attention_agrees_with_the_oracle_and_with_autograd():
    B = 5
    g = torch.Generator().manual_seed(5)
    audio, video, text = (torch.randn(B, 256, generator=g, dtype=F64) for _ in range(3))
    P = {}
    for n in ("query_proj", "key_proj", "value_proj"):
        P[n + ".weight"], P[n + ".bias"] = torch.randn(256, 256, generator=g, dtype=F64) / 16, torch.randn(256, generator=g, dtype=F64) / 4
    P["uncertainty_gate.0.weight"], P["uncertainty_gate.0.bias"] = torch.randn(64, 768, generator=g, dtype=F64) / 28, torch.zeros(64, dtype=F64)
    P["uncertainty_gate.2.weight"], P["uncertainty_gate.2.bias"] = torch.randn(2, 64, generator=g, dtype=F64), torch.zeros(2, dtype=F64)
    lin = lambda x, n: x @ P[n + ".weight"].t() + P[n + ".bias"]
    gl = torch.relu(torch.cat([audio, video, text], 1) @ P["uncertainty_gate.0.weight"].t()) @ P["uncertainty_gate.2.weight"].t()
    args = [lin(text, "query_proj"), lin(audio, "key_proj"), lin(audio, "value_proj"), lin(video, "key_proj"), lin(video, "value_proj"), gl]
    oa, ov = O.cross_modal_attention(P, audio, video, text)
    f = R.cross_modal_attn(*args)
    assert _rel(f["out_a"].v, oa) < 1e-13 and _rel(f["out_v"].v, ov) < 1e-13
    g_a, g_v = torch.randn(B, 32, generator=g, dtype=F64), torch.randn(B, 32, generator=g, dtype=F64)
    leaves = [t.clone().requires_grad_(True) for t in args]
    ff = R.cross_modal_attn(*leaves)
    ((ff["out_a"].v * g_a).sum() + (ff["out_v"].v * g_v).sum()).backward()
    b = R.cross_modal_attn_bwd(*args, g_a, g_v)
    for k, t in zip(("dq", "dka", "dva", "dkv", "dvv", "dgl"), leaves):
        assert _rel(b[k].v, t.grad) < 1e-12, k


def test_lstm_cell_agrees_with_the_oracle_and_with_autograd():
    B, H = 7, 3
    g = torch.Generator().manual_seed(6)
    x = torch.randn(B, 5, generator=g, dtype=F64)
    P = {}
    for sfx in ("", "_reverse"):
        P["weight_ih_l0" + sfx] = torch.randn(4 * H, 5, generator=g, dtype=F64)
        P["bias_ih_l0" + sfx], P["bias_hh_l0" + sfx] = torch.randn(4 * H, generator=g, dtype=F64), torch.randn(4 * H, generator=g, dtype=F64)
    gates = torch.cat([x @ P["weight_ih_l0" + s].t() + P["bias_ih_l0" + s] + P["bias_hh_l0" + s] for s in ("", "_reverse")], -1)
    assert _rel(R.lstm_cell_t1(gates, H, 2).v, O.lstm_t1_bidir(x, P, "", layers=1, hidden=H)) < 1e-13
    dout = torch.randn(B, 2 * H, generator=g, dtype=F64)
    leaf = gates.clone().requires_grad_(True)
    (R.lstm_cell_t1(leaf, H, 2).v * dout).sum().backward()
    b = R.lstm_cell_t1_bwd(gates, dout, H, 2)
    assert _rel(b.v, leaf.grad) < 1e-12
    assert bool((b.v.view(B, 2, 4, H)[:, :, 1] == 0).all()) and bool((b.s.view(B, 2, 4, H)[:, :, 1] == 0).all())


# =========================================================================== convert
def test_convert_is_round_to_nearest_even():
    bits = np.concatenate([R.convert_values(), np.random.default_rng(1).integers(0, 2 ** 32, 100000, dtype=np.uint64).astype(np.uint32)])
    x = torch.from_numpy(bits.view(np.int32).copy()).view(torch.float32)
    want = x.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    got = R.convert(bits)
    nan = np.isnan(x.numpy())
    assert (got[~nan] == want[~nan]).all()
    assert ((got[nan] & 0x7F80) == 0x7F80).all() and ((got[nan] & 0x007F) != 0).all()            # a NaN stays a NaN
    named = dict(zip(R.convert_values().tolist(), R.convert(R.convert_values()).tolist()))
    assert named[0x3F808000] == 0x3F80 and named[0x3F818000] == 0x3F82 and named[0x3F808001] == 0x3F81     # ties to even, just above a tie
    assert named[0x7F7FFFFF] == 0x7F80 and named[0x7F7F7FFF] == 0x7F7F and named[0x80000000] == 0x8000     # rounds to inf; stays finite; -0
    assert named[0x00008000] == 0x0000 and named[0x00018000] == 0x0002 and named[0x00000001] == 0x0000     # bf16 denormals: ties to even


# =========================================================================== the dropout draw
def test_threshold_edges():
    assert R.drop_threshold(0.0) == (0xFFFFFFFF, 1.0)                                           # saturated: 2^32 does not fit
    assert R.drop_threshold(1.0) == (0, 0.0) and R.drop_threshold(1.5) == (0, 0.0)
    p = float(np.float32(0.3))                                                                  # 0.3 as a C float: 0.300000011920929
    t, s = R.drop_threshold(0.3)
    assert t == int((1.0 - p) * 2 ** 32) == 3006477056 and t != int(0.7 * 2 ** 32)
    assert s == float(np.float32(1.0 / (1.0 - p))) == O.drop_scale(0.3)
    assert R.drop_threshold(2.0 ** -33)[0] == 0xFFFFFFFF and R.drop_threshold(2.0 ** -31)[0] == 0xFFFFFFFE
    for site in (1, 5, 9):
        assert R.drop_keep(site, 300, 32, 0.0, 1234, 5).all()                                   # p = 0 keeps everything
        assert not R.drop_keep(site, 300, 32, 1.0, 1234, 5).any()                               # p >= 1 keeps nothing
        assert not R.drop_keep(site, 300, 32, 1.25, 1234, 5).any()
    # mix32 is the lowbias32 finaliser: a bijection with mix32(0) = 0; the key takes both halves of seed and offset
    assert int(R.mix32(0)) == 0 and len(set(R.mix32(np.arange(100000)).tolist())) == 100000
    assert len({R.drop_key(s, sd, of) for s in (1, 2) for sd in (0, 1, 2 ** 32) for of in (0, 1, 2 ** 32)}) == 18
    # the row offset of a mask is the row index itself
    assert (R.drop_rand(3, 10, 4, 7, 9)[4:] == R.drop_rand(3, 6, 4, 7, 9, row0=4)).all()


DROP_BASES = [(1 + (3 * i + j) % 9, p, sd, of) for i, p in enumerate((0.1, 0.3, 0.5, 0.9))
              for j, (sd, of) in enumerate(((1234, 5), (0, 0), (2 ** 40 + 7, 2 ** 33 + 1)))]
DROP_Z = {}


def _z(count, n, q):
    return (np.asarray(count, dtype=np.float64) - n * q) / math.sqrt(n * q * (1 - q))


@pytest.mark.parametrize("site,p,seed,offset", DROP_BASES)
def test_dropout_draw_statistics(site, p, seed, offset):
    """z-scores against the binomial with q = thresh / 2^32 on a 4096 x 512 mask: |z| < 6 for the keep rate (total, every column, every
    row) and for the joint keep with the horizontal and vertical neighbour, the next offset, another site, seed + 2^32, offset + 2^32
    (q^2: independence)."""
    rows, cols = 4096, 512
    thresh = R.drop_threshold(p)[0]
    q = thresh / 2.0 ** 32
    k = R.drop_rand(site, rows, cols, seed, offset) < np.uint64(thresh)
    z = {"total": _z(k.sum(), rows * cols, q), "column": _z(k.sum(0), rows, q), "row": _z(k.sum(1), cols, q),
         "horizontal": _z((k[:, 1:] & k[:, :-1]).sum(), rows * (cols - 1), q * q),
         "vertical": _z((k[1:] & k[:-1]).sum(), (rows - 1) * cols, q * q)}
    others = {"offset+1": (site, seed, offset + 1), "other site": (site % 9 + 1, seed, offset),
              "seed+2^32": (site, seed + 2 ** 32, offset), "offset+2^32": (site, seed, offset + 2 ** 32)}
    for name, (s2, sd2, of2) in others.items():
        k2 = R.drop_rand(s2, rows, cols, sd2, of2) < np.uint64(thresh)
        z[name] = _z((k & k2).sum(), rows * cols, q * q)
    for name, v in z.items():
        w = float(np.abs(v).max())
        DROP_Z[name] = max(DROP_Z.get(name, 0.0), w)
        assert w < 6.0, (name, w)
    print("\n   worst |z| so far: " + "  ".join(f"{n} {v:.2f}" for n, v in DROP_Z.items()))
