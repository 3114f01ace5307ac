"""Stack B's training step with dropout live (the configuration ``bench.py --workload stackb_train`` runs) against float64.

A. fp32, the whole step: ``train_step_fused`` (and, at B = 33, the autograd route) at a fixed dropout step against the oracle's
   training-mode forward + autograd in float64 ON THE SAME MASKS -- the masks are drawn on the CPU by tests/stackb_ref.py from the
   uint32 restatement of the counter hash at the sites ``stackb_layers.py`` states, never by the library (one guard test ties the two
   draws together per site).  tests/test_cpu_stackb_ref.py shows that a wrong site number, a lost ``>> 5``, the estimator at the
   config's p or a head's ``dcol`` off by one head moves the reference by >= 40 x these bounds, which are the suite's own for fp32
   against float64 on this model (test_gpu_stackb.py): loss rel 3e-4, outputs rtol 3e-4 / atol 3e-5, gradients rtol 3e-3 /
   atol 3e-3 max|ref|.
   Where the step decided a ReLU the other way than the float64 input's sign -- allowed only within 1e-5 of the layer's largest input,
   asserted -- the reference takes the step's side at exactly those units (stackb_ref.py, "ReLU decisions": at B = 515 one unit of
   3.7 M, input +4.5e-6, moves one row of trimodal_fusion.4.weight by 1.16 x the bound; forcing that unit in the float64 reference on
   the CPU reproduces the 1.16 to four digits).
   MEASURED on the MI355X, as fractions of the bounds: loss <= 4e-3 (1.1e-6 relative), outputs <= 0.10 (mu at B = 515; 0.06 at 33),
   gradients <= 1.6e-3 at every B (1.4e-3 at B = 515 with the one disputed unit taken from the step; 1.16 without).

B, C. bf16, ONE fused step, every launch on its own stored inputs ("teacher forcing", as tests/test_gpu_bf16_layers.py does for
   Stack C): every tensor of the forward tape, every matrix of the opt-in backward tape (``model.keep_backward_tape``), every
   parameter gradient.  The rule, from test_gpu_bf16_layers.py (``ordered``, ``FLIP_FRAC``):

    * bf16 tensor: finite; every element within ONE bf16 ulp of the float64 restatement rounded to bf16 -- differences below
      1e-5 max|ref| are not counted in ulps (an fp32 sum's absolute error against an element that cancelled) but are that small by
      definition, so no element goes unchecked; at most max(2, FLIP_FRAC n) of the n elements differ at all (the floor of two: at
      B = 2 a tensor has 512 elements and ONE legitimate flip is 2e-3);
    * fp32 tensor (LayerNorm statistics, weights / uncertainties of the attention mix, fused32, evidence, planes, every parameter
      gradient against the float64 product dy^T x / the column sums of dy of its STORED operands): within 1e-5 of its largest
      element; the 128 -> 4 evidence layers 2e-6.

   Under the chain plan three kinds of matrix stay in LDS and reach no tape: LayerNorm(y) before a residual block's bypass is added,
   the gradient a LayerNorm backward reads, and dz W before the bypass gradient is added.  A restated stand-in would carry the
   reference's own rounding flips into the next comparison (a flip in a LayerNorm backward's input moves the gamma gradient by
   4e-3 / sqrt(B) of a term), so they are taken from a launch-by-launch twin of the same step, which stores them -- after the twin's
   whole tape, forward and backward, was found bit-equal to the chain step's.  If the chain's LDS copy differed from the twin's
   matrix, the chain's next stored tensor would miss its restatement: the comparison can only fail more, not less.

   MEASURED on the MI355X (the test prints the table per tensor): never more than one ulp; worst flip fraction among tensors of
   >= 4096 elements 2.0e-4 (B = 100), 1.3e-4 (515), 2.4e-4 (1366), against FLIP_FRAC = 1.5e-3; every fp32 tensor within 7.5e-7 of its
   largest element when scaled to the 1e-5 rule (planes 5.8e-7; the evidence layers 1.5e-7 against their 2e-6).  The first run of this test found the attention-mix backward's d_pre at 1.46e-3
   (B = 515) and 1.66e-3 (B = 1366, over the cap): the softmax backward w_k (dw_k - w . dw) lost its relative accuracy in saturated
   rows and the whole 256-wide d_pre row inherited it; the kernel now forms it pairwise (csrc/stackb_train.hip): 1.1e-4 and 5.7e-5.
"""
import copy
import json
import os

import numpy as np
import pytest
import torch

from mmdeer import _lib, stackb, synth
from mmdeer.stackb_layers import ENC, FUS, HID
from oracle import deer_oracle as O

from . import stackb_ref as SR
from .rowkernel_ref import drop_keep
from .test_gpu_bf16_layers import FLIP_FRAC, ordered
from .test_oracle_golden import stackb_oracle_gradients

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
STEP = 5
DIMS = ("valence", "arousal", "dominance")
ENCODERS = ("audio_encoder", "video_encoder", "text_encoder")
ATT, FUSE = "attention_module", "fusion_module"
EST, WN = ATT + ".uncertainty_estimator.estimator", ATT + ".weight_network"


def _model(compute, **cfg):
    with open(os.path.join(GOLDEN, "stackb_state_dict_names.json")) as fh:
        shapes = json.load(fh)
    m = stackb.CompleteDEERModel(stackb.ModelConfig(**cfg), compute_dtype=compute)
    P = {k: torch.from_numpy(v) for k, v in synth.module_fill("stackb2", shapes).items()}
    m.load_state_dict(P)
    return m.to("cuda:0").train(), P


def _batch(B):
    b = synth.make_batch(B, seed=40 + B)
    return b, [torch.from_numpy(b[k]).cuda() for k in ("audio", "video", "text")], torch.from_numpy(b["targets"]).cuda()


def test_cpu_draw_is_the_library_draw_at_every_site():
    """Guard: the reference's masks are drawn on the CPU; per site, that draw is mmdeer_dropout_mask's."""
    m, _ = _model("fp32")
    lib, B = _lib.load(), 33
    for s in SR.sites(m):
        rows, cols = s.rows * B, (s.dcol + s.N - 1 >> s.shift) + 1
        got = torch.empty(rows, cols, dtype=torch.uint8, device="cuda:0")
        _lib.check(lib.mmdeer_dropout_mask(s.site, rows, cols, s.p, int(m.config.dropout_seed), STEP, got.data_ptr(), _lib.current_stream()))
        torch.cuda.synchronize()
        want = drop_keep(s.site, rows, cols, s.p, int(m.config.dropout_seed), STEP)
        assert np.array_equal(got.cpu().numpy().astype(bool), want), s.name


# =============================================================================================== A. fp32, the whole step
_REF = {}


def _reference(B, dropout, T=None):
    """The float64 step on the CPU-drawn masks: computed once per (B, config), shared, never changed.  With a step's tape T: where the
    step decided a ReLU the other way than the reference's sign -- which it may only within stackb_ref.RELU_BAND of zero -- the
    reference with THOSE units decided as the step did (a second evaluation, not kept), and the lines that say so."""
    key = (B, dropout)
    if key not in _REF:
        m, P = _model("fp32", dropout=dropout)
        b, _, _ = _batch(B)
        ss = SR.sites(m)
        full = SR.draw(ss, B, int(m.config.dropout_seed), STEP)
        masks, p = SR.oracle_masks(ss, full, B)
        assert ("est" in masks) and (len(masks) == 21 if dropout > 0 else len(masks) == 1)
        seen = {}
        ref = stackb_oracle_gradients(O, P, b, dict(masks, relu_seen=seen), p, dtype=torch.float64, outputs=True)
        _REF[key] = (ref, seen, full, masks, p, P, b)
    ref, seen, full, masks, p, P, b = _REF[key]
    if T is None:
        return ref, []
    decide, rows = SR.disputed_relus(seen, SR.tape_relu_decisions(T, full, B))
    if decide:
        ref = stackb_oracle_gradients(O, P, b, dict(masks, relu=decide), p, dtype=torch.float64, outputs=True)
    return ref, rows


def _check_step(tag, loss, outs, grads, ref):
    """loss (float), outs {mu, nu, alpha, beta (B, 3), attention_weights, modality_uncertainties (B, 3)}, grads {name: tensor | None}."""
    (rl, rg, ro), notes = ref
    rows = [f"\n{tag}: loss {loss:.7f} (float64 {float(rl):.7f}, rel {abs(loss - float(rl)) / abs(float(rl)):.1e})"] + notes
    want = {k: torch.stack([ro[f"{d}_{k}"] for d in DIMS], 1) for k in ("mu", "nu", "alpha", "beta")}
    want.update(attention_weights=ro["attention_weights"], modality_uncertainties=ro["modality_uncertainties"])
    fails = []
    if not abs(loss - float(rl)) <= 3e-4 * abs(float(rl)):
        fails.append("loss")
    for k, w in want.items():
        g = outs[k].detach().double().cpu()
        assert g.shape == w.shape, k
        r = float(((g - w).abs() / (3e-4 * w.abs() + 3e-5)).max())
        rows.append(f"  {k:24s} worst distance / bound {r:.2e}")
        if not r <= 1.0:
            fails.append(k)
    worst, seen = ("", 0.0), 0
    for n, w in rg.items():
        g = grads[n]
        if w is None:                                      # the calibration layer: off the path
            assert g is None or float(g.abs().max()) == 0.0, n
            continue
        g = g.detach().double().cpu()
        if float(w.abs().max()) == 0.0:                    # one key per query: the query / key projections, exact zeros
            assert ".query_proj." in n or ".key_proj." in n, n
            assert float(g.abs().max()) == 0.0, n
            continue
        r = float(((g - w).abs() / (3e-3 * w.abs() + 3e-3 * w.abs().max())).max())
        worst = max(worst, (n, r), key=lambda t: t[1])
        seen += 1
        if not r <= 1.0:
            fails.append(n)
    rows.append(f"  {seen} gradients, worst distance / bound {worst[1]:.2e} ({worst[0]})")
    print("\n".join(rows))
    assert seen == 104 and not fails, fails


def _fused(m, xs, y):
    m._train_step = STEP
    ld = m.train_step_fused(*xs, y)
    torch.cuda.synchronize()
    T = ld["_keep"][0]
    pl = ld["_planes"]
    outs = {k: pl[i] for i, k in enumerate(("mu", "nu", "alpha", "beta"))}
    outs.update(attention_weights=T["w4"][:, :3], modality_uncertainties=T["u4"][:, :3])
    return float(ld["total_loss"]), outs, {n: p.grad for n, p in m.named_parameters()}, ld


@pytest.mark.parametrize("B,dropout", [(1, 0.3), (2, 0.3), (33, 0.3), (515, 0.3), (33, 0.0)])
def test_fp32_fused_step_with_dropout_against_float64(B, dropout):
    """B = 1, 2: the (1, 4)-operand and 8-element-minimum branches of the backward; 515: ragged against every tile; dropout = 0.0:
    the estimator's own 0.2 stays live and every other site is open."""
    m, _ = _model("fp32", dropout=dropout)
    _, xs, y = _batch(B)
    loss, outs, grads, ld = _fused(m, xs, y)
    assert not ld["_keep"][0]["chain"]                       # fp32 runs launch by launch
    _check_step(f"A fused fp32 B={B} dropout={dropout}", loss, outs, grads, _reference(B, dropout, ld["_keep"][0]))


def test_fp32_autograd_route_with_dropout_against_float64():
    B = 33
    m, _ = _model("fp32")
    _, xs, y = _batch(B)
    m._train_step = STEP
    out = m(*xs)
    ld = m.compute_loss(out, y)
    ld["total_loss"].backward()
    outs = {k: torch.stack([out[f"{d}_{k}"] for d in DIMS], 1) for k in ("mu", "nu", "alpha", "beta")}
    outs.update(attention_weights=out["attention_weights"], modality_uncertainties=out["modality_uncertainties"])
    _check_step(f"A autograd fp32 B={B}", float(ld["total_loss"]), outs, {n: p.grad for n, p in m.named_parameters()}, _reference(B, 0.3))


# =============================================================================================== the opt-in backward tape
@pytest.mark.parametrize("plan", ["ops", "auto"])
def test_backward_tape_changes_no_bit(plan):
    m1, _ = _model("bf16")
    m1.train_plan = plan
    m2 = copy.deepcopy(m1)
    m2.keep_backward_tape = True
    _, xs, y = _batch(33)
    l1, _, _, d1 = _fused(m1, xs, y)
    l2, _, _, d2 = _fused(m2, xs, y)
    T1, T2 = d1["_keep"][0], d2["_keep"][0]
    assert bool(T1["chain"]) == bool(T2["chain"]) == (plan == "auto")
    assert "bwd" not in T1 and T1["ops"] is None and len(T2["bwd"]) >= 30
    assert (len(T2["ops"]) == 0) == (plan == "auto")
    assert l1 == l2 and np.isfinite(l1)
    assert torch.equal(m1._flat_state["g"], m2._flat_state["g"]) and float(m1._flat_state["g"].abs().max()) > 0


# =============================================================================================== B, C. bf16, launch by launch
class Report:
    def __init__(self):
        self.rows, self.flip, self.err32, self.fails = [], ("", 0.0), ("", 0.0), []

    def bf16(self, name, got, ref):
        """got: the stored tensor; ref: the float64 restatement (rounded here)."""
        ref = O._bf16_round(ref)
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        assert torch.isfinite(got).all(), name
        d = (ordered(got.float()) - ordered(ref.float())).abs()
        n = d.numel()
        count = int((d > 0).sum())
        tiny = (got - ref).abs() <= 1e-5 * float(ref.abs().max())
        worst = int(d[~tiny].max()) if (~tiny).any() else 0
        frac = count / max(n, 1)
        self.rows.append(f"  {name:34s} bf16 {tuple(got.shape)!s:14s} differing {frac:.2e} ({count})   max ulp distance {worst}")
        if n >= 4096:                                        # (the worst FRACTION is reported for tensors the floor of two does not govern)
            self.flip = max(self.flip, (name, frac), key=lambda t: t[1])
        if worst > 1 or count > max(2, FLIP_FRAC * n):
            self.fails.append((name, worst, count, n))

    def f32(self, name, got, ref, tol=1e-5):
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        assert torch.isfinite(got).all(), name
        scale = max(float(ref.abs().max()), 1e-30)
        err = float((got.double() - ref.double()).abs().max()) / scale
        self.rows.append(f"  {name:34s} fp32 {tuple(got.shape)!s:14s} max error / max element {err:.2e}")
        self.err32 = max(self.err32, (name, err / tol * 1e-5), key=lambda t: t[1])
        if not err <= tol:
            self.fails.append((name, err, tol))

    def zero(self, name, got):
        if got.numel() and not bool((got == 0).all()):
            self.fails.append((name, "not exact zeros"))


def c(t):
    return t.detach().double().cpu()


def _tape_tensors(T):
    """Every tensor of a step's tape, forward and backward, by name."""
    out = {k: T[k] for k in ("E", "VV", "S", "X", "H1", "H2", "pre", "AV", "T", "r", "w4", "u4", "R2", "G", "fused", "fused32", "H0", "H3", "ev", "planes")}
    for nm in ("av", "tri"):
        out.update({f"{nm}.{i}": t for i, t in enumerate(T[nm])})
    for m, t in enumerate(T["enc"]):
        out.update({f"enc{m}.y0": t["y0"], f"enc{m}.m0": t["m0"], f"enc{m}.r0": t["r0"]})
        for l, h in enumerate(t["h"]):
            out[f"enc{m}.h{l}"] = h
        for l, (y, st) in enumerate(zip(t["y"], t["st"])):
            out.update({f"enc{m}.y{l}": y, f"enc{m}.mean{l}": st[0], f"enc{m}.rstd{l}": st[1]})
    for k, v in T["bwd"].items():
        if k == "enc":
            for m, t in enumerate(v):
                out[f"bwd.enc{m}.dz0"] = t["dz0"]
                out.update({f"bwd.enc{m}.dz{l}": z for l, z in enumerate(t["dz"])})
        elif v is not None:
            out["bwd." + k] = v
    return out


BF16_CASES = [(2, 0.3, "auto"), (100, 0.0, "auto"), (100, 0.0, "ops"), (515, 0.3, "auto"), (1366, 0.3, "auto")]


@pytest.mark.parametrize("B,dropout,plan", BF16_CASES, ids=lambda v: str(v))
def test_bf16_step_every_launch_on_its_own_inputs(B, dropout, plan):
    """B = 2: the smallest batch of the unc8 path; 100 / dropout 0.0: 300 rows, ragged against 16, the estimator's 0.2 live, under both
    plans; 515: ragged; 1366: 3 B = 4098 rows, the 32-sample chain workgroups of the attention and estimator runs with a last
    workgroup of two rows, beside 16-sample workgroups for the B-row runs."""
    m, _ = _model("bf16", dropout=dropout)
    m.train_plan, m.keep_backward_tape = plan, True
    twin = None
    if plan == "auto":
        twin = copy.deepcopy(m)
        twin.train_plan = "ops"
    _, xs, y = _batch(B)
    loss, _, _, ld = _fused(m, xs, y)
    T, g4 = ld["_keep"][0], ld["_keep"][1]
    assert bool(T["chain"]) == (plan == "auto") and np.isfinite(loss)
    OPS = T["ops"]
    if twin is not None:
        # the launch-by-launch twin of the same step: bit-equal in everything both store, and the source of what only it stores
        loss2, _, _, ld2 = _fused(twin, xs, y)
        T2 = ld2["_keep"][0]
        assert not T2["chain"] and loss2 == loss
        a, b = _tape_tensors(T), _tape_tensors(T2)
        assert sorted(a) == sorted(b)
        for k in a:
            assert torch.equal(a[k], b[k]), (k, int((a[k] != b[k]).sum()))
        assert torch.equal(m._flat_state["g"], twin._flat_state["g"])
        OPS = T2["ops"]
    assert len(OPS) == 9 + 9 + 14                            # LayerNorm rows of 9 blocks, dz W of 9 blocks, the inputs of 14 LayerNorm backwards

    ss = SR.sites(m)
    full = SR.draw(ss, B, int(m.config.dropout_seed), STEP)
    assert sorted(full) == (sorted(s.name for s in ss) if dropout > 0 else ["est"])
    mk = full.get
    pc = float(dropout)
    P = {k: c(v) for k, v in m.state_dict().items()}
    Gd = {n: c(p.grad) for n, p in m.named_parameters()}
    Wb = lambda pre: (P[pre + ".weight"], P[pre + ".bias"])
    R = Report()
    bw = T["bwd"]
    seen = set()

    def dw(pre, dy, x):                                      # a Linear's gradients from its stored operands
        gw, gb = O.k_dw(dy, x)
        R.f32("dW " + pre, Gd[pre + ".weight"], gw.double()); R.f32("db " + pre, Gd[pre + ".bias"], gb.double())
        seen.update((pre + ".weight", pre + ".bias"))

    def ln_bwd(tag, pre_ln, dln, ystored, mean, rstd, p, dz_got):
        ref, dg, db = O.k_ln_bwd(dln, ystored, mean, rstd, P[pre_ln + ".weight"], p=p)
        R.bf16(tag, dz_got, ref)
        R.f32("d gamma " + pre_ln, Gd[pre_ln + ".weight"], dg.double()); R.f32("d beta " + pre_ln, Gd[pre_ln + ".bias"], db.double())
        seen.update((pre_ln + ".weight", pre_ln + ".bias"))

    # ------------------------------------------------------------------------------------------------ B. forward
    E = c(T["E"])
    for mi, (t, e) in enumerate(zip(T["enc"], ENCODERS)):
        x, hs, nres = c(t["xin"]), [c(h) for h in t["h"]], len(t["y"])
        assert x.shape == (B, m.config.audio_dim if mi == 0 else (m.config.video_dim, m.config.text_dim)[mi - 1]) and nres == 3
        y0 = c(t["y0"])
        R.bf16(f"enc{mi} stem Linear", y0, O.k_linear(x, *Wb(e + ".input_projection.0"), relu=True))
        ref, mu, rs = O.k_ln_fwd(y0, *Wb(e + ".input_projection.2"))
        R.bf16(f"enc{mi} stem LayerNorm", hs[0], ref); R.f32(f"enc{mi} stem mean", c(t["m0"]), mu); R.f32(f"enc{mi} stem rstd", c(t["r0"]), rs)
        for l in range(nres):
            q = f"{e}.encoder_layers.{l}.layers"
            yl = c(t["y"][l])
            R.bf16(f"enc{mi} res{l} Linear", yl, O.k_linear(hs[l], *Wb(q + ".0"), relu=True, mask=mk(f"res.{mi}.{l}"), p=pc))
            lnr = c(OPS[f"lnr.enc{mi}.res{l}"])
            ref, ln, mu, rs = SR.residual_ln(hs[l], yl, *Wb(q + ".3"), ln_out=lnr)
            R.bf16(f"enc{mi} res{l} LayerNorm (ops)", lnr, ln)
            R.bf16(f"enc{mi} res{l} h + LayerNorm", hs[l + 1], ref)
            R.f32(f"enc{mi} res{l} mean", c(t["st"][l][0]), mu); R.f32(f"enc{mi} res{l} rstd", c(t["st"][l][1]), rs)
        R.bf16(f"enc{mi} output_projection", E[:, mi * ENC:(mi + 1) * ENC], O.k_linear(hs[-1], *Wb(e + ".output_projection")))
    E3 = E.reshape(3 * B, ENC)
    VV, S, X, H1, H2, pre = (c(T[k]) for k in ("VV", "S", "X", "H1", "H2", "pre"))
    sa, ca = ATT + ".self_attention", ATT + ".cross_attention"
    R.bf16("self value_proj (+ head dropout)", VV[:, :ENC], O.k_linear(E3, *Wb(sa + ".value_proj"), mask=mk("attn_self"), p=pc))
    R.bf16("cross value_proj (+ head dropout)", VV[:, ENC:], O.k_linear(E3, *Wb(ca + ".value_proj"), mask=mk("attn_cross"), p=pc))
    R.bf16("self output_proj", S, O.k_linear(VV[:, :ENC], *Wb(sa + ".output_proj")))
    R.bf16("cross output_proj", X, O.k_linear(VV[:, ENC:], *Wb(ca + ".output_proj")))
    R.bf16("estimator.0", H1, O.k_linear(E3, *Wb(EST + ".0"), relu=True, mask=mk("est"), p=0.2))
    R.bf16("estimator.3", H2, O.k_linear(H1, *Wb(EST + ".3"), relu=True))
    wn0 = P[WN + ".0.weight"]
    R.bf16("weight_network.0 (features)", pre, O.k_linear(S.reshape(B, 3 * ENC), wn0[:, :3 * ENC], P[WN + ".0.bias"]))
    AV, Tt, r_, w4, u4 = (c(T[k]) for k in ("AV", "T", "r", "w4", "u4"))
    w3, w1u, w2 = P[EST + ".5.weight"].reshape(-1), wn0[:, 3 * ENC:], P[WN + ".3.weight"]
    av_r, text_r, r_r, w_r, u_r = SR.attn_mix_fwd(H2, pre, S, X, w3, P[EST + ".5.bias"], w1u, w2, P[WN + ".3.bias"], keep=mk("wn"), p=pc)
    R.bf16("attn mix AV", AV, av_r); R.bf16("attn mix text", Tt[:, FUS:], text_r); R.bf16("attn mix r", r_, r_r)
    R.f32("attn mix weights", w4[:, :3], w_r); R.f32("attn mix uncertainties", u4[:, :3], u_r)
    R.zero("w4[:, 3]", w4[:, 3]); R.zero("u4[:, 3]", u4[:, 3])
    stages = {}
    for nm, inp, out in (("av", AV, Tt[:, :FUS]), ("tri", Tt, c(T["R2"]))):
        q = f"{FUSE}.{nm if nm == 'av' else 'trimodal'}_fusion"
        a1, n1, mean, rstd = (c(t) for t in T[nm])
        R.bf16(f"{nm} stage .0", a1, O.k_linear(inp, *Wb(q + ".0"), relu=True, mask=mk(nm), p=pc))
        ref, mu, rs = O.k_ln_fwd(a1, *Wb(q + ".3"))
        R.bf16(f"{nm} stage LayerNorm", n1, ref); R.f32(f"{nm} stage mean", mean, mu); R.f32(f"{nm} stage rstd", rstd, rs)
        R.bf16(f"{nm} stage .4", out, O.k_linear(n1, *Wb(q + ".4"), relu=True))
        stages[nm] = (q, a1, n1, mean, rstd, inp)
    R2, Gt, fused, fused32 = (c(T[k]) for k in ("R2", "G", "fused", "fused32"))
    R.bf16("fusion_gate.0", Gt, O.k_linear(Tt, *Wb(FUSE + ".fusion_gate.0")))
    ref = SR.gate_mix(Gt, R2, Tt[:, :FUS])
    R.bf16("gate mix", fused, ref); R.f32("gate mix fused32", fused32, ref)
    H0, H3, ev, planes = (c(T[k]) for k in ("H0", "H3", "ev", "planes"))
    hq = lambda d, l: f"prediction_heads.{DIMS[d]}.evidence_network.{l}"
    for d in range(3):
        R.bf16(f"head {d} .0", H0[:, d * HID:(d + 1) * HID], O.k_linear(fused, *Wb(hq(d, 0)), relu=True, mask=mk(f"h0.{d}"), p=pc))
        R.bf16(f"head {d} .3", H3[:, d * 128:(d + 1) * 128], O.k_linear(H0[:, d * HID:(d + 1) * HID], *Wb(hq(d, 3)), relu=True, mask=mk(f"h3.{d}"), p=pc))
        R.f32(f"head {d} .6 (evidence)", ev[:, 4 * d:4 * d + 4], H3[:, d * 128:(d + 1) * 128] @ O._bf16_round(P[hq(d, 6) + ".weight"]).t() + P[hq(d, 6) + ".bias"], 2e-6)
    pr = SR.head_planes(ev)
    for i, nm in enumerate(("mu", "nu", "alpha", "beta", "aleatoric", "epistemic", "total")):
        R.f32("planes " + nm, planes[i], pr[i])
    R.f32("planes calibrated", planes[7], SR.head_calibrated(pr[6], [c(t) for t in T["cal_keep"]]))

    # ------------------------------------------------------------------------------------------------ C. backward
    g = {k: (c(v) if torch.is_tensor(v) else v) for k, v in bw.items()}
    R.bf16("head bwd d evidence", g["dev_"], SR.head_bwd(ev, c(g4)))
    for d in range(3):
        h3, h0 = H3[:, d * 128:(d + 1) * 128], H0[:, d * HID:(d + 1) * HID]
        dev_d, dh3, dh0 = g["dev_"][:, 8 * d:8 * d + 4], g["dH3"][:, d * 128:(d + 1) * 128], g["dH0"][:, d * HID:(d + 1) * HID]
        R.zero(f"d evidence head {d} columns 4..7", g["dev_"][:, 8 * d + 4:8 * d + 8])
        R.bf16(f"dX head {d} .6", dh3, O.k_dx(dev_d, P[hq(d, 6) + ".weight"], ymask=h3, p=pc))
        R.bf16(f"dX head {d} .3", dh0, O.k_dx(dh3, P[hq(d, 3) + ".weight"], ymask=h0, p=pc))
        dw(hq(d, 6), dev_d, h3); dw(hq(d, 3), dh3, h0); dw(hq(d, 0), dh0, fused)
    R.bf16("dX heads .0 (stacked)", g["dfused"], O.k_dx(g["dH0"], torch.cat([P[hq(d, 0) + ".weight"] for d in range(3)], 0)))
    for nm, ref in zip(("dG", "dZ4", "dav_a"), SR.gate_mix_bwd(g["dfused"], Gt, R2, Tt[:, :FUS])):
        R.bf16("gate mix bwd " + nm, g[nm], ref)

    def stage_bwd(nm, dz4, dz0, din):
        q, a1, n1, mean, rstd, inp = stages[nm]
        dln = c(OPS[f"dln.{nm}.w0"])
        R.bf16(f"dX {nm} stage .4 (ops)", dln, O.k_dx(dz4, P[q + ".4.weight"]))
        ln_bwd(f"{nm} stage LayerNorm bwd", q + ".3", dln, a1, mean, rstd, pc, dz0)
        R.bf16(f"dX {nm} stage .0", din, O.k_dx(dz0, P[q + ".0.weight"]))
        dw(q + ".4", dz4, n1); dw(q + ".0", dz0, inp)
    stage_bwd("tri", g["dZ4"], g["dz0_tri"], g["dT"])
    R.bf16("dX fusion_gate.0", g["dT2"], O.k_dx(g["dG"], P[FUSE + ".fusion_gate.0.weight"]))
    dw(FUSE + ".fusion_gate.0", g["dG"], Tt)
    R.bf16("d text (add)", g["dtext"], SR.add_masked(g["dT"][:, FUS:], g["dT2"][:, FUS:]))
    R.bf16("d av partial (add)", g["tmp"], SR.add_masked(g["dT"][:, :FUS], g["dT2"][:, :FUS]))
    R.bf16("d av (masked add)", g["dz4_av"], SR.add_masked(g["tmp"], g["dav_a"], mask=Tt[:, :FUS]))
    stage_bwd("av", g["dz4_av"], g["dz0_av"], g["dAV"])
    ms = O.drop_scale(pc) if pc > 0 else 1.0
    refs = SR.attn_mix_bwd(H2, S, X, r_, w4[:, :3], u4[:, :3], g["dAV"], g["dtext"], w3, w1u, w2, ms)
    for nm, got, ref in zip(("d self", "d cross", "d pre", "d logits", "d z", "d h2"),
                            (g["dS_a"], g["dX"], g["dpre"], g["dlog8"][:, :3], g["dz8e"][:, 0].reshape(B, 3), g["dh2"]), refs):
        R.bf16("attn mix bwd " + nm, got, ref)
    R.zero("dlog8[:, 3:]", g["dlog8"][:, 3:]); R.zero("dz8e[:, 1:]", g["dz8e"][:, 1:])
    assert (g["unc8"] is not None) == (B >= 2)
    unc = u4[:, :3]
    if g["unc8"] is not None:
        assert torch.equal(g["unc8"][:, :3], O._bf16_round(u4[:, :3])) and float(g["unc8"][:, 3:].abs().max()) == 0.0
        unc = g["unc8"][:, :3]
    dw(WN + ".3", g["dlog8"][:, :3], r_)
    gw, gb = O.k_dw(g["dpre"], S.reshape(B, 3 * ENC))
    R.f32("dW weight_network.0 (features)", Gd[WN + ".0.weight"][:, :3 * ENC], gw.double()); R.f32("db weight_network.0", Gd[WN + ".0.bias"], gb.double())
    R.f32("dW weight_network.0 (uncertainties)", Gd[WN + ".0.weight"][:, 3 * ENC:], O.k_dw(g["dpre"], unc)[0].double())
    seen.update((WN + ".0.weight", WN + ".0.bias"))
    R.bf16("dX weight_network.0 (features)", g["dS_b"], O.k_dx(g["dpre"], wn0[:, :3 * ENC]))
    R.bf16("d self (add)", g["dS"], SR.add_masked(g["dS_a"], g["dS_b"].reshape(3 * B, ENC)))
    dw(EST + ".5", g["dz8e"][:, :1], H2)
    R.bf16("dX estimator.3", g["dH1"], O.k_dx(g["dh2"], P[EST + ".3.weight"], ymask=H1, p=0.2))
    R.bf16("dX estimator.0", g["dE_est"], O.k_dx(g["dH1"], P[EST + ".0.weight"]))
    dw(EST + ".3", g["dh2"], H1); dw(EST + ".0", g["dH1"], E3)
    R.bf16("dX self output_proj (regenerated)", g["dVV"][:, :ENC], O.k_dx(g["dS"], P[sa + ".output_proj.weight"], p=pc, keep=mk("attn_self")))
    R.bf16("dX cross output_proj (regenerated)", g["dVV"][:, ENC:], O.k_dx(g["dX"], P[ca + ".output_proj.weight"], p=pc, keep=mk("attn_cross")))
    R.bf16("dX value_proj (stacked)", g["dE_v"], O.k_dx(g["dVV"], torch.cat([P[sa + ".value_proj.weight"], P[ca + ".value_proj.weight"]], 0)))
    dw(sa + ".output_proj", g["dS"], VV[:, :ENC]); dw(ca + ".output_proj", g["dX"], VV[:, ENC:])
    dw(sa + ".value_proj", g["dVV"][:, :ENC], E3); dw(ca + ".value_proj", g["dVV"][:, ENC:], E3)
    R.bf16("d E (add)", g["dE"], SR.add_masked(g["dE_v"], g["dE_est"]).reshape(B, 3 * ENC))
    for mi, (t, e) in enumerate(zip(T["enc"], ENCODERS)):
        dEm, hs, tb = g["dE"][:, mi * ENC:(mi + 1) * ENC], [c(h) for h in t["h"]], bw["enc"][mi]
        dw(e + ".output_projection", dEm, hs[-1])
        want = O.k_dx(dEm, P[e + ".output_projection.weight"])
        for l in reversed(range(3)):
            q = f"{e}.encoder_layers.{l}.layers"
            dln, dz = c(OPS[f"dln.enc{mi}.res{l}"]), c(tb["dz"][l])
            R.bf16(f"enc{mi} d h{l + 1} (ops)", dln, want)
            ln_bwd(f"enc{mi} res{l} LayerNorm bwd", q + ".3", dln, c(t["y"][l]), c(t["st"][l][0]), c(t["st"][l][1]), pc, dz)
            dw(q + ".0", dz, hs[l])
            dxr = c(OPS[f"dxr.enc{mi}.res{l}"])
            R.bf16(f"enc{mi} dX res{l} (ops)", dxr, O.k_dx(dz, P[q + ".0.weight"]))
            want = SR.add_masked(dln, dxr)
        dln, dz0 = c(OPS[f"dln.enc{mi}.w0"]), c(tb["dz0"])
        R.bf16(f"enc{mi} d h0 (ops)", dln, want)
        ln_bwd(f"enc{mi} stem LayerNorm bwd", e + ".input_projection.2", dln, c(t["y0"]), c(t["m0"]), c(t["r0"]), 0.0, dz0)
        dw(e + ".input_projection.0", dz0, c(t["xin"]))
    # every parameter was met; the query / key projections, the calibration layer and the alignment gaps hold exact zeros
    st = m._flat_state
    for n, p in m.named_parameters():
        if n not in seen:
            assert ".query_proj." in n or ".key_proj." in n or n.startswith("calibration_layer."), n
            R.zero("gradient of " + n, Gd[n])
        off = st["offs"][n]
        R.zero("alignment gap behind " + n, st["g"][off + p.numel():off + (p.numel() + 63) // 64 * 64])
    assert len(seen) == 104, len(seen)
    print(f"\nteacher-forced launch checks, Stack B, B = {B}, dropout {dropout}, plan {plan} (loss {loss:.6f}):")
    print("\n".join(R.rows))
    print(f"worst: flip fraction {R.flip[1]:.2e} ({R.flip[0]}); fp32 error (scaled to the 1e-5 rule) {R.err32[1]:.2e} ({R.err32[0]})")
    assert not R.fails, R.fails
