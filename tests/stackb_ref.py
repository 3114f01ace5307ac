"""References for Stack B's training step (tests/test_cpu_stackb_ref.py, tests/test_gpu_stackb_step.py).  TEST INFRASTRUCTURE.

Two things, both on the CPU in plain torch / numpy:

 * the dropout masks of a step, drawn with ``rowkernel_ref.drop_keep`` (the uint32 restatement of the library's counter hash, tied bit
   for bit to ``mmdeer_dropout_mask`` by tests/test_gpu_rowkernels.py) at the sites ``stackb_layers.py`` states -- one ``Site`` per
   ``nn.Dropout`` of the path, its number, shift, column offset, rows per sample and p read from the ``Lin`` records and ``SITE_WN``
   -- in the two forms the references take them: per column of the launch that applies them (``draw``), and as the oracle's
   ``stackb_forward(masks=..., p=...)`` names them (``oracle_masks`` / ``keep_masks``);
 * float64 restatements of the row operators between the GEMM launches, each from the tensors that launch reads (the Linear, dX, dW and
   LayerNorm launches are the oracle's generic ``k_linear`` / ``k_dx`` / ``k_dw`` / ``k_ln_fwd`` / ``k_ln_bwd``).  The attention-mix
   forward and the gate mix are the float64 references of tests/test_gpu_row_ops.py, imported; the rest (head, masked add) are the
   formulas that file's tests state inline."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Tuple

import numpy as np
import torch

from mmdeer.stackb_layers import FUS, HID, SITE_WN, Layers
from oracle import deer_oracle as O

from .rowkernel_ref import drop_keep

F64 = torch.float64


# ------------------------------------------------------------------------------------------------------------- dropout sites
@dataclass
class Site:
    name: str          # the oracle's name of the site
    site: int          # the number the library hashes
    rows: int          # mask rows per sample (3: the (sample, modality) rows of the shared-weight attention layers)
    N: int             # columns of the launch that applies it
    shift: int         # one decision per 2^shift columns
    dcol: int          # mask column of the launch's column 0
    p: float


def sites(model) -> List[Site]:
    """The dropout sites of the path, in path order."""
    L = Layers(model)
    pc = float(model.config.dropout)
    users: Dict[int, int] = {}
    for r in L.all:
        if r.site >= 0:
            users[r.site] = users.get(r.site, 0) + 1

    def of(name, r, rows=1):
        # records that share a site are the members of one stacked layer: each at its column of the stacked operand
        return Site(name, r.site, rows, r.N, r.shift, r.area[1] if users[r.site] > 1 else 0, pc if r.p is None else float(r.p))
    out = [of(f"res.{m}.{l}", r) for m, e in enumerate(L.enc) for l, r in enumerate(e.res)]
    out += [of("attn_self", L.vs, 3), of("attn_cross", L.vc, 3), of("est", L.e1, 3)]
    out.append(Site("wn", SITE_WN, 1, L.wn0.N, 0, 0, pc))               # inside the attention row kernel
    out += [of("av", L.av[0]), of("tri", L.tri[0])]
    out += [of(f"h0.{d}", r) for d, r in enumerate(L.h0)] + [of(f"h3.{d}", r) for d, r in enumerate(L.h3)]
    return out


def draw(ss: List[Site], B: int, seed: int, step: int) -> Dict[str, torch.Tensor]:
    """{site name: keep (rows * B, N) bool}, per column of the launch; a site whose p is 0 is open and absent."""
    full = {}
    for s in ss:
        if s.p <= 0:
            continue
        idx = (s.dcol + np.arange(s.N)) >> s.shift
        full[s.name] = torch.from_numpy(np.ascontiguousarray(drop_keep(s.site, s.rows * B, int(idx.max()) + 1, s.p, seed, step)[:, idx]))
    return full


def oracle_masks(ss: List[Site], full: Dict[str, torch.Tensor], B: int) -> Tuple[Dict[str, torch.Tensor], Dict[str, float]]:
    """(masks, p) as ``oracle.stackb_forward`` takes them: float64 0/1, one column per decision, the modality on axis 1."""
    masks, p = {}, {}
    for s in ss:
        if s.name not in full:
            continue
        k = full[s.name].to(F64)[:, ::1 << s.shift]
        masks[s.name] = k.reshape(B, s.rows, -1) if s.rows > 1 else k
        p[s.name] = s.p
    return masks, p


def keep_masks(model, B: int, step: int):
    """The masks and probabilities of the training step ``model`` takes at dropout step ``step`` on a batch of B."""
    ss = sites(model)
    return oracle_masks(ss, draw(ss, B, int(model.config.dropout_seed), step), B)


# ------------------------------------------------------------------------------------------------------------- ReLU decisions
# A gradient is compared across a ReLU only where both sides take the same decision.  Deep in the network an fp32 step carries an error
# of a few 1e-6 of a layer's scale (the oracle's own fp32 evaluation on the CPU does: 1e-6 .. 1e-5 at B = 515), and among the 3.7 M
# ReLU inputs of a B = 515 step a handful lie closer to zero than that.  A unit that the fp32 step switches the other way moves one
# sample's whole contribution into or out of a row of a weight gradient: ~1 / B of it, which at B = 515 is the size of the step test's
# bound (measured: tri stage unit 212 of sample 450, input +4.5e-6 in float64 against a layer maximum of 4.8, moved
# trimodal_fusion.4.weight by 1.16 x its bound, every other row of it by 1e-6 x).  Either side's derivative is a correct answer there.
# So the float64 reference takes, at exactly the units where the step's stored activation and its own sign disagree, the step's side
# -- and every such unit has to lie within RELU_BAND of zero, or the disagreement is an error and the comparison fails.
RELU_BAND = 1e-5       # of the layer's largest input: the suite's fp32 rule (1e-5 of a tensor's largest element)


def tape_relu_decisions(T, full, B):
    """{the oracle's ReLU name: (on, kept)} read from a step's stored activations (on: stored value > 0) and the step's keep masks
    (kept None: no dropout behind this ReLU; a dropped unit stores zero whatever was decided, and its decision reaches no gradient)."""
    c = lambda t: t.detach().float().cpu()
    out = {}
    for m, t in enumerate(T["enc"]):
        out[f"stem.{m}"] = (c(t["y0"]) > 0, None)
        for l, y in enumerate(t["y"]):
            out[f"res.{m}.{l}"] = (c(y) > 0, full.get(f"res.{m}.{l}"))
    H1, H2 = c(T["H1"]).reshape(B, 3, -1), c(T["H2"]).reshape(B, 3, -1)
    est = full.get("est")
    for i in range(3):
        out[f"est.0.{i}"] = (H1[:, i] > 0, None if est is None else est.reshape(B, 3, -1)[:, i])
        out[f"est.3.{i}"] = (H2[:, i] > 0, None)
    out["wn"] = (c(T["r"]) > 0, full.get("wn"))
    out["av.0"], out["av.4"] = (c(T["av"][0]) > 0, full.get("av")), (c(T["T"])[:, :FUS] > 0, None)
    out["tri.0"], out["tri.4"] = (c(T["tri"][0]) > 0, full.get("tri")), (c(T["R2"]) > 0, None)
    H0, H3 = c(T["H0"]), c(T["H3"])
    for d in range(3):
        out[f"h0.{d}"] = (H0[:, d * HID:(d + 1) * HID] > 0, full.get(f"h0.{d}"))
        out[f"h3.{d}"] = (H3[:, d * (HID // 2):(d + 1) * (HID // 2)] > 0, full.get(f"h3.{d}"))
    return out


def disputed_relus(seen, decisions, band=RELU_BAND):
    """({name: int8 tensor for ``masks["relu"]``}, report lines): the units whose decision in ``decisions`` differs from the sign of the
    reference's input ``seen[name]`` (dropped units aside).  Raises if one of them lies further from zero than band * max|input|."""
    assert sorted(seen) == sorted(decisions), (sorted(seen), sorted(decisions))
    decide, rows = {}, []
    for name, (on, kept) in decisions.items():
        z = seen[name]
        diff = (z > 0) != on
        if kept is not None:
            diff &= kept
        if diff.any():
            lim = band * float(z.abs().max())
            assert float(z[diff].abs().max()) <= lim, (name, diff.nonzero().tolist()[:4], z[diff].tolist()[:4], lim)
            d = torch.full(z.shape, -1, dtype=torch.int8)
            d[diff] = on[diff].to(torch.int8)
            decide[name] = d
            rows.append(f"  ReLU {name}: {int(diff.sum())} unit(s) decided the other way, inputs {[f'{v:.1e}' for v in z[diff].tolist()]} (band {lim:.1e})")
    return decide, rows


# ------------------------------------------------------------------------------------------------------------- row operators
def residual_ln(h, y, gamma, beta, ln_out=None):
    """h + LayerNorm(y) as the bf16 step stores it: the LayerNorm rounded to bf16, then the sum.  ``ln_out``: the stored LayerNorm
    rows to add instead of the restated ones.  Returns (sum, LayerNorm rows, mean, rstd)."""
    ln, mean, rstd = O.k_ln_fwd(y, gamma, beta)
    return O._bf16_round(h + (ln if ln_out is None else ln_out)), ln, mean, rstd


def attn_mix_fwd(H2, pre, S, X, w3, b3, w1u, w2, b2, keep=None, p=0.0):
    """mmdeer_stackb_attn_mix_train_fwd: (AV (B, 512), text (B, 256), r (B, 256), weights (B, 3), uncertainties (B, 3)), float64,
    unrounded.  H2 (3B, 64), S / X (3B, 256): rows (sample, modality)."""
    from .test_gpu_row_ops import _attn_forward64
    B = pre.shape[0]
    fac = torch.ones(B, 256, dtype=F64) if keep is None else keep.to(F64) * O.drop_scale(p)
    R = _attn_forward64(dict(h2=H2.reshape(B, 3, 64), pre=pre, s=S.reshape(B, 3, 256), c=X.reshape(B, 3, 256)),
                        dict(w3=w3, b3=b3, w1u=w1u, w2=w2, b2=b2), B, fac, False)
    return R["out"][:, :2].reshape(B, 512), R["out"][:, 2], R["h"], R["w"], R["u"]


def attn_mix_bwd(H2, S, X, r, w, u, dAV, dtext, w3, w1u, w2, mask_scale):
    """mmdeer_stackb_attn_mix_bwd from the forward's stored r, weights and uncertainties: float64, unrounded
    (d self (3B, 256), d cross (3B, 256), d pre (B, 256), d logits (B, 3), d z (B, 3), d h2 (3B, 64)).
    out_m = w_m S_m + (1 - u_m) X_m; w = softmax(r W2^T + b2); r = (pre + u W1u^T) * (r > 0) * mask_scale; u = sigmoid(h2 . w3 + b3);
    the estimator's last ReLU: d h2 only where h2 > 0."""
    B = r.shape[0]
    s, c = S.reshape(B, 3, 256), X.reshape(B, 3, 256)
    G = torch.cat([dAV.reshape(B, 2, 256), dtext.reshape(B, 1, 256)], 1)
    d_self = G * w[:, :, None]
    d_cross = G * (1.0 - u)[:, :, None]
    dw = (G * s).sum(-1)
    # softmax backward in its pairwise form, w_k sum_j w_j (dw_k - dw_j): the same quantity as w_k (dw_k - w . dw) for weights that sum
    # to one, but evaluated on the STORED fp32 weights it does not depend on how the largest of them was rounded (a saturated row)
    dl = w * (w[:, None, :] * (dw[:, :, None] - dw[:, None, :])).sum(-1)
    dpre = (dl @ w2) * ((r > 0).to(F64) * mask_scale)
    du = dpre @ w1u - (G * c).sum(-1)
    dz = du * u * (1.0 - u)
    dh2 = dz[:, :, None] * w3 * (H2.reshape(B, 3, 64) > 0)
    return d_self.reshape(3 * B, 256), d_cross.reshape(3 * B, 256), dpre, dl, dz, dh2.reshape(3 * B, 64)


def gate_mix(G, R2, av):
    from .test_gpu_row_ops import _gate_ref
    return _gate_ref(G, R2, av)[0]


def gate_mix_bwd(dout, G, R2, av):
    """(d gate logits, d tri -- zero where the stored tri <= 0, its ReLU --, d av)."""
    s = torch.sigmoid(G)
    return dout * (R2 - av) * s * (1.0 - s), dout * s * (R2 > 0), dout * (1.0 - s)


def _softplus(x):
    from .test_gpu_row_ops import _softplus64
    return _softplus64(x)


def head_planes(ev):
    """mmdeer_stackb_head, planes 0..6 (mu, nu, alpha, beta, aleatoric, epistemic, total) from the evidence (B, 12): nu, alpha, beta
    rounded to fp32 before the uncertainties are formed, as the kernel and torch do."""
    from .test_gpu_row_ops import EPS32
    r = ev.reshape(-1, 3, 4)
    nu = (_softplus(r[..., 1]) + EPS32).float().double()
    alpha = (_softplus(r[..., 2]) + 1.0).float().double()
    beta = (_softplus(r[..., 3]) + EPS32).float().double()
    am1 = alpha - 1.0
    alea, epi = beta / am1, beta / (nu * am1)
    return torch.stack([r[..., 0], nu, alpha, beta, alea, epi, alea + epi])


def head_calibrated(total, cps):
    """plane 7: sigmoid(MLP(total / temperature[d])); cps as the kernel takes them (temperature, w1, b1, w2 (16 x 32), b2, w3, b3)."""
    T, w1, b1, w2, b2, w3, b3 = (t.double() for t in cps)
    sc = total / T[None, :]
    h1 = torch.relu(sc[..., None] * w1 + b1)
    h2 = torch.relu(h1 @ w2.reshape(16, 32).t() + b2)
    return torch.sigmoid(h2 @ w3 + b3)


def head_bwd(ev, g4):
    """mmdeer_stackb_head_bwd: d evidence (B, 24), head d in columns 8 d .. 8 d + 3, zeros behind; g4 (4, B, 3)."""
    from .test_gpu_row_ops import EPS32
    B = ev.shape[0]
    r = ev.reshape(B, 3, 4).clone().requires_grad_(True)
    planes = torch.stack([r[..., 0], _softplus(r[..., 1]) + EPS32, _softplus(r[..., 2]) + 1.0, _softplus(r[..., 3]) + EPS32])
    (planes * g4).sum().backward()
    out = torch.zeros(B, 3, 8, dtype=F64)
    out[..., :4] = r.grad
    return out.reshape(B, 24)


def add_masked(x, y=None, mask=None, scale=1.0):
    s = x if y is None else x + y
    return s if mask is None else torch.where(mask > 0, s * scale, torch.zeros_like(s))
