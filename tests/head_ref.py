"""Float64 restatement of the evidential head as modules of its own (deer.DEERLayer, deer.MultiDimensionalDEER) and of the
evidence tail operator (mmdeer_evidence_tail_fwd / _bwd), written from their semantics: Linear-ReLU layers, the last Linear
read as (output, 4) evidence, mu = e0, nu = softplus(e1) + 1e-6, alpha = softplus(e2) + 1, beta = softplus(e3) + 1e-6
(softplus with torch's threshold 20), aleatoric = beta / (alpha - 1), epistemic = beta / (nu (alpha - 1)), their sum.  alpha is
rounded to fp32 before alpha - 1 is formed, as every fp32 implementation does: below an evidence of about -17 the difference
is exactly 0 and the uncertainties are inf.  Runs on whatever device its tensors are on.  A helper module, not a test module;
it also holds the case tables of tests/golden/deer_head.npz and the gradient checker of its tests.

``rnd``: optional rounding (e.g. ``bf16``) applied where the HIP path stores bf16: the input, the weights and each hidden layer
going forward; coming back the gradient at each hidden layer, its masked form and dX.

``masks``: the dropout decisions of a training forward, float64 keep * scale per site (``sites_layer`` / ``sites_multi`` list
them, temporal_ref.draw draws them); None is evaluation mode."""
from __future__ import annotations

import numpy as np
import torch

NIG_KEYS = ("mu", "nu", "alpha", "beta", "aleatoric_uncertainty", "epistemic_uncertainty", "uncertainty")
DIM_NAMES = ("valence", "arousal", "dominance")

# tag -> (input_dim, emotion_dims, hidden_dim, B) / (input_dim, output_dim, hidden_dim, B)
MD_CASES = {"md192x3x128": (192, 3, 128, 9), "md320x2x64": (320, 2, 64, 9), "md768x3x512": (768, 3, 512, 5)}
DL_CASES = {"dl96x3x64": (96, 3, 64, 5), "dl256x1x128": (256, 1, 128, 7), "dl40x8x16": (40, 8, 16, 3)}
DLX_CASE = (8, 4, 16, 4)
EXTREME_E = (-104.0, -25.0, -3.0, 25.0)


def extreme_state(sd: dict) -> dict:
    """The extreme case's parameters from its closed-form fill: last weight 0, every mu bias 0.3, the (nu^, alpha^, beta^) biases
    of output o = EXTREME_E[o] -- the evidence then does not depend on the input."""
    sd = {k: np.array(v, copy=True) for k, v in sd.items()}
    sd["evidence_net.6.weight"][...] = 0.0
    b = sd["evidence_net.6.bias"].reshape(-1, 4)
    b[:, 0] = 0.3
    for o, e in enumerate(EXTREME_E):
        b[o, 1:] = e
    return sd


def bf16(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.bfloat16).to(x.dtype)


class _Round(torch.autograd.Function):
    """a rounding of a stored value; the gradient passes unchanged"""

    @staticmethod
    def forward(ctx, x, fn):
        return fn(x)

    @staticmethod
    def backward(ctx, g):
        return g, None


class _RoundGrad(torch.autograd.Function):
    """identity; the gradient passing through is rounded (a gradient the HIP path stores in bf16)"""

    @staticmethod
    def forward(ctx, x, fn):
        ctx.fn = fn
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return ctx.fn(g), None


def _g(x, rnd):
    return x if rnd is None else _RoundGrad.apply(x, rnd)


def _f32(x: torch.Tensor) -> torch.Tensor:
    return x.float().to(x.dtype)


def _r(x, rnd):
    return x if rnd is None else _Round.apply(x, rnd)


def softplus(x: torch.Tensor) -> torch.Tensor:
    return torch.where(x > 20, x, torch.log1p(torch.exp(torch.clamp(x, max=20.0))))


def softplus_grad(x: torch.Tensor) -> torch.Tensor:
    return torch.where(x > 20, torch.ones_like(x), torch.sigmoid(x))


def nig(evid: torch.Tensor):
    """evid (..., 4) -> the seven outputs in NIG_KEYS order (autograd-differentiable)."""
    mu = evid[..., 0]
    nu = softplus(evid[..., 1]) + 1e-6
    alpha = _Round.apply(softplus(evid[..., 2]) + 1.0, _f32)
    beta = softplus(evid[..., 3]) + 1e-6
    am1 = alpha - 1.0
    alea = beta / am1
    epi = beta / (nu * am1)
    return mu, nu, alpha, beta, alea, epi, alea + epi


def tail_evidence(x, w, b):
    """x (B, G K), w (G, 4 O, K), b (G, 4 O) -> evidence (B, G O, 4)."""
    G, R, K = w.shape
    B = x.shape[0]
    e = torch.einsum("bgk,grk->bgr", x.reshape(B, G, K), w) + b
    return e.reshape(B, G * (R // 4), 4)


def tail_bwd(x, w, evid, gouts, mask_scale=0.0, devid=None):
    """The tail's backward by its formulas: gouts = the seven upstream gradients (B, G O) or None.  A None plane drops its terms.
    -> devid (B, G O, 4), dx (B, G K), dw (G, 4 O, K), db (G, 4 O).  With ``devid`` given, dx / dw / db are formed from it
    (teacher forcing) and evid / gouts are not used."""
    G, R, K = w.shape
    B = x.shape[0]
    if devid is not None:
        return (devid,) + _tail_products(x, w, devid, mask_scale)
    mu, nu, alpha, beta, *_ = nig(evid)
    am1 = alpha - 1.0
    z = torch.zeros_like(mu)
    g = gouts
    dnu = g[1] if g[1] is not None else z
    dal = g[2] if g[2] is not None else z
    dbe = g[3] if g[3] is not None else z
    if g[4] is not None or g[6] is not None:
        gA = (g[4] if g[4] is not None else z) + (g[6] if g[6] is not None else z)
        dal = dal - gA * beta / (am1 * am1)
        dbe = dbe + gA / am1
    if g[5] is not None or g[6] is not None:
        gE = (g[5] if g[5] is not None else z) + (g[6] if g[6] is not None else z)
        dnu = dnu - gE * beta / (nu * nu * am1)
        dal = dal - gE * beta / (nu * (am1 * am1))
        dbe = dbe + gE / (nu * am1)
    devid = torch.stack([g[0] if g[0] is not None else z, softplus_grad(evid[..., 1]) * dnu, softplus_grad(evid[..., 2]) * dal,
                         softplus_grad(evid[..., 3]) * dbe], dim=-1)
    return (devid,) + _tail_products(x, w, devid, mask_scale)


def _tail_products(x, w, devid, mask_scale):
    G, R, K = w.shape
    B = x.shape[0]
    d = devid.reshape(B, G, R)
    dx = torch.einsum("bgr,grk->bgk", d, w).reshape(B, G * K)
    if mask_scale > 0:
        dx = dx * (x > 0) * mask_scale
    dw = torch.einsum("bgr,bgk->grk", d, x.reshape(B, G, K))
    return dx, dw, d.sum(0)


def _lin(x, P, name, rnd, relu=True, keep=None):
    y = _g(x, rnd) @ _r(P[name + ".weight"], rnd).t() + P[name + ".bias"]
    if not relu:
        return y                    # the tail operator: its evidence gradient stays fp32 (csrc/nig_tail.hip), only dx is stored
    y = torch.relu(_g(y, rnd))
    if keep is not None:
        y = y * keep.to(y.device)
    return _g(_r(y, rnd), rnd)


def sites_layer(B: int, hidden_dim: int, p: float) -> list:
    """DEERLayer's two sites, (name, site, rows, cols, p): behind evidence_net.0 and evidence_net.3."""
    from mmdeer import head
    return [("ev0", head._SITE_EV0, B, hidden_dim, p), ("ev1", head._SITE_EV1, B, hidden_dim // 2, p)]


def sites_multi(B: int, hidden_dim: int, emotion_dims: int, p: float) -> list:
    """MultiDimensionalDEER's sites: the two shared layers, layer 0 of all heads as ONE (B, D hidden / 2) draw at _SITE_H0 (head d
    in columns [d hidden / 2, (d + 1) hidden / 2)), layer 1 of head d its own (B, hidden / 4) draw at _SITE_H1 + d."""
    from mmdeer import head
    return ([("fp0", head._SITE_FP0, B, hidden_dim, p), ("fp1", head._SITE_FP1, B, hidden_dim, p),
             ("h0", head._SITE_H0, B, emotion_dims * (hidden_dim // 2), p)] +
            [(f"h1.{d}", head._SITE_H1 + d, B, hidden_dim // 4, p) for d in range(emotion_dims)])


def deer_layer(P: dict, x: torch.Tensor, prefix: str = "", rnd=None, masks=None) -> dict:
    """DEERLayer; parameters under their state_dict names (+ prefix); ``masks`` None or {"ev0", "ev1"}.
    -> NIG_KEYS -> (B, output_dim)."""
    p = prefix + "evidence_net."
    m = masks or {}
    h = _lin(_r(x, rnd), P, p + "0", rnd, keep=m.get("ev0"))
    h = _lin(h, P, p + "3", rnd, keep=m.get("ev1"))
    e = _lin(h, P, p + "6", rnd, relu=False)
    return dict(zip(NIG_KEYS, nig(e.reshape(x.shape[0], -1, 4))))


def multi_dim(P: dict, x: torch.Tensor, emotion_dims: int = 3, rnd=None, masks=None) -> dict:
    """MultiDimensionalDEER -> the reference's output dictionary; ``masks`` None or {"fp0", "fp1", "h0", "h1.<d>"}."""
    m = masks or {}
    f = _lin(_r(x, rnd), P, "feature_processor.0", rnd, keep=m.get("fp0"))
    f = _lin(f, P, "feature_processor.3", rnd, keep=m.get("fp1"))
    out = {}
    for d, n in enumerate(DIM_NAMES[:emotion_dims]):
        hm = None
        if masks is not None:
            w = m["h0"].shape[1] // emotion_dims
            hm = {"ev0": m["h0"][:, d * w:(d + 1) * w], "ev1": m[f"h1.{d}"]}
        for k, v in deer_layer(P, f, f"deer_heads.{d}.", rnd, hm).items():
            out[f"{n}_{k}"] = v
    out["mu_all"] = torch.cat([out[f"{n}_mu"] for n in DIM_NAMES[:emotion_dims]], dim=1)
    out["uncertainty_all"] = torch.cat([out[f"{n}_uncertainty"] for n in DIM_NAMES[:emotion_dims]], dim=1)
    return out


def check_grads(g, tag, grads, dx, rtol, atol_frac):
    """Gradients of case `tag` against the fixture (make_golden.store_grads' format): whole tensors, or l2 norm + 1024 samples.
    The absolute term is atol_frac of each tensor's scale (max |ref|; for sampled tensors also norm / sqrt(numel))."""
    seen = 0
    for k in g.files:
        if not k.startswith(tag + "."):
            continue
        kind, _, name = k[len(tag) + 1:].partition(".")
        if kind == "grad":
            ref = g[k]
            np.testing.assert_allclose(grads[name].detach().cpu().numpy(), ref, rtol=rtol, atol=atol_frac * float(np.abs(ref).max()), err_msg=k)
        elif kind == "gradnorm":
            v = grads[name].detach().double().cpu().reshape(-1)
            assert abs(float(v.norm()) - float(g[k])) <= rtol * float(g[k]), k
            ref = g[f"{tag}.gradsample.{name}"]
            idx = torch.linspace(0, v.numel() - 1, 1024).round().long()
            scale = max(float(np.abs(ref).max()), float(g[k]) / v.numel() ** 0.5)
            np.testing.assert_allclose(v[idx].numpy(), ref, rtol=rtol, atol=atol_frac * scale, err_msg=k)
        elif kind == "dx":
            np.testing.assert_allclose(dx.detach().cpu().numpy(), g[k], rtol=rtol, atol=atol_frac * float(np.abs(g[k]).max()), err_msg=k)
        else:
            continue
        seen += 1
    assert seen >= 7, (tag, seen)
