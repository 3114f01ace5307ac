"""TEST INFRASTRUCTURE, CPU only: the three stand-alone loss kernels of csrc/nig.hip (deer_v1_kernel + deer_v1_final_kernel,
unc_reg_kernel, calibration_kernel) and the two streaming-metric kernels of csrc/evalstats.hip (eval_accumulate_kernel,
eval_ece_bins_kernel) restated in float64, with a SCALE for every value, in the manner of tests/nig_ref.py (whose comparison rule
``worst_ratio`` / ``assert_close`` is used unchanged).

 * ``deer_v1_reference`` / ``unc_reg_reference`` / ``calibration_reference``: float32 inputs, float64 values and gradients.  The scale
   of a value is the float64 sum of the ABSOLUTE values of the pieces that are added to form it; a function of a sum (the logarithm of
   the mean variance) carries that sum's scale times the function's derivative.  Gradients are autograd over the float64 expression
   with every mask (KL clamp, error clamp, bin membership) a constant.
 * ``float32_eval_v1`` / ``float32_eval_unc_reg`` / ``float32_eval_calibration``: the same formulas in float32 on the CPU in the
   kernels' structure, each with ONE optional seeded fault.  The constants K of tests/test_gpu_loss_kernels.py are set from them and
   tests/test_cpu_loss_ref.py proves that the comparison rejects every fault.
 * ``accumulate_reference`` / ``sample_means_reference`` / ``ece_bins_reference``: the streaming-metric kernels in numpy.
 * the case builders, each with the conditions the comparisons rest on asserted (conditions of the REFERENCE, not measurements).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from .nig_ref import EPS, ULP, _next, assert_close, conf32, regular_case, worst_ratio  # noqa: F401  (re-exported to the tests)

TINY = 2.0 ** -126        # float32 holds nothing between 0 and 2^-149: every gradient scale carries this floor
MIN_GAP = 1e-3            # smallest |mean conf - mean acc| of a populated bin: its float32 sign is then the float64 one
MIN_KL = 1e-4             # smallest |kl| of a sample: the float32 clamp then gates as the float64 one does


def _f32(*ts):
    for t in ts:
        assert t.dtype == torch.float32, "float32 inputs"
    return [t.reshape(-1) for t in ts]


def _grads_of(pieces, leaves):
    """pieces: scalars (already weighted).  Returns (sum of their gradients, sum of the absolute values) per leaf."""
    g = [torch.zeros_like(t) for t in leaves]
    s = [torch.zeros_like(t) for t in leaves]
    for p in pieces:
        if not torch.is_tensor(p) or not p.requires_grad:
            continue
        for j, t in enumerate(torch.autograd.grad(p, leaves, retain_graph=True, allow_unused=True)):
            if t is not None:
                g[j] += t
                s[j] += t.abs()
    return torch.stack(g), torch.stack(s)


# =========================================================================== deer.DEERLoss, variant 1 (mmdeer_deer_loss_v1)
@dataclass
class V1Ref:
    out: torch.Tensor            # [5] float64: total, nll, evidence_reg, kl_reg, mse
    out_scale: torch.Tensor
    grads: torch.Tensor          # [4, n] float64 at (mu, nu, alpha, beta)
    grad_scale: torch.Tensor
    min_abs_kl: float            # smallest |kl| before the clamp
    min_kl_margin: float         # smallest |kl| / (2^-24 * scale of kl): how many float32 roundings the sign is away from flipping
    neg_frac: float              # share of samples with kl < 0


def deer_v1_reference(mu, nu, alpha, beta, y, ew: float = 1.0, kw: float = 1.0) -> V1Ref:
    """deer.py:125-195 on flattened float32 tensors.  The clamp mask is the float64 sign of kl (kl >= 0 passes, as torch.clamp's
    backward does).  log(pi / nu), log(2 beta) and log(2 pi beta) count as the sums of logarithms they are."""
    mu, nu, alpha, beta, y = _f32(mu, nu, alpha, beta, y)
    n = mu.numel()
    m, nv, a, b = (t.double().requires_grad_(True) for t in (mu, nu, alpha, beta))
    d = y.double() - m
    se = d * d
    ah = a + 0.5
    om = b + nv * se / 2
    const = lambda v: torch.full_like(se.detach(), v)
    lg_a, lg_ah, lb = torch.lgamma(a), torch.lgamma(ah), torch.log(b)
    nll_p = [const(0.5 * math.log(math.pi)), -0.5 * torch.log(nv), -a * math.log(2.0), -a * lb, lg_a, -lg_ah, ah * torch.log(om)]
    reg_p = [se / (2 * (1 + nv)), b / nv]                        # (nu se + 2 beta (1 + nu)) / (2 nu (1 + nu))
    kl_p = [0.5 * nv, const(-0.5), a * lb, -lg_a, lg_ah, const(-0.5 * math.log(2 * math.pi)), -0.5 * lb]
    klr = sum(kl_p).detach()
    klr_s = sum(p.detach().abs() for p in kl_p)
    keep = (klr >= 0).double()
    vals = [sum(nll_p), sum(reg_p), keep * sum(kl_p), se]
    scal = [sum(p.detach().abs() for p in nll_p), sum(p.detach().abs() for p in reg_p), keep * klr_s, se.detach()]
    mean = [v.detach().sum() / n for v in vals]
    mean_s = [s.sum() / n for s in scal]
    out = torch.stack([mean[0] + ew * mean[1] + kw * mean[2], *mean])
    out_s = torch.stack([mean_s[0] + abs(ew) * mean_s[1] + abs(kw) * mean_s[2], *mean_s])
    pieces = [p.sum() / n for p in nll_p] + [ew * p.sum() / n for p in reg_p] + [kw * (keep * p).sum() / n for p in kl_p]
    grads, gscale = _grads_of(pieces, (m, nv, a, b))
    return V1Ref(out=out, out_scale=out_s, grads=grads, grad_scale=gscale + TINY, min_abs_kl=float(klr.abs().min()),
                 min_kl_margin=float((klr.abs() / (ULP * klr_s)).min()), neg_frac=float((klr < 0).double().mean()))


V1_FAULTS = ("kl_grad_ungated", "fold_first_256")


def float32_eval_v1(mu, nu, alpha, beta, y, ew: float = 1.0, kw: float = 1.0, fault: Optional[str] = None):
    """deer_v1_kernel + deer_v1_final_kernel in float32 torch-CPU arithmetic: (out [5], grads [4, n])."""
    assert fault is None or fault in V1_FAULTS
    m, nv, a, b, y = _f32(mu, nu, alpha, beta, y)
    n = m.numel()
    f = torch.float32
    pi = torch.tensor(math.pi, dtype=f)
    d = y - m
    se = d * d
    ah = a + 0.5
    om = b + nv * se / 2.0
    nll = 0.5 * torch.log(pi / nv) - a * torch.log(2.0 * b) + torch.lgamma(a) - torch.lgamma(ah) + ah * torch.log(om)
    reg = (nv * se + 2.0 * b * (1.0 + nv)) / (2.0 * nv * (1.0 + nv))
    klr = 0.5 * (nv - 1.0) + a * torch.log(b) - torch.lgamma(a) + torch.lgamma(ah) - 0.5 * torch.log(2.0 * pi * b)
    per = torch.stack([nll, reg, torch.clamp(klr, min=0.0), se], dim=1)               # [n, 4]
    nblk = (n + 255) // 256
    part = torch.cat([per, torch.zeros(nblk * 256 - n, 4, dtype=f)]).view(nblk, 256, 4).sum(1)    # one partial per block
    if fault == "fold_first_256":
        part = part[:256]
    lanes = torch.zeros(256, 4, dtype=f)                       # lane t of the final kernel: partials t, t + 256, ... in that order
    for j in range(0, part.shape[0], 256):
        chunk = part[j:j + 256]
        lanes[:chunk.shape[0]] += chunk
    v = lanes.sum(0)
    inv = torch.tensor(1.0, dtype=f) / torch.tensor(float(n), dtype=f)
    mean = v * inv
    out = torch.stack([mean[0] + ew * mean[1] + kw * mean[2], mean[0], mean[1], mean[2], mean[3]])
    dpsi = torch.digamma(a) - torch.digamma(ah)
    kg = torch.full_like(a, kw) if fault == "kl_grad_ungated" else torch.where(klr >= 0, torch.full_like(a, kw), torch.zeros_like(a))
    g_mu = -ah * nv * d / om - ew * d / (1.0 + nv)
    g_nu = -0.5 / nv + ah * (se / 2.0) / om + ew * (-se / (2.0 * (1.0 + nv) * (1.0 + nv)) - b / (nv * nv)) + kg * 0.5
    g_al = -torch.log(2.0 * b) + dpsi + torch.log(om) + kg * (torch.log(b) - dpsi)
    g_be = -a / b + ah / om + ew / nv + kg * (a / b - 0.5 / b)
    return out, torch.stack([g_mu, g_nu, g_al, g_be]) * inv


# =========================================================================== UncertaintyRegularizationLoss (mmdeer_uncertainty_reg_loss)
@dataclass
class UncRef:
    out: torch.Tensor            # [3] float64: reg_loss, diversity_loss, sparsity_loss
    out_scale: torch.Tensor
    grads: torch.Tensor          # [2, B, D] at (alpha, beta)
    grad_scale: torch.Tensor


def _den(alpha32: torch.Tensor, a64: torch.Tensor, den64: bool) -> torch.Tensor:
    """alpha - 1 + 1e-8 as the float32 program forms it (conf32's rule), carrying a64's graph; ``den64``: formed in float64, which
    is what a float64 run of the reference program does (tests/test_cpu_loss_ref.py compares with one)."""
    if den64:
        return a64 - 1 + EPS
    return (alpha32 - 1 + EPS).double() + (a64 - a64.detach())


def unc_reg_reference(alpha, beta, dw: float = 0.1, sw: float = 0.01, den64: bool = False) -> UncRef:
    """losses.py:363-416 on float32 [B, D]: u = beta / (alpha - 1 + 1e-8), diversity = -log(mean_d var_B(u) + 1e-8) with the
    unbiased variance, sparsity = mean(u).  B = 1: 0 / 0 in the variance, NaN values and NaN gradients as the reference gives them.
    Scales: a centred square (u - m)^2 = (u - m) u - (u - m) m counts |u - m| (|u| + mean|u|); the logarithm carries its own absolute
    value plus the scale of its argument over the argument."""
    assert alpha.dtype == torch.float32 and beta.dtype == torch.float32 and alpha.dim() == 2 and alpha.shape == beta.shape
    B, D = alpha.shape
    a, b = alpha.double().requires_grad_(True), beta.double().requires_grad_(True)
    den = _den(alpha, a, den64)
    u = b / den
    mean = u.mean(0)
    c = u - mean
    bm1 = torch.tensor(float(B - 1), dtype=torch.float64)
    var = (c * c).sum(0) / bm1
    vm = var.mean()
    div = -torch.log(vm + EPS)
    spars = u.mean()
    total = dw * div + sw * spars
    ud, cd = u.detach(), c.detach()
    mean_s = ud.abs().mean(0)
    vm_s = ((cd.abs() * (ud.abs() + mean_s)).sum(0) / bm1).mean() + EPS
    rel = vm_s / (vm.detach() + EPS)                         # scale of (vm + eps) in units of itself
    div_s = div.detach().abs() + rel
    spars_s = ud.abs().mean()
    out = torch.stack([total.detach(), div.detach(), spars.detach()])
    out_s = torch.stack([abs(dw) * div_s + abs(sw) * spars_s, div_s, spars_s])
    ga, gb = torch.autograd.grad(total, (a, b))
    # d total / d u = cdiv (u - m) + cs with cdiv = -dw / (vm + eps) * 2 / (D (B - 1)), cs = sw / (B D)
    cdiv = (-dw / (vm.detach() + EPS) * 2.0 / (D * bm1)).abs()
    gu_s = cdiv * (ud.abs() + mean_s) + cdiv * cd.abs() * rel + abs(sw) / (B * D)
    dd = den.detach()
    gs = torch.stack([gu_s * (ud / dd).abs(), gu_s / dd.abs()])
    return UncRef(out=out, out_scale=out_s, grads=torch.stack([ga, gb]), grad_scale=gs + TINY)


UNC_FAULTS = ("biased_variance", "diversity_grad_no_1_over_D", "raw_sum_variance")


def _lane_sums(x: torch.Tensor) -> torch.Tensor:
    """Sum over dim 0 as one workgroup of 256 lanes forms it: lane t adds rows t, t + 256, ... in that order, then the lanes fold."""
    n = x.shape[0]
    lanes = torch.zeros(256, *x.shape[1:], dtype=x.dtype)
    for j in range(0, n, 256):
        chunk = x[j:j + 256]
        lanes[:chunk.shape[0]] += chunk
    return lanes.sum(0)


def float32_eval_unc_reg(alpha, beta, dw: float = 0.1, sw: float = 0.01, fault: Optional[str] = None):
    """unc_reg_kernel in float32 torch-CPU arithmetic: (out [3], grads [2, B, D])."""
    assert fault is None or fault in UNC_FAULTS
    f = torch.float32
    B, D = alpha.shape
    Bf, Df = torch.tensor(float(B), dtype=f), torch.tensor(float(D), dtype=f)
    eps = torch.tensor(EPS, dtype=f)
    den = alpha - 1.0 + eps
    u = beta / den
    s1 = _lane_sums(u)
    total = s1.sum()
    mean = s1 / Bf
    c = u - mean
    s2 = _lane_sums(c * c)
    if fault == "raw_sum_variance":
        s2 = _lane_sums(u * u) - s1 * s1 / Bf
    vm = (s2 / (Bf if fault == "biased_variance" else Bf - 1.0)).sum() / Df
    div = -torch.log(vm + eps)
    spars = total / (Bf * Df)
    out = torch.stack([dw * div + sw * spars, div, spars])
    dgrad = 1.0 if fault == "diversity_grad_no_1_over_D" else Df
    cdiv = -dw / (vm + eps) * 2.0 / (dgrad * (Bf - 1.0))
    cs = sw / (Bf * Df)
    gu = cdiv * c + cs
    return out, torch.stack([gu * (-u / den), gu / den])


# =========================================================================== CalibrationLoss (mmdeer_calibration_loss[_bins])
def cal_edges32(n_bins: int) -> torch.Tensor:
    return torch.linspace(0, 1, n_bins + 1, dtype=torch.float32)


def cal_masks(conf: torch.Tensor, edges32: torch.Tensor, fault: Optional[str] = None) -> torch.Tensor:
    """[n_bins, n] boolean: bin k is [edge[k], edge[k + 1]) in float32, the last bin [lo, hi] (losses.py:470-476)."""
    assert conf.dtype == torch.float32 and edges32.dtype == torch.float32 and conf.dim() == 1
    lo, hi = edges32[:-1].view(-1, 1), edges32[1:].view(-1, 1)
    if fault == "bins_lo_open":                               # a seeded error: (lo, hi]
        return (conf > lo) & (conf <= hi)
    m = (conf >= lo) & (conf < hi)
    if fault != "last_bin_open":
        m[-1] |= conf == edges32[-1]
    return m


@dataclass
class CalRef:
    loss: torch.Tensor           # [1] float64
    loss_scale: torch.Tensor
    counts: torch.Tensor         # [n_bins] int64, exact
    grads: torch.Tensor          # [3, n] at (gamma, alpha, beta)
    grad_scale: torch.Tensor
    min_gap: float               # smallest |mean conf - mean acc| over the populated bins
    clamp_same: bool             # the float32 program clamps the same samples as float64 does
    min_clamp_margin: float      # smallest | |y - gamma| / 2 - 1 | over the samples that are not exactly ON the clamp
    documented_nan: torch.Tensor  # [n] bool: u == inf in float32 (see calibration_reference)


def calibration_reference(gamma, alpha, beta, y, edges32, masks: Optional[torch.Tensor] = None, den64: bool = False) -> CalRef:
    """losses.py:431-497 on flattened float32 tensors.  Membership: conf32 against the float32 edges (a constant mask; ``masks``
    overrides it).  Means and the loss in float64; the clamp of |y - gamma| / 2 passes the gradient for 0 <= h <= 1; sign(0) = 0.

    ``documented_nan`` marks the samples whose float32 u = beta / (alpha - 1 + 1e-8) is inf.  Their confidence is 0 (bin 0 under
    [lo, hi)), and the float32 reference program's d/d alpha there is d conf/d u * d u/d alpha = (-0) * (-inf) = NaN, d/d beta
    (-0) * 1e8 = -0: that, not the float64 value (about 1e-31 / n, formed from factors float32 cannot hold), is what a float32
    program gives, and the kernel gives the same."""
    gamma, alpha, beta, y = _f32(gamma, alpha, beta, y)
    n = gamma.numel()
    nb = edges32.numel() - 1
    c32 = conf32(alpha, beta)
    if masks is None:
        masks = cal_masks(c32, edges32)
    m = masks.double()
    g, a, b = (t.double().requires_grad_(True) for t in (gamma, alpha, beta))
    d = y.double() - g
    h = d.abs() / 2.0
    hc = h.clamp(0, 1)
    conf = 1.0 / (1.0 + b / _den(alpha, a, den64))
    counts = masks.sum(1).to(torch.int64)
    loss, loss_s, gaps = torch.zeros((), dtype=torch.float64), torch.zeros((), dtype=torch.float64), []
    for k in range(nb):
        cnt = float(counts[k])
        if cnt > 0:
            cm, am = (m[k] * conf).sum() / cnt, (m[k] * (1.0 - hc)).sum() / cnt
            diff = cm - am
            loss = loss + (cnt / n) * diff.abs()
            loss_s = loss_s + (cnt / n) * ((m[k] * conf.detach().abs()).sum() / cnt + 1.0 + (m[k] * hc.detach()).sum() / cnt)
            gaps.append(abs(float(diff.detach())))
    if loss.requires_grad:
        grads = torch.stack([t if t is not None else torch.zeros(n, dtype=torch.float64)
                             for t in torch.autograd.grad(loss, (g, a, b), allow_unused=True)])
    else:
        grads = torch.zeros(3, n, dtype=torch.float64)
    d32 = (y - gamma).abs() / 2.0
    clamp_same = bool(((d32 <= 1.0) == (h.detach() <= 1.0)).all())
    u32 = beta / (alpha - 1 + EPS)
    off = (h.detach() - 1.0).abs()
    off = off[off > 0]
    return CalRef(loss=loss.detach().reshape(1), loss_scale=loss_s.reshape(1), counts=counts, grads=grads,
                  grad_scale=grads.abs() + TINY, min_gap=min(gaps) if gaps else float("inf"), clamp_same=clamp_same,
                  min_clamp_margin=float(off.min()) if off.numel() else float("inf"), documented_nan=torch.isinf(u32))


CAL_FAULTS = ("bins_lo_open", "last_bin_open", "no_err_clamp", "dgamma_sign")


def float32_eval_calibration(gamma, alpha, beta, y, edges32, fault: Optional[str] = None):
    """calibration_kernel in float32 torch-CPU arithmetic: (loss [1], counts [n_bins] int64, grads [3, n])."""
    assert fault is None or fault in CAL_FAULTS
    gamma, alpha, beta, y = _f32(gamma, alpha, beta, y)
    f = torch.float32
    n = gamma.numel()
    nb = edges32.numel() - 1
    nf = torch.tensor(float(n), dtype=f)
    den = alpha - 1.0 + torch.tensor(EPS, dtype=f)
    u = beta / den
    conf = 1.0 / (1.0 + u)
    masks = cal_masks(conf, edges32, fault)
    d = y - gamma
    h = d.abs() / 2.0
    acc = 1.0 - (h if fault == "no_err_clamp" else h.clamp(0, 1))
    loss = torch.zeros((), dtype=f)
    sgn = torch.zeros(nb, dtype=f)
    counts = torch.zeros(nb, dtype=torch.int64)
    for k in range(nb):
        mk = masks[k].to(f)
        v = _lane_sums(torch.stack([mk, mk * conf, mk * acc], dim=1))
        counts[k] = int(v[0])
        if v[0] > 0:
            diff = v[1] / v[0] - v[2] / v[0]
            loss = loss + (v[0] / nf) * diff.abs()
            sgn[k] = torch.sign(diff)
    inv = 1.0 / nf
    s = (masks.to(f) * sgn.view(-1, 1)).sum(0) * inv                       # 0 outside every bin
    inside = torch.ones_like(h, dtype=torch.bool) if fault == "no_err_clamp" else (h >= 0) & (h <= 1)
    dg = torch.where(inside, -s * 0.5 * torch.sign(d), torch.zeros_like(s))
    if fault == "dgamma_sign":
        dg = -dg
    gu = -s * conf * conf
    return loss.reshape(1), counts, torch.stack([dg, gu * (-u / den), gu / den])


def compare_calibration(got_loss, got_counts, got_grads, ref: CalRef, K: float, log: Optional[list] = None, tag: str = ""):
    """What every test of the calibration loss asserts: exact counts, the loss and 3 x n gradient elements by the scale rule; at a
    documented sample (float32 u == inf) d/d alpha must be NaN and d/d beta zero."""
    assert torch.equal(got_counts.detach().cpu().to(torch.int64).reshape(-1), ref.counts), \
        f"{tag} bin counts {got_counts.reshape(-1).tolist()} != {ref.counts.tolist()}"
    assert_close(f"{tag} loss", got_loss, ref.loss, ref.loss_scale, K, log)
    if got_grads is None:
        return
    got = got_grads.detach().double().cpu().clone()
    doc = ref.documented_nan
    if bool(doc.any()):
        assert bool(torch.isnan(got[1, doc]).all()), f"{tag}: d/d alpha where u == inf is {got[1, doc].tolist()}, the reference program has NaN"
        assert bool((got[2, doc] == 0).all()), f"{tag}: d/d beta where u == inf is {got[2, doc].tolist()}, the reference program has 0"
        got[1:, doc] = ref.grads[1:, doc]
    assert_close(f"{tag} gradients", got, ref.grads, ref.grad_scale, K, log)


# =========================================================================== streaming metrics (csrc/evalstats.hip)
def accumulate_reference(pred: np.ndarray, target: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """acc[d][8] = {n, sum p, sum t, sum p^2, sum t^2, sum p t, sum |p - t|, sum (p - t)^2} in float64 over the rows where neither
    value is NaN, and the sums of the absolute values (the scale)."""
    assert pred.dtype == np.float32 and target.dtype == np.float32 and pred.shape == target.shape and pred.shape[1] == 3
    acc, scale = np.zeros((3, 8)), np.zeros((3, 8))
    for d in range(3):
        p, t = pred[:, d].astype(np.float64), target[:, d].astype(np.float64)
        ok = ~(np.isnan(p) | np.isnan(t))
        p, t = p[ok], t[ok]
        e = p - t
        cols = [np.ones_like(p), p, t, p * p, t * t, p * t, np.abs(e), e * e]
        acc[d] = [math.fsum(c) for c in cols]
        scale[d] = [math.fsum(np.abs(c)) for c in cols]
    return acc, scale


def sample_means_reference(pred: np.ndarray, target: np.ndarray, unc: Optional[np.ndarray]) -> Tuple[np.ndarray, Optional[np.ndarray]]:
    """The per-sample mean |p - t| and mean u as float32 programs: three float32 additions from 0, one division by 3."""
    three = np.float32(3.0)
    with np.errstate(invalid="ignore"):
        e = np.zeros(pred.shape[0], dtype=np.float32)
        for d in range(3):
            e = e + np.abs(pred[:, d] - target[:, d])
        err = e / three
        if unc is None:
            return err, None
        u = np.zeros(pred.shape[0], dtype=np.float32)
        for d in range(3):
            u = u + unc[:, d]
        return err, u / three


def ece_valid(err: np.ndarray, unc: np.ndarray) -> np.ndarray:
    return ~(np.isnan(err) | np.isnan(unc) | np.isinf(unc))


def ece_bins_reference(err: np.ndarray, unc: np.ndarray, edges64: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """bins[i] = {count, sum (1 - u), sum (1 - e)} over the valid samples with edges[i] <= u < edges[i + 1] in float64, and the
    scales {count, sum (1 + |u|), sum (1 + |e|)}."""
    assert err.dtype == np.float32 and unc.dtype == np.float32 and edges64.dtype == np.float64
    ok = ece_valid(err, unc)
    e, u = err[ok].astype(np.float64), unc[ok].astype(np.float64)
    nb = len(edges64) - 1
    bins, scale = np.zeros((nb, 3)), np.zeros((nb, 3))
    for i in range(nb):
        m = (u >= edges64[i]) & (u < edges64[i + 1])
        bins[i] = [float(m.sum()), math.fsum(1.0 - u[m]), math.fsum(1.0 - e[m])]
        scale[i] = [float(m.sum()), math.fsum(1.0 + np.abs(u[m])), math.fsum(1.0 + np.abs(e[m]))]
    return bins, scale


# =========================================================================== inputs of the tests
def flat_case(n: int, seed: int = 1):
    """nig_ref.regular_case flattened: (mu, nu, alpha, beta, y), n float32 elements each."""
    rows = (n + 2) // 3
    return tuple(t.reshape(-1)[:n].contiguous() for t in regular_case(rows, seed=seed))


# ---- deer loss, variant 1.  Sizes in flattened elements: 1; 255, 256, 257 (one block, then two); 65,536 (256 partials: one pass of
# the final fold); 65,537 (257: lane 0 takes two); 3 x 4097.
V1_N = (1, 255, 256, 257, 65536, 65537, 3 * 4097)
V1_WEIGHTS = ((1.0, 1.0), (0.7, 0.3))
V1_EXTRA = (((1.0, 0.0), 257), ((0.0, 1.0), 257), ((1.0, 0.0), 3 * 4097), ((0.0, 1.0), 3 * 4097))
V1_SEED: Dict[int, int] = {65536: 3, 65537: 3}   # generator seeds at which a size meets the conditions (searched on the CPU; default 1)


def v1_cases() -> List[Tuple[str, tuple, float, float]]:
    cases = [(f"v1-n{n}-ew{ew}-kw{kw}", flat_case(n, V1_SEED.get(n, 1)), ew, kw) for n in V1_N for ew, kw in V1_WEIGHTS]
    cases += [(f"v1-n{n}-ew{ew}-kw{kw}", flat_case(n, V1_SEED.get(n, 1)), ew, kw) for (ew, kw), n in V1_EXTRA]
    return cases


def checked_v1_reference(tag, inputs, ew, kw) -> V1Ref:
    ref = deer_v1_reference(*inputs, ew, kw)
    assert ref.min_abs_kl >= MIN_KL, f"{tag}: a sample with |kl| = {ref.min_abs_kl:.3g}: choose another seed"
    assert ref.min_kl_margin >= 64, f"{tag}: a kl only {ref.min_kl_margin:.3g} float32 roundings from 0: choose another seed"
    if inputs[0].numel() >= 255:
        assert 0.0 < ref.neg_frac < 1.0, f"{tag}: one sign of kl only"
    return ref


# ---- uncertainty regulariser
UNC_B = (1, 2, 255, 256, 257, 1000)
UNC_D = (1, 3, 8)
UNC_WEIGHTS = ((0.1, 0.01), (1.0, 0.0))


def unc_case(B: int, D: int, seed: int = 1):
    _, _, alpha, beta, _ = flat_case(B * D, seed)
    return alpha.view(B, D).contiguous(), beta.view(B, D).contiguous()


def near_constant_case(B: int = 1000, D: int = 3):
    """Column 1 holds u = 1e-3 + 1e-6 x (alpha = 2: the denominator is exactly 1): raw power sums would lose the variance."""
    alpha, beta = unc_case(B, D, seed=3)
    x = torch.randn(B, generator=torch.Generator().manual_seed(7))
    alpha[:, 1] = 2.0
    beta[:, 1] = (1e-3 + 1e-6 * x.double()).float()
    assert float(beta[:, 1].min()) > 9e-4
    return alpha, beta


def offset_case(B: int = 1000, D: int = 3):
    """Every column holds u = c_d + 1e-3 x around c = (10, 20, 5): a mean variance of 1e-6, far above the 1e-8 inside the logarithm
    (which hides the variance of the column of near_constant_case), that raw power sums lose altogether."""
    x = torch.randn(B, D, generator=torch.Generator().manual_seed(8)).double()
    beta = (torch.tensor([10.0, 20.0, 5.0, 10.0, 20.0, 5.0, 10.0, 20.0][:D], dtype=torch.float64) + 1e-3 * x).float()
    return torch.full((B, D), 2.0, dtype=torch.float32), beta


def alpha_one_case(B: int = 257, D: int = 3):
    """One row of column 0 has alpha == 1.0f: u = beta / float32(1e-8), about 1e8."""
    alpha, beta = unc_case(B, D, seed=4)
    alpha[100, 0], beta[100, 0] = 1.0, 1.0
    return alpha, beta


def unc_cases() -> List[Tuple[str, tuple, float, float]]:
    cases = [(f"unc-B{B}-D{D}-dw{dw}-sw{sw}", unc_case(B, D), dw, sw) for B in UNC_B for D in UNC_D for dw, sw in UNC_WEIGHTS]
    cases += [(f"unc-near-constant-dw{dw}-sw{sw}", near_constant_case(), dw, sw) for dw, sw in UNC_WEIGHTS]
    cases += [(f"unc-offset-dw{dw}-sw{sw}", offset_case(), dw, sw) for dw, sw in UNC_WEIGHTS]
    cases += [(f"unc-alpha-one-dw{dw}-sw{sw}", alpha_one_case(), dw, sw) for dw, sw in UNC_WEIGHTS]
    return cases


# ---- calibration loss
CAL_BINS = (1, 7, 10, 15, 32)
CAL_N = (1, 255, 256, 257, 1000, 3 * 4097)
CAL_SEED: Dict[Tuple[int, int], int] = {}     # (n_bins, n) -> generator seed at which the case meets the conditions (default 1)
EXACT_EDGES = {7: [1, 2, 4, 5, 6], 10: list(range(1, 10)), 15: [k for k in range(1, 15) if k != 7]}


def _conf_of_beta(beta: float) -> float:
    return float(conf32(torch.tensor([2.0], dtype=torch.float32), torch.tensor([beta], dtype=torch.float32))[0])


def cal_edge_betas(n_bins: int):
    """alpha = 2: the float32 denominator is exactly 1 and conf = 1 / (1 + beta).  For every interior edge k of the float32
    linspace(0, 1, n_bins + 1): (k, beta_on or None, beta_below, beta_above) -- a beta whose confidence IS the edge where one exists
    within 64 ulp of 1 / edge - 1, and the betas of the nearest attainable confidences on both sides."""
    edges = cal_edges32(n_bins)
    res = []
    for k in range(1, n_bins):
        edge = float(edges[k])
        b0 = float(torch.tensor(1.0 / edge - 1.0, dtype=torch.float32))
        cands, lo, hi = [b0], b0, b0
        for _ in range(64):
            lo, hi = _next(lo, False), _next(hi, True)
            cands += [lo, hi]
        on = [b for b in cands if _conf_of_beta(b) == edge]
        b = b0
        while _conf_of_beta(b) >= edge:            # the confidence falls as beta grows
            b = _next(b, True)
        b_below = b
        b = b0
        while _conf_of_beta(b) <= edge:
            b = _next(b, False)
        res.append((k, on[0] if on else None, b_below, b))
    if n_bins in EXACT_EDGES:
        assert [k for k, on, *_ in res if on is not None] == EXACT_EDGES[n_bins], (n_bins, [k for k, on, *_ in res if on is not None])
    return res


def cal_edge_case(n_bins: int, seed: int = 1):
    """The edge samples as flat (gamma, alpha, beta, y) and ``expect`` = [(row, bin or -1)]:
    every interior edge (on it where float32 has such a beta: upper bin; next below: lower bin; next above: upper bin), conf == 1
    (last bin, closed), alpha == 1.0f (u near 1e8: bin 0), alpha < 1 twice (conf > 1, conf < 0: no bin), u == inf (conf == 0: bin
    0), |y - gamma| exactly 2, next above, next below, and y == gamma."""
    rows, expect = [], []

    def put(alpha, beta, bin_):
        expect.append((len(rows), bin_))
        rows.append((alpha, beta))

    for k, b_on, b_below, b_above in cal_edge_betas(n_bins):
        if b_on is not None:
            put(2.0, b_on, k)
        put(2.0, b_below, k - 1)
        put(2.0, b_above, k)
    put(2.0, 1e-9, n_bins - 1)                     # 1 + 1e-9 == 1: conf == 1
    put(1.0, 1.0, 0)                               # alpha == 1.0f
    put(0.5, 0.25, -1)                             # u = -0.5: conf = 2
    put(0.5, 1.0, -1)                              # u = -2: conf = -1
    put(1.0, 1e31, 0)                              # u = inf: conf == 0
    mid = n_bins // 2 if n_bins > 1 else 0         # conf = 0.5: bin floor(n_bins / 2) for every n_bins used (0.5 is an edge only for even n_bins: upper bin)
    first_y = len(rows)
    for _ in range(4):
        put(2.0, 1.0, mid)
    E = len(rows)
    gen = torch.Generator().manual_seed(1000 * seed + n_bins)
    gamma = torch.randn(E, generator=gen)
    y = torch.tanh(torch.randn(E, generator=gen))
    two = 2.0
    gamma[first_y:first_y + 4] = 0.0
    y[first_y:first_y + 4] = torch.tensor([two, _next(two, True), _next(two, False), 0.0])
    alpha = torch.tensor([r[0] for r in rows], dtype=torch.float32)
    beta = torch.tensor([r[1] for r in rows], dtype=torch.float32)
    return gamma, alpha, beta, y, expect


def cal_mixed_edge_case(n_bins: int, seed: int = 1):
    """The edge samples spread through a regular batch of 300."""
    ge, ae, be, ye, expect = cal_edge_case(n_bins, seed)
    g, _, a, b, y = flat_case(300, seed=9)
    E = ge.numel()
    rows = [3 + (i * 296) // E for i in range(E)]
    assert len(set(rows)) == E and rows[-1] < 300
    for dst, src in ((g, ge), (a, ae), (b, be), (y, ye)):
        dst[rows] = src
    return g, a, b, y, [(rows[r], k) for r, k in expect]


def cal_cases() -> List[Tuple[str, tuple, int, bool]]:
    """(tag, (gamma, alpha, beta, y), n_bins, regular)"""
    cases = []
    for nb in CAL_BINS:
        for n in CAL_N:
            mu, _, a, b, y = flat_case(n, CAL_SEED.get((nb, n), 1))
            cases.append((f"cal-nb{nb}-n{n}", (mu, a, b, y), nb, True))
        cases.append((f"cal-nb{nb}-edges-alone", cal_edge_case(nb)[:4], nb, False))
        cases.append((f"cal-nb{nb}-edges-in-300", cal_mixed_edge_case(nb)[:4], nb, False))
    return cases


FULL_N = 3 * 4097          # at this size every bin of every n_bins of CAL_BINS is populated (asserted)


def checked_cal_reference(tag, inputs, n_bins, regular) -> CalRef:
    ref = calibration_reference(*inputs, cal_edges32(n_bins))
    if regular and inputs[0].numel() >= FULL_N:
        assert int(ref.counts.min()) > 0, f"{tag}: an empty bin {ref.counts.tolist()}"
    assert ref.min_gap >= MIN_GAP, f"{tag}: a bin gap of {ref.min_gap:.3g}: choose another seed"
    assert ref.clamp_same, f"{tag}: float32 rounds an |y - gamma| / 2 across the clamp: choose another seed"
    return ref
