"""TEST INFRASTRUCTURE, CPU only: MultiTaskDEERLoss and the NIG head's last-layer backward restated in float64, with a SCALE for
every value, and the comparison rule the GPU tests of csrc/nig_dev.h / nig.hip / the chain prologue use.

 * ``reference``: the 105 sums, the 20 outputs of MMDEER_LOSS_OUT, the 30 bin counts and the gradient at (gamma, nu, alpha, beta) of
   float32 inputs [B, 3].  Bin membership is decided as the reference program decides it -- the confidence in float32, compared
   with float32 ``torch.linspace(0, 1, 11)`` under (lo, hi] (losses.py:215) -- and is a constant mask; everything else is float64,
   the gradient is autograd over the float64 expression.
 * the scale of a value is the float64 sum of the ABSOLUTE values of the pieces that are added to form it (for a gradient element:
   of the contributions of the four log-probability pieces, the regulariser, the two KL pieces, the ECE and the three pairs of
   the cross-dimension term).  ``worst_ratio`` measures |got - ref| in units of 2^-24 * scale, so a term that cancels cannot hide
   an error and a term that is small next to the others still has to be right to float32 rounding of the whole.
 * ``float32_eval``: the same formulas evaluated in float32 on the CPU in the kernels' structure (per-sample terms, 256-sample block
   partials, the fold in two halves, the finals, the closed-form gradient), optionally with ONE seeded error: the constants K of
   the GPU tests are set from it and tests/test_cpu_nig_ref.py proves that the comparison rejects every seeded error.
 * ``head_reference``: d evidence by the softplus chain rule, dz2, dW3, db3 from a loss gradient, each with its scale.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, Optional, Sequence, Tuple

import torch

EPS = 1e-8
ULP = 2.0 ** -24
NSTAT = 35                       # per dimension: logprob, reg, kla, klb, u, 10 x conf, 10 x |err|, 10 x count
EDGES32 = torch.linspace(0, 1, 11, dtype=torch.float32)


@dataclass(frozen=True)
class LossConfig:
    reg_w: float = 0.1
    kl_w: float = 0.01
    ece_w: float = 0.05
    cross_w: float = 0.05
    task_w: Tuple[float, float, float] = (1.0, 1.0, 1.0)


def conf32(alpha: torch.Tensor, beta: torch.Tensor) -> torch.Tensor:
    """The confidence as the float32 program computes it (losses.py:198-199)."""
    assert alpha.dtype == torch.float32 and beta.dtype == torch.float32
    return 1.0 / (1.0 + beta / (alpha - 1 + EPS))


def bin_masks(conf: torch.Tensor, half_open_left: bool = False) -> torch.Tensor:
    """[10, ...] boolean: bin k is (edge[k], edge[k+1]] in float32.  conf == 0 is in no bin."""
    assert conf.dtype == torch.float32
    lo, hi = EDGES32[:-1].view(-1, *[1] * conf.dim()), EDGES32[1:].view(-1, *[1] * conf.dim())
    if half_open_left:            # a seeded error: [lo, hi)
        return (conf >= lo) & (conf < hi)
    return (conf > lo) & (conf <= hi)


@dataclass
class Ref:
    out: torch.Tensor            # [20] float64
    out_scale: torch.Tensor
    sums: torch.Tensor           # [105] float64 (this batch's own)
    sums_scale: torch.Tensor
    counts: torch.Tensor         # [3, 10] int64 (of the statistics the finals were made of)
    grads: torch.Tensor          # [4, B, 3] float64
    grad_scale: torch.Tensor
    bin_population: torch.Tensor  # [3, 10] int64 of this batch
    min_gap: float               # smallest |mean conf - mean acc| over populated bins


def _finals(S, A, N, cfg: LossConfig):
    """The 20 outputs from per-dimension sums S [3, 35]; A: the sums of absolute pieces, for the scales.  Differentiable in S."""
    out, sc = [None] * 20, [None] * 20
    tot, tot_s = 0.0, 0.0
    ubar, ubar_s = [], []
    gaps = []
    for d in range(3):
        nll, nll_s = -S[d, 0] / N, A[d, 0] / N
        reg, reg_s = S[d, 1] / N, A[d, 1] / N
        kl, kl_s = S[d, 2] / N + 0.1 * (S[d, 3] / N), A[d, 2] / N + 0.1 * (A[d, 3] / N)
        ece, ece_s = torch.zeros((), dtype=torch.float64), torch.zeros((), dtype=torch.float64)
        for k in range(10):
            cnt = S[d, 25 + k].detach()
            if cnt > 0:
                cm, am = S[d, 5 + k] / cnt, S[d, 15 + k] / cnt
                diff = cm - (1.0 - am)                                   # losses.py:219-224
                ece = ece + (cnt / N) * diff.abs()
                ece_s = ece_s + (cnt / N) * (cm.abs() + 1.0 + am.abs()).detach()
                gaps.append(abs(float(diff.detach())))
        total = nll + cfg.reg_w * reg + cfg.kl_w * kl + cfg.ece_w * ece   # losses.py:121
        total_s = nll_s + abs(cfg.reg_w) * reg_s + abs(cfg.kl_w) * kl_s + abs(cfg.ece_w) * ece_s
        for j, (v, s) in enumerate(((total, total_s), (nll, nll_s), (reg, reg_s), (kl, kl_s), (ece, ece_s))):
            out[d * 5 + j], sc[d * 5 + j] = v, s
        tot, tot_s = tot + cfg.task_w[d] * total, tot_s + abs(cfg.task_w[d]) * total_s
        ubar.append(S[d, 4] / N)
        ubar_s.append(A[d, 4] / N)
    cross, cross_s = 0.0, 0.0
    for i in range(3):
        for j in range(i + 1, 3):
            cross = cross + (ubar[i] - ubar[j]) ** 2
            cross_s = cross_s + (ubar_s[i] + ubar_s[j]) ** 2
    cross, cross_s = cross / 3.0, cross_s / 3.0                           # losses.py:339-346
    if cfg.cross_w > 0:
        tot, tot_s = tot + cfg.cross_w * cross, tot_s + cfg.cross_w * cross_s
    out[15], sc[15] = cross, cross_s
    out[16], sc[16] = tot / 3.0, tot_s / 3.0                              # losses.py:314
    for j in (1, 2, 3):                                                   # training.py:187-190
        out[16 + j] = (out[j] + out[5 + j] + out[10 + j]) / 3.0
        sc[16 + j] = (sc[j] + sc[5 + j] + sc[10 + j]) / 3.0
    return out, sc, gaps


def reference(gamma, nu, alpha, beta, targets, cfg: LossConfig = LossConfig(), global_stats: Optional[torch.Tensor] = None,
              masks: Optional[torch.Tensor] = None) -> Ref:
    """float32 [B, 3] tensors in, float64 out.  ``global_stats`` (106 values, as mmdeer_loss_stats returns them, summed over the
    ranks): the finals come from them and the gradient is this batch's share of the union's.  ``masks`` [10, B, 3] overrides the
    float32 membership (tests/test_cpu_nig_ref.py, for a confidence next to an edge)."""
    for t in (gamma, nu, alpha, beta, targets):
        assert t.dtype == torch.float32 and t.dim() == 2 and t.shape[1] == 3, "float32 [B, 3] tensors"
    B = gamma.shape[0]
    if masks is None:
        masks = bin_masks(conf32(alpha, beta))
    m = masks.to(torch.float64)
    g, n, a, b = (t.detach().double().requires_grad_(True) for t in (gamma, nu, alpha, beta))
    y = targets.double()
    err = y - g
    e2 = err * err
    A_ = b + 0.5 * n * e2 + EPS
    lb = torch.log(b + EPS)
    lp = (0.5 * torch.log(n / (2 * math.pi + EPS)), a * lb, -torch.lgamma(a + EPS), -(a + 0.5) * torch.log(A_))   # losses.py:144-150
    reg = e2 * (2 * b + n * e2)                                            # losses.py:165-167
    kla = (a - 1) ** 2
    klb = (lb - math.log(1 + EPS)) ** 2
    u = b / (a - 1 + EPS)
    conf = 1.0 / (1.0 + u)
    aerr = err.abs()

    def sums_of(lp_parts, absolute):
        f = (lambda t: t.abs()) if absolute else (lambda t: t)
        cols = [sum(f(p) for p in lp_parts) if absolute else sum(lp_parts), f(reg), f(kla), f(klb), f(u)]
        S = [c.sum(0) for c in cols]                                       # each [3]
        S += [(m[k] * f(conf)).sum(0) for k in range(10)] + [(m[k] * aerr).sum(0) for k in range(10)] + [m[k].sum(0) for k in range(10)]
        return torch.stack(S, dim=1)                                       # [3, 35]

    population = m.sum(1).t().to(torch.int64)                              # [3, 10]

    def with_global(S):
        if global_stats is None:
            return S, float(B)
        G = global_stats.double()
        return S + (G[:105].view(3, NSTAT) - S.detach()), float(G[105])

    S_loc = sums_of(lp, False)
    A_loc = sums_of(lp, True).detach()
    S, N = with_global(S_loc)
    A = A_loc if global_stats is None else torch.maximum(A_loc, S.detach().abs())
    out, sc, gaps = _finals(S, A, N, cfg)

    # the components of the total, each differentiated on its own: their gradients add up to the gradient, their absolute values to its scale
    def only(which):
        """The sums with every piece but one group detached to zero."""
        zero = torch.zeros_like(reg)
        parts = [p if f"lp{i}" == which else zero for i, p in enumerate(lp)]
        cols = [sum(parts), reg if which == "reg" else zero, kla if which == "kla" else zero, klb if which == "klb" else zero,
                u if which.startswith("cross") else zero]
        Sx = [c.sum(0) for c in cols]
        on = which == "ece"
        Sx += [(m[k] * (conf if on else zero)).sum(0) for k in range(10)] + [(m[k] * (aerr if on else zero)).sum(0) for k in range(10)]
        Sx += [m[k].sum(0) for k in range(10)]
        return torch.stack(Sx, dim=1)

    w = cfg.task_w
    comps = []
    for i in range(4):
        Sx = only(f"lp{i}")
        comps.append(sum(w[d] * (-Sx[d, 0] / N) for d in range(3)) / 3.0)
    comps.append(sum(w[d] * cfg.reg_w * only("reg")[d, 1] / N for d in range(3)) / 3.0)
    comps.append(sum(w[d] * cfg.kl_w * only("kla")[d, 2] / N for d in range(3)) / 3.0)
    comps.append(sum(w[d] * cfg.kl_w * 0.1 * only("klb")[d, 3] / N for d in range(3)) / 3.0)
    ece_total = sum(w[d] * cfg.ece_w * out[d * 5 + 4] for d in range(3)) / 3.0
    comps.append(ece_total)
    leaves = (g, n, a, b)
    grads = torch.zeros(4, B, 3, dtype=torch.float64)
    gscale = torch.zeros(4, B, 3, dtype=torch.float64)

    def add(c, with_scale=True):
        if not torch.is_tensor(c) or not c.requires_grad:
            return
        for j, t in enumerate(torch.autograd.grad(c, leaves, retain_graph=True, allow_unused=True)):
            if t is not None:
                grads[j] += t
                if with_scale:
                    gscale[j] += t.abs()

    for i, c in enumerate(comps):
        add(c, with_scale=i != 2)
    # -lgamma's derivative is -digamma, which float32 forms on [1, 6) as a sum itself: the recurrence terms 1 / (x + i) up to
    # x + i >= 6, then log x - 1 / (2 x) - ...: those are its pieces (digamma has a zero at 1.46, they have none)
    x = (a + EPS).detach().clone()
    dig_s = torch.zeros_like(x)
    for _ in range(5):
        low = x < 6.0
        dig_s += torch.where(low, 1.0 / x, torch.zeros_like(x))
        x = torch.where(low, x + 1.0, x)
    dig_s += torch.log(x).abs() + 0.5 / x
    gscale[2] += torch.tensor([abs(wd) for wd in w], dtype=torch.float64) / (3.0 * N) * dig_s
    if cfg.cross_w > 0:
        ub = [S[d, 4] / N for d in range(3)]
        cross = sum((ub[i] - ub[j]) ** 2 for i in range(3) for j in range(i + 1, 3)) / 3.0
        add(cfg.cross_w * cross / 3.0, with_scale=False)
        # its pieces: 2/3 (ubar_d - ubar_j) for the two other dimensions j, each a difference of two means of u
        du = torch.autograd.grad(u.sum(), leaves, retain_graph=True, allow_unused=True)
        ua = [float(A[d, 4] / N) for d in range(3)]
        pair = torch.tensor([sum(ua[d] + ua[j] for j in range(3) if j != d) for d in range(3)], dtype=torch.float64)
        for j, t in enumerate(du):
            if t is not None:
                gscale[j] += (cfg.cross_w / 3.0) * (2.0 / 3.0) * pair / N * t.abs()
    det = lambda v: v.detach().double() if torch.is_tensor(v) else torch.tensor(float(v), dtype=torch.float64)
    counts = S.detach()[:, 25:35].round().to(torch.int64)
    return Ref(out=torch.stack([det(v) for v in out]), out_scale=torch.stack([det(v) for v in sc]),
               sums=S_loc.detach().reshape(-1), sums_scale=A_loc.reshape(-1), counts=counts, grads=grads, grad_scale=gscale,
               bin_population=population, min_gap=min(gaps) if gaps else float("inf"))


# --------------------------------------------------------------------------- the comparison rule
def worst_ratio(got: torch.Tensor, ref: torch.Tensor, scale: torch.Tensor) -> float:
    """max |got - ref| / (2^-24 * scale) over ALL elements.  A reference value that float32 cannot hold, or that is not finite, must
    come out as the same inf / NaN (ratio 0), anything else there counts as inf; so does a non-finite value where the reference
    is finite."""
    got, ref, scale = got.detach().double().cpu().reshape(-1), ref.double().reshape(-1), scale.double().reshape(-1)
    assert got.shape == ref.shape == scale.shape, (got.shape, ref.shape, scale.shape)
    ref32 = ref.float().double()                      # overflow to inf as float32 does
    special = ~torch.isfinite(ref32)
    same = (torch.isnan(got) & torch.isnan(ref32)) | (got == ref32)
    r = (got - ref).abs() / (ULP * scale)
    r = torch.where((got == ref), torch.zeros_like(r), r)              # 0 / 0 where a value and its scale are both exactly zero
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    r = torch.where(special, torch.where(same, torch.zeros_like(r), torch.full_like(r, float("inf"))), r)
    return float(r.max()) if r.numel() else 0.0


def assert_close(name: str, got, ref, scale, K: float, log: Optional[list] = None) -> float:
    r = worst_ratio(got, ref, scale)
    if log is not None:
        log.append((name, r))
    assert r <= K, f"{name}: |got - ref| is {r:.3g} x 2^-24 x scale (allowed {K})"
    return r


def compare_loss(got_out, got_counts, got_grads, ref: Ref, K_loss: float, K_grad: float, log: Optional[list] = None, tag: str = ""):
    """What every GPU test of the loss asserts: 20 outputs and 4 x B x 3 gradient elements by the scale rule, 30 exact counts."""
    assert torch.equal(got_counts.detach().cpu().reshape(3, 10).to(torch.int64), ref.counts), \
        f"{tag} bin counts {got_counts.reshape(3, 10).tolist()} != {ref.counts.tolist()}"
    assert_close(f"{tag} loss_out", got_out, ref.out, ref.out_scale, K_loss, log)
    if got_grads is not None:
        assert_close(f"{tag} gradients", got_grads, ref.grads, ref.grad_scale, K_grad, log)


# --------------------------------------------------------------------------- float32 evaluation in the kernels' structure
FAULTS = ("half_open_left", "ece_sign", "kl_beta_factor", "cross_third", "no_upper_half", "last_partial_twice", "task_w_ignored")


def _digamma32(x):
    return torch.digamma(x)


def float32_eval(gamma, nu, alpha, beta, targets, cfg: LossConfig = LossConfig(), fault: Optional[str] = None, block: int = 256,
                 global_stats: Optional[torch.Tensor] = None):
    """csrc/nig_dev.h in float32 torch-CPU arithmetic: returns (out [20], counts [3, 10], grads [4, B, 3], stats [105]).
    ``fault``: one of FAULTS, a deliberately wrong kernel."""
    assert fault is None or fault in FAULTS
    f = torch.float32
    g, n, a, b, y = (t.to(f) for t in (gamma, nu, alpha, beta, targets))
    B = g.shape[0]
    eps = torch.tensor(EPS, dtype=f)
    err = y - g
    e2 = err * err
    A_ = b + 0.5 * n * e2 + eps
    lb = torch.log(b + eps)
    two_pi = torch.tensor(2 * math.pi + EPS, dtype=f)
    logprob = 0.5 * torch.log(n / two_pi) + a * lb - torch.lgamma(a + eps) - (a + 0.5) * torch.log(A_)
    aerr = err.abs()
    reg = e2 * (2.0 * b + n * e2)
    am1 = a - 1.0
    kla, klb = am1 * am1, lb * lb
    u = b / (am1 + eps)
    conf = 1.0 / (1.0 + u)
    m = bin_masks(conf, half_open_left=fault == "half_open_left")
    mf = m.to(f)
    per = torch.stack([logprob, reg, kla, klb, u] + [mf[k] * conf for k in range(10)] + [mf[k] * aerr for k in range(10)]
                      + [mf[k] for k in range(10)], dim=2)                 # [B, 3, 35]
    nblk = (B + block - 1) // block
    pad = torch.zeros(nblk * block - B, 3, NSTAT, dtype=f)
    part = torch.cat([per, pad], dim=0).view(nblk, block, 3, NSTAT).sum(1)   # block partials
    half = (nblk + 1) >> 1
    lower, upper = part[:half].sum(0), part[half:].sum(0)
    if fault == "no_upper_half":
        upper = torch.zeros_like(upper)
    if fault == "last_partial_twice":                                     # the clamped index of a batch of 16 not masked
        lower = lower + part[half - 1]
        if nblk > half:
            upper = upper + part[nblk - 1]
    S = lower + upper                                                      # [3, 35]
    stats = S.reshape(-1).clone()
    N = torch.tensor(float(B), dtype=f)
    if global_stats is not None:
        S = global_stats[:105].to(f).view(3, NSTAT)
        N = global_stats[105].to(f)
    tw = (1.0, 1.0, 1.0) if fault == "task_w_ignored" else cfg.task_w
    out = torch.zeros(20, dtype=f)
    sign = torch.zeros(3, 10, dtype=f)
    counts = S[:, 25:35].to(torch.int64)
    tot = torch.zeros((), dtype=f)
    ubar = []
    for d in range(3):
        ece = torch.zeros((), dtype=f)
        for k in range(10):
            cnt = S[d, 25 + k]
            if cnt > 0:
                diff = S[d, 5 + k] / cnt - (1.0 - S[d, 15 + k] / cnt)
                ece = ece + (cnt / N) * diff.abs()
                sign[d, k] = torch.sign(diff)
        nll, rg = -S[d, 0] / N, S[d, 1] / N
        kl = S[d, 2] / N + 0.1 * (S[d, 3] / N)
        total = nll + cfg.reg_w * rg + cfg.kl_w * kl + cfg.ece_w * ece
        out[d * 5:d * 5 + 5] = torch.stack([total, nll, rg, kl, ece])
        tot = tot + tw[d] * total
        ubar.append(S[d, 4] / N)
    d01, d02, d12 = ubar[0] - ubar[1], ubar[0] - ubar[2], ubar[1] - ubar[2]
    cross = (d01 * d01 + d02 * d02 + d12 * d12) / 3.0
    dcross = torch.stack([(2.0 / 3.0) * (d01 + d02), (2.0 / 3.0) * (-d01 + d12), (2.0 / 3.0) * (-d02 - d12)]).to(f)
    if cfg.cross_w > 0:
        tot = tot + cfg.cross_w * cross
    out[15], out[16] = cross, tot / 3.0
    out[17], out[18], out[19] = (out[1] + out[6] + out[11]) / 3.0, (out[2] + out[7] + out[12]) / 3.0, (out[3] + out[8] + out[13]) / 3.0
    # the closed-form gradient (loss_grad)
    invN = 1.0 / N
    cd = torch.tensor([w / 3.0 for w in tw], dtype=f)
    ah = a + 0.5
    sg = (mf * sign.t().unsqueeze(1)).sum(0)                               # [B, 3]: the sign of the sample's bin, 0 outside every bin
    if fault == "ece_sign":
        sg = -sg
    den = am1 + eps
    du_db, du_da = 1.0 / den, -u / den
    dconf_du = -conf * conf
    serr = torch.sign(err)
    third = 1.0 if fault == "cross_third" else 3.0
    gu = (cfg.cross_w / third) * dcross * invN
    cross_a = gu * du_da if cfg.cross_w > 0 else torch.zeros_like(u)
    cross_b = gu * du_db if cfg.cross_w > 0 else torch.zeros_like(u)
    klf = 1.0 if fault == "kl_beta_factor" else 0.2
    in_bin = sg != 0
    ece_a = torch.where(in_bin, cfg.ece_w * sg * dconf_du * du_da, torch.zeros_like(u))
    ece_b = torch.where(in_bin, cfg.ece_w * sg * dconf_du * du_db, torch.zeros_like(u))
    g_mu = cd * invN * (-(ah * n * err) / A_ + cfg.reg_w * (2.0 * b + 2.0 * n * e2) * (-2.0 * err) + cfg.ece_w * sg * (-serr))
    g_nu = cd * invN * (-(0.5 / n - ah * 0.5 * e2 / A_) + cfg.reg_w * e2 * e2)
    g_al = cd * invN * (-(lb - _digamma32(a + eps) - torch.log(A_)) + cfg.kl_w * 2.0 * am1 + ece_a) + cross_a
    g_be = cd * invN * (-(a / (b + eps) - ah / A_) + cfg.reg_w * 2.0 * e2 + cfg.kl_w * klf * lb / (b + eps) + ece_b) + cross_b
    return out, counts, torch.stack([g_mu, g_nu, g_al, g_be]), stats


# --------------------------------------------------------------------------- the head's last layer
def nig_activations64(evid: torch.Tensor):
    """deer.py:90-98 in float64 from float32 evidence [B, 3, 4]: (7 x [B, 3] values, 7 scales)."""
    e = evid.double()
    sp = torch.nn.functional.softplus
    mu, nu, alpha, beta = e[..., 0], sp(e[..., 1]) + 1e-6, sp(e[..., 2]) + 1.0, sp(e[..., 3]) + 1e-6
    vals = [mu, nu, alpha, beta]
    scales = [mu.abs(), nu, alpha, beta]
    return vals, scales


def uncertainties64(nu, alpha, beta):
    """deer.py:96-98 from the float32 NIG parameters the kernel itself stored."""
    n, a, b = nu.double(), alpha.float().double(), beta.double()
    am1 = (alpha - 1.0).double()                       # exact in float32 for alpha in [1, 2], one rounding above: the kernel's own
    alea = b / am1
    epis = b / (n * am1)
    return [alea, epis, alea + epis], [alea.abs(), epis.abs(), alea.abs() + epis.abs()]


def head_reference(evid, e2, w3: Sequence[torch.Tensor], grads, grad_scale, mask_scale: float = 1.0, w3_read=None):
    """nig_bwd_kernel after the loss gradient: dE = g * (1, softplus'(e1), softplus'(e2), softplus'(e3)), dz2 = (dE . W3) * (e2 > 0)
    * mask_scale, dW3 = dE^T e2, db3 = sum dE.  evid [B, 3, 4] float32, e2 [B, 192] (the stored activation, as float32), w3: three
    [4, 64] (as the kernel reads them: ``w3_read`` rounds them, e.g. to bf16), grads / grad_scale [4, B, 3] float64.
    Returns a dict name -> (value, scale)."""
    B = evid.shape[0]
    x = evid.double()
    sg = torch.sigmoid(x)
    chain = torch.stack([torch.ones(B, 3, dtype=torch.float64), sg[..., 1], sg[..., 2], sg[..., 3]], dim=2)    # [B, 3, 4]
    dE = grads.permute(1, 2, 0) * chain
    dE_s = grad_scale.permute(1, 2, 0) * chain
    X = e2.double().view(B, 3, 64)
    keep = (X > 0).double() * mask_scale
    out: Dict[str, Tuple[torch.Tensor, torch.Tensor]] = {"dE": (dE, dE_s)}
    dz, dz_s, dw, dw_s, db, db_s = [], [], [], [], [], []
    for d in range(3):
        W = (w3_read(w3[d]) if w3_read else w3[d]).double()
        dz.append((dE[:, d] @ W) * keep[:, d])
        dz_s.append((dE_s[:, d] @ W.abs()) * keep[:, d])
        dw.append(dE[:, d].t() @ X[:, d])
        dw_s.append(dE_s[:, d].t() @ X[:, d].abs())
        db.append(dE[:, d].sum(0))
        db_s.append(dE_s[:, d].sum(0))
    out["dz2"] = (torch.cat(dz, dim=1), torch.cat(dz_s, dim=1))
    out["dW3"] = (torch.stack(dw), torch.stack(dw_s))
    out["db3"] = (torch.stack(db), torch.stack(db_s))
    return out


# --------------------------------------------------------------------------- inputs of the tests
def regular_case(B: int, seed: int = 0):
    """NIG parameters from evidence randn * (1, 2, 3, 3), one generator seed per dimension, targets tanh(randn): every dimension
    spreads over all ten bins."""
    sp = torch.nn.functional.softplus
    cols, ys = [], []
    for d in range(3):
        gen = torch.Generator().manual_seed(1000 * seed + 17 * d + 5)
        e = torch.randn(B, 4, generator=gen) * torch.tensor([1.0, 2.0, 3.0, 3.0])
        cols.append(e)
        ys.append(torch.tanh(torch.randn(B, generator=gen)))
    e = torch.stack(cols, dim=1)                                           # [B, 3, 4]
    gamma, nu, alpha, beta = e[..., 0].contiguous(), sp(e[..., 1]) + 1e-6, sp(e[..., 2]) + 1.0, sp(e[..., 3]) + 1e-6
    return gamma, nu, alpha, beta, torch.stack(ys, dim=1)


def _next(x: float, up: bool) -> float:
    t = torch.tensor(x, dtype=torch.float32)
    return float(torch.nextafter(t, torch.tensor(float("inf") if up else float("-inf"), dtype=torch.float32)))


def _conf_of_beta(beta: float) -> float:
    return float(conf32(torch.tensor([2.0], dtype=torch.float32), torch.tensor([beta], dtype=torch.float32))[0])


def edge_betas():
    """With alpha = 2 the denominator alpha - 1 + 1e-8 is exactly 1 in float32, so conf = 1 / (1 + beta).  For every interior edge
    k = 1..9: a beta whose confidence IS the float32 edge, and the betas of the attainable confidences next to it on either side.
    Returns a list of (k, beta_on, beta_below, beta_above) -- 'below' / 'above' speak of the confidence."""
    res = []
    for k in range(1, 10):
        edge = float(EDGES32[k])
        b0 = float(torch.tensor(1.0 / edge - 1.0, dtype=torch.float32))
        cands = [b0]
        lo = hi = b0
        for _ in range(64):
            lo, hi = _next(lo, False), _next(hi, True)
            cands += [lo, hi]
        on = [b for b in cands if _conf_of_beta(b) == edge]
        assert on, f"no float32 beta gives conf == edge {k}"
        b_on = on[0]
        b = b_on
        while _conf_of_beta(b) >= edge:      # confidence falls as beta grows
            b = _next(b, True)
        b_below = b
        b = b_on
        while _conf_of_beta(b) <= edge:
            b = _next(b, False)
        b_above = b
        res.append((k, b_on, b_below, b_above))
    return res


def edge_case(with_conf0: bool = True, seed: int = 1):
    """The edge samples as [E, 3] NIG parameters: for every interior edge the three confidences (on, below, above), conf == 1
    (bin 9), alpha == 1.0f exactly (u near 1e8: bin 0) and, in dimension 0 only, conf == 0 (beta / 1e-8 overflows: no bin).
    Returns (gamma, nu, alpha, beta, targets, expect) with expect = list of (row, expected bin) for dimension 0."""
    rows, expect = [], []
    for k, b_on, b_below, b_above in edge_betas():
        for bval, bin_ in ((b_on, k - 1), (b_below, k - 1), (b_above, k)):
            expect.append((len(rows), bin_))
            rows.append((2.0, bval))
    expect.append((len(rows), 9)); rows.append((2.0, 1e-9))               # 1 + 1e-9 == 1: conf == 1
    expect.append((len(rows), 0)); rows.append((1.0, 1.0))                # alpha == 1.0f: u = 1 / 1e-8
    if with_conf0:
        expect.append((len(rows), -1)); rows.append((1.0, 1e31))          # u = inf, conf == 0
    E = len(rows)
    gen = torch.Generator().manual_seed(seed)
    alpha = torch.tensor([r[0] for r in rows], dtype=torch.float32).view(E, 1).repeat(1, 3)
    beta = torch.tensor([r[1] for r in rows], dtype=torch.float32).view(E, 1).repeat(1, 3)
    if with_conf0:                   # inf - inf between two dimensions' mean u would be NaN where one inf is inf: dimension 0 only
        alpha[-1, 1:], beta[-1, 1:] = 2.0, 0.5
    # rotate the rows of the other dimensions so that a dimension mix-up shows
    alpha[:E - 1, 1], beta[:E - 1, 1] = alpha[:E - 1, 0].roll(1), beta[:E - 1, 0].roll(1)
    alpha[:E - 1, 2], beta[:E - 1, 2] = alpha[:E - 1, 0].roll(2), beta[:E - 1, 0].roll(2)
    gamma = torch.randn(E, 3, generator=gen)
    nu = torch.nn.functional.softplus(torch.randn(E, 3, generator=gen) * 2) + 1e-6
    y = torch.tanh(torch.randn(E, 3, generator=gen))
    return gamma, nu, alpha.contiguous(), beta.contiguous(), y, expect


# --------------------------------------------------------------------------- the cases of the stand-alone operator
# B by the number of 256-sample blocks the statistics kernel leaves for compute_finals: 1 block (upper half empty), 2, 3 (halves of 2
# and 1), 16, 17, 32 (one full batch of 16 per half), 33 (17 + 16: a second batch with one live entry), 34, 65 (three batches in a half)
FOLD_B = (1, 2, 255, 256, 257, 513, 4096, 4097, 8192, 8193, 8449, 16385)
CONFIGS = {
    "default": LossConfig(),
    "task_weights": LossConfig(task_w=(0.5, 1.0, 2.0)),
    "no_cross": LossConfig(cross_w=0.0),
    "no_ece": LossConfig(ece_w=0.0),
    "nll_only": LossConfig(reg_w=0.0, kl_w=0.0, ece_w=0.0, cross_w=0.0),
    "reg_only": LossConfig(reg_w=0.1, kl_w=0.0, ece_w=0.0, cross_w=0.0),
    "kl_only": LossConfig(reg_w=0.0, kl_w=0.01, ece_w=0.0, cross_w=0.0),
    "ece_50": LossConfig(ece_w=50.0),
    "cross_only": LossConfig(cross_w=1.0, task_w=(0.0, 0.0, 0.0)),
}
CONFIG_B = (513, 8193)
MIN_GAP = 1e-3
# generator seeds at which every case meets the conditions of checked_reference (searched on the CPU; most sizes take seed 1)
CASE_SEED = {4097: 2, 8192: 2}


def _seed(B: int) -> int:
    return CASE_SEED.get(B, 1)


def mixed_edge_case(with_conf0: bool):
    """The edge samples spread through a regular batch of 300 (every tenth row from row 3 on)."""
    ge, ne, ae, be, ye, expect = edge_case(with_conf0)
    g, n, a, b, y = regular_case(300, seed=9)
    rows = [3 + 9 * i for i in range(ge.shape[0])]
    assert rows[-1] < 300
    for dst, src in ((g, ge), (n, ne), (a, ae), (b, be), (y, ye)):
        dst[rows] = src
    return g, n, a, b, y, [(rows[r], k) for r, k in expect]


def loss_cases():
    """(tag, (gamma, nu, alpha, beta, targets), LossConfig, regular) of every stand-alone case."""
    cases = [(f"fold-B{B}", regular_case(B, seed=_seed(B)), LossConfig(), True) for B in FOLD_B]
    for name, cfg in CONFIGS.items():
        cases += [(f"cfg-{name}-B{B}", regular_case(B, seed=_seed(B)), cfg, True) for B in CONFIG_B]
    # conf == 0 means u = inf in float32: the cross term of its dimension is inf by definition (in the reference too), so the
    # set with that sample runs without the cross term, the set without it under the default configuration
    cases.append(("edges-alone-conf0", edge_case(True)[:5], LossConfig(cross_w=0.0), False))
    cases.append(("edges-alone", edge_case(False)[:5], LossConfig(), False))
    cases.append(("edges-in-300-conf0", mixed_edge_case(True)[:5], LossConfig(cross_w=0.0), False))
    cases.append(("edges-in-300", mixed_edge_case(False)[:5], LossConfig(), False))
    return cases


def checked_reference(tag, inputs, cfg, regular, **kw) -> Ref:
    """The reference of a case with the conditions the comparisons rest on (not measurements: the REFERENCE must meet them)."""
    ref = reference(*inputs, cfg, **kw)
    B = inputs[0].shape[0]
    if regular and B >= 255:
        assert int(ref.bin_population.min()) > 0, f"{tag}: an empty bin {ref.bin_population.tolist()}"
    # a float32 bin gap this far from zero cannot have another sign than the float64 one
    assert ref.min_gap >= MIN_GAP, f"{tag}: a bin gap of {ref.min_gap:.3g}: choose another seed"
    return ref
