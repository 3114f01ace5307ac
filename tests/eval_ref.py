"""float64 numpy restatement of the evaluator statistics (csrc/evalstats.hip) on explicit bootstrap indices.

It states what the kernels compute in the plainest numpy there is: gather by index, mask NaN pairs, sum.  It reads nothing
of the reference project; tests/golden/eval_cases.npz holds the reference's own results for comparison."""
from __future__ import annotations

import math

import numpy as np

from mmdeer import synth

NAN = float("nan")


# ---- 2a: moments of one replicate -----------------------------------------------------------------------------------------
def moments(pred, target, idx):
    """mom[D][6] = {n, sum p, sum t, sum p^2, sum t^2, sum pt} over the drawn rows without NaN, and flags[D] (bit 0: the
    drawn valid p are all equal, bit 1: t, bit 2: both and the constants are equal)."""
    pred, target = np.asarray(pred), np.asarray(target)
    D = pred.shape[1]
    mom, flags = np.zeros((D, 6)), np.zeros(D, dtype=np.int32)
    for d in range(D):
        pf, tf = pred[idx, d], target[idx, d]
        ok = ~(np.isnan(pf) | np.isnan(tf))
        pf, tf = pf[ok], tf[ok]
        p, t = pf.astype(np.float64), tf.astype(np.float64)
        mom[d] = [p.size, p.sum(), t.sum(), (p * p).sum(), (t * t).sum(), (p * t).sum()]
        if p.size:
            pc, tc = bool(pf.min() == pf.max()), bool(tf.min() == tf.max())
            flags[d] = pc | (tc << 1) | ((pc and tc and pf.min() == tf.min()) << 2)
    return mom, flags


def bootstrap_moments(pred, target, R, seed):
    N = len(pred)
    out = [moments(pred, target, synth.bootstrap_indices(seed, r, N)) for r in range(R)]
    return np.stack([m for m, _ in out]), np.stack([f for _, f in out])


# ---- 2b: metric per replicate, percentile ------------------------------------------------------------------------------------
def metric_value(m, flag, N, metric):
    """CCC (metric 0) or Pearson (1) of one replicate from its moments, with the reference's 0.0 / NaN rules."""
    n = m[0]
    if metric == 0:
        if n < 2:
            return 0.0
    elif n < N or N < 2:
        return NAN
    if metric == 0 and flag & 4:
        return 0.0
    if flag & 3:
        return NAN
    mp, mt = m[1] / n, m[2] / n
    vp, vt, cov = m[3] / n - mp * mp, m[4] / n - mt * mt, m[5] / n - mp * mt
    rho = min(1.0, max(-1.0, cov / math.sqrt(vp * vt)))
    if metric != 0:
        return rho
    den = vp + vt + (mp - mt) ** 2
    return 0.0 if den == 0 else 2.0 * rho * math.sqrt(vt * vp) / den


def percentile_linear(sorted_values, q):
    """np.percentile(values, 100 q), method 'linear', on an ascending array."""
    n = len(sorted_values)
    virt = (n - 1) * q
    lo = min(max(int(math.floor(virt)), 0), n - 1)
    hi = min(lo + 1, n - 1)
    a, b, t = sorted_values[lo], sorted_values[hi], virt - lo
    d = b - a
    r = a + d * t
    if t >= 0.5:
        r = b - d * (1 - t)
    return a if d == 0 else r


def confidence_intervals(mom, flags, N, metric, confidence_level):
    """ci[D][2] and nkept[D] from mom[R][D][6], flags[R][D]."""
    R, D = flags.shape
    q_lo = ((1 - confidence_level) / 2 * 100) / 100
    q_hi = ((1 + confidence_level) / 2 * 100) / 100
    ci, nkept = np.zeros((D, 2)), np.zeros(D, dtype=np.int64)
    for d in range(D):
        v = np.array([metric_value(mom[r, d], int(flags[r, d]), N, metric) for r in range(R)], dtype=np.float64)
        v = np.sort(v[~np.isnan(v)])
        nkept[d] = v.size
        if v.size:
            ci[d] = [percentile_linear(v, q_lo), percentile_linear(v, q_hi)]
    return ci, nkept


# ---- 2c: stable order, average ranks, Spearman ---------------------------------------------------------------------------------
def average_ranks(x):
    """scipy.stats.rankdata(x, 'average') restated: 1-based ranks, ties share the mean of their positions.  NaN keys count
    as one run of ties at the end (numpy sorts them last)."""
    x = np.asarray(x)
    order = np.argsort(x, kind="stable")
    s = x[order]
    n = len(x)
    new_run = np.ones(n, dtype=bool)
    new_run[1:] = ~((s[1:] == s[:-1]) | (np.isnan(s[1:]) & np.isnan(s[:-1])))
    starts = np.flatnonzero(new_run)
    ends = np.append(starts[1:], n)
    run = np.cumsum(new_run) - 1
    ranks = np.empty(n, dtype=np.float64)
    ranks[order] = 0.5 * (starts[run] + 1 + ends[run])
    return ranks


def rank_moments(ra, rb):
    c = 0.5 * (len(ra) + 1)
    a, b = ra - c, rb - c
    return np.array([(a * a).sum(), (b * b).sum(), (a * b).sum()])


def correlations(pred, target):
    """Per dimension {pearson, spearman, t statistic} in float64; NaN for a column with a NaN or a constant column."""
    pred, target = np.asarray(pred), np.asarray(target)
    N, D = pred.shape
    out = np.full((D, 3), NAN)
    for d in range(D):
        p, t = pred[:, d].astype(np.float64), target[:, d].astype(np.float64)
        if np.isnan(p).any() or np.isnan(t).any() or p.min() == p.max() or t.min() == t.max():
            continue
        pm, tm = p - p.mean(), t - t.mean()
        r = min(1.0, max(-1.0, (pm * tm).sum() / math.sqrt((pm * pm).sum() * (tm * tm).sum())))
        saa, sbb, sab = rank_moments(average_ranks(pred[:, d]), average_ranks(target[:, d]))
        rs = min(1.0, max(-1.0, sab / math.sqrt(saa * sbb)))
        with np.errstate(divide="ignore", invalid="ignore"):
            ts = float(np.float64(r) * np.sqrt(np.float64(N - 2) / (1.0 - np.float64(r) ** 2)))
        out[d] = [r, rs, ts]
    return out


def agreement(pred, target):
    """Per dimension {ccc, mae, rmse} of the NaN-masked full sample in float64."""
    pred, target = np.asarray(pred), np.asarray(target)
    out = []
    for d in range(pred.shape[1]):
        p, t = pred[:, d].astype(np.float64), target[:, d].astype(np.float64)
        ok = ~(np.isnan(p) | np.isnan(t))
        p, t = p[ok], t[ok]
        mom, flags = moments(pred[:, d:d + 1], target[:, d:d + 1], np.arange(len(pred)))
        ccc = metric_value(mom[0], int(flags[0]), len(pred), 0) if p.size >= 2 else 0.0
        out.append([ccc, np.abs(p - t).mean() if p.size else NAN, math.sqrt(((p - t) ** 2).mean()) if p.size else NAN])
    return np.array(out, dtype=np.float64)


# ---- 2d: calibration bins ----------------------------------------------------------------------------------------------------
def calibration_bins(pred, target, unc, n_bins=15):
    """One dimension (1-D float32 arrays): stats {max u, threshold, bad, threshold is NaN} and bins[2][n_bins][3] =
    {count, sum conf, sum acc} under rule 0 ([lo, hi), last bin closed) and rule 1 ((lo, hi], first bin closed).
    Confidence and threshold in float32, as numpy forms them from float32 arrays."""
    p, t, u = (np.asarray(x, dtype=np.float32) for x in (pred, target, unc))
    finite = np.isfinite(u)
    umax = np.float32(u[finite].max()) if finite.any() else np.float32(-np.inf)
    with np.errstate(all="ignore"):
        conf = (np.float32(1.0) - u / np.float32(umax + np.float32(1e-8))).astype(np.float32)
        err = np.abs(p - t)
        s = np.sort(err)
        n = len(err)
        thr = np.float32(NAN) if np.isnan(err).any() else np.float32((s[(n - 1) // 2] + s[n // 2]) / np.float32(2.0))
        acc = (err <= thr).astype(np.float64)
    c = conf.astype(np.float64)
    edges = np.linspace(0, 1, n_bins + 1)
    bins = np.zeros((2, n_bins, 3))
    for b in range(n_bins):
        lo, hi = edges[b], edges[b + 1]
        in0 = (c >= lo) & ((c < hi) | ((b == n_bins - 1) & (c <= hi)))
        in1 = ((b == 0) | (c > lo)) & ((b == n_bins - 1) | (c <= hi))
        for rule, m in ((0, in0), (1, in1)):
            bins[rule, b] = [m.sum(), c[m].sum(), acc[m].sum()]
    bad = (not finite.all()) or bool((~((c >= 0) & (c <= 1))).any())
    return np.array([float(umax), float(thr), float(bad), float(np.isnan(thr))]), bins


def ece(pred, target, unc, n_bins=15):
    """The reference's compute_ece from the bin tables, zip quirk included: n_bins weights against the non-empty bins only."""
    stats, bins = calibration_bins(pred, target, unc, n_bins)
    if stats[2]:
        return 0.0
    w = bins[0, :, 0] / len(pred)
    ne = bins[1, :, 0] != 0
    frac, mean = bins[1, ne, 2] / bins[1, ne, 0], bins[1, ne, 1] / bins[1, ne, 0]
    total = 0.0
    for k in range(min(len(w), len(frac))):
        if w[k] > 0:
            total += w[k] * abs(frac[k] - mean[k])
    return total
