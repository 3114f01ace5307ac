"""float64 numpy restatement of mmdeer_uncertainty_table (csrc/evalstats.hip) and of the four sections of
UncertaintyAnalyzer.analyze_uncertainty_quality built on it.

Plain numpy: the errors are the float32 |p - t| the kernel forms, everything after that is float64; the order is
np.argsort(kind='stable') (ties in index order, NaN last).  It reads nothing of the reference project;
tests/golden/uncertainty_cases.npz holds the reference's own results for comparison.  The p-values are the module's
(mmdeer.evaluation.pearson_p_value: host arithmetic, checked against scipy's stored values in test_cpu_evaluation.py)."""
from __future__ import annotations

import math

import numpy as np

from mmdeer.evaluation import pearson_p_value

from . import eval_ref as E

NAN = float("nan")
DIMS = ("valence", "arousal", "dominance")
FRACTIONS = np.linspace(0.1, 1.0, 10)
LEVELS = (0.5, 0.95)
TABLE = 40


def cuts(n):
    """int(frac * n) for the reference's ten fractions, in Python floats."""
    return [int(float(f) * n) for f in FRACTIONS]


def errors32(pred, target):
    with np.errstate(invalid="ignore"):
        return np.abs(np.asarray(pred, dtype=np.float32) - np.asarray(target, dtype=np.float32))


def table(pred, target, unc, n_keep=None, levels=LEVELS, errors64=False):
    """table[D][40] as include/mmdeer.h lays it out.  ``errors64``: |p - t| subtracted in float64 instead, which is what the
    reference sees when it is handed float64 copies of the arrays (the `f64` captures of the fixture)."""
    unc = np.asarray(unc, dtype=np.float32)
    err = np.abs(np.asarray(pred, dtype=np.float64) - np.asarray(target, dtype=np.float64)) if errors64 else errors32(pred, target)
    N, D = unc.shape
    n_keep = cuts(N) if n_keep is None else list(n_keep)
    out = np.zeros((D, TABLE))
    with np.errstate(invalid="ignore"):
        for d in range(D):
            u, e = unc[:, d].astype(np.float64), err[:, d].astype(np.float64)
            du, de = u - u.sum() / N, e - e.sum() / N
            un, en = bool(np.isnan(u).any()), bool(np.isnan(e).any())
            out[d, :13] = [N, u.sum(), e.sum(), (du * du).sum(), (de * de).sum(), (du * de).sum(), u.sum() / N, (du * du).sum() / N,
                           u.min(), u.max(), e.min(), e.max(), un + 2 * en]
            order = np.argsort(unc[:, d], kind="stable")
            se = e[order]
            for k, n in enumerate(n_keep):
                out[d, 16 + k] = se[:n].sum()
            su = u[order]
            for k, q in enumerate(levels):
                out[d, 32 + k] = NAN if un else E.percentile_linear(su, q)
    return out


def trapezoid(y, x):
    y, x = np.asarray(y, dtype=np.float64), np.asarray(x, dtype=np.float64)
    return float(np.sum((x[1:] - x[:-1]) * (y[1:] + y[:-1]) / 2.0))


def correlation(tb):
    D = tb.shape[0]
    out = {}
    for d, dim in enumerate(DIMS[:D]):
        if tb[d, 12] or tb[d, 8] == tb[d, 9] or tb[d, 10] == tb[d, 11]:
            r = NAN
        else:
            r = min(1.0, max(-1.0, tb[d, 5] / math.sqrt(tb[d, 3] * tb[d, 4])))
        out[f"{dim}_correlation"] = float(r)
        out[f"{dim}_p_value"] = pearson_p_value(float(r), int(tb[d, 0]))
    out["average_correlation"] = float(np.mean([out[f"{dim}_correlation"] for dim in DIMS[:D]]))
    return out


def sparsification(tb):
    out = {}
    keep = cuts(int(tb[0, 0]))
    for d, dim in enumerate(DIMS[: tb.shape[0]]):
        means = [float(tb[d, 16 + k] / n) if n > 0 else 0.0 for k, n in enumerate(keep)]
        out[f"{dim}_ause"] = trapezoid(means, FRACTIONS)
        out[f"{dim}_sparsification_curve"] = {"fractions": FRACTIONS.tolist(), "errors": means}
    return out


def distribution(tb):
    out = {}
    for d, dim in enumerate(DIMS[: tb.shape[0]]):
        out.update({f"{dim}_mean": float(tb[d, 6]), f"{dim}_std": float(np.sqrt(tb[d, 7])), f"{dim}_min": float(tb[d, 8]),
                    f"{dim}_max": float(tb[d, 9]), f"{dim}_median": float(tb[d, 32]), f"{dim}_percentile_95": float(tb[d, 33])})
    return out


def calibration(pred, target, unc, n_bins=15):
    """analyze_calibration: the ECE of eval_ref and sklearn's non-empty (lo, hi] bins; no curve key where calibration_curve
    would raise."""
    pred, target, unc = (np.asarray(x, dtype=np.float32) for x in (pred, target, unc))
    out = {}
    for d, dim in enumerate(DIMS[: pred.shape[1]]):
        stats, bins = E.calibration_bins(pred[:, d], target[:, d], unc[:, d], n_bins)
        out[f"{dim}_ece"] = float(E.ece(pred[:, d], target[:, d], unc[:, d], n_bins))
        if stats[2]:
            continue
        b = bins[1][bins[1][:, 0] != 0]
        out[f"{dim}_calibration_curve"] = {"mean_predicted_value": (b[:, 1] / b[:, 0]).tolist(),
                                           "fraction_of_positives": (b[:, 2] / b[:, 0]).tolist()}
    return out


def analyze(pred, target, unc, errors64=False):
    tb = table(pred, target, unc, errors64=errors64)
    return {"uncertainty_error_correlation": correlation(tb), "calibration_analysis": calibration(pred, target, unc),
            "sparsification_analysis": sparsification(tb), "uncertainty_distribution": distribution(tb)}


def flatten(res, prefix=""):
    """{'section.key[.sub]': float array} of a result dictionary, for storing and comparing."""
    out = {}
    for k, v in res.items():
        if isinstance(v, dict):
            out.update(flatten(v, f"{prefix}{k}."))
        else:
            out[f"{prefix}{k}"] = np.atleast_1d(np.asarray(v, dtype=np.float64))
    return out


def unpack(npz, meta, tag):
    """The flattened result dictionary stored under `<case>.<f32|f64>` in tests/golden/uncertainty_cases.npz."""
    values, out, at = npz[tag], {}, 0
    for key, size in meta["layout"][tag]:
        out[key] = values[at:at + size]
        at += size
    assert at == len(values)
    return out
