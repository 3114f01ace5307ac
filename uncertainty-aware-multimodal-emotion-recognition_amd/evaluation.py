"""The reference's evaluator (src/training/evaluation.py) with every statistic computed on the GPU (csrc/evalstats.hip).

``DEERModelEvaluator.evaluate_model`` returns an ``EvaluationResults`` with per-dimension CCC / MAE / RMSE / ECE,
significance tests and bootstrap confidence intervals, like the reference's.  The (N, D) prediction, target and
uncertainty arrays stay in HBM: what reaches the host is a few dozen moment sums, the bin tables and ``ci[D][2]``.

Inputs of the statistics classes are (N, D) float32 GPU tensors, 1 <= D <= 3; there is no CPU path.  Returned numbers are
Python floats.  scipy and sklearn are not used: the Student-t / Beta distribution functions the p-values need are written
out below on ``math.lgamma``.

Differences from the reference, all deliberate:

* ``evaluate_model`` in the reference ignores its own ``n_bootstrap`` and always resamples 1000 times
  (evaluation.py:209-211); here the constructor's value is used (the default is 1000 either way).
* The bootstrap draws one row index per (replicate, draw) and uses it for all D dimensions; the reference draws per
  dimension.  Each interval is a marginal statistic of one dimension, so its distribution is the same.  The draws are a
  counter hash of ``seed`` (``synth.bootstrap_indices``), not numpy's global generator: a call is reproducible.
* Spearman sorts on the device, at most 2**20 samples; a larger N is refused with a message.
* ``UncertaintyAnalyzer`` orders the samples by uncertainty with the device's STABLE sort (ties in index order, NaN last).
  The reference calls ``np.argsort`` with its default kind, whose order among equal uncertainties is unspecified (and
  differs from the stable one in practice).  The sparsification results agree whenever no run of equal uncertainties
  straddles a cut point ``int(frac * N)``; where one does, the stable order is the definition here.  2 <= N <= 2**20.
"""
from __future__ import annotations

import math
import time
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib

EMOTION_DIMS = ("valence", "arousal", "dominance")
NAN = float("nan")


# ---------------------------------------------------------------------------------------------------------------------
# distribution functions (regularised incomplete beta by its continued fraction, modified Lentz)
def _betacf(a: float, b: float, x: float) -> float:
    tiny, eps = 1e-300, 1e-16
    qab, qap, qam = a + b, a + 1.0, a - 1.0
    c, d = 1.0, 1.0 - qab * x / qap
    if abs(d) < tiny:
        d = tiny
    d = 1.0 / d
    h = d
    for m in range(1, 200001):
        m2 = 2 * m
        aa = m * (b - m) * x / ((qam + m2) * (a + m2))
        d = 1.0 + aa * d
        if abs(d) < tiny:
            d = tiny
        c = 1.0 + aa / c
        if abs(c) < tiny:
            c = tiny
        d = 1.0 / d
        h *= d * c
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2))
        d = 1.0 + aa * d
        if abs(d) < tiny:
            d = tiny
        c = 1.0 + aa / c
        if abs(c) < tiny:
            c = tiny
        d = 1.0 / d
        delta = d * c
        h *= delta
        if abs(delta - 1.0) < eps:
            break
    return h


def betainc(a: float, b: float, x: float, y: Optional[float] = None) -> float:
    """Regularised incomplete beta I_x(a, b); ``y`` = 1 - x when the caller knows it more exactly than the subtraction."""
    if y is None:
        y = 1.0 - x
    if math.isnan(x) or math.isnan(y) or a <= 0 or b <= 0:
        return NAN
    if x <= 0.0:
        return 0.0
    if y <= 0.0:
        return 1.0
    lfront = math.lgamma(a + b) - math.lgamma(a) - math.lgamma(b) + a * math.log(x) + b * math.log(y)
    if x < (a + 1.0) / (a + b + 2.0):
        return math.exp(lfront) * _betacf(a, b, x) / a
    return 1.0 - math.exp(lfront) * _betacf(b, a, y) / b


def student_t_sf(t: float, df: float) -> float:
    """P(T > t) of Student's t with df degrees of freedom."""
    if math.isnan(t) or not df > 0:
        return NAN
    if math.isinf(t):
        return 0.0 if t > 0 else 1.0
    t2 = t * t
    tail = 0.5 * betainc(0.5 * df, 0.5, df / (df + t2), t2 / (df + t2))
    return tail if t >= 0 else 1.0 - tail


def student_t_cdf(t: float, df: float) -> float:
    return student_t_sf(-t, df) if not math.isnan(t) else NAN


def pearson_p_value(r: float, n: int) -> float:
    """Two-sided p-value of scipy.stats.pearsonr: r ~ Beta(n/2 - 1, n/2 - 1) on [-1, 1] under the null."""
    if math.isnan(r):
        return NAN
    if n == 2:
        return 1.0
    ab = 0.5 * n - 1.0
    return min(1.0, 2.0 * betainc(ab, ab, 0.5 * (1.0 - abs(r)), 0.5 * (1.0 + abs(r))))


def spearman_p_value(rs: float, n: int) -> float:
    """Two-sided p-value of scipy.stats.spearmanr: t = rs sqrt(dof / ((rs + 1)(1 - rs))), Student's t with dof = n - 2."""
    dof = n - 2
    if math.isnan(rs) or dof <= 0:
        return NAN
    with np.errstate(divide="ignore", invalid="ignore"):
        t = float(np.float64(rs) * np.sqrt(np.clip(np.float64(dof) / ((np.float64(rs) + 1.0) * (1.0 - np.float64(rs))), 0, None)))
    return min(1.0, 2.0 * student_t_sf(abs(t), dof))


def t_test(corr: float, n: int) -> Tuple[float, float]:
    """The reference's t-test against zero correlation, literally (evaluation.py:599-601): the p-value is
    2 * (1 - cdf(|t|)), a difference from 1 that is exactly 0.0 for a large t."""
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.float64(corr)
        t = float(c * np.sqrt(np.float64(n - 2) / (1.0 - c ** 2)))
    if math.isnan(t) or n - 2 <= 0:
        return t, NAN
    return t, 2.0 * (1.0 - student_t_cdf(abs(t), n - 2))


# ---------------------------------------------------------------------------------------------------------------------
def _gpu2d(t, what: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"mmdeer.evaluation: {what} must be a GPU tensor (there is no CPU fallback)")
    t = t.detach()
    if t.dim() == 1:
        t = t[:, None]
    if t.dim() != 2 or not 1 <= t.shape[1] <= 3:
        raise ValueError(f"mmdeer.evaluation: {what} must be (N, D) with 1 <= D <= 3, got {tuple(t.shape)}")
    return t.float().contiguous()


def _pair(pred, tgt) -> Tuple[torch.Tensor, torch.Tensor]:
    p, t = _gpu2d(pred, "predictions"), _gpu2d(tgt, "targets")
    if p.shape != t.shape:
        raise ValueError(f"mmdeer.evaluation: predictions {tuple(p.shape)} and targets {tuple(t.shape)} differ in shape")
    if p.shape[0] == 0:
        raise ValueError("mmdeer.evaluation: no samples")
    return p, t


def _pad3(x: torch.Tensor) -> torch.Tensor:
    """(N, D) -> (N, 3) with NaN columns (mmdeer_eval_accumulate skips NaN pairs): plumbing for D < 3."""
    if x.shape[1] == 3:
        return x
    return torch.cat([x, torch.full((x.shape[0], 3 - x.shape[1]), NAN, dtype=x.dtype, device=x.device)], dim=1).contiguous()


def full_sample_sums(p: torch.Tensor, t: torch.Tensor) -> np.ndarray:
    """acc[3][8] of mmdeer_eval_accumulate over the whole sample, on the host (192 bytes)."""
    acc = torch.zeros(3, 8, dtype=torch.float64, device=p.device)
    p3, t3 = _pad3(p), _pad3(t)          # named: a temporary would be freed (and its memory reused) before the launch
    _lib.check(_lib.load().mmdeer_eval_accumulate(p3.data_ptr(), t3.data_ptr(), None, acc.data_ptr(), None, None,
                                                  p.shape[0], _lib.current_stream()))
    return acc.cpu().numpy()


def _pearson_from_sums(s) -> float:
    n, sp, st, spp, stt, spt = (float(v) for v in s[:6])
    mp, mt = sp / n, st / n
    vp, vt, cov = spp / n - mp * mp, stt / n - mt * mt, spt / n - mp * mt
    if not (vp > 0 and vt > 0):
        return NAN
    return max(-1.0, min(1.0, cov / math.sqrt(vp * vt)))


def bootstrap_moments(p: torch.Tensor, t: torch.Tensor, n_bootstrap: int, seed: int = 0):
    """mom (R, D, 6) float64 and flags (R, D) int32 device tensors of mmdeer_bootstrap_moments."""
    lib = _lib.load()
    N, D = p.shape
    R = int(n_bootstrap)
    mom = torch.empty(max(R, 0), D, 6, dtype=torch.float64, device=p.device)
    flags = torch.empty(max(R, 0), D, dtype=torch.int32, device=p.device)
    nbytes = int(lib.mmdeer_bootstrap_scratch(N, R))
    scratch = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=p.device)
    _lib.check(lib.mmdeer_bootstrap_moments(p.data_ptr(), t.data_ptr(), N, D, R, int(seed) & 0xFFFFFFFFFFFFFFFF, mom.data_ptr(),
                                            flags.data_ptr(), scratch.data_ptr(), scratch.numel(), _lib.current_stream()))
    return mom, flags


def bootstrap_ci(mom: torch.Tensor, flags: torch.Tensor, N: int, metric: int, q_lo: float, q_hi: float):
    """ci (D, 2) float64 and nkept (D,) int32 device tensors of mmdeer_bootstrap_ci."""
    R, D = flags.shape
    ci = torch.empty(D, 2, dtype=torch.float64, device=mom.device)
    nkept = torch.empty(D, dtype=torch.int32, device=mom.device)
    _lib.check(_lib.load().mmdeer_bootstrap_ci(mom.data_ptr(), flags.data_ptr(), N, D, R, metric, q_lo, q_hi, ci.data_ptr(),
                                               nkept.data_ptr(), _lib.current_stream()))
    return ci, nkept


def sort_pairs(keys: torch.Tensor, column: int = 0):
    """Stable ascending order (int32, == np.argsort(kind='stable')) of keys[:, column] and the sorted-pair scratch."""
    lib = _lib.load()
    k = keys if keys.dim() == 2 else keys[:, None]
    n, stride = k.shape
    order = torch.empty(n, dtype=torch.int32, device=k.device)
    nbytes = int(lib.mmdeer_sort_pairs_scratch(n))
    scratch = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=k.device)
    _lib.check(lib.mmdeer_sort_pairs(k.data_ptr() + 4 * column, stride, n, order.data_ptr(), scratch.data_ptr(), nbytes,
                                     _lib.current_stream()))
    return order, scratch


def average_ranks(keys: torch.Tensor, column: int = 0) -> torch.Tensor:
    """Tie-averaged 1-based ranks (float64) of keys[:, column]: scipy.stats.rankdata."""
    k = keys if keys.dim() == 2 else keys[:, None]
    _, scratch = sort_pairs(k, column)
    ranks = torch.empty(k.shape[0], dtype=torch.float64, device=k.device)
    _lib.check(_lib.load().mmdeer_average_ranks(scratch.data_ptr(), k.shape[0], ranks.data_ptr(), _lib.current_stream()))
    return ranks


def calibration_bins(p: torch.Tensor, t: torch.Tensor, u: torch.Tensor, n_bins: int):
    """(stats (D, 4), bins (D, 2, n_bins, 3)) of mmdeer_calibration_bins, as float64 numpy arrays on the host."""
    lib = _lib.load()
    N, D = p.shape
    dev = p.device
    edges = torch.from_numpy(np.linspace(0, 1, n_bins + 1)).to(dev) if n_bins >= 1 else torch.zeros(1, dtype=torch.float64, device=dev)
    stats = torch.empty(D, 4, dtype=torch.float64, device=dev)
    bins = torch.empty(D, 2, max(n_bins, 1), 3, dtype=torch.float64, device=dev)
    scratch = torch.empty(16, dtype=torch.float32, device=dev)
    _lib.check(lib.mmdeer_calibration_bins(p.data_ptr(), t.data_ptr(), u.data_ptr(), N, D, edges.data_ptr(), n_bins, stats.data_ptr(),
                                           bins.data_ptr(), scratch.data_ptr(), _lib.current_stream()))
    return stats.cpu().numpy(), bins.cpu().numpy()


SPARSIFICATION_FRACTIONS = np.linspace(0.1, 1.0, 10)
UNC_TABLE = _lib.UNC_TABLE
UNC_LEVELS = (0.5, 0.95)               # np.median, np.percentile(., 95)


def sparsification_cuts(n: int) -> List[int]:
    """The reference's own expression (evaluation.py:445-449), in Python floats: int(0.30000000000000004 * n) is the contract."""
    return [int(float(frac) * n) for frac in SPARSIFICATION_FRACTIONS]


def ause_from_means(errors, fractions=SPARSIFICATION_FRACTIONS) -> float:
    """np.trapz(errors, fractions), written out (the name left numpy 2)."""
    e, f = np.asarray(errors, dtype=np.float64), np.asarray(fractions, dtype=np.float64)
    return float(np.sum((f[1:] - f[:-1]) * (e[1:] + e[:-1]) / 2.0))


def uncertainty_table_device(p: torch.Tensor, t: torch.Tensor, u: torch.Tensor, n_keep, levels=UNC_LEVELS) -> torch.Tensor:
    """table (D, 40) float64 device tensor of mmdeer_uncertainty_table: include/mmdeer.h has the layout.  ``n_keep`` are
    ascending cut points in [0, N], ``levels`` quantile levels in [0, 1].  Enqueues only."""
    import ctypes as C
    lib = _lib.load()
    N, D = p.shape
    table = torch.empty(D, UNC_TABLE, dtype=torch.float64, device=p.device)
    nbytes = int(lib.mmdeer_uncertainty_table_scratch(N, D))
    scratch = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=p.device)
    keep = (C.c_longlong * max(len(n_keep), 1))(*[int(k) for k in n_keep])
    lev = (C.c_double * max(len(levels), 1))(*[float(q) for q in levels])
    _lib.check(lib.mmdeer_uncertainty_table(p.data_ptr(), t.data_ptr(), u.data_ptr(), N, D, keep, len(n_keep), lev, len(levels),
                                            table.data_ptr(), scratch.data_ptr(), nbytes, _lib.current_stream()))
    return table


def uncertainty_table(p: torch.Tensor, t: torch.Tensor, u: torch.Tensor, n_keep, levels=UNC_LEVELS) -> np.ndarray:
    """``uncertainty_table_device`` copied to the host (D x 320 bytes)."""
    return uncertainty_table_device(p, t, u, n_keep, levels).cpu().numpy()


def ece_from_bins(weight_bins, curve_bins, n: int) -> float:
    """The reference's sum (evaluation.py:511-524) from the two bin tables [n_bins][3] = {count, sum conf, sum acc}.

    ``weight_bins`` follow the reference's own rule ([lo, hi), last bin closed) and give the n_bins weights;
    ``curve_bins`` follow sklearn's calibration_curve ((lo, hi]), which returns its NON-EMPTY bins only.  The reference
    zips the n_bins weights with those shorter lists, so with an empty bin the triples are misaligned and the tail is cut:
    that is the value reproduced here."""
    weight_bins, curve_bins = np.asarray(weight_bins, dtype=np.float64), np.asarray(curve_bins, dtype=np.float64)
    weights = weight_bins[:, 0] / n
    nonzero = curve_bins[:, 0] != 0
    frac_pos = curve_bins[nonzero, 2] / curve_bins[nonzero, 0]
    mean_pred = curve_bins[nonzero, 1] / curve_bins[nonzero, 0]
    return float(np.sum([w * np.abs(a - c) for w, a, c in zip(weights, frac_pos, mean_pred) if w > 0]))


# ---------------------------------------------------------------------------------------------------------------------
@dataclass
class EvaluationResults:
    """Container of evaluation.py:42-103 (same fields, same ``to_dict``)."""
    ccc_valence: float
    ccc_arousal: float
    ccc_dominance: float
    ccc_average: float
    mae_valence: float
    mae_arousal: float
    mae_dominance: float
    mae_average: float
    rmse_valence: float
    rmse_arousal: float
    rmse_dominance: float
    rmse_average: float
    ece_valence: float
    ece_arousal: float
    ece_dominance: float
    ece_average: float
    significance_tests: Dict[str, Dict[str, float]]
    confidence_intervals: Dict[str, Tuple[float, float]]
    sample_size: int
    evaluation_time: float
    model_parameters: int

    def to_dict(self) -> Dict[str, Any]:
        return {
            "performance": {
                "ccc_valence": self.ccc_valence, "ccc_arousal": self.ccc_arousal, "ccc_dominance": self.ccc_dominance,
                "ccc_average": self.ccc_average, "mae_average": self.mae_average, "rmse_average": self.rmse_average,
                "ece_average": self.ece_average,
            },
            "detailed_metrics": {
                "mae": {"valence": self.mae_valence, "arousal": self.mae_arousal, "dominance": self.mae_dominance},
                "rmse": {"valence": self.rmse_valence, "arousal": self.rmse_arousal, "dominance": self.rmse_dominance},
                "ece": {"valence": self.ece_valence, "arousal": self.ece_arousal, "dominance": self.ece_dominance},
            },
            "statistical_validation": {
                "significance_tests": self.significance_tests,
                "confidence_intervals": self.confidence_intervals,
            },
            "meta": {"sample_size": self.sample_size, "evaluation_time": self.evaluation_time,
                     "model_parameters": self.model_parameters},
        }


class CalibrationAnalyzer:
    """evaluation.py:485-563: ``compute_ece`` and ``analyze_calibration``."""

    def compute_ece(self, predictions, targets, uncertainties, n_bins: int = 15) -> float:
        """ECE of 1-D GPU tensors as the reference computes it, quirks included (see ``ece_from_bins``): confidence
        1 - u / (max u + 1e-8) and the median threshold in float32, 0.0 when sklearn's calibration_curve would raise (a
        confidence outside [0, 1], i.e. a negative uncertainty, or a non-finite one)."""
        p, t = _pair(predictions, targets)
        u = _gpu2d(uncertainties, "uncertainties")
        if u.shape != p.shape:
            raise ValueError("mmdeer.evaluation: uncertainties and predictions differ in shape")
        return self._ece_all(p, t, u, n_bins)[0]

    def _ece_all(self, p, t, u, n_bins: int) -> List[float]:
        stats, bins = calibration_bins(p, t, u, n_bins)
        return [0.0 if stats[d, 2] != 0 else ece_from_bins(bins[d, 0], bins[d, 1], p.shape[0]) for d in range(p.shape[1])]

    def analyze_calibration(self, predictions, targets, uncertainties, n_bins: int = 15) -> Dict[str, Any]:
        """``{dim}_ece`` and ``{dim}_calibration_curve`` {'mean_predicted_value', 'fraction_of_positives'} per dimension of
        (N, D) GPU tensors: sklearn's non-empty bins ((lo, hi], rule 1 of ``calibration_bins``).  Where calibration_curve
        would raise (a confidence outside [0, 1] or a non-finite uncertainty) the reference logs a warning and leaves the
        curve key out, and its ECE is 0.0; so here."""
        p, t = _pair(predictions, targets)
        u = _gpu2d(uncertainties, "uncertainties")
        if u.shape != p.shape:
            raise ValueError("mmdeer.evaluation: uncertainties and predictions differ in shape")
        stats, bins = calibration_bins(p, t, u, n_bins)
        out: Dict[str, Any] = {}
        for d, dim in enumerate(EMOTION_DIMS[: p.shape[1]]):
            if stats[d, 2] != 0:
                out[f"{dim}_ece"] = 0.0
                continue
            out[f"{dim}_ece"] = ece_from_bins(bins[d, 0], bins[d, 1], p.shape[0])
            curve = bins[d, 1][bins[d, 1][:, 0] != 0]
            out[f"{dim}_calibration_curve"] = {"mean_predicted_value": (curve[:, 1] / curve[:, 0]).tolist(),
                                               "fraction_of_positives": (curve[:, 2] / curve[:, 0]).tolist()}
        return out


class UncertaintyAnalyzer:
    """evaluation.py:358-482.  One call of mmdeer_uncertainty_table serves the correlation, sparsification and
    distribution sections; the calibration section is ``CalibrationAnalyzer.analyze_calibration``.  What reaches the host
    is that table (D x 40 doubles) and the bin tables.

    The three private methods keep the reference's names and arguments, on (N, D) GPU tensors; ``errors`` are absolute
    errors (they enter as |errors - 0|).  ``table`` lets ``analyze_uncertainty_quality`` compute the table once."""

    def __init__(self):
        self.calibration_analyzer = CalibrationAnalyzer()

    def analyze_uncertainty_quality(self, predictions, targets, uncertainties) -> Dict[str, Any]:
        p, t = _pair(predictions, targets)
        u = _gpu2d(uncertainties, "uncertainties")
        if u.shape != p.shape:
            raise ValueError("mmdeer.evaluation: uncertainties and predictions differ in shape")
        table = uncertainty_table(p, t, u, sparsification_cuts(p.shape[0]))
        return {
            "uncertainty_error_correlation": self._compute_uncertainty_error_correlation(u, None, table),
            "calibration_analysis": self.calibration_analyzer.analyze_calibration(p, t, u),
            "sparsification_analysis": self._compute_sparsification_analysis(u, None, table),
            "uncertainty_distribution": self._analyze_uncertainty_distribution(u, table),
        }

    @staticmethod
    def _table(uncertainties, errors, table) -> np.ndarray:
        if table is not None:
            return table
        u = _gpu2d(uncertainties, "uncertainties")
        e = u if errors is None else _gpu2d(errors, "errors")
        if e.shape != u.shape:
            raise ValueError("mmdeer.evaluation: uncertainties and errors differ in shape")
        return uncertainty_table(e, torch.zeros_like(e), u, sparsification_cuts(u.shape[0]))

    def _compute_uncertainty_error_correlation(self, uncertainties, errors, table=None) -> Dict[str, float]:
        """Pearson correlation of (u, |error|) per dimension with scipy's p-value; NaN for a column with a NaN or a constant
        column (exactly: min == max), as pearsonr."""
        tb = self._table(uncertainties, errors, table)
        out: Dict[str, float] = {}
        for d, dim in enumerate(EMOTION_DIMS[: tb.shape[0]]):
            n, suu, see, sue = int(tb[d, 0]), float(tb[d, 3]), float(tb[d, 4]), float(tb[d, 5])
            if tb[d, 12] != 0 or tb[d, 8] == tb[d, 9] or tb[d, 10] == tb[d, 11] or not (suu > 0 and see > 0):
                corr = NAN
            else:
                corr = max(-1.0, min(1.0, sue / math.sqrt(suu * see)))
            out[f"{dim}_correlation"] = corr
            out[f"{dim}_p_value"] = pearson_p_value(corr, n)
        out["average_correlation"] = float(np.mean([out[f"{dim}_correlation"] for dim in EMOTION_DIMS[: tb.shape[0]]]))
        return out

    def _compute_sparsification_analysis(self, uncertainties, errors, table=None) -> Dict[str, Any]:
        """Mean error of the int(frac * N) least uncertain samples for frac = 0.1 .. 1.0 (0.0 where that count is 0) and
        the area under those ten means (AUSE, trapezoid rule)."""
        tb = self._table(uncertainties, errors, table)
        keep = sparsification_cuts(int(tb[0, 0]))
        out: Dict[str, Any] = {}
        for d, dim in enumerate(EMOTION_DIMS[: tb.shape[0]]):
            means = [float(tb[d, 16 + k]) / n_keep if n_keep > 0 else 0.0 for k, n_keep in enumerate(keep)]
            out[f"{dim}_ause"] = ause_from_means(means)
            out[f"{dim}_sparsification_curve"] = {"fractions": SPARSIFICATION_FRACTIONS.tolist(), "errors": means}
        return out

    def _analyze_uncertainty_distribution(self, uncertainties, table=None) -> Dict[str, float]:
        tb = self._table(uncertainties, None, table)
        out: Dict[str, float] = {}
        for d, dim in enumerate(EMOTION_DIMS[: tb.shape[0]]):
            out[f"{dim}_mean"] = float(tb[d, 6])
            out[f"{dim}_std"] = math.sqrt(tb[d, 7]) if tb[d, 7] >= 0 else NAN
            out[f"{dim}_min"] = float(tb[d, 8])
            out[f"{dim}_max"] = float(tb[d, 9])
            out[f"{dim}_median"] = float(tb[d, 32])
            out[f"{dim}_percentile_95"] = float(tb[d, 33])
        return out


class StatisticalValidator:
    """evaluation.py:566-682."""

    def __init__(self, confidence_level: float = 0.95):
        self.confidence_level = confidence_level
        self.alpha = 1.0 - confidence_level

    def run_significance_tests(self, predictions, targets) -> Dict[str, Dict[str, float]]:
        """Pearson, Spearman (average ranks for ties) and the t-test against zero correlation per dimension.  A NaN
        anywhere in a dimension's column, or a constant column, makes all six values of that dimension NaN, as scipy
        does.  N must be at least 2 (pearsonr raises below that) and at most 2**20 (the device sort)."""
        p, t = _pair(predictions, targets)
        N, D = p.shape
        if N < 2:
            raise ValueError("`x` and `y` must have length at least 2.")
        lib = _lib.load()
        sums = full_sample_sums(p, t)
        rm = torch.empty(D, 3, dtype=torch.float64, device=p.device)
        for d in range(D):
            ra, rb = average_ranks(p, d), average_ranks(t, d)
            _lib.check(lib.mmdeer_rank_moments(ra.data_ptr(), rb.data_ptr(), N, rm[d].data_ptr(), _lib.current_stream()))
        rm = rm.cpu().numpy()
        results: Dict[str, Dict[str, float]] = {}
        for d, dim in enumerate(EMOTION_DIMS[:D]):
            saa, sbb, sab = (float(v) for v in rm[d])
            # centred ranks are exact in float64: a zero sum of squares is a constant column (every rank (N + 1) / 2)
            if sums[d, 0] < N or saa == 0.0 or sbb == 0.0:
                corr = rs = NAN
            else:
                corr = _pearson_from_sums(sums[d])
                rs = max(-1.0, min(1.0, sab / math.sqrt(saa * sbb)))
            t_stat, t_p = t_test(corr, N)
            results[dim] = {
                "pearson_correlation": corr, "pearson_p_value": pearson_p_value(corr, N),
                "spearman_correlation": rs, "spearman_p_value": spearman_p_value(rs, N),
                "t_test_statistic": t_stat, "t_test_p_value": t_p,
            }
        return results

    def compute_confidence_intervals(self, predictions, targets, metric: str = "ccc", n_bootstrap: int = 1000,
                                     seed: int = 0) -> Dict[str, Tuple[float, float]]:
        """Percentile bootstrap intervals; ``metric`` 'ccc' or 'pearson' (anything else is Pearson, as in the reference).
        A NaN replicate is dropped before the percentile; with none left the interval is (0.0, 0.0).  ``seed`` selects the
        draws (``synth.bootstrap_indices``)."""
        p, t = _pair(predictions, targets)
        mom, flags = bootstrap_moments(p, t, n_bootstrap, seed)
        q_lo = ((1 - self.confidence_level) / 2 * 100) / 100
        q_hi = ((1 + self.confidence_level) / 2 * 100) / 100
        ci, nkept = bootstrap_ci(mom, flags, p.shape[0], 0 if metric.lower() == "ccc" else 1, q_lo, q_hi)
        ci, nkept = ci.cpu().numpy(), nkept.cpu().numpy()
        return {dim: ((float(ci[d, 0]), float(ci[d, 1])) if nkept[d] > 0 else (0.0, 0.0)) for d, dim in enumerate(EMOTION_DIMS[: p.shape[1]])}


class DEERModelEvaluator:
    """evaluation.py:106-355 for the models of this package (``MultimodalDEER``, ``stackb.CompleteDEERModel``: anything
    with ``get_predictions_and_uncertainties``), dict batches or (audio, video, text, targets) tuples.

    Unlike the reference, which ignores its own ``n_bootstrap`` in ``evaluate_model`` and always resamples 1000 times
    (evaluation.py:209-211), the constructor's value is used here."""

    def __init__(self, emotion_dims: Optional[List[str]] = None, confidence_level: float = 0.95, n_bootstrap: int = 1000):
        self.emotion_dims = list(emotion_dims) if emotion_dims is not None else list(EMOTION_DIMS)
        self.confidence_level = confidence_level
        self.n_bootstrap = n_bootstrap
        self.uncertainty_analyzer = UncertaintyAnalyzer()
        self.calibration_analyzer = CalibrationAnalyzer()
        self.statistical_validator = StatisticalValidator(confidence_level)

    def _per_dim(self, values: List[float]) -> Dict[str, float]:
        out = {dim: (values[i] if i < len(values) else 0.0) for i, dim in enumerate(self.emotion_dims)}
        out["average"] = float(np.mean([out[dim] for dim in self.emotion_dims]))
        return out

    def compute_scores(self, predictions, targets, uncertainties=None) -> Dict[str, Dict[str, float]]:
        """{'ccc' | 'mae' | 'rmse' | 'ece': {dimension: value, 'average': mean}} of (N, D) GPU tensors
        (_compute_ccc_scores / _mae_ / _rmse_ / _ece_scores, evaluation.py:257-316), from the sums of
        mmdeer_eval_accumulate: NaN pairs are masked; the CCC is 0.0 without a valid pair or for a zero denominator and
        NaN for a constant column (pearsonr)."""
        p, t = _pair(predictions, targets)
        D = p.shape[1]
        sums = full_sample_sums(p, t)
        ccc, mae, rmse = [], [], []
        for d in range(D):
            n, sp, st, spp, stt, spt, sabs, ssq = (float(v) for v in sums[d])
            if n == 0:
                ccc.append(0.0); mae.append(NAN); rmse.append(NAN)
                continue
            mp, mt = sp / n, st / n
            vp, vt, cov = spp / n - mp * mp, stt / n - mt * mt, spt / n - mp * mt
            den = vp + vt + (mp - mt) ** 2
            if den == 0:
                ccc.append(0.0)
            elif not (vp > 0 and vt > 0):
                ccc.append(NAN)
            else:
                rho = max(-1.0, min(1.0, cov / math.sqrt(vp * vt)))
                ccc.append(2.0 * rho * math.sqrt(vt * vp) / den)
            mae.append(sabs / n)
            rmse.append(math.sqrt(ssq / n))
        out = {"ccc": self._per_dim(ccc), "mae": self._per_dim(mae), "rmse": self._per_dim(rmse)}
        if uncertainties is not None:
            u = _gpu2d(uncertainties, "uncertainties")
            k = min(D, u.shape[1])
            out["ece"] = self._per_dim(self.calibration_analyzer._ece_all(p[:, :k].contiguous(), t[:, :k].contiguous(),
                                                                          u[:, :k].contiguous(), 15))
        else:
            out["ece"] = {**{dim: 0.0 for dim in self.emotion_dims}, "average": 0.0}
        return out

    @torch.no_grad()
    def evaluate_model(self, model, dataloader, device, return_predictions: bool = False):
        """Forward the loader, keep predictions / targets / uncertainties on the device and compute every statistic
        there.  ``return_predictions=True`` also returns the three (N, 3) device tensors."""
        from .trainer import unpack_batch
        start = time.time()
        device = torch.device(device)
        model.eval()
        ps, ts, us = [], [], []
        for batch in dataloader:
            a, v, x, y = unpack_batch(batch, device)
            out = model(a, v, x)
            pr, un = model.get_predictions_and_uncertainties(out)
            ps.append(pr.detach().float())
            ts.append(y.float())
            if un is not None:
                us.append(un.detach().float())
        if not ps:
            raise ValueError("mmdeer.evaluation: the dataloader gave no batch")
        predictions, targets = torch.cat(ps).contiguous(), torch.cat(ts).contiguous()
        uncertainties = torch.cat(us).contiguous() if us else None
        evaluation_time = time.time() - start
        scores = self.compute_scores(predictions, targets, uncertainties)
        significance = self.statistical_validator.run_significance_tests(predictions, targets)
        intervals = self.statistical_validator.compute_confidence_intervals(predictions, targets, metric="ccc",
                                                                            n_bootstrap=self.n_bootstrap)
        results = EvaluationResults(
            **{f"{m}_{k}": scores[m].get(k, 0.0) for m in ("ccc", "mae", "rmse", "ece") for k in (*EMOTION_DIMS, "average")},
            significance_tests=significance, confidence_intervals=intervals, sample_size=int(targets.shape[0]),
            evaluation_time=evaluation_time, model_parameters=sum(p.numel() for p in model.parameters()))
        if return_predictions:
            return results, predictions, targets, uncertainties
        return results


def evaluate_deer_model(model, dataloader, device, config: Optional[Dict] = None) -> EvaluationResults:
    """evaluation.py:785-808: a ``DEERModelEvaluator`` from ``config`` ('emotion_dims', 'confidence_level',
    'n_bootstrap'), returns its ``EvaluationResults``."""
    config = config or {}
    evaluator = DEERModelEvaluator(emotion_dims=config.get("emotion_dims", list(EMOTION_DIMS)),
                                   confidence_level=config.get("confidence_level", 0.95),
                                   n_bootstrap=config.get("n_bootstrap", 1000))
    return evaluator.evaluate_model(model, dataloader, device)
