#!/usr/bin/env python3
"""Capture tests/golden/eval_cases.npz from the IMPORTED reference evaluator (build container only).

Run from the repo root:  python tests/golden/make_golden_eval.py
src/training/evaluation.py is imported with an empty `seaborn` stub (scipy, sklearn, pandas, matplotlib are installed).
For the bootstrap, np.random.choice is replaced during the call by a function that returns synth.bootstrap_indices for
replicate (call number % R): the reference then computes its intervals on OUR draws.

Every case is captured twice: on the float32 arrays (`f32`: what evaluate_model feeds the reference) and on float64 copies
of the same values (`f64`: the reference's arithmetic is then exact to ~1e-16 and pins the formulas); compute_ece on
float32 only, since its dtype rules are the point.  meta.ref_vs_f64.<quantity> is the distance measured here between the
reference on float32 arrays and tests/eval_ref.py (float64 sums): the reference's own rounding, which the GPU tests allow
for (4 x) when they compare with the f32 capture.
"""
import contextlib
import io
import json
import os
import sys
import types
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as G  # noqa: E402  (sets up the import paths of the reference and of mmdeer)
import numpy as np  # noqa: E402

sys.path.insert(0, os.path.join(G.REF, "src", "training"))
sys.path.insert(0, os.path.join(G.ROOT, "tests"))

import eval_ref as E  # noqa: E402
from mmdeer import evaluation as M  # noqa: E402
from mmdeer import synth  # noqa: E402

R, SEED = 200, 20240917
LEVELS = (0.95, 0.8)
METRICS = ("ccc", "pearson")
SIG_KEYS = ("pearson_correlation", "pearson_p_value", "spearman_correlation", "spearman_p_value", "t_test_statistic",
            "t_test_p_value")
DIMS = ("valence", "arousal", "dominance")
N_BINS = 15


def reference_module():
    if "seaborn" not in sys.modules:
        m = types.ModuleType("seaborn")
        m.__spec__ = __import__("importlib.machinery").machinery.ModuleSpec("seaborn", None)
        sys.modules["seaborn"] = m
    with contextlib.redirect_stdout(io.StringIO()):
        import evaluation as ref  # (reference)
    return ref


def make_cases():
    """name -> (pred, target, unc) float32 (N, 3)."""
    def base(stream, n, noise):
        p = synth.normal(stream, n * 3).reshape(n, 3) * np.array([0.6, 0.5, 0.7]) + np.array([0.1, -0.2, 0.05])
        t = p * np.array([0.9, 1.1, 0.8]) + noise * synth.normal(stream + 1, n * 3).reshape(n, 3) + np.array([0.05, 0.0, -0.1])
        u = 0.02 + 0.5 * synth.uniform01(stream + 2, n * 3).reshape(n, 3)
        return p.astype(np.float32), t.astype(np.float32), u.astype(np.float32)

    cases = {}
    cases["plain"] = base(900, 1001, 0.3)                      # odd N; uncertainties fill all 15 bins
    p, t, u = base(910, 2000, 0.5)                             # even N; confidences leave bins empty (the misaligned zip)
    w = synth.uniform01(913, 2000 * 3).reshape(2000, 3)
    u = np.where(w < 0.5, 0.05 + 0.1 * w, 0.6 + 0.3 * w).astype(np.float32)
    u[0] = 1.0
    cases["even"] = (p, t, u)
    p, t, u = base(920, 1500, 0.4)                             # heavy ties; one negative uncertainty in dimension 1
    p, t = (np.round(p * 16) / 16).astype(np.float32), (np.round(t * 8) / 8).astype(np.float32)
    u[7, 1] = -0.01
    cases["ties"] = (p, t, u)
    p, t, u = base(930, 800, 0.3)                              # NaN rows in predictions and targets
    p[5::37, 0] = np.nan
    t[11::53, 0] = np.nan
    t[3::41, 1] = np.nan
    p[100] = np.nan
    cases["nan"] = (p, t, u)
    p, t, u = base(940, 500, 0.3)                              # a constant prediction column
    p[:, 1] = 0.25
    cases["constpred"] = (p, t, u)
    cases["n3"] = base(950, 3, 0.3)                            # replicates that are constant by chance
    cases["big"] = base(960, 5000, 0.6)
    return cases


def ref_intervals(ref, p, t, metric, level):
    N = len(p)
    calls = [0]

    def choice(n, size=None, replace=True):
        r = calls[0] % R
        calls[0] += 1
        return synth.bootstrap_indices(SEED, r, N)

    orig = np.random.choice
    np.random.choice = choice
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ci = ref.StatisticalValidator(level).compute_confidence_intervals(p, t, metric=metric, n_bootstrap=R)
    finally:
        np.random.choice = orig
    return np.array([ci[d] for d in DIMS], dtype=np.float64)


def populations(p, t, u):
    """Bin populations of both rules per dimension on the reference's float32 confidences ([D][2][N_BINS]), or -1 rows where
    the confidence leaves [0, 1]."""
    out = np.zeros((3, 2, N_BINS), dtype=np.int64)
    edges = np.linspace(0, 1, N_BINS + 1)
    for d in range(3):
        conf = 1.0 - (u[:, d] / (np.max(u[:, d]) + 1e-8))
        assert conf.dtype == np.float32
        for b in range(N_BINS):
            m = (conf >= edges[b]) & (conf < edges[b + 1])
            if b == N_BINS - 1:
                m = (conf >= edges[b]) & (conf <= edges[b + 1])
            out[d, 0, b] = m.sum()
        out[d, 1] = np.bincount(np.searchsorted(edges[1:-1], conf), minlength=N_BINS)[:N_BINS]
    return out


def own_sig(p, t):
    """eval_ref's correlations with the module's p-values, in SIG_KEYS order."""
    c = E.correlations(p, t)
    n = len(p)
    return np.array([[r, M.pearson_p_value(r, n), rs, M.spearman_p_value(rs, n), *M.t_test(r, n)] for r, rs, _ in c])


def rel(a, b, floor=0.0):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    ok = ~(np.isnan(a) | np.isnan(b)) & (np.abs(b) >= floor) & (b != 0)
    return float(np.max(np.abs(a[ok] - b[ok]) / np.abs(b[ok]))) if ok.any() else 0.0


def absd(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    ok = ~(np.isnan(a) | np.isnan(b))
    return float(np.max(np.abs(a[ok] - b[ok]))) if ok.any() else 0.0


def capture():
    ref = reference_module()
    out = {}
    dist = {k: 0.0 for k in ("ci", "ccc", "mae", "rmse", "ece", "pearson", "spearman", "t_stat", "pearson_p", "spearman_p", "t_p")}
    names = []
    for name, (p32, t32, u32) in make_cases().items():
        names.append(name)
        out[f"{name}.pred"], out[f"{name}.target"], out[f"{name}.unc"] = p32, t32, u32
        N = len(p32)
        mom, flags = E.bootstrap_moments(p32, t32, R, SEED)
        has_nan = bool(np.isnan(p32).any() or np.isnan(t32).any())
        for variant, (p, t) in (("f32", (p32, t32)), ("f64", (p32.astype(np.float64), t32.astype(np.float64)))):
            ev = ref.DEERModelEvaluator()
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                for metric in METRICS:
                    for level in LEVELS:
                        ci = ref_intervals(ref, p, t, metric, level)
                        out[f"{name}.{variant}.ci.{metric}.{level}"] = ci
                        if variant == "f32":
                            own, _ = E.confidence_intervals(mom, flags, N, 0 if metric == "ccc" else 1, level)
                            dist["ci"] = max(dist["ci"], absd(ci, own))
                sig = ref.StatisticalValidator(0.95).run_significance_tests(p, t)
                sig = np.array([[float(sig[d][k]) for k in SIG_KEYS] for d in DIMS], dtype=np.float64)
                ccc = np.array([float(ev._compute_ccc_scores(p, t)[d]) for d in DIMS])
                if has_nan:           # sklearn's mean_absolute_error refuses NaN: nothing to capture
                    mae = rmse = np.full(3, np.nan)
                else:
                    mae = np.array([float(ev._compute_mae_scores(p, t)[d]) for d in DIMS])
                    rmse = np.array([float(ev._compute_rmse_scores(p, t)[d]) for d in DIMS])
            out[f"{name}.{variant}.sig"], out[f"{name}.{variant}.ccc"] = sig, ccc
            out[f"{name}.{variant}.mae"], out[f"{name}.{variant}.rmse"] = mae, rmse
            if variant == "f32":
                o = own_sig(p32, t32)
                a = E.agreement(p32, t32)
                dist["ccc"] = max(dist["ccc"], absd(ccc, a[:, 0]))
                dist["mae"] = max(dist["mae"], absd(mae, a[:, 1]))
                dist["rmse"] = max(dist["rmse"], absd(rmse, a[:, 2]))
                dist["pearson"] = max(dist["pearson"], absd(sig[:, 0], o[:, 0]))
                dist["spearman"] = max(dist["spearman"], absd(sig[:, 2], o[:, 2]))
                dist["t_stat"] = max(dist["t_stat"], rel(o[:, 4], sig[:, 4]))
                dist["pearson_p"] = max(dist["pearson_p"], rel(o[:, 1], sig[:, 1], 1e-290))
                dist["spearman_p"] = max(dist["spearman_p"], rel(o[:, 3], sig[:, 3], 1e-290))
                dist["t_p"] = max(dist["t_p"], absd(sig[:, 5], o[:, 5]))
        with warnings.catch_warnings(), contextlib.redirect_stderr(io.StringIO()):
            warnings.simplefilter("ignore")
            ece = np.array([float(ref.CalibrationAnalyzer().compute_ece(p32[:, d], t32[:, d], u32[:, d], N_BINS)) for d in range(3)])
        out[f"{name}.ece"] = ece
        out[f"{name}.bin_counts"] = populations(p32, t32, u32)
        dist["ece"] = max(dist["ece"], absd(ece, [E.ece(p32[:, d], t32[:, d], u32[:, d], N_BINS) for d in range(3)]))
    meta = {"cases": names, "R": R, "seed": SEED, "levels": list(LEVELS), "metrics": list(METRICS), "sig_keys": list(SIG_KEYS),
            "n_bins": N_BINS, "ref_vs_f64": dist}
    out["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    return out, meta


if __name__ == "__main__":
    data, meta = capture()
    path = os.path.join(HERE, "eval_cases.npz")
    np.savez_compressed(path, **data)
    print(json.dumps(meta["ref_vs_f64"], indent=1))
    print("wrote", path, os.path.getsize(path), "bytes")
