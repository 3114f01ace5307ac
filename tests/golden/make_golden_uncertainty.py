#!/usr/bin/env python3
"""Capture tests/golden/uncertainty_cases.npz from the IMPORTED reference's UncertaintyAnalyzer (build container only).

Run from the repo root:  python tests/golden/make_golden_uncertainty.py
src/training/evaluation.py is imported with the empty `seaborn` stub of make_golden_eval.py.

Cases.  `plain`, `big`, `n3`, `nan`, `constpred`, `even`, `ties` reuse the inputs stored in eval_cases.npz (only results are
stored for them); `n7`, `nanunc`, `cancel`, `heavyties` bring their own inputs.  Every case is captured on the float32
arrays (`f32`) and on float64 copies (`f64`: the reference's arithmetic is then exact to ~1e-16 and pins the formulas); the
calibration section on float32 only, since its dtype rules are the point (as in make_golden_eval.py).  A result dictionary
is stored flattened, `<section>.<key>[.<sub>]` -> values (a list as it is, an absent key absent), all values of one
`<case>.<f32|f64>` in one array; meta.layout has the keys and lengths (tests/uncertainty_ref.py: unpack).

Checks made here.  For every case the reference on float64 copies must equal tests/uncertainty_ref.py (with |p - t| subtracted in float64, as
those copies give it) to 1e-12 (p-values: 1e-9 relative, scipy's Beta function against the module's).  The sparsification section depends on the ORDER among equal
uncertainties: the reference's np.argsort is not stable, the restatement's is.  A case whose sparsification section misses
1e-12 is listed in meta.restatement_only and that section of it is compared with the restatement only; the five cases whose
uncertainties are pairwise distinct in every column (checked) must not be among them.

meta.ref_vs_f64.<section> is the distance measured here between the reference on float32 arrays and the restatement: the
reference's own float32 rounding, which the GPU tests allow for (4 x).  Absolute, except `correlation_p` (relative).
"""
import contextlib
import io
import json
import logging
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden_eval as GE  # noqa: E402  (import paths of the reference and of mmdeer, the seaborn stub)
import numpy as np  # noqa: E402

from mmdeer import synth  # noqa: E402
from tests import uncertainty_ref as U  # noqa: E402

REUSED = ("plain", "big", "n3", "nan", "constpred", "even", "ties")
DISTINCT = ("plain", "big", "n3", "nan", "constpred")
SECTIONS = {"uncertainty_error_correlation": "correlation", "sparsification_analysis": "sparsification",
            "uncertainty_distribution": "distribution", "calibration_analysis": "calibration"}
P_FLOOR = 1e-290


def own_cases():
    """name -> (pred, target, unc) float32 (N, 3)."""
    def base(stream, n):
        p = synth.normal(stream, n * 3).reshape(n, 3) * 0.6
        t = 0.9 * p + 0.3 * synth.normal(stream + 1, n * 3).reshape(n, 3)
        u = 0.02 + 0.5 * synth.uniform01(stream + 2, n * 3).reshape(n, 3)
        u = u + 0.3 * np.abs(p - t)                                  # uncertainty that does rise with the error
        return p.astype(np.float32), t.astype(np.float32), u.astype(np.float32)

    cases = {}
    cases["n7"] = base(1000, 7)                                      # int(0.1 * 7) = 0: the first curve entry is 0.0
    p, t, u = base(1010, 300)                                        # one NaN uncertainty, in column 1
    u[123, 1] = np.nan
    cases["nanunc"] = (p, t, u)
    p, t, u = base(1020, 1500)                                       # cancellation in the variance and the correlation
    u = (1e-3 + 1e-6 * synth.uniform01(1023, 1500 * 3).reshape(1500, 3)).astype(np.float32)
    cases["cancel"] = (p, t, u)
    p, t, u = base(1030, 1000)                                       # heavy ties: runs of equal uncertainties at every cut
    cases["heavyties"] = (p, t, (np.round(u * 50) / 50).astype(np.float32))
    return cases


def run_reference(ref, p, t, u, with_calibration):
    """The four sections of the reference, each on its own (a section that raises is left out and reported)."""
    an = ref.UncertaintyAnalyzer()
    err = np.abs(p - t)
    calls = {"uncertainty_error_correlation": lambda: an._compute_uncertainty_error_correlation(u, err),
             "sparsification_analysis": lambda: an._compute_sparsification_analysis(u, err),
             "uncertainty_distribution": lambda: an._analyze_uncertainty_distribution(u)}
    if with_calibration:
        calls["calibration_analysis"] = lambda: an.calibration_analyzer.analyze_calibration(p, t, u)
    out, raised = {}, []
    logging.disable(logging.CRITICAL)
    try:
        with warnings.catch_warnings(), contextlib.redirect_stderr(io.StringIO()), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            for name, call in calls.items():
                try:
                    out[name] = call()
                except Exception as e:  # noqa: BLE001
                    raised.append(f"{name}: {type(e).__name__}")
    finally:
        logging.disable(logging.NOTSET)
    return out, raised


def distance(a, b, relative=False):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)), (a, b)
    ok = ~np.isnan(b)
    if relative:
        ok &= np.abs(b) >= P_FLOOR
        return float(np.max(np.abs(a[ok] - b[ok]) / np.abs(b[ok]))) if ok.any() else 0.0
    return float(np.max(np.abs(a[ok] - b[ok]))) if ok.any() else 0.0


def section_distance(got, want):
    """(absolute distance over the values, relative distance over the p-values) of two flattened sections with equal keys."""
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    d_abs = max([distance(got[k], want[k]) for k in want if not k.endswith("_p_value")] + [0.0])
    d_rel = max([distance(got[k], want[k], relative=True) for k in want if k.endswith("_p_value")] + [0.0])
    scale = max([float(np.nanmax(np.abs(want[k]))) for k in want if not k.endswith("_p_value") and not np.isnan(want[k]).all()] + [1.0])
    return d_abs, d_rel, scale


def capture():
    ref = GE.reference_module()
    Z = np.load(os.path.join(HERE, "eval_cases.npz"))
    cases = {name: (Z[f"{name}.pred"], Z[f"{name}.target"], Z[f"{name}.unc"]) for name in REUSED}
    own = own_cases()
    cases.update(own)
    out = {}
    for name, (p, t, u) in own.items():
        out[f"{name}.pred"], out[f"{name}.target"], out[f"{name}.unc"] = p, t, u
    dist = {k: 0.0 for k in ("correlation", "correlation_p", "sparsification", "distribution", "calibration")}
    restatement_only, ref_raised, nan_curves, stored = [], {}, set(), {}
    for name, (p32, t32, u32) in cases.items():
        assert p32.dtype == t32.dtype == u32.dtype == np.float32
        if name in DISTINCT:
            assert all(len(np.unique(u32[:, d])) == len(u32) for d in range(3)), name
        own_res = {sec: U.flatten(v) for sec, v in U.analyze(p32, t32, u32).items()}
        own_res64 = {sec: U.flatten(v) for sec, v in U.analyze(p32, t32, u32, errors64=True).items()}    # |p - t| as float64 copies give it
        for variant in ("f64", "f32"):            # f64 first: it decides whether the order agrees
            arrays = (p32, t32, u32) if variant == "f32" else tuple(x.astype(np.float64) for x in (p32, t32, u32))
            res, raised = run_reference(ref, *arrays, with_calibration=variant == "f32")
            if raised:
                ref_raised[f"{name}.{variant}"] = raised
            for sec, val in res.items():
                flat = U.flatten(val)
                short = SECTIONS[sec]
                order_free = short != "sparsification"
                if variant == "f64":
                    d_abs, d_rel, scale = section_distance(own_res64[sec], flat)
                    agrees = d_abs <= 1e-12 * scale and d_rel <= 1e-9
                    assert agrees or not order_free, (name, sec, d_abs, d_rel)
                    if not agrees:
                        assert name not in DISTINCT, (name, d_abs)
                        restatement_only.append(name)
                        continue
                else:
                    if not order_free and name in restatement_only:
                        continue
                    if short == "calibration":
                        # A NaN uncertainty makes every confidence NaN.  This sklearn's calibration_curve does not raise on
                        # that: the reference returns one bin whose mean is NaN.  The product treats a non-finite uncertainty
                        # like the cases that do raise (no curve key, ECE 0.0 -- the ECE is 0.0 in the reference too), so
                        # such a curve is not stored.
                        for k in [k for k in flat if k not in own_res[sec]]:
                            assert k.split(".")[0].endswith("_calibration_curve") and (k.endswith("fraction_of_positives") or
                                                                                       np.isnan(flat[k]).all()), (name, k, flat[k])
                            nan_curves.add(f"{name}.{k.split('_')[0]}")
                            del flat[k]
                    d_abs, d_rel, _ = section_distance(own_res[sec], flat)
                    dist[short] = max(dist[short], d_abs)
                    if short == "correlation":
                        dist["correlation_p"] = max(dist["correlation_p"], d_rel)
                for k, v in flat.items():
                    stored.setdefault(f"{name}.{variant}", {})[f"{sec}.{k}"] = v
    assert len([c for c in DISTINCT if c not in restatement_only]) == 5
    layout = {}
    for tag, flat in stored.items():          # one array per (case, variant): hundreds of tiny entries cost more than their data
        layout[tag] = [[k, int(v.size)] for k, v in flat.items()]
        out[tag] = np.concatenate(list(flat.values()))
    meta = {"cases": list(cases), "layout": layout, "own_inputs": list(own), "reused_inputs": list(REUSED), "restatement_only": sorted(set(restatement_only)),
            "ref_raised": ref_raised, "nan_curves_not_stored": sorted(nan_curves), "ref_vs_f64": dist}
    out["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    return out, meta


if __name__ == "__main__":
    data, meta = capture()
    path = os.path.join(HERE, "uncertainty_cases.npz")
    np.savez_compressed(path, **data)
    print(json.dumps({k: meta[k] for k in ("restatement_only", "ref_raised", "nan_curves_not_stored", "ref_vs_f64")}, indent=1))
    print("wrote", path, os.path.getsize(path), "bytes")
