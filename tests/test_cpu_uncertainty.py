"""UncertaintyAnalyzer without a GPU: the float64 restatement (tests/uncertainty_ref.py) against the reference's results
captured in tests/golden/uncertainty_cases.npz, the cut points int(frac * N), the trapezoid rule of the AUSE, every refusal
mmdeer_uncertainty_table decides on the host, the compat re-export and the refusal of CPU tensors."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from mmdeer import _lib, evaluation as M

from . import uncertainty_ref as U
from .test_cpu_evaluation import P_FLOOR, close, close_p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z = np.load(os.path.join(ROOT, "tests", "golden", "uncertainty_cases.npz"))
ZE = np.load(os.path.join(ROOT, "tests", "golden", "eval_cases.npz"))
META = json.loads(bytes(Z["meta"]).decode())
CASES, DIST = META["cases"], META["ref_vs_f64"]
SECTIONS = {"uncertainty_error_correlation": "correlation", "sparsification_analysis": "sparsification",
            "uncertainty_distribution": "distribution", "calibration_analysis": "calibration"}


def inputs(case):
    src = Z if case in META["own_inputs"] else ZE
    return src[f"{case}.pred"], src[f"{case}.target"], src[f"{case}.unc"]


def near_capture32(got, want, key):
    """A flattened result against the reference's capture on float32 arrays: |got - ref| <= max(4 x the distance the
    generator measured between the reference and the restatement, 1e-9 |ref|), NaN matching NaN; p-values relative."""
    section = SECTIONS[key.split(".")[0]]
    if key.endswith("_p_value"):
        for x, y in zip(np.ravel(got), np.ravel(want)):
            if np.isnan(y):
                assert np.isnan(x), key
            elif y >= P_FLOOR:
                assert abs(x - y) <= max(4 * DIST["correlation_p"], 1e-9) * y, (key, x, y)
            else:
                assert x < P_FLOOR, (key, x, y)
        return
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)), (key, got, want)
    ok = ~np.isnan(want)
    assert (np.abs(got[ok] - want[ok]) <= np.maximum(4 * DIST[section], 1e-9 * np.abs(want[ok]))).all(), (key, got, want)


def expected_keys(own, case, variant):
    """The keys the fixture must hold for a case: the restatement's, without the calibration section on float64 copies and
    without the sparsification section of a case whose order the reference does not share."""
    keys = set(own)
    if variant == "f64":
        keys = {k for k in keys if not k.startswith("calibration_analysis")}
    if case in META["restatement_only"]:
        keys = {k for k in keys if not k.startswith("sparsification_analysis")}
    return keys


def test_fixture_holds_every_case_the_analyzer_is_specified_on():
    assert set(CASES) == {"plain", "big", "n3", "nan", "constpred", "even", "ties", "n7", "nanunc", "cancel", "heavyties"}
    assert set(META["own_inputs"]) == {"n7", "nanunc", "cancel", "heavyties"}
    assert not any(f"{c}.pred" in Z.files for c in META["reused_inputs"])           # only results are stored for them
    assert not {"plain", "big", "n3", "nan", "constpred"} & set(META["restatement_only"])
    assert len(Z["n7.pred"]) == 7
    u = Z["nanunc.unc"]
    assert np.isnan(u).sum() == 1 and np.isnan(u[:, 1]).sum() == 1
    u = Z["cancel.unc"]
    assert u.min() >= 1e-3 and u.max() < 1.0011e-3
    u = Z["heavyties.unc"]
    assert all(len(np.unique(u[:, d])) < 60 for d in range(3))
    for case in ("even", "ties"):
        u = ZE[f"{case}.unc"]
        assert sum(len(u) - len(np.unique(u[:, d])) for d in range(3)) >= 1
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "uncertainty_cases.npz")) < 700 * 1024


@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_the_reference_on_float64_inputs(case):
    p, t, u = inputs(case)
    own = U.flatten(U.analyze(p, t, u, errors64=True))
    ref = U.unpack(Z, META, f"{case}.f64")
    assert set(ref) == expected_keys(own, case, "f64")
    for key, want in ref.items():
        if key.endswith("_p_value"):
            close_p(own[key], want, 1e-9)
        else:
            close(own[key], want, 1e-11, 1e-13)


@pytest.mark.parametrize("case", CASES)
def test_restatement_is_within_the_measured_distance_of_the_reference_on_float32_inputs(case):
    p, t, u = inputs(case)
    own = U.flatten(U.analyze(p, t, u))
    ref = U.unpack(Z, META, f"{case}.f32")
    assert set(ref) == expected_keys(own, case, "f32")
    for key, want in ref.items():
        near_capture32(own[key], want, key)


def test_fixture_special_cases_say_what_the_issue_says():
    n7 = U.unpack(Z, META, "n7.f64")
    for dim in U.DIMS:
        assert n7[f"sparsification_analysis.{dim}_sparsification_curve.errors"][0] == 0.0      # n_keep = 0
        assert len(n7[f"sparsification_analysis.{dim}_sparsification_curve.errors"]) == 10
    nu = U.unpack(Z, META, "nanunc.f32")
    for key, v in nu.items():
        sec, name = key.split(".")[:2]
        if sec in ("uncertainty_error_correlation", "uncertainty_distribution"):
            assert np.isnan(v).all() == (name.startswith("arousal") or name == "average_correlation"), key
    assert nu["calibration_analysis.arousal_ece"][0] == 0.0
    assert "calibration_analysis.arousal_calibration_curve.mean_predicted_value" not in nu
    ties = U.unpack(Z, META, "ties.f32")                 # one negative uncertainty in dimension 1: calibration_curve raises
    assert "calibration_analysis.arousal_calibration_curve.mean_predicted_value" not in ties
    assert ties["calibration_analysis.arousal_ece"][0] == 0.0
    assert "calibration_analysis.valence_calibration_curve.mean_predicted_value" in ties


def test_cut_points_are_the_reference_expression_in_python_floats():
    want = {7: [0, 1, 2, 2, 3, 4, 4, 5, 6, 7], 10: [1, 2, 3, 4, 5, 6, 7, 8, 9, 10], 37: [3, 7, 11, 14, 18, 22, 25, 29, 33, 37],
            1001: [100, 200, 300, 400, 500, 600, 700, 800, 900, 1001]}
    for n, keep in want.items():
        assert M.sparsification_cuts(n) == keep == U.cuts(n)
        assert keep == [int(frac * n) for frac in np.linspace(0.1, 1.0, 10)]             # the reference's line, literally
        assert all(type(k) is int for k in M.sparsification_cuts(n))
    assert float(np.linspace(0.1, 1.0, 10)[2]) == 0.30000000000000004
    for n in range(2, 3000):                                                              # ascending and within [0, N]: what the kernel checks
        k = M.sparsification_cuts(n)
        assert k == sorted(k) and k[0] >= 0 and k[-1] == n


def test_ause_is_the_trapezoid_rule_over_the_ten_means():
    f = np.linspace(0.1, 1.0, 10)
    assert M.ause_from_means(f) == pytest.approx((1.0 - 0.01) / 2, rel=1e-14)             # integral of x over [0.1, 1]
    assert M.ause_from_means(np.full(10, 0.25)) == pytest.approx(0.9 * 0.25, rel=1e-14)
    assert M.ause_from_means(f * f) == pytest.approx((1.0 - 0.001) / 3 + 0.9 * 0.1 ** 2 / 6, rel=1e-13)   # + (b - a) h^2 / 12 f''
    e = [0.0, 0.3, 0.1, 0.4, 0.1, 0.5, 0.9, 0.2, 0.6, 0.5]
    assert M.ause_from_means(e) == pytest.approx(0.1 * (sum(e) - 0.5 * (e[0] + e[-1])), rel=1e-13)
    assert np.isnan(M.ause_from_means([0.1] * 4 + [float("nan")] + [0.1] * 5))


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """No GPU is touched: every case is refused by the host checks (A is a plausible address, never dereferenced)."""
    lib = _lib.load()
    A = 1 << 20
    err = lambda: lib.mmdeer_last_error().decode()  # noqa: E731
    names = ("pred", "target", "unc", "N", "D", "keep", "n_cuts", "levels", "n_q", "table", "scratch", "nbytes", "stream")

    def call(keep=(10, 20, 100), levels=(0.5, 0.95), **k):
        base = dict(pred=A, target=A, unc=A, N=100, D=3, n_cuts=len(keep), n_q=len(levels), table=A, scratch=A, nbytes=1 << 30, stream=None)
        base["keep"] = (C.c_longlong * max(len(keep), 1))(*keep)
        base["levels"] = (C.c_double * max(len(levels), 1))(*levels)
        for name, v in k.items():
            base[name.replace("_ptr", "")] = v
        return lib.mmdeer_uncertainty_table(*[base[n] for n in names])

    for name in ("pred", "target", "unc", "table", "scratch", "keep_ptr", "levels_ptr"):
        assert call(**{name: None}) != 0 and "NULL" in err(), name
    assert call(keep_ptr=None, n_cuts=0, levels_ptr=None, n_q=0, scratch=A + 4) != 0 and "aligned" in err()    # unused arrays may be NULL
    assert call(N=1) != 0 and "N >= 2" in err()
    assert call(N=0) != 0 and call(N=-5) != 0
    assert call(N=(1 << 20) + 1) != 0 and "limit" in err()
    assert call(D=0) != 0 and call(D=4) != 0 and "D <= 3" in err()
    assert call(n_cuts=17) != 0 and "n_cuts <= 16" in err()
    assert call(n_cuts=-1) != 0
    assert call(n_q=9) != 0 and "n_q <= 8" in err()
    assert call(n_q=-1) != 0
    assert call(keep=(10, 5, 100)) != 0 and "ascending" in err()
    assert call(keep=(10, 20, 101)) != 0 and "outside [0, N" in err()
    assert call(keep=(-1, 20, 100)) != 0 and "outside [0, N" in err()
    assert call(levels=(0.5, 1.5)) != 0 and "[0, 1]" in err()
    assert call(levels=(-0.1,)) != 0 and call(levels=(float("nan"),)) != 0
    need = lib.mmdeer_uncertainty_table_scratch(100, 3)
    assert call(nbytes=need - 1) != 0 and "scratch" in err() and str(need) in err()
    assert call(scratch=A + 4) != 0 and "aligned" in err()
    # sorted pairs [D][P] | partials [D][S][7 + 3] | segment sums [D][chunks of 2048][16], doubles
    assert need == 3 * 8 * (128 + 10 + 16)
    assert lib.mmdeer_uncertainty_table_scratch(1 << 20, 1) == 8 * ((1 << 20) + 64 * 10 + 512 * 16)
    assert lib.mmdeer_uncertainty_table_scratch(100000, 2) == 2 * 8 * ((1 << 17) + 13 * 10 + 49 * 16)
    for n, d in ((1, 3), ((1 << 20) + 1, 3), (100, 0), (100, 4)):
        assert lib.mmdeer_uncertainty_table_scratch(n, d) == 0


def test_compat_evaluation_exports_the_uncertainty_analyzer():
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "from evaluation import UncertaintyAnalyzer, CalibrationAnalyzer, DEERModelEvaluator\n"
            "import mmdeer.evaluation as E\n"
            "assert UncertaintyAnalyzer is E.UncertaintyAnalyzer\n"
            "ev = DEERModelEvaluator()\n"
            "assert isinstance(ev.uncertainty_analyzer, UncertaintyAnalyzer)\n"
            "assert isinstance(ev.uncertainty_analyzer.calibration_analyzer, CalibrationAnalyzer)\n"
            "assert callable(CalibrationAnalyzer().analyze_calibration)\n"
            "print('ok')\n") % (ROOT, os.path.join(ROOT, "compat"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-2000:]


def test_analyzers_refuse_cpu_tensors_and_arrays():
    p = torch.zeros(8, 3)
    an = M.UncertaintyAnalyzer()
    for call in (lambda: an.analyze_uncertainty_quality(p, p, p),
                 lambda: an.analyze_uncertainty_quality(p.numpy(), p.numpy(), p.numpy()),
                 lambda: an._compute_uncertainty_error_correlation(p, p),
                 lambda: an._compute_sparsification_analysis(p, p),
                 lambda: an._analyze_uncertainty_distribution(p),
                 lambda: M.CalibrationAnalyzer().analyze_calibration(p, p, p)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
