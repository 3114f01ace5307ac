"""The evaluator without a GPU: the float64 restatement (tests/eval_ref.py) against the reference's results captured in
tests/golden/eval_cases.npz, the module's Student-t / Beta p-values against the stored scipy values, the bootstrap index
recipe, the host logic of compute_ece's zip, the compat re-exports and every refusal decided on the host."""
import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from mmdeer import _lib, evaluation as M, synth

from . import eval_ref as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z = np.load(os.path.join(ROOT, "tests", "golden", "eval_cases.npz"))
META = json.loads(bytes(Z["meta"]).decode())
CASES = META["cases"]
R, SEED, DIST = META["R"], META["seed"], META["ref_vs_f64"]
SIG = META["sig_keys"]
P_FLOOR = 1e-290


def same_nan(a, b):
    return np.array_equal(np.isnan(np.asarray(a, dtype=np.float64)), np.isnan(np.asarray(b, dtype=np.float64)))


def close(a, b, rtol, atol=0.0):
    """|a - b| <= atol + rtol |b| elementwise, NaN matching NaN."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert same_nan(a, b), (a, b)
    ok = ~np.isnan(b)
    err = np.abs(a[ok] - b[ok])
    bound = atol + rtol * np.abs(b[ok])
    assert (err <= bound).all(), (a, b, err.max())


def close_p(a, b, rtol):
    """p-values: relative where the stored value is >= 1e-290, both below 1e-290 otherwise."""
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    assert same_nan(a, b), (a, b)
    for x, y in zip(a, b):
        if math.isnan(y):
            continue
        if y >= P_FLOOR:
            assert abs(x - y) <= rtol * y, (x, y)
        else:
            assert x < P_FLOOR, (x, y)


def test_fixture_holds_every_case_the_evaluator_is_specified_on():
    assert {"plain", "even", "ties", "nan", "constpred", "n3"} <= set(CASES)
    assert len(Z["plain.pred"]) % 2 == 1 and len(Z["even.pred"]) % 2 == 0 and len(Z["n3.pred"]) == 3
    assert all(len(Z[f"{c}.pred"]) <= 5000 for c in CASES)
    assert np.isnan(Z["nan.pred"]).any() and np.isnan(Z["nan.target"]).any()
    counts = {c: Z[f"{c}.bin_counts"] for c in CASES}
    assert (counts["plain"] > 0).all()                                    # a set that fills all 15 bins
    assert (counts["even"][:, 1] == 0).any(axis=1).all()                  # at least one empty bin: the misaligned zip
    assert (Z["ties.unc"] < 0).sum() == 1 and Z["ties.ece"][1] == 0.0       # one negative uncertainty -> 0.0
    assert np.isnan(Z["constpred.f64.sig"][1]).all() and (Z["constpred.f64.ci.ccc.0.95"][1] == 0).all()


@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_the_reference_intervals_on_float64_inputs(case):
    p, t = Z[f"{case}.pred"], Z[f"{case}.target"]
    mom, flags = E.bootstrap_moments(p, t, R, SEED)
    for mi, metric in enumerate(META["metrics"]):
        for level in META["levels"]:
            ci, _ = E.confidence_intervals(mom, flags, len(p), mi, level)
            close(ci, Z[f"{case}.f64.ci.{metric}.{level}"], 1e-9)


@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_the_reference_correlations_on_float64_inputs(case):
    p, t = Z[f"{case}.pred"], Z[f"{case}.target"]
    sig = Z[f"{case}.f64.sig"]
    c = E.correlations(p, t)
    close(c[:, 0], sig[:, SIG.index("pearson_correlation")], 1e-9)
    close(c[:, 1], sig[:, SIG.index("spearman_correlation")], 1e-9)
    close(c[:, 2], sig[:, SIG.index("t_test_statistic")], 1e-9)
    a = E.agreement(p, t)
    close(a[:, 0], Z[f"{case}.f64.ccc"], 1e-9)
    if not np.isnan(Z[f"{case}.f64.mae"]).all():
        close(a[:, 1], Z[f"{case}.f64.mae"], 1e-9)
        close(a[:, 2], Z[f"{case}.f64.rmse"], 1e-9)


@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_the_reference_bins_and_ece(case):
    p, t, u = Z[f"{case}.pred"], Z[f"{case}.target"], Z[f"{case}.unc"]
    for d in range(3):
        stats, bins = E.calibration_bins(p[:, d], t[:, d], u[:, d], META["n_bins"])
        if not stats[2]:
            assert np.array_equal(bins[:, :, 0].astype(np.int64), Z[f"{case}.bin_counts"][d])     # populations: exactly
        ref = Z[f"{case}.ece"][d]
        got = E.ece(p[:, d], t[:, d], u[:, d], META["n_bins"])
        print(case, d, got, ref)
        assert abs(got - ref) <= max(4 * DIST["ece"], 1e-9 * abs(ref))


@pytest.mark.parametrize("case", CASES)
def test_student_t_and_beta_functions_against_the_stored_scipy_p_values(case):
    """The p-values the module derives from the reference's own statistic (float64 capture) against the reference's."""
    sig = Z[f"{case}.f64.sig"]
    n = len(Z[f"{case}.pred"])
    for d in range(3):
        r, pr, rs, ps, ts, pt = sig[d]
        close_p([M.pearson_p_value(r, n)], [pr], 1e-9)
        close_p([M.spearman_p_value(rs, n)], [ps], 1e-9)
        t_stat, t_p = M.t_test(r, n)
        close([t_stat], [ts], 1e-12)
        close([t_p], [pt], 0.0, 1e-12)


def test_student_t_function_at_known_values():
    assert M.student_t_sf(0.0, 7) == pytest.approx(0.5, abs=1e-15)
    assert M.student_t_sf(1.0, 1) == pytest.approx(0.25, rel=1e-13)              # Cauchy: 1/2 - atan(1)/pi
    assert M.student_t_sf(12.706204736174694, 1) == pytest.approx(0.025, rel=1e-12)
    assert M.student_t_sf(2.0, 2) == pytest.approx(0.5 - 1.0 / math.sqrt(6.0), rel=1e-13)   # df = 2: 1/2 - t / (2 sqrt(2 + t^2))
    assert M.student_t_cdf(-2.0, 2) == pytest.approx(0.5 - 1.0 / math.sqrt(6.0), rel=1e-13)
    assert M.student_t_sf(float("inf"), 5) == 0.0 and math.isnan(M.student_t_sf(float("nan"), 5))
    assert M.betainc(2.0, 3.0, 0.25) == pytest.approx(0.26171875, rel=1e-13)     # closed form of I_x(2, 3)
    assert M.pearson_p_value(0.3, 2) == 1.0 and math.isnan(M.pearson_p_value(float("nan"), 10))


def test_bootstrap_index_recipe_range_determinism_and_frequencies():
    for n in (1, 2, 3, 7, 1000, 100003):
        idx = synth.bootstrap_indices(SEED, 5, n)
        assert idx.dtype == np.int64 and idx.shape == (n,) and idx.min() >= 0 and idx.max() < n
    a, b = synth.bootstrap_indices(3, 11, 5000), synth.bootstrap_indices(3, 11, 5000)
    assert np.array_equal(a, b)
    assert not np.array_equal(a, synth.bootstrap_indices(3, 12, 5000))
    assert not np.array_equal(a, synth.bootstrap_indices(4, 11, 5000))
    assert len(np.unique(a)) > 3000            # about 1 - 1/e of the rows appear in a replicate
    with pytest.raises(ValueError):
        synth.bootstrap_indices(0, 0, 0)
    # 70,000 draws at n = 7 (10,000 replicates of 7): each count within 5 sigma of 10,000, sigma = sqrt(70000 * 1/7 * 6/7) = 92.6
    draws = np.concatenate([synth.bootstrap_indices(0, r, 7) for r in range(10000)])
    assert draws.size == 70000
    counts = np.bincount(draws, minlength=7)
    print("counts at n = 7:", counts, "worst", np.abs(counts - 10000).max())
    assert np.abs(counts - 10000).max() <= 463
    # the same bound inside one replicate: 70,000 draws at n = 70,000 folded into 7 equal classes of rows
    one = synth.bootstrap_indices(1, 0, 70000) // 10000
    assert np.abs(np.bincount(one, minlength=7) - 10000).max() <= 463


def test_ece_zip_on_hand_made_bin_tables():
    """ece_from_bins: weights of the [lo, hi) rule zipped with the NON-EMPTY bins of the (lo, hi] rule."""
    def table(counts, conf_mean, acc_mean):
        c = np.asarray(counts, dtype=np.float64)
        return np.stack([c, c * np.asarray(conf_mean), c * np.asarray(acc_mean)], axis=1)

    # all full, both rules agree: the textbook ECE
    cnt, cm, am = [2, 3, 5], [0.1, 0.5, 0.9], [0.5, 1.0, 0.6]
    t = table(cnt, cm, am)
    want = sum(c / 10 * abs(a - m) for c, m, a in zip(cnt, cm, am))
    assert M.ece_from_bins(t, t, 10) == pytest.approx(want, rel=1e-15)
    # empty first bin: weight 0 is skipped, but it still consumes the first non-empty curve entry -> misaligned, tail cut
    t = table([0, 4, 6], [0.0, 0.5, 0.9], [0.0, 1.0, 0.5])
    want = 0.4 * abs(0.5 - 0.9)                       # weight of bin 1 against the curve entry of bin 2; the weight of bin 2 is cut
    assert M.ece_from_bins(t, t, 10) == pytest.approx(want, rel=1e-15)
    # empty middle bin: bin 0 aligned, bin 1 (weight 0) eats bin 2's entry
    t = table([5, 0, 5], [0.2, 0.0, 0.8], [0.4, 0.0, 1.0])
    assert M.ece_from_bins(t, t, 10) == pytest.approx(0.5 * abs(0.4 - 0.2), rel=1e-15)
    # the two rules may differ in population (a confidence on an edge): weights from the first, curve from the second
    w = table([3, 7], [0.25, 0.75], [1.0, 1.0])
    c = table([4, 6], [0.3, 0.8], [0.5, 1.0])
    assert M.ece_from_bins(w, c, 10) == pytest.approx(0.3 * abs(0.5 - 0.3) + 0.7 * abs(1.0 - 0.8), rel=1e-15)
    # nothing at all
    assert M.ece_from_bins(np.zeros((3, 3)), np.zeros((3, 3)), 10) == 0.0


def test_results_container_matches_the_reference_layout():
    r = M.EvaluationResults(*[0.1 * i for i in range(16)], {"valence": {"pearson_correlation": 0.5}}, {"valence": (0.1, 0.2)}, 7, 0.5, 11)
    d = r.to_dict()
    assert list(d) == ["performance", "detailed_metrics", "statistical_validation", "meta"]
    assert list(d["performance"]) == ["ccc_valence", "ccc_arousal", "ccc_dominance", "ccc_average", "mae_average", "rmse_average",
                                      "ece_average"]
    assert d["meta"] == {"sample_size": 7, "evaluation_time": 0.5, "model_parameters": 11}
    assert d["detailed_metrics"]["rmse"]["arousal"] == r.rmse_arousal
    json.dumps(d)


def test_compat_evaluation_exports_the_evaluator_classes():
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "from evaluation import DEERModelEvaluator, StatisticalValidator, CalibrationAnalyzer, EvaluationResults, evaluate_deer_model\n"
            "import mmdeer.evaluation as E, mmdeer.trainer as T\n"
            "assert DEERModelEvaluator is E.DEERModelEvaluator and StatisticalValidator is E.StatisticalValidator\n"
            "assert evaluate_deer_model is T.evaluate_deer_model\n"
            "print('ok')\n") % (ROOT, os.path.join(ROOT, "compat"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-2000:]


def test_public_classes_refuse_cpu_tensors_and_arrays():
    p = torch.zeros(8, 3)
    for call in (lambda: M.StatisticalValidator().compute_confidence_intervals(p, p),
                 lambda: M.StatisticalValidator().run_significance_tests(p, p),
                 lambda: M.StatisticalValidator().compute_confidence_intervals(p.numpy(), p.numpy()),
                 lambda: M.CalibrationAnalyzer().compute_ece(p[:, 0], p[:, 0], p[:, 0]),
                 lambda: M.DEERModelEvaluator().compute_scores(p, p, p)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """No GPU is touched: every case is refused by the host checks (A is a plausible address, never dereferenced)."""
    lib = _lib.load()
    A = 1 << 20
    err = lambda: lib.mmdeer_last_error().decode()  # noqa: E731
    moments = lambda **k: lib.mmdeer_bootstrap_moments(*[{**dict(pred=A, target=A, N=100, D=3, R=10, seed=0, mom=A, flags=A, scratch=A,  # noqa: E731
                                                                 nbytes=1 << 30, stream=None), **k}[n]
                                                         for n in ("pred", "target", "N", "D", "R", "seed", "mom", "flags", "scratch", "nbytes", "stream")])
    assert moments(pred=None) != 0 and "NULL" in err()
    assert moments(scratch=None) != 0 and "NULL" in err()
    assert moments(N=0) != 0 and "N" in err()
    assert moments(D=4) != 0 and "D <= 3" in err()
    assert moments(D=0) != 0
    assert moments(R=4097) != 0 and "R <= 4096" in err()
    assert moments(R=0) != 0
    assert moments(nbytes=64) != 0 and "scratch" in err()
    assert moments(scratch=A + 4) != 0 and "aligned" in err()
    assert lib.mmdeer_bootstrap_scratch(100, 10) == 100 * 32 + 10 * (18 * 8 + 12 * 4) and lib.mmdeer_bootstrap_scratch(0, 10) == 0
    ci = lambda **k: lib.mmdeer_bootstrap_ci(*[{**dict(mom=A, flags=A, N=100, D=3, R=10, metric=0, lo=0.025, hi=0.975, ci=A, nk=A, stream=None),  # noqa: E731
                                                **k}[n] for n in ("mom", "flags", "N", "D", "R", "metric", "lo", "hi", "ci", "nk", "stream")])
    assert ci(mom=None) != 0 and "NULL" in err()
    assert ci(N=0) != 0 and ci(D=4) != 0 and ci(R=4097) != 0
    assert ci(metric=2) != 0 and "metric" in err()
    assert ci(hi=1.5) != 0 and "[0, 1]" in err()
    assert lib.mmdeer_sort_pairs(None, 1, 10, A, A, 1 << 20, None) != 0 and "NULL" in err()
    assert lib.mmdeer_sort_pairs(A, 1, 0, A, A, 1 << 20, None) != 0
    assert lib.mmdeer_sort_pairs(A, 1, (1 << 20) + 1, A, A, 1 << 30, None) != 0 and "limit" in err()
    assert lib.mmdeer_sort_pairs(A, 0, 10, A, A, 1 << 20, None) != 0 and "stride" in err()
    assert lib.mmdeer_sort_pairs(A, 1, 10, A, A, 64, None) != 0 and "scratch" in err()
    assert lib.mmdeer_sort_pairs_scratch(10) == 16 * 8 and lib.mmdeer_sort_pairs_scratch(1 << 20) == 8 << 20
    assert lib.mmdeer_sort_pairs_scratch((1 << 20) + 1) == 0
    assert lib.mmdeer_average_ranks(None, 10, A, None) != 0 and lib.mmdeer_average_ranks(A, 0, A, None) != 0
    assert lib.mmdeer_rank_moments(A, None, 10, A, None) != 0 and lib.mmdeer_rank_moments(A, A, 0, A, None) != 0
    cal = lambda **k: lib.mmdeer_calibration_bins(*[{**dict(p=A, t=A, u=A, N=100, D=3, edges=A, nb=15, stats=A, bins=A, scratch=A, stream=None),  # noqa: E731
                                                     **k}[n] for n in ("p", "t", "u", "N", "D", "edges", "nb", "stats", "bins", "scratch", "stream")])
    assert cal(u=None) != 0 and "NULL" in err()
    assert cal(N=0) != 0 and cal(D=4) != 0
    assert cal(nb=33) != 0 and "n_bins <= 32" in err()
    assert cal(nb=0) != 0
    assert lib.mmdeer_calibration_bins_scratch(3) == 48 and lib.mmdeer_calibration_bins_scratch(4) == 0
    assert lib.mmdeer_abi_version() == _lib.ABI_VERSION
