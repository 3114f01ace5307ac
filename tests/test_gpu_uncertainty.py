"""UncertaintyAnalyzer on the GPU (mmdeer_uncertainty_table in csrc/evalstats.hip, mmdeer/evaluation.py): the raw table
against the float64 restatement (tests/uncertainty_ref.py) at the sizes where the launches change shape, bit-identical
relaunches, the public classes against the reference's results in tests/golden/uncertainty_cases.npz, fewer than three
dimensions, the refusals, and evaluate_model -> analyze_uncertainty_quality end to end on Stack B.

Tolerances.  Sums of non-negative fp64 terms in another order (sum u, sum e, the centred squares, the prefix sums of e):
rtol 1e-10 -- N eps = 1.2e-10 is the worst case at N = 2**20 and the pairwise trees stay far below it; the bound
test_gpu_evaluation.py uses for its sums.  The centred cross sum has terms of both signs: 1e-10 of sqrt(Suu See), its
Cauchy-Schwarz bound.  Minima, maxima, flags and order statistics: exact (the lerp is restated operation for operation).
Public results against the restatement: 1e-9 (one division or square root after those sums); against the capture on float32
arrays max(4 x meta.ref_vs_f64.<section>, 1e-9 relative), the distance make_golden_uncertainty.py measured between the
reference and the restatement -- the reference's own float32 rounding, not a property of the code under test."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mmdeer import evaluation as M, synth  # noqa: E402

from . import uncertainty_ref as U  # noqa: E402
from .test_cpu_evaluation import close, close_p  # noqa: E402
from .test_cpu_uncertainty import CASES, META, Z, expected_keys, inputs, near_capture32  # noqa: E402

DEV = "cuda:0"
EXACT = ("_min", "_max", "_median", "_percentile_95")


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def tied_case(n, d, stream):
    """Errors that are all different and uncertainties that are not: column 0 takes 8 values (runs of equal uncertainties
    straddle every cut point, so an order that is not the stable one changes every prefix sum), column 1 is distinct with
    NaN uncertainties at low row numbers (they must sort last), column 2 takes 5 values, among them -0.0 and +0.0 (one
    image).  A NaN prediction in the last column sits in the last quarter of its order: prefixes up to there are finite."""
    p = (0.3 + synth.normal(stream, n * d).reshape(n, d)).astype(np.float32)
    t = (0.8 * p + 0.5 * synth.normal(stream + 1, n * d).reshape(n, d) - 0.1).astype(np.float32)
    w = synth.uniform01(stream + 2, n * d).reshape(n, d)
    u = np.empty((n, d), dtype=np.float32)
    for c in range(d):
        kind = c % 3
        if kind == 0:
            u[:, c] = np.floor(w[:, c] * 8) / 8 + 0.125
        elif kind == 1:
            u[:, c] = 0.02 + w[:, c]
            if n >= 9:
                u[1, c] = u[n // 3, c] = np.nan
        else:
            u[:, c] = np.floor(w[:, c] * 5) / 4 - 0.25
            u[u[:, c] == 0.0, c] = np.where(np.arange((u[:, c] == 0.0).sum()) % 2 == 0, -0.0, 0.0)
    if n >= 9:
        order = np.argsort(u[:, d - 1], kind="stable")
        p[order[(3 * n) // 4], d - 1] = np.nan
    return p, t, u


def check_table(got, want):
    assert got.shape == want.shape
    assert np.array_equal(got[:, 0], want[:, 0]) and np.array_equal(got[:, 12], want[:, 12])
    assert np.array_equal(got[:, 13:16], np.zeros_like(got[:, 13:16]))
    assert np.array_equal(got[:, 8:12], want[:, 8:12], equal_nan=True)                  # min / max of u and e: exactly, NaN propagated
    exact = np.isnan(want[:, 32:]) & np.isnan(got[:, 32:]) | (got[:, 32:] == want[:, 32:])
    print("order statistics that differ:", [(float(g).hex(), float(w).hex()) for g, w in zip(got[:, 32:][~exact], want[:, 32:][~exact])])
    assert exact.all()                                                                  # order statistics: exactly
    for col in (1, 2, 3, 4, 6, 7):
        np.testing.assert_allclose(got[:, col], want[:, col], rtol=1e-10, atol=0.0, err_msg=f"column {col}")
    with np.errstate(invalid="ignore"):
        bound = 1e-10 * np.sqrt(want[:, 3] * want[:, 4])
    assert np.array_equal(np.isnan(got[:, 5]), np.isnan(want[:, 5]))
    ok = ~np.isnan(want[:, 5])
    assert (np.abs(got[ok, 5] - want[ok, 5]) <= bound[ok]).all(), (got[:, 5], want[:, 5])
    print("prefix max rel err", np.nanmax(np.abs(got[:, 16:32] - want[:, 16:32]) / np.maximum(np.abs(want[:, 16:32]), 1e-300)))
    np.testing.assert_allclose(got[:, 16:32], want[:, 16:32], rtol=1e-10, atol=0.0)     # NaN must match NaN


# ---- 1. the raw table ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d", [(2, 1), (9, 3), (10, 2), (11, 3), (255, 1), (256, 2), (257, 3), (2049, 3), (100003, 2), (1 << 20, 3)])
def test_table_against_the_restatement(n, d):
    p, t, u = tied_case(n, d, 700 + n % 89)
    keep = U.cuts(n)
    got = M.uncertainty_table(dev(p), dev(t), dev(u), keep)
    want = U.table(p, t, u, keep)
    check_table(got, want)
    if n >= 9:
        assert np.isnan(got[d - 1, 16 + 9]) and not np.isnan(got[d - 1, 16 + 5])        # the NaN error enters after 3/4 of the order
        if d >= 2:                                                                      # NaN uncertainties: no order statistics
            assert np.isnan(got[1, 8:10]).all() and np.isnan(got[1, 32:34]).all() and int(got[1, 12]) & 1
        if d == 3:                                                                      # ... but they sort last: finite prefixes
            assert got[1, 12] == 1 and not np.isnan(got[1, 16:26]).any()
    # the stable order matters here: the same sum over an order that breaks ties the other way round differs
    if n >= 255:
        rev = np.arange(n)[::-1]
        other = rev[np.argsort(u[rev, 0], kind="stable")]
        e = U.errors32(p, t)[:, 0].astype(np.float64)
        assert abs(e[other][:keep[2]].sum() - want[0, 16 + 2]) > 1e-6 * want[0, 16 + 2]


def test_table_with_sixteen_cuts_and_eight_levels():
    n, d = 5000, 3
    p, t, u = tied_case(n, d, 733)
    keep = [0, 0, 1, 2, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097, 4999, 5000, 5000]       # chunk and tree edges, repeats, 0 and N
    levels = [0.0, 1.0, 0.5, 0.95, 0.25, 1.0 / 3.0, 0.9999, 1e-9]
    got = M.uncertainty_table(dev(p), dev(t), dev(u), keep, levels)
    want = U.table(p, t, u, keep, levels)
    check_table(got, want)
    assert (got[:, 16] == 0.0).all() and (got[:, 17] == 0.0).all()
    assert np.array_equal(got[[0, 2], 32], want[[0, 2], 8]) and np.array_equal(got[[0, 2], 33], want[[0, 2], 9])     # levels 0 and 1: min and max
    none = M.uncertainty_table(dev(p), dev(t), dev(u), [], [])
    assert np.array_equal(none[:, :13], got[:, :13], equal_nan=True) and (none[:, 13:] == 0).all()


def test_two_calls_give_bit_identical_tables():
    p, t, u = tied_case(100003, 3, 741)
    P, T, Uu = dev(p), dev(t), dev(u)
    keep = U.cuts(len(p))
    a, b = M.uncertainty_table(P, T, Uu, keep), M.uncertainty_table(P, T, Uu, keep)
    assert a.tobytes() == b.tobytes()
    an = M.UncertaintyAnalyzer()
    assert repr(an.analyze_uncertainty_quality(P, T, Uu)) == repr(an.analyze_uncertainty_quality(P, T, Uu))


# ---- 2. the public classes against the fixture --------------------------------------------------------------------------------
def check_against_restatement(got, own):
    """A flattened public result against the flattened restatement: same keys in the same order, same lengths, NaN where it
    has NaN, values as the module docstring says."""
    assert list(got) == list(own)
    for key, want in own.items():
        g = got[key]
        assert g.shape == want.shape and np.array_equal(np.isnan(g), np.isnan(want)), (key, g, want)
        if key.endswith("_p_value"):
            # d ln p / d r is about n r / (1 - r^2) <= 5000 * 0.95 / 0.1 = 5e4, times the 1e-9 the correlations may differ by
            close_p(g, want, 5e-5)
        elif key.endswith(EXACT) or key.endswith("fractions"):
            assert np.array_equal(g, want, equal_nan=True), (key, g, want)
        elif key.endswith("_correlation"):
            close(g, want, 0.0, 1e-9)
        else:
            close(g, want, 1e-9, 1e-300)


def plain_types(res):
    for v in res.values():
        if isinstance(v, dict):
            plain_types(v)
        elif isinstance(v, list):
            assert all(type(x) is float for x in v)
        else:
            assert type(v) is float, (type(v), v)


@pytest.mark.parametrize("case", CASES)
def test_analyzer_against_the_reference_and_the_restatement(case):
    p, t, u = inputs(case)
    P, T, Uu = dev(p), dev(t), dev(u)
    res = M.UncertaintyAnalyzer().analyze_uncertainty_quality(P, T, Uu)
    assert list(res) == ["uncertainty_error_correlation", "calibration_analysis", "sparsification_analysis", "uncertainty_distribution"]
    plain_types(res)
    for dim in U.DIMS:
        curve = res["sparsification_analysis"][f"{dim}_sparsification_curve"]
        assert len(curve["fractions"]) == len(curve["errors"]) == 10 and curve["fractions"] == np.linspace(0.1, 1.0, 10).tolist()
    got = U.flatten(res)
    check_against_restatement(got, U.flatten(U.analyze(p, t, u)))
    ref = U.unpack(Z, META, f"{case}.f32")
    assert set(ref) == expected_keys(got, case, "f32")                 # an absent curve key is absent here too
    for key, want in ref.items():
        near_capture32(got[key], want, key)
    print(case, {k: v for k, v in res["uncertainty_error_correlation"].items()}, res["sparsification_analysis"]["valence_ause"])
    # analyze_calibration on its own, and the private methods on device errors, return the same sections
    cal = M.CalibrationAnalyzer().analyze_calibration(P, T, Uu)
    assert repr(cal) == repr(res["calibration_analysis"])
    an = M.UncertaintyAnalyzer()
    E = (P - T).abs()
    assert repr(an._compute_sparsification_analysis(Uu, E)) == repr(res["sparsification_analysis"])
    assert repr(an._compute_uncertainty_error_correlation(Uu, E)) == repr(res["uncertainty_error_correlation"])
    assert repr(an._analyze_uncertainty_distribution(Uu)) == repr(res["uncertainty_distribution"])


def test_analyze_calibration_with_other_bin_counts_and_a_refused_one():
    p, t, u = inputs("plain")
    P, T, Uu = dev(p), dev(t), dev(u)
    for nb in (1, 7, 32):
        got = U.flatten(M.CalibrationAnalyzer().analyze_calibration(P, T, Uu, n_bins=nb))
        own = U.flatten(U.calibration(p, t, u, nb))
        check_against_restatement(got, own)
        assert len(got["valence_calibration_curve.mean_predicted_value"]) <= nb
    with pytest.raises(RuntimeError, match="n_bins <= 32"):
        M.CalibrationAnalyzer().analyze_calibration(P, T, Uu, n_bins=33)


# ---- 3. fewer dimensions, refusals ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 2])
def test_fewer_than_three_dimensions(d):
    p, t, u = tied_case(999, 3, 760)
    p, t, u = (np.ascontiguousarray(x[:, :d]) for x in (p, t, u))
    res = M.UncertaintyAnalyzer().analyze_uncertainty_quality(dev(p), dev(t), dev(u))
    dims = U.DIMS[:d]
    assert list(res["uncertainty_error_correlation"]) == [f"{x}_{k}" for x in dims for k in ("correlation", "p_value")] + ["average_correlation"]
    assert list(res["uncertainty_distribution"]) == [f"{x}_{k}" for x in dims for k in ("mean", "std", "min", "max", "median", "percentile_95")]
    assert [k for k in res["sparsification_analysis"] if k.endswith("_ause")] == [f"{x}_ause" for x in dims]
    assert [k for k in res["calibration_analysis"] if k.endswith("_ece")] == [f"{x}_ece" for x in dims]
    check_against_restatement(U.flatten(res), U.flatten(U.analyze(p, t, u)))
    if d == 1:                                                          # 1-D tensors are one dimension
        flat = M.UncertaintyAnalyzer().analyze_uncertainty_quality(dev(p[:, 0]), dev(t[:, 0]), dev(u[:, 0]))
        assert repr(flat) == repr(res)


def test_refused_calls_raise_with_a_message():
    from .test_cpu_uncertainty import test_analyzers_refuse_cpu_tensors_and_arrays, test_entry_point_refuses_bad_arguments_before_any_launch
    test_entry_point_refuses_bad_arguments_before_any_launch()
    test_analyzers_refuse_cpu_tensors_and_arrays()
    an = M.UncertaintyAnalyzer()
    one = torch.zeros(1, 3, device=DEV)
    with pytest.raises(RuntimeError, match="N >= 2"):
        an.analyze_uncertainty_quality(one, one, one)
    big = torch.zeros((1 << 20) + 1, 1, device=DEV)
    with pytest.raises(RuntimeError, match="limit"):
        an.analyze_uncertainty_quality(big, big, big)
    g = torch.zeros(8, 3, device=DEV)
    with pytest.raises(ValueError):
        an.analyze_uncertainty_quality(g, g, g[:, :2])
    with pytest.raises(ValueError):
        an.analyze_uncertainty_quality(g[:0], g[:0], g[:0])
    with pytest.raises(ValueError):
        an.analyze_uncertainty_quality(torch.zeros(8, 4, device=DEV), torch.zeros(8, 4, device=DEV), torch.zeros(8, 4, device=DEV))
    with pytest.raises(RuntimeError, match="ascending"):
        M.uncertainty_table(g, g, g, [4, 2])
    with pytest.raises(RuntimeError, match="n_q <= 8"):
        M.uncertainty_table(g, g, g, [4], [0.5] * 9)
    torch.cuda.synchronize()
    # constant columns: a correlation of NaN, everything else defined
    res = an.analyze_uncertainty_quality(g, g, g + 0.5)
    assert math.isnan(res["uncertainty_error_correlation"]["valence_correlation"]) and math.isnan(res["uncertainty_error_correlation"]["valence_p_value"])
    assert res["uncertainty_distribution"]["valence_std"] == 0.0 and res["sparsification_analysis"]["valence_ause"] == 0.0


# ---- 4. end to end ------------------------------------------------------------------------------------------------------------
def test_evaluate_model_then_uncertainty_analysis_on_stack_b():
    from mmdeer import stackb

    from .test_gpu_evaluation import loader
    torch.manual_seed(7)
    model = stackb.CompleteDEERModel(compute_dtype="fp32").to(DEV)
    n = 96
    ev = M.DEERModelEvaluator(n_bootstrap=20)
    assert isinstance(ev.uncertainty_analyzer, M.UncertaintyAnalyzer)
    results, P, T, Uu = ev.evaluate_model(model, loader(n, 32, 23, True), torch.device(DEV), return_predictions=True)
    assert isinstance(results, M.EvaluationResults) and results.sample_size == n
    assert all(x.is_cuda and x.shape == (n, 3) for x in (P, T, Uu))
    res = ev.uncertainty_analyzer.analyze_uncertainty_quality(P, T, Uu)
    plain_types(res)
    p, t, u = (x.cpu().numpy() for x in (P, T, Uu))
    check_against_restatement(U.flatten(res), U.flatten(U.analyze(p, t, u)))
    assert res["calibration_analysis"]["valence_ece"] == results.ece_valence
