"""The on-device evaluator (csrc/evalstats.hip, mmdeer/evaluation.py) on the GPU: bootstrap moments against the index
restatement (exact where the data are integers), bit-identical relaunches, the public classes against the reference's
results in tests/golden/eval_cases.npz, the stable sort and ranks against numpy exactly, evaluate_model end to end on both
model stacks, and the host checks.

Tolerances.  GPU against tests/eval_ref.py (float64 sums of <= 5000 terms on identical indices, another summation order):
1e-9 relative.  GPU against the reference's capture on float32 arrays: the reference itself sums in float32 there, so the
bound is max(4 x meta.ref_vs_f64.<quantity>, 1e-9 relative) -- the distance make_golden_eval.py measured between the
reference and eval_ref, not a property of the code under test.  Bin populations, orders and ranks: exact."""
import json
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mmdeer import _lib, evaluation as M, synth  # noqa: E402

from . import eval_ref as E  # noqa: E402
from .test_cpu_evaluation import CASES, DIST, META, P_FLOOR, R, SEED, SIG, Z, close, close_p, same_nan  # noqa: E402

DEV = "cuda:0"
DIMS = ("valence", "arousal", "dominance")


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def near_ref32(got, ref, dist):
    """|got - ref| <= max(4 dist, 1e-9 |ref|) elementwise, NaN matching NaN (ref: the reference on float32 arrays)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert same_nan(got, ref), (got, ref)
    ok = ~np.isnan(ref)
    err = np.abs(got[ok] - ref[ok])
    print("  err", err.max() if err.size else 0.0, "bound 4 x", dist)
    assert (err <= np.maximum(4 * dist, 1e-9 * np.abs(ref[ok]))).all(), (got, ref)


def random_case(n, d, stream, nan_rows=0):
    p = (0.3 + synth.normal(stream, n * d).reshape(n, d)).astype(np.float32)
    t = (0.8 * p + 0.5 * synth.normal(stream + 1, n * d).reshape(n, d) - 0.1).astype(np.float32)
    if nan_rows:
        p[:: max(n // nan_rows, 1), 0] = np.nan
        t[1:: max(n // nan_rows, 1), d - 1] = np.nan
    return p, t


# ---- 1. moments ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 255, 8193, 100003])
def test_bootstrap_moments_of_row_numbers_are_the_integer_sums_of_the_indices(n):
    """pred[:, d] = row number: sum p of replicate r is the integer sum of synth's indices, exactly; n exact with NaN rows."""
    reps = 7
    p = np.repeat(np.arange(n, dtype=np.float32)[:, None], 3, axis=1)
    t = np.ones((n, 3), dtype=np.float32)
    t[::5, 1] = np.nan
    mom, _ = M.bootstrap_moments(dev(p), dev(t), reps, seed=SEED)
    mom = mom.cpu().numpy()
    for r in range(reps):
        idx = synth.bootstrap_indices(SEED, r, n)
        assert mom[r, 0, 0] == n and mom[r, 0, 1] == float(idx.sum()) and mom[r, 2, 1] == float(idx.sum())
        keep = idx[idx % 5 != 0]
        assert mom[r, 1, 0] == keep.size and mom[r, 1, 1] == float(keep.sum()) and mom[r, 1, 2] == keep.size


@pytest.mark.parametrize("n,d,nan_rows", [(2, 1, 0), (257, 2, 3), (5000, 3, 0), (20000, 3, 40), (100000, 3, 0)])
def test_bootstrap_moments_and_flags_against_the_restatement(n, d, nan_rows):
    reps = 5
    p, t = random_case(n, d, 300 + d, nan_rows)
    mom, flags = M.bootstrap_moments(dev(p), dev(t), reps, seed=3)
    want, wflags = E.bootstrap_moments(p, t, reps, 3)
    got = mom.cpu().numpy()
    assert np.array_equal(got[:, :, 0], want[:, :, 0])
    print("max rel err", np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300)))
    np.testing.assert_allclose(got, want, rtol=1e-10, atol=0.0)     # fp64, another summation order: N eps = 1e-11 at N = 100,000
    assert np.array_equal(flags.cpu().numpy(), wflags)


def test_constant_flags_come_from_the_drawn_values():
    """N = 3: a resample of a non-constant column is constant by chance in about one replicate in nine."""
    p, t = Z["n3.pred"], Z["n3.target"]
    mom, flags = M.bootstrap_moments(dev(p), dev(t), 400, seed=SEED)
    want_m, want_f = E.bootstrap_moments(p, t, 400, SEED)
    f = flags.cpu().numpy()
    assert np.array_equal(f, want_f)
    assert 20 <= int((f[:, 0] & 1).sum()) <= 80          # 400 / 9 = 44 expected
    both = np.ones((50, 2), dtype=np.float32)
    _, fl = M.bootstrap_moments(dev(both), dev(both), 4, seed=1)
    assert (fl.cpu().numpy() == 7).all()
    _, fl = M.bootstrap_moments(dev(both), dev(both * 2), 4, seed=1)
    assert (fl.cpu().numpy() == 3).all()


# ---- 2. determinism ----------------------------------------------------------------------------------------------------------
def test_two_launches_give_bit_identical_moments_and_intervals():
    p, t = random_case(100000, 3, 320, nan_rows=10)
    P, T = dev(p), dev(t)
    m1, f1 = M.bootstrap_moments(P, T, 300, seed=9)
    c1, k1 = M.bootstrap_ci(m1, f1, len(p), 0, 0.025, 0.975)
    m2, f2 = M.bootstrap_moments(P, T, 300, seed=9)
    c2, k2 = M.bootstrap_ci(m2, f2, len(p), 0, 0.025, 0.975)
    assert torch.equal(m1, m2) and torch.equal(f1, f2) and torch.equal(c1, c2) and torch.equal(k1, k2)
    assert bool(torch.isfinite(c1).all()) and (k1 == 300).all()
    m3, _ = M.bootstrap_moments(P, T, 300, seed=10)
    assert not torch.equal(m1, m3)


# ---- 3. public classes against the fixture -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_confidence_intervals_against_the_reference_and_the_restatement(case):
    p, t = Z[f"{case}.pred"], Z[f"{case}.target"]
    P, T = dev(p), dev(t)
    mom, flags = E.bootstrap_moments(p, t, R, SEED)
    for mi, metric in enumerate(META["metrics"]):
        for level in META["levels"]:
            got = M.StatisticalValidator(level).compute_confidence_intervals(P, T, metric=metric, n_bootstrap=R, seed=SEED)
            assert list(got) == list(DIMS) and all(type(v) is float for iv in got.values() for v in iv)
            g = np.array([got[d] for d in DIMS])
            own, nkept = E.confidence_intervals(mom, flags, len(p), mi, level)
            print(case, metric, level, g.tolist(), "kept", nkept.tolist())
            close(g, own, 1e-9)
            close(g, Z[f"{case}.f64.ci.{metric}.{level}"], 1e-9)
            near_ref32(g, Z[f"{case}.f32.ci.{metric}.{level}"], DIST["ci"])
    other = M.StatisticalValidator(0.95).compute_confidence_intervals(P, T, metric="spearman", n_bootstrap=R, seed=SEED)
    assert other == M.StatisticalValidator(0.95).compute_confidence_intervals(P, T, metric="Pearson", n_bootstrap=R, seed=SEED)


@pytest.mark.parametrize("case", CASES)
def test_significance_tests_against_the_reference(case):
    p, t = Z[f"{case}.pred"], Z[f"{case}.target"]
    got = M.StatisticalValidator().run_significance_tests(dev(p), dev(t))
    assert list(got) == list(DIMS) and all(list(v) == SIG and all(type(x) is float for x in v.values()) for v in got.values())
    g = np.array([[got[d][k] for k in SIG] for d in DIMS])
    f64, f32 = Z[f"{case}.f64.sig"], Z[f"{case}.f32.sig"]
    print(case, g.tolist())
    c = E.correlations(p, t)
    close(g[:, 0], c[:, 0], 1e-9); close(g[:, 2], c[:, 1], 1e-9); close(g[:, 4], c[:, 2], 1e-9)
    close(g[:, 0], f64[:, 0], 1e-9); close(g[:, 2], f64[:, 2], 1e-9); close(g[:, 4], f64[:, 4], 1e-9)
    n = len(p)
    # the p-values of the device statistic against the module's functions on the restated statistic: d ln p / d r is about
    # n r / (1 - r^2) <= 5000 * 0.95 / 0.1 = 5e4 here, times the 1e-9 the statistics may differ by
    for d in range(3):
        close_p([g[d, 1]], [M.pearson_p_value(c[d, 0], n)], 5e-5)
        close_p([g[d, 3]], [M.spearman_p_value(c[d, 1], n)], 5e-5)
    near_ref32(g[:, 0], f32[:, 0], DIST["pearson"])
    near_ref32(g[:, 2], f32[:, 2], DIST["spearman"])
    near_ref32(g[:, 5], f32[:, 5], DIST["t_p"])
    assert same_nan(g, f32)
    for col, key in ((4, "t_stat"), (1, "pearson_p"), (3, "spearman_p")):
        for d in range(3):
            x, y = g[d, col], f32[d, col]
            if math.isnan(y):
                continue
            if col != 4 and y < P_FLOOR:
                assert x < P_FLOOR
            else:
                assert abs(x - y) <= max(4 * DIST[key], 1e-9) * abs(y), (key, x, y)


@pytest.mark.parametrize("case", CASES)
def test_ece_and_bin_populations_against_the_reference(case):
    p, t, u = Z[f"{case}.pred"], Z[f"{case}.target"], Z[f"{case}.unc"]
    P, T, U = dev(p), dev(t), dev(u)
    stats, bins = M.calibration_bins(P, T, U, META["n_bins"])
    ca = M.CalibrationAnalyzer()
    for d in range(3):
        wstats, wbins = E.calibration_bins(p[:, d], t[:, d], u[:, d], META["n_bins"])
        assert stats[d, 2] == wstats[2] and stats[d, 3] == wstats[3]
        assert stats[d, 0] == wstats[0]
        assert stats[d, 1] == wstats[1] or (math.isnan(stats[d, 1]) and math.isnan(wstats[1]))      # float32 threshold: exactly
        if not stats[d, 2]:
            assert np.array_equal(bins[d, :, :, 0].astype(np.int64), Z[f"{case}.bin_counts"][d])        # populations: exactly
            assert np.array_equal(bins[d, :, :, 2], wbins[:, :, 2])                                     # and the accuracy counts
            np.testing.assert_allclose(bins[d, :, :, 1], wbins[:, :, 1], rtol=1e-12)
        got = ca.compute_ece(P[:, d], T[:, d], U[:, d], META["n_bins"])
        assert type(got) is float
        ref = Z[f"{case}.ece"][d]
        print(case, d, got, ref)
        assert abs(got - E.ece(p[:, d], t[:, d], u[:, d], META["n_bins"])) <= 1e-9 * abs(ref)
        assert abs(got - ref) <= max(4 * DIST["ece"], 1e-9 * abs(ref))
    assert ca.compute_ece(P[:, 0], T[:, 0], torch.full_like(U[:, 0], float("inf"))) == 0.0
    assert ca.compute_ece(P[:, 0], T[:, 0], U[:, 0], n_bins=32) >= 0.0


@pytest.mark.parametrize("case", CASES)
def test_agreement_scores_against_the_reference(case):
    p, t, u = Z[f"{case}.pred"], Z[f"{case}.target"], Z[f"{case}.unc"]
    s = M.DEERModelEvaluator().compute_scores(dev(p), dev(t), dev(u))
    a = E.agreement(p, t)
    for col, key in enumerate(("ccc", "mae", "rmse")):
        g = np.array([s[key][d] for d in DIMS])
        print(case, key, g.tolist())
        close(g, a[:, col], 1e-9)
        if not np.isnan(Z[f"{case}.f64.{key}"]).all():
            close(g, Z[f"{case}.f64.{key}"], 1e-9)
            near_ref32(g, Z[f"{case}.f32.{key}"], DIST[key])
        assert s[key]["average"] == pytest.approx(float(np.mean(g)), nan_ok=True)
    near_ref32([s["ece"][d] for d in DIMS], Z[f"{case}.ece"], DIST["ece"])


# ---- 4. sort and ranks ----------------------------------------------------------------------------------------------------------
def sort_keys(n, stream):
    """Ties, +-0.0, +-inf, denormals, NaN."""
    k = np.round(synth.normal(stream, n) * 8).astype(np.float32) / 8
    special = np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 1e-40, 0.0, -0.0, np.nan, 3e38, -3e38, np.nan], dtype=np.float32)
    pos = (np.arange(len(special)) * 7919) % n
    if n > len(special):
        k[pos] = special
    fine = synth.normal(stream + 1, n).astype(np.float32)
    k[n // 2:] = np.where(np.arange(n - n // 2) % 3 == 0, fine[n // 2:], k[n // 2:])
    return k


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 2048, 2049, 4097, 100003, 1 << 20])
def test_sort_pairs_is_the_stable_argsort_and_ranks_are_rankdata(n):
    k = sort_keys(n, 400 + n % 97)
    if n == 2:
        k = np.array([0.0, -0.0], dtype=np.float32)       # equal keys: index order decides
    K = dev(k)
    order, _ = M.sort_pairs(K)
    assert np.array_equal(order.cpu().numpy().astype(np.int64), np.argsort(k, kind="stable"))
    assert np.array_equal(M.average_ranks(K).cpu().numpy(), E.average_ranks(k))
    kk = k[~np.isnan(k)]
    if kk.size:                                            # without NaN the restated ranks are scipy's: spot-check the definition
        r = E.average_ranks(kk)
        assert r.sum() == kk.size * (kk.size + 1) / 2 and r.min() >= 1 and r.max() <= kk.size
        assert r[np.argmin(kk)] == (1 + (kk == kk.min()).sum()) / 2


def test_sort_pairs_reads_a_strided_column_and_refuses_more_than_its_limit():
    x = synth.normal(77, 3000 * 3).reshape(3000, 3).astype(np.float32)
    X = dev(x)
    for d in range(3):
        order, _ = M.sort_pairs(X, d)
        assert np.array_equal(order.cpu().numpy().astype(np.int64), np.argsort(x[:, d], kind="stable"))
    big = torch.zeros((1 << 20) + 1, dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError, match="limit"):
        M.sort_pairs(big)


def test_rank_moments_against_the_restatement():
    x, y = sort_keys(50001, 500), sort_keys(50001, 502)
    x, y = np.nan_to_num(x, nan=0.5), np.nan_to_num(y, nan=-0.5)
    ra, rb = M.average_ranks(dev(x)), M.average_ranks(dev(y))
    out = torch.empty(3, dtype=torch.float64, device=DEV)
    _lib.check(_lib.load().mmdeer_rank_moments(ra.data_ptr(), rb.data_ptr(), len(x), out.data_ptr(), _lib.current_stream()))
    np.testing.assert_allclose(out.cpu().numpy(), E.rank_moments(E.average_ranks(x), E.average_ranks(y)), rtol=1e-12)


# ---- 4b. the shared order-statistic selection, through both entry points -------------------------------------------------------------
def select_keys(n, stream):
    """Heavy ties (about nine distinct values), negatives, +-0.0, denormals and +-3e38; finite, no NaN."""
    k = np.round(synth.normal(stream, n) * 2).astype(np.float32) / 2
    special = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, 3e38, -3e38, -0.0, 0.0], dtype=np.float32)
    if n > len(special):
        k[(np.arange(len(special)) * 37) % n] = special
    elif n == 2:
        k = np.array([-0.0, -3e38], dtype=np.float32)
    return k


def quantile_select(err, unc, nq):
    vals = torch.full((nq, 2), -1.0, dtype=torch.float32, device=DEV)
    frac = torch.full((nq,), -1.0, dtype=torch.float64, device=DEV)
    nv = torch.full((1,), -1, dtype=torch.int64, device=DEV)
    E_, U_ = dev(err), dev(unc)
    _lib.check(_lib.load().mmdeer_eval_quantile_select(E_.data_ptr(), U_.data_ptr(), len(err), nq, vals.data_ptr(), frac.data_ptr(),
                                                       nv.data_ptr(), _lib.current_stream()))
    return vals.cpu().numpy(), frac.cpu().numpy(), int(nv.item())


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 1000])
def test_radix_selection_is_the_sorted_order_statistic_through_both_entry_points(n):
    """Integer-exact: the selected 32-bit image is that of the k-th smallest key, so every comparison is == (-0.0 == 0.0)."""
    i = np.arange(n)
    # quantile path: a sample counts when its error is not NaN and its uncertainty is finite
    unc = select_keys(n, 610 + n % 89)
    err = np.abs(select_keys(n, 611 + n % 89))
    err[i % 7 == 3] = np.nan
    unc[i % 11 == 5] = np.inf
    unc[i % 13 == 6] = -np.inf
    unc[i % 17 == 8] = np.nan
    valid = ~np.isnan(err) & np.isfinite(unc)
    s = np.sort(unc[valid])
    nv = len(s)
    assert nv >= 1 and (nv < n or n <= 3)
    for nq in (2, 11):
        vals, frac, nvalid = quantile_select(err, unc, nq)
        q = np.linspace(0, 1, nq)
        virt = q * (nv - 1)
        lo = np.floor(virt).astype(np.int64)
        hi = np.minimum(lo + 1, nv - 1)
        assert nvalid == nv, (nq, nvalid, nv)
        assert np.array_equal(vals[:, 0], s[lo]) and np.array_equal(vals[:, 1], s[hi]), (nq, vals.tolist(), s[lo].tolist(), s[hi].tolist())
        assert np.array_equal(frac, virt - lo), (nq, frac.tolist(), (virt - lo).tolist())
        vals, frac, nvalid = quantile_select(np.full(n, np.nan, dtype=np.float32), unc, nq)
        assert nvalid == 0 and not vals.any() and not frac.any()
    vals, frac, nvalid = quantile_select(err, np.full(n, -np.inf, dtype=np.float32), 11)
    assert nvalid == 0 and not vals.any() and not frac.any()
    # calibration path: stats[d, 1] is np.median of the float32 |p - t| (odd n: the middle one, even n: the float32 mean of two)
    p = np.stack([select_keys(n, 620 + n % 89), select_keys(n, 621 + n % 89)], axis=1)
    t = np.stack([np.zeros(n, dtype=np.float32), np.round(synth.normal(622 + n % 89, n)).astype(np.float32)], axis=1)
    u = (0.5 + np.abs(synth.normal(623 + n % 89, 2 * n)).reshape(n, 2)).astype(np.float32)
    e = np.abs(p - t)
    assert e.dtype == np.float32 and not np.isnan(e).any()
    stats, _ = M.calibration_bins(dev(p), dev(t), dev(u), 10)
    want = np.median(e, axis=0)
    assert want.dtype == np.float32 and np.array_equal(stats[:, 1], want.astype(np.float64)), (stats[:, 1].tolist(), want.tolist())
    assert not stats[:, 3].any()
    p[n // 3, 0] = np.nan
    stats, _ = M.calibration_bins(dev(p), dev(t), dev(u), 10)
    assert math.isnan(stats[0, 1]) and stats[0, 3] == 1.0 and stats[1, 1] == float(want[1]) and stats[1, 3] == 0.0


# ---- 5. evaluate_model end to end ----------------------------------------------------------------------------------------------
def loader(n, bs, seed, as_dict):
    b = synth.make_batch(n, seed=seed)
    if as_dict:
        return [{"audio_features": torch.from_numpy(b["audio"][i:i + bs]), "video_features": torch.from_numpy(b["video"][i:i + bs]),
                 "text_features": torch.from_numpy(b["text"][i:i + bs]), "targets": torch.from_numpy(b["targets"][i:i + bs])}
                for i in range(0, n, bs)]
    ds = torch.utils.data.TensorDataset(*(torch.from_numpy(b[k]) for k in ("audio", "video", "text", "targets")))
    return torch.utils.data.DataLoader(ds, batch_size=bs, shuffle=False)


@pytest.mark.parametrize("stack,as_dict", [("c", True), ("c", False), ("b", True), ("b", False)])
def test_evaluate_model_end_to_end(stack, as_dict):
    from mmdeer import stackb
    from mmdeer.model import ModelConfig, MultimodalDEER
    torch.manual_seed(5)
    model = (MultimodalDEER(ModelConfig(compute_dtype="fp32", dropout=0.0)) if stack == "c"
             else stackb.CompleteDEERModel(compute_dtype="fp32")).to(DEV)
    n, reps = 200, 120
    ev = M.DEERModelEvaluator(n_bootstrap=reps, confidence_level=0.9)
    res, P, T, U = ev.evaluate_model(model, loader(n, 64, 21, as_dict), torch.device(DEV), return_predictions=True)
    assert all(isinstance(x, torch.Tensor) and x.is_cuda and x.shape == (n, 3) for x in (P, T, U))
    assert isinstance(res, M.EvaluationResults)
    assert res.sample_size == n and res.model_parameters == sum(q.numel() for q in model.parameters()) and res.evaluation_time > 0
    p, t, u = (x.cpu().numpy() for x in (P, T, U))
    a = E.agreement(p, t)
    mom, flags = E.bootstrap_moments(p, t, reps, 0)
    ci, _ = E.confidence_intervals(mom, flags, n, 0, 0.9)
    c = E.correlations(p, t)
    for d, dim in enumerate(DIMS):
        close([getattr(res, f"ccc_{dim}"), getattr(res, f"mae_{dim}"), getattr(res, f"rmse_{dim}")], a[d], 1e-9)
        close([getattr(res, f"ece_{dim}")], [E.ece(p[:, d], t[:, d], u[:, d])], 1e-9)
        close(res.confidence_intervals[dim], ci[d], 1e-9)
        s = res.significance_tests[dim]
        close([s["pearson_correlation"], s["spearman_correlation"], s["t_test_statistic"]], c[d], 1e-9)
        close_p([s["pearson_p_value"]], [M.pearson_p_value(c[d, 0], n)], 5e-5)
    for key in ("ccc", "mae", "rmse", "ece"):
        assert getattr(res, f"{key}_average") == pytest.approx(np.mean([getattr(res, f"{key}_{dim}") for dim in DIMS]), rel=1e-12)
    d = json.loads(json.dumps(res.to_dict()))
    assert d["meta"]["sample_size"] == n and len(d["statistical_validation"]["confidence_intervals"]["arousal"]) == 2
    plain = M.evaluate_deer_model(model, loader(n, 64, 21, as_dict), torch.device(DEV), {"n_bootstrap": reps, "confidence_level": 0.9})
    assert isinstance(plain, M.EvaluationResults) and plain.confidence_intervals == res.confidence_intervals
    assert plain.ccc_valence == res.ccc_valence and plain.significance_tests == res.significance_tests


def test_fewer_than_three_dimensions():
    p, t = random_case(999, 2, 340)
    ci = M.StatisticalValidator().compute_confidence_intervals(dev(p), dev(t), n_bootstrap=50, seed=2)
    assert list(ci) == ["valence", "arousal"]
    mom, flags = E.bootstrap_moments(p, t, 50, 2)
    own, _ = E.confidence_intervals(mom, flags, len(p), 0, 0.95)
    close(np.array([ci[d] for d in ci]), own, 1e-9)
    sig = M.StatisticalValidator().run_significance_tests(dev(p), dev(t))
    close([sig["arousal"]["pearson_correlation"], sig["arousal"]["spearman_correlation"]], E.correlations(p, t)[1, :2], 1e-9)
    s = M.DEERModelEvaluator().compute_scores(dev(p), dev(t))
    assert s["ccc"]["dominance"] == 0.0 and s["ece"]["average"] == 0.0


# ---- 6. host checks ------------------------------------------------------------------------------------------------------------
def test_host_checks_refuse_without_launching():
    from .test_cpu_evaluation import test_entry_points_refuse_bad_arguments_before_any_launch, test_public_classes_refuse_cpu_tensors_and_arrays
    test_entry_points_refuse_bad_arguments_before_any_launch()
    test_public_classes_refuse_cpu_tensors_and_arrays()
    g = torch.zeros(8, 3, device=DEV)
    with pytest.raises(ValueError):
        M.StatisticalValidator().compute_confidence_intervals(torch.zeros(8, 4, device=DEV), torch.zeros(8, 4, device=DEV))
    with pytest.raises(ValueError):
        M.StatisticalValidator().compute_confidence_intervals(g[:0], g[:0])
    with pytest.raises(RuntimeError, match="R <= 4096"):
        M.StatisticalValidator().compute_confidence_intervals(g, g, n_bootstrap=4097)
    with pytest.raises(RuntimeError, match="n_bins <= 32"):
        M.CalibrationAnalyzer().compute_ece(g[:, 0], g[:, 0], g[:, 0], n_bins=33)
    torch.cuda.synchronize()
