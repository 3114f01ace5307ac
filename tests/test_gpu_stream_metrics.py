"""The streaming-metric kernels of csrc/evalstats.hip (eval_accumulate_kernel, eval_ece_bins_kernel) through the C ABI, and
metrics.StreamingMetrics / metrics.device_calibration_error on top of them, against the numpy restatements of tests/loss_ref.py.

 * mmdeer_eval_accumulate on small integers: the eight sums per dimension are integers below 2^53 and compare ==, at every block
   boundary of the 256-lane loop, with NaN in one column of pred, in another of target and in a whole row, over three successive
   calls into one accumulator; the per-sample float32 means bit for bit (NaN rows: NaN on both sides).
 * on real data the sums within 4 N 2^-53 of their scale; CCC / RMSE / MAE of StreamingMetrics.compute() on a nearly constant and on
   a constant column within the bound the conditioning of the raw power sums gives (derived below, distances printed).
 * mmdeer_eval_ece_bins with uncertainties ON the bin edges (upper bin), on the last edge and below the first (no bin), NaN / inf
   (skipped): exact counts, sums within 4 n 2^-53 of their scale, exact on integers.
 * device_calibration_error on heavily tied uncertainties against metrics.uncertainty_calibration_error.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mmdeer import _lib, metrics  # noqa: E402

from . import loss_ref as L  # noqa: E402

DEV = "cuda:0"
EPS53 = 2.0 ** -53
SENT = -123.0


def accumulate(pred, target, unc=None, acc=None, want_err=True, want_unc=True, B=None):
    """mmdeer_eval_accumulate: (rc, acc [3, 8] device tensor, sample_err, sample_unc as numpy or None)."""
    lib = _lib.load()
    p, t = torch.from_numpy(pred).to(DEV), torch.from_numpy(target).to(DEV)
    u = torch.from_numpy(unc).to(DEV) if unc is not None else None
    n = pred.shape[0]
    if acc is None:
        acc = torch.zeros(3, 8, dtype=torch.float64, device=DEV)
    err = torch.full((max(n, 1),), SENT, dtype=torch.float32, device=DEV) if want_err else None
    su = torch.full((max(n, 1),), SENT, dtype=torch.float32, device=DEV) if want_unc else None
    rc = lib.mmdeer_eval_accumulate(p.data_ptr(), t.data_ptr(), _lib.ptr(u), acc.data_ptr(), _lib.ptr(err), _lib.ptr(su),
                                    n if B is None else B, _lib.current_stream())
    torch.cuda.synchronize()
    return rc, acc, (err.cpu().numpy() if err is not None else None), (su.cpu().numpy() if su is not None else None)


def _same_float32(got, want):
    """Bit for bit; where the float32 program has NaN, NaN."""
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got[~nan].view(np.int32), want[~nan].view(np.int32))


def integer_batch(B, seed):
    rng = np.random.default_rng(seed)
    pred = rng.integers(-8, 9, size=(B, 3)).astype(np.float32)
    target = rng.integers(-8, 9, size=(B, 3)).astype(np.float32)
    unc = (rng.integers(0, 17, size=(B, 3)) / 8.0).astype(np.float32)
    if B >= 255:
        pred[B // 5, 0] = np.nan                   # in pred of one dimension only
        target[B // 3, 1] = np.nan                 # in target of another dimension only
        pred[B // 2], target[B // 2] = np.nan, np.nan        # a row that is all NaN
        pred[B - 1, 2] = np.nan                    # the last row (the last lane of the last pass)
    return pred, target, unc


# =========================================================================== mmdeer_eval_accumulate
@pytest.mark.parametrize("B", [1, 255, 256, 257, 1000])
def test_accumulate_integer_data_is_exact_over_three_calls(B):
    acc = torch.zeros(3, 8, dtype=torch.float64, device=DEV)
    want = np.zeros((3, 8))
    for call in range(3):
        pred, target, unc = integer_batch(B, seed=10 * B + call)
        ref, _ = L.accumulate_reference(pred, target)
        want += ref
        rc, acc, err, su = accumulate(pred, target, unc, acc=acc)
        assert rc == 0
        assert np.array_equal(acc.cpu().numpy(), want), (B, call)
        e_ref, u_ref = L.sample_means_reference(pred, target, unc)
        _same_float32(err, e_ref)
        _same_float32(su, u_ref)
    if B >= 255:
        assert want[0, 0] == 3 * (B - 2) and want[1, 0] == 3 * (B - 2) and want[2, 0] == 3 * (B - 2)    # each column lost 2 rows a call
    assert float(np.abs(want).max()) < 2.0 ** 53


def test_accumulate_pointer_rules_and_the_empty_batch():
    lib = _lib.load()
    pred, target, unc = integer_batch(257, seed=5)
    ref, _ = L.accumulate_reference(pred, target)
    e_ref, _ = L.sample_means_reference(pred, target, None)
    rc, acc, err, su = accumulate(pred, target, None, want_err=True, want_unc=False)        # unc NULL with sample_err set
    assert rc == 0 and np.array_equal(acc.cpu().numpy(), ref)
    _same_float32(err, e_ref)
    rc, acc, err, su = accumulate(pred, target, None, want_err=False, want_unc=False)       # sums only
    assert rc == 0 and np.array_equal(acc.cpu().numpy(), ref)
    acc = torch.full((3, 8), SENT, dtype=torch.float64, device=DEV)
    rc, acc, err, su = accumulate(pred, target, None, acc=acc, want_err=True, want_unc=True)  # sample_unc without unc
    assert rc == -1 and b"unc" in lib.mmdeer_last_error()
    assert bool((acc == SENT).all()) and bool((err == SENT).all()) and bool((su == SENT).all())
    rc, acc, err, su = accumulate(pred, target, unc, acc=acc, B=0)                          # B = 0: nothing happens
    assert rc == 0 and bool((acc == SENT).all()) and bool((err == SENT).all()) and bool((su == SENT).all())
    rc, acc, err, su = accumulate(pred, target, unc, acc=acc, B=-1)
    assert rc == -1 and bool((acc == SENT).all())


def real_batch(N, seed):
    rng = np.random.default_rng(seed)
    target = np.tanh(rng.standard_normal((N, 3))).astype(np.float32)
    pred = (0.7 * target + 0.3 * rng.standard_normal((N, 3))).astype(np.float32)
    unc = np.abs(rng.standard_normal((N, 3))).astype(np.float32)
    pred[N // 7, 1] = np.nan
    return pred, target, unc


@pytest.mark.parametrize("N", [257, 3000])
def test_accumulate_real_data_within_float64_rounding(N):
    pred, target, unc = real_batch(N, seed=N)
    ref, scale = L.accumulate_reference(pred, target)
    rc, acc, err, su = accumulate(pred, target, unc)
    assert rc == 0
    got = acc.cpu().numpy()
    ratio = np.abs(got - ref) / (N * EPS53 * scale)
    print(f"\nN = {N}: worst |sum - ref| = {ratio.max():.3f} x N 2^-53 x scale (allowed 4)")
    assert float(ratio.max()) <= 4.0
    assert np.array_equal(got[:, 0], ref[:, 0])
    _same_float32(err, L.sample_means_reference(pred, target, unc)[0])
    _same_float32(su, L.sample_means_reference(pred, target, unc)[1])
    rc, acc2, *_ = accumulate(pred, target, unc)
    assert np.array_equal(acc2.cpu().numpy().view(np.int64), got.view(np.int64))             # a second launch: identical bits


def _two_pass(p, t):
    """CCC, MAE, RMSE by the two-pass float64 formulas (metrics.py:59-125)."""
    p, t = p.astype(np.float64), t.astype(np.float64)
    mp, mt = p.mean(), t.mean()
    vp, vt, cov = ((p - mp) ** 2).mean(), ((t - mt) ** 2).mean(), ((p - mp) * (t - mt)).mean()
    ccc = 2 * cov / (vp + vt + (mp - mt) ** 2) if vp > 0 and vt > 0 else 0.0
    return ccc, np.abs(p - t).mean(), np.sqrt(((p - t) ** 2).mean()), (vp, vt, mp, mt)


def _streamed(pred, target, chunks=3):
    sm = metrics.StreamingMetrics(DEV)
    for idx in np.array_split(np.arange(pred.shape[0]), chunks):
        sm.update(torch.from_numpy(pred[idx]).to(DEV), torch.from_numpy(target[idx]).to(DEV))
    return sm.compute()


def test_compute_on_a_nearly_constant_and_on_a_constant_column():
    """compute() forms variances and the covariance from raw power sums: E[x^2] - mean^2 loses E[x^2] / var(x) digits.  A raw sum
    of N terms accumulated in float64 is within N 2^-53 of its scale, so a variance is within E[x^2] / var(x) N 2^-53 relative;
    the CCC is a ratio of the covariance and the two variances (and is at most 1): 8 times that covers the three of them and the
    products of the means.  Column 0: p = 0.3 + 1e-4 x against a target of the same kind; column 1: p the constant float32(0.3)
    (true variance 0: the same ABSOLUTE error 8 E[x^2] N 2^-53 of the raw-sum (co)variance over the true denominator bounds
    |ccc|, whose two-pass value is 0); column 2 ordinary.
    Measured on an MI355X: distance 2.6e-9 under a bound of 2.4e-5 (column 0), 1.7e-18 under 4.3e-12 (column 1: compute() sees a
    variance of a few 1e-18 where two passes see 0, and reports that tiny CCC, not 0), 0 under 3.7e-12 (column 2)."""
    N = 3000
    rng = np.random.default_rng(17)
    x, z = rng.standard_normal(N), rng.standard_normal(N)
    pred, target, _ = real_batch(N, seed=18)
    pred[N // 7, 1] = 0.0
    pred[:, 0] = (0.3 + 1e-4 * x).astype(np.float32)
    target[:, 0] = (0.3 + 1e-4 * (0.8 * x + 0.6 * z)).astype(np.float32)
    pred[:, 1] = np.float32(0.3)
    got = _streamed(pred, target)
    print()
    for d, name in enumerate(metrics.DIMENSION_NAMES):
        p, t = pred[:, d], target[:, d]
        ccc, mae, rmse, (vp, vt, mp, mt) = _two_pass(p, t)
        ex2 = max(float((p.astype(np.float64) ** 2).mean()), float((t.astype(np.float64) ** 2).mean()))
        if d == 1:
            assert vp == 0.0 and ccc == 0.0
            delta = 8 * ex2 * N * EPS53                         # absolute error of a raw-sum variance / covariance
            bound = 2 * delta / (vt + (mp - mt) ** 2 - 2 * delta)
        else:
            bound = 8 * ex2 / min(vp, vt) * N * EPS53
        dist = abs(got[f"ccc_{name}"] - ccc)
        print(f"   {name}: ccc {got[f'ccc_{name}']:.12g} (two-pass {ccc:.12g}), distance {dist:.3g}, derived bound {bound:.3g}")
        assert dist <= bound, (name, dist, bound)
        assert got[f"mae_{name}"] == pytest.approx(mae, rel=4 * N * EPS53, abs=0)
        assert got[f"rmse_{name}"] == pytest.approx(rmse, rel=4 * N * EPS53, abs=0)
        host = metrics.DEERMetrics()
        assert host.concordance_correlation_coefficient(t, p) == pytest.approx(ccc, abs=1e-9)


# =========================================================================== mmdeer_eval_ece_bins
def ece_bins(err, unc, edges, n_bins=None, n=None):
    lib = _lib.load()
    e, u = torch.from_numpy(err).to(DEV), torch.from_numpy(unc).to(DEV)
    ed = torch.from_numpy(edges).to(DEV)
    nb = len(edges) - 1 if n_bins is None else n_bins
    bins = torch.full((max(nb, 1), 3), SENT, dtype=torch.float64, device=DEV)
    rc = lib.mmdeer_eval_ece_bins(e.data_ptr(), u.data_ptr(), len(err) if n is None else n, ed.data_ptr(), nb, bins.data_ptr(),
                                  _lib.current_stream())
    torch.cuda.synchronize()
    return rc, bins.cpu().numpy()


def ece_case(n, nb, seed):
    """Uniform data on float32 edges promoted to double, with samples ON the interior edges, on the last edge, below the first,
    and the kinds ece_valid skips."""
    rng = np.random.default_rng(seed)
    edges = np.linspace(0, 1, nb + 1, dtype=np.float32).astype(np.float64)
    unc = rng.random(n, dtype=np.float32)
    err = rng.random(n, dtype=np.float32)
    planted = {}
    if n >= 255:
        rows = iter(range(5, n, 7))
        for k in range(1, nb):
            r = next(rows)
            unc[r] = np.float32(edges[k])
            planted[r] = k                          # ON edge k: the upper bin
        for value in (np.float32(edges[-1]), np.float32(-0.25), -np.float32(1e-30)):      # the last edge itself, negative: no bin
            r = next(rows)
            unc[r] = value
            planted[r] = -1
        for e_val, u_val in ((np.nan, 0.5), (0.5, np.nan), (0.5, np.inf), (0.5, -np.inf)):  # skipped
            r = next(rows)
            err[r], unc[r] = e_val, u_val
            planted[r] = -2
    return err, unc, edges, planted


@pytest.mark.parametrize("nb", [1, 10, 15, 16])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_ece_bins_against_float64(n, nb):
    err, unc, edges, planted = ece_case(n, nb, seed=100 * nb + n)
    ref, scale = L.ece_bins_reference(err, unc, edges)
    for r, k in planted.items():                                # the reference puts the planted samples where they were built to go
        if k >= 0:
            assert edges[k] <= np.float64(unc[r]) < edges[k + 1] and np.float64(unc[r]) == edges[k]
    valid_in_range = int(sum(1 for r in range(n) if L.ece_valid(err[r:r + 1], unc[r:r + 1])[0] and 0 <= unc[r] < 1))
    assert int(ref[:, 0].sum()) == valid_in_range == n - sum(1 for k in planted.values() if k < 0)
    rc, got = ece_bins(err, unc, edges)
    assert rc == 0
    assert np.array_equal(got[:, 0], ref[:, 0]), (got[:, 0], ref[:, 0])
    ratio = np.abs(got[:, 1:] - ref[:, 1:]) / (n * EPS53 * np.maximum(scale[:, 1:], 1e-300))
    ratio = np.where(got[:, 1:] == ref[:, 1:], 0.0, ratio)
    print(f"\nn = {n}, {nb} bins: populations {ref[:, 0].astype(int).tolist()}, worst sum {ratio.max():.3f} x n 2^-53 x scale (allowed 4)")
    assert float(ratio.max()) <= 4.0
    rc, again = ece_bins(err, unc, edges)
    assert rc == 0 and np.array_equal(again.view(np.int64), got.view(np.int64))


@pytest.mark.parametrize("nb", [1, 10, 16])
def test_ece_bins_every_edge_as_a_sample(nb):
    """Samples edges[0 .. nb]: bin i holds exactly the sample ON edge i, the sample on the last edge is in no bin."""
    edges = np.linspace(0, 1, nb + 1, dtype=np.float32).astype(np.float64)
    unc = edges.astype(np.float32)
    err = np.full(nb + 1, 0.25, dtype=np.float32)
    rc, got = ece_bins(err, unc, edges)
    assert rc == 0
    assert np.array_equal(got[:, 0], np.ones(nb)) and np.array_equal(got[:, 1], 1.0 - edges[:-1]) and np.array_equal(got[:, 2], np.full(nb, 0.75))


@pytest.mark.parametrize("n", [257, 1000])
def test_ece_bins_integer_data_is_exact(n):
    rng = np.random.default_rng(n)
    nb = 16
    edges = np.arange(nb + 1, dtype=np.float64)
    unc = rng.integers(-2, nb + 2, size=n).astype(np.float32)
    err = rng.integers(-8, 9, size=n).astype(np.float32)
    ref, _ = L.ece_bins_reference(err, unc, edges)
    rc, got = ece_bins(err, unc, edges)
    assert rc == 0 and np.array_equal(got, ref)
    assert int(ref[:, 0].sum()) == int(((unc >= 0) & (unc < nb)).sum()) < n


def test_ece_bins_refusals_write_nothing():
    lib = _lib.load()
    err, unc, edges, _ = ece_case(257, 16, seed=1)
    wide = np.linspace(0, 1, 18)
    for kw in (dict(edges=wide, n_bins=17), dict(edges=edges, n_bins=0), dict(edges=edges, n=0), dict(edges=edges, n=-1)):
        rc, got = ece_bins(err, unc, **kw)
        assert rc == -1 and len(lib.mmdeer_last_error()) > 0
        assert bool((got == SENT).all())


# =========================================================================== device_calibration_error end to end
@pytest.mark.parametrize("n,n_bins", [(257, 10), (1000, 10), (1000, 15)])
def test_device_calibration_error_on_heavy_ties(n, n_bins):
    """Uncertainties rounded to 1 / 8: most quantile edges coincide with many samples."""
    rng = np.random.default_rng(n + n_bins)
    unc = (np.round(np.abs(rng.standard_normal(n)) * 8) / 8).astype(np.float32)
    err = np.abs(rng.standard_normal(n)).astype(np.float32) * 0.5
    unc[3], err[5], unc[7] = np.nan, np.nan, np.inf
    ok = L.ece_valid(err, unc)
    edges = np.quantile(unc[ok].astype(np.float64), np.linspace(0, 1, n_bins + 1))
    on_edge = int(np.isin(unc[ok].astype(np.float64), edges[1:-1]).sum())
    assert on_edge > n // 10 and len(np.unique(unc[ok])) < 40                   # heavy ties, many samples ON an interior edge
    want = metrics.uncertainty_calibration_error(err, np.zeros_like(err), unc, n_bins=n_bins)
    got = metrics.device_calibration_error(torch.from_numpy(err).to(DEV), torch.from_numpy(unc).to(DEV), n_bins=n_bins)
    print(f"\nn = {n}, {n_bins} bins: {on_edge} samples on an interior edge, ece {got:.15g} (numpy {want:.15g})")
    assert 0.0 < want < 1.0
    assert got == pytest.approx(want, rel=1e-12, abs=0)
