"""The three stand-alone loss kernels of csrc/nig.hip (deer_v1_kernel + deer_v1_final_kernel, unc_reg_kernel, calibration_kernel)
through the C ABI and through the classes of mmdeer.losses, against the float64 restatements of tests/loss_ref.py.

Sizes: every block boundary of the 256-element blocks, the final fold of the variant-1 loss over exactly 256 and over 257 partials,
the strided loops of the two single-workgroup kernels below, at and above one pass; D = 1, 3, 8 and B = 1, 2 for the regulariser;
1 to 32 bins with confidences on, next to and outside every bin edge, empty bins, bins of one sample, |y - gamma| / 2 on and next to
the clamp; the values-only mode, the refusals, the embedded 15-bin table, two launches bit for bit.

Tolerance: |got - ref| <= K * 2^-24 * scale (tests/nig_ref.py), the scale being the float64 sum of the absolute values of the pieces
that form the value (tests/loss_ref.py).  Each K is twice the worst ratio the SAME formulas in float32 on the CPU
(loss_ref.float32_eval_*) show against the restatement over all cases of this file, never below 8; the factor 2 is for the device's
lgammaf / logf and the series digamma.  Measured on the CPU:
    variant-1 values          worst 3.28 (v1-n255)                 -> K_V1      = 8
    variant-1 gradients       worst 10.94 (v1-n65537)              -> K_V1_GRAD = 22
    regulariser, both         worst 4.10 (unc-alpha-one, values)   -> K_UNC     = 9
    calibration, both         worst 5.53 (cal-*-n12291, gradients) -> K_CAL     = 12
Worst ratios seen on an MI355X over this file (pytest -s prints them): 1.80 (K_V1: v1-n1), 7.86 (K_V1_GRAD: v1-n65536), 3.34 (K_UNC),
5.83 (K_CAL: the CalibrationLoss class under an upstream gradient of 2.5; 5.53 through the C ABI).
Bin counts are exact.  The basic losses.DEERLoss runs by nig_ref's rule and constants (K_LOSS = 9, K_GRAD = 14).
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from mmdeer import _lib, losses  # noqa: E402
from mmdeer.spec import DIM_NAMES  # noqa: E402

from . import loss_ref as L  # noqa: E402
from . import nig_ref as R  # noqa: E402

DEV = "cuda:0"
K_V1, K_V1_GRAD, K_UNC, K_CAL = 8.0, 22.0, 9.0, 12.0
K_NIG_LOSS, K_NIG_GRAD = 9.0, 14.0          # tests/test_gpu_nig_loss.py
SENT = -123.0
V1_CASES = {tag: (inputs, ew, kw) for tag, inputs, ew, kw in L.v1_cases()}
UNC_CASES = {tag: (inputs, dw, sw) for tag, inputs, dw, sw in L.unc_cases()}
CAL_CASES = {tag: (inputs, nb, regular) for tag, inputs, nb, regular in L.cal_cases()}
WORST = {}
_REFS = {}


def ref_of(tag):
    """The reference of a case, computed once (its conditions asserted) and left unchanged."""
    if tag not in _REFS:
        if tag in V1_CASES:
            _REFS[tag] = L.checked_v1_reference(tag, *V1_CASES[tag])
        elif tag in UNC_CASES:
            inputs, dw, sw = UNC_CASES[tag]
            _REFS[tag] = L.unc_reg_reference(*inputs, dw, sw)
        else:
            _REFS[tag] = L.checked_cal_reference(tag, *CAL_CASES[tag])
    return _REFS[tag]


def _note(kind, log):
    for _name, r in log:
        WORST[kind] = max(WORST.get(kind, 0.0), r)
    print("   " + "  ".join(f"{name}: {r:.2f}" for name, r in log) + f"   [worst so far {kind}: {WORST.get(kind, 0.0):.2f}]")


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _dev(ts):
    return [t.to(DEV).contiguous() for t in ts]


# =========================================================================== the C ABI
def v1_call(inputs, ew, kw, want_grads=True, pad=64, grad_ptrs=None):
    """mmdeer_deer_loss_v1: (rc, out [5], grads [4, n], scratch with `pad` floats past its stated size), CPU tensors."""
    lib = _lib.load()
    m, nv, a, b, y = _dev(t.reshape(-1) for t in inputs)
    n = m.numel()
    ns = int(lib.mmdeer_deer_loss_v1_scratch(n))
    scratch = torch.full((ns + pad,), SENT, dtype=torch.float32, device=DEV)
    grads = torch.full((4, n), SENT, dtype=torch.float32, device=DEV)
    out = torch.full((5,), SENT, dtype=torch.float32, device=DEV)
    gp = grad_ptrs(grads) if grad_ptrs else [grads[i].data_ptr() if want_grads else None for i in range(4)]
    rc = lib.mmdeer_deer_loss_v1(m.data_ptr(), nv.data_ptr(), a.data_ptr(), b.data_ptr(), y.data_ptr(), n, ew, kw, out.data_ptr(), *gp,
                                 scratch.data_ptr(), _lib.current_stream())
    torch.cuda.synchronize()
    return rc, out.cpu(), grads.cpu(), scratch.cpu(), ns


def unc_call(alpha, beta, dw, sw, want_grads=True, B=None, D=None):
    lib = _lib.load()
    a, b = _dev((alpha, beta))
    B = a.shape[0] if B is None else B
    D = a.shape[1] if D is None else D
    grads = torch.full((2, *a.shape), SENT, dtype=torch.float32, device=DEV)
    out = torch.full((3,), SENT, dtype=torch.float32, device=DEV)
    gp = [grads[i].data_ptr() if want_grads else None for i in range(2)]
    rc = lib.mmdeer_uncertainty_reg_loss(a.data_ptr(), b.data_ptr(), B, D, dw, sw, out.data_ptr(), *gp, _lib.current_stream())
    torch.cuda.synchronize()
    return rc, out.cpu(), grads.cpu()


def cal_call(inputs, n_bins, want_grads=True, embedded=False, edges=None):
    """mmdeer_calibration_loss_bins (or, ``embedded``, mmdeer_calibration_loss): (rc, loss [1], counts [n_bins], grads [3, n])."""
    lib = _lib.load()
    g, a, b, y = _dev(t.reshape(-1) for t in inputs)
    n = g.numel()
    grads = torch.full((3, n), SENT, dtype=torch.float32, device=DEV)
    out = torch.full((1,), SENT, dtype=torch.float32, device=DEV)
    bins = torch.full((max(n_bins, 1),), -7, dtype=torch.int32, device=DEV)
    gp = [grads[i].data_ptr() if want_grads else None for i in range(3)]
    if embedded:
        rc = lib.mmdeer_calibration_loss(g.data_ptr(), a.data_ptr(), b.data_ptr(), y.data_ptr(), n, out.data_ptr(), bins.data_ptr(), *gp,
                                         _lib.current_stream())
    else:
        e = L.cal_edges32(n_bins) if edges is None else edges
        rc = lib.mmdeer_calibration_loss_bins(g.data_ptr(), a.data_ptr(), b.data_ptr(), y.data_ptr(), n,
                                              (C.c_float * e.numel())(*[float(x) for x in e]), n_bins, out.data_ptr(), bins.data_ptr(), *gp,
                                              _lib.current_stream())
    torch.cuda.synchronize()
    return rc, out.cpu(), bins.cpu(), grads.cpu()


# =========================================================================== mmdeer_deer_loss_v1
@pytest.mark.parametrize("tag", list(V1_CASES))
def test_deer_loss_v1_against_float64(tag):
    inputs, ew, kw = V1_CASES[tag]
    ref = ref_of(tag)
    rc, out, grads, scratch, ns = v1_call(inputs, ew, kw)
    assert rc == 0
    print(f"\n{tag}: smallest |kl| {ref.min_abs_kl:.3g}, {100 * ref.neg_frac:.0f} % of kl < 0")
    log_v, log_g = [], []
    try:
        L.assert_close(f"{tag} values", out, ref.out, ref.out_scale, K_V1, log_v)
        L.assert_close(f"{tag} gradients", grads, ref.grads, ref.grad_scale, K_V1_GRAD, log_g)
    finally:
        _note("K_V1", log_v); _note("K_V1_GRAD", log_g)
    assert bool((scratch[ns:] == SENT).all()) and bool((scratch[:ns] != SENT).all())      # mmdeer_deer_loss_v1_scratch(n) floats, no more
    # values only: the same five values bit for bit, the gradient buffers untouched
    rc, out_v, grads_v, _, _ = v1_call(inputs, ew, kw, want_grads=False)
    assert rc == 0 and _same_bits(out_v, out) and bool((grads_v == SENT).all())
    rc, out2, grads2, _, _ = v1_call(inputs, ew, kw)
    assert rc == 0 and _same_bits(out2, out) and _same_bits(grads2, grads)


def test_deer_loss_v1_refuses_three_gradient_pointers_of_four():
    lib = _lib.load()
    inputs, ew, kw = V1_CASES["v1-n257-ew1.0-kw1.0"]
    for missing in range(4):
        rc, out, grads, scratch, _ = v1_call(inputs, ew, kw, grad_ptrs=lambda g: [None if i == missing else g[i].data_ptr() for i in range(4)])
        assert rc == -1 and len(lib.mmdeer_last_error()) > 0
        assert bool((out == SENT).all()) and bool((grads == SENT).all()) and bool((scratch == SENT).all())


# =========================================================================== mmdeer_uncertainty_reg_loss
@pytest.mark.parametrize("tag", list(UNC_CASES))
def test_uncertainty_reg_loss_against_float64(tag):
    (alpha, beta), dw, sw = UNC_CASES[tag]
    ref = ref_of(tag)
    rc, out, grads = unc_call(alpha, beta, dw, sw)
    assert rc == 0
    if alpha.shape[0] == 1:                                   # the reference's 0 / 0 in the unbiased variance
        assert bool(torch.isnan(ref.out[:2]).all()) and bool(torch.isnan(ref.grads).all()) and bool(torch.isfinite(ref.out[2]))
    else:
        assert bool(torch.isfinite(ref.out).all()) and bool(torch.isfinite(ref.grads).all())
    log = []
    try:
        L.assert_close(f"{tag} values", out, ref.out, ref.out_scale, K_UNC, log)
        L.assert_close(f"{tag} gradients", grads, ref.grads, ref.grad_scale, K_UNC, log)
    finally:
        print()
        _note("K_UNC", log)
    rc, out_v, grads_v = unc_call(alpha, beta, dw, sw, want_grads=False)
    assert rc == 0 and _same_bits(out_v, out) and bool((grads_v == SENT).all())
    rc, out2, grads2 = unc_call(alpha, beta, dw, sw)
    assert rc == 0 and _same_bits(out2, out) and _same_bits(grads2, grads)


def test_uncertainty_reg_loss_refusals_write_nothing():
    lib = _lib.load()
    alpha, beta = L.unc_case(4, 9)
    for kw in (dict(), dict(B=0), dict(D=0), dict(B=-1)):     # D = 9; B = 0; D = 0; B < 0
        rc, out, grads = unc_call(alpha, beta, 0.1, 0.01, **kw)
        assert rc == -1 and len(lib.mmdeer_last_error()) > 0
        assert bool((out == SENT).all()) and bool((grads == SENT).all())
    a, b = _dev(L.unc_case(4, 3))
    out = torch.full((3,), SENT, device=DEV)
    g = torch.full((4, 3), SENT, device=DEV)
    for gp in ((g.data_ptr(), None), (None, g.data_ptr())):                        # one gradient pointer of two
        assert lib.mmdeer_uncertainty_reg_loss(a.data_ptr(), b.data_ptr(), 4, 3, 0.1, 0.01, out.data_ptr(), *gp, _lib.current_stream()) == -1
    torch.cuda.synchronize()
    assert bool((out == SENT).all()) and bool((g == SENT).all())


# =========================================================================== mmdeer_calibration_loss_bins / mmdeer_calibration_loss
@pytest.mark.parametrize("tag", list(CAL_CASES))
def test_calibration_loss_against_float64(tag):
    inputs, nb, regular = CAL_CASES[tag]
    ref = ref_of(tag)
    rc, loss, bins, grads = cal_call(inputs, nb)
    assert rc == 0
    print(f"\n{tag}: populations {ref.counts.tolist()}, smallest gap {ref.min_gap:.3g}")
    log = []
    try:
        L.compare_calibration(loss, bins, grads, ref, K_CAL, log, tag)
    finally:
        _note("K_CAL", log)
    rc, loss_v, bins_v, grads_v = cal_call(inputs, nb, want_grads=False)
    assert rc == 0 and _same_bits(loss_v, loss) and torch.equal(bins_v, bins) and bool((grads_v == SENT).all())
    rc, loss2, bins2, grads2 = cal_call(inputs, nb)
    assert rc == 0 and _same_bits(loss2, loss) and torch.equal(bins2, bins) and _same_bits(grads2, grads)


@pytest.mark.parametrize("nb", L.CAL_BINS)
@pytest.mark.parametrize("mixed", [False, True])
def test_calibration_edge_samples_are_counted_where_they_were_built_to_go(nb, mixed):
    g, a, b, y, expect = L.cal_mixed_edge_case(nb) if mixed else L.cal_edge_case(nb)
    rc, loss, bins, grads = cal_call((g, a, b, y), nb)
    assert rc == 0
    outside = [row for row, k in expect if k < 0]
    assert int(bins.sum()) == g.numel() - len(outside)
    if not mixed:
        want = torch.zeros(nb, dtype=torch.int32)
        for _row, k in expect:
            if k >= 0:
                want[k] += 1
        assert torch.equal(bins, want)
    for row in outside:                                        # alpha < 1: in no bin, no gradient at alpha and beta
        assert float(grads[1, row]) == 0.0 and float(grads[2, row]) == 0.0


def test_calibration_refusals_write_nothing():
    lib = _lib.load()
    inputs, _, _ = CAL_CASES["cal-nb32-n257"]
    for nb in (33, 0):
        rc, loss, bins, grads = cal_call(inputs, nb, edges=torch.linspace(0, 1, 34))
        assert rc == -1 and len(lib.mmdeer_last_error()) > 0
        assert bool((loss == SENT).all()) and bool((bins == -7).all()) and bool((grads == SENT).all())


@pytest.mark.parametrize("tag", ["cal-nb15-n12291", "cal-nb15-edges-alone", "cal-nb15-edges-in-300"])
def test_embedded_15_bin_table_gives_the_bits_of_linspace(tag):
    """mmdeer_calibration_loss (kCalEdges15) against mmdeer_calibration_loss_bins with torch.linspace(0, 1, 16)."""
    inputs, nb, _ = CAL_CASES[tag]
    assert nb == 15
    rc, loss, bins, grads = cal_call(inputs, 15, edges=torch.linspace(0, 1, 16))
    rc_e, loss_e, bins_e, grads_e = cal_call(inputs, 15, embedded=True)
    assert rc == 0 and rc_e == 0
    assert _same_bits(loss_e, loss) and torch.equal(bins_e, bins) and _same_bits(grads_e, grads)
    assert torch.equal(bins.to(torch.int64), ref_of(tag).counts)
    rc_v, loss_v, bins_v, grads_v = cal_call(inputs, 15, embedded=True, want_grads=False)
    assert rc_v == 0 and _same_bits(loss_v, loss) and torch.equal(bins_v, bins) and bool((grads_v == SENT).all())


# =========================================================================== the classes
UP = 2.5          # a non-unit upstream gradient


def test_class_deer_loss_v1_through_autograd():
    tag = "v1-n12291-ew0.7-kw0.3"
    inputs, ew, kw = V1_CASES[tag]
    ref = ref_of(tag)
    leaves = [t.view(4097, 3).clone().to(DEV).requires_grad_(True) for t in inputs[:4]]
    got = losses.DEERLossV1(ew, kw)(dict(zip(("mu", "nu", "alpha", "beta"), leaves)), inputs[4].view(4097, 3).to(DEV))
    (UP * got["total_loss"]).backward()
    log = []
    vec = torch.stack([got[k].detach() for k in ("total_loss", "nll_loss", "evidence_reg", "kl_reg", "mse")])
    L.assert_close("DEERLossV1 values", vec, ref.out, ref.out_scale, K_V1, log)
    _note("K_V1", log)
    log = []
    L.assert_close("DEERLossV1 gradients", torch.stack([t.grad.reshape(-1) for t in leaves]), UP * ref.grads, UP * ref.grad_scale, K_V1_GRAD, log)
    _note("K_V1_GRAD", log)


def test_class_uncertainty_regularization_through_autograd():
    tag = "unc-B1000-D3-dw0.1-sw0.01"
    (alpha, beta), dw, sw = UNC_CASES[tag]
    ref = ref_of(tag)
    a, b = (t.clone().to(DEV).requires_grad_(True) for t in (alpha, beta))
    got = losses.UncertaintyRegularizationLoss(dw, sw)({"alpha": a, "beta": b}, torch.zeros(1000, 3, device=DEV))
    (UP * got["reg_loss"]).backward()
    log = []
    vec = torch.stack([got[k].detach() for k in ("reg_loss", "diversity_loss", "sparsity_loss")])
    L.assert_close("UncertaintyRegularizationLoss values", vec, ref.out, ref.out_scale, K_UNC, log)
    L.assert_close("UncertaintyRegularizationLoss gradients", torch.stack([a.grad, b.grad]), UP * ref.grads, UP * ref.grad_scale, K_UNC, log)
    _note("K_UNC", log)


@pytest.mark.parametrize("nb", [15, 7])
def test_class_calibration_loss_through_autograd(nb):
    tag = f"cal-nb{nb}-n1000"
    inputs, _, _ = CAL_CASES[tag]
    ref = ref_of(tag)
    g, a, b = (t.clone().to(DEV).requires_grad_(True) for t in inputs[:3])
    mod = losses.CalibrationLoss(n_bins=nb)
    got = mod({"mu": g, "alpha": a, "beta": b}, inputs[3].to(DEV))
    (UP * got).backward()
    log = []
    assert torch.equal(mod.last_bin_counts.cpu().to(torch.int64), ref.counts)
    L.assert_close("CalibrationLoss value", got.detach().reshape(1), ref.loss, ref.loss_scale, K_CAL, log)
    L.assert_close("CalibrationLoss gradients", torch.stack([g.grad, a.grad, b.grad]), UP * ref.grads, UP * ref.grad_scale, K_CAL, log)
    _note("K_CAL", log)


def test_class_combined_loss_with_flat_keys_through_autograd():
    """Per-dimension AND flat keys: multi-task loss + regulariser + 0.1 x calibration loss, every term with its own K and scale."""
    B = 513
    inputs = R.regular_case(B, seed=1)                         # fold-B513 of tests/test_gpu_nig_loss.py
    mt = R.checked_reference("combined", inputs, R.LossConfig(), True)
    ur = L.unc_reg_reference(inputs[2], inputs[3], 0.1, 0.01)
    flat = (inputs[0], inputs[2], inputs[3], inputs[4])
    cal = L.checked_cal_reference("combined", flat, 15, False)
    leaves = [t.clone().to(DEV).requires_grad_(True) for t in inputs[:4]]
    pred = dict(zip(("gamma", "nu", "alpha", "beta"), leaves))
    for i, d in enumerate(DIM_NAMES):
        for j, k in enumerate(("mu", "nu", "alpha", "beta")):
            pred[f"{d}_{k}"] = leaves[j][:, i:i + 1]
    got = losses.CombinedDEERLoss()(pred, inputs[4].to(DEV))
    (UP * got["combined_total_loss"]).backward()
    ref_total = mt.out[16] + ur.out[0] + 0.1 * cal.loss[0]
    allowed = K_NIG_LOSS * mt.out_scale[16] + K_UNC * ur.out_scale[0] + K_CAL * 0.1 * cal.loss_scale[0]
    log = []
    L.assert_close("combined_total_loss", got["combined_total_loss"].detach().reshape(1), ref_total.reshape(1), allowed.reshape(1), 1.0, log)
    L.assert_close("reg_loss", got["reg_loss"].detach().reshape(1), ur.out[0:1], ur.out_scale[0:1], K_UNC, log)
    L.assert_close("calibration_loss", got["calibration_loss"].detach().reshape(1), cal.loss, cal.loss_scale, K_CAL, log)
    grads = mt.grads.clone()                                   # [4, B, 3] at (gamma, nu, alpha, beta)
    allowed = K_NIG_GRAD * mt.grad_scale.clone()
    for j, (u_i, c_i) in enumerate(((None, 0), (None, None), (0, 1), (1, 2))):
        if u_i is not None:
            grads[j] += ur.grads[u_i]
            allowed[j] += K_UNC * ur.grad_scale[u_i]
        if c_i is not None:
            grads[j] += 0.1 * cal.grads[c_i].view(B, 3)
            allowed[j] += K_CAL * 0.1 * cal.grad_scale[c_i].view(B, 3)
    L.assert_close("combined gradients", torch.stack([t.grad for t in leaves]), UP * grads, UP * allowed, 1.0, log)
    print()
    _note("combined (K = 1 on the summed allowances)", log)


def test_basic_deer_loss_is_dimension_0_of_the_multitask_kernel():
    """losses.DEERLoss on (257, 3): 771 flattened rows as dimension 0 with task weights (3, 0, 0), by nig_ref's rule and constants."""
    B = 257
    mu, nu, alpha, beta, y = R.regular_case(B, seed=1)
    mod = losses.DEERLoss(reg_weight=0.2, kl_weight=0.03, ece_weight=0.4)
    leaves = [t.clone().to(DEV).requires_grad_(True) for t in (mu, nu, alpha, beta)]
    got = mod(dict(zip(("gamma", "nu", "alpha", "beta"), leaves)), y.to(DEV))
    (UP * got["total_loss"]).backward()
    three = tuple(t.reshape(-1, 1).expand(-1, 3).contiguous() for t in (mu, nu, alpha, beta, y))
    assert three[0].shape[0] == 771
    cfg = R.LossConfig(reg_w=0.2, kl_w=0.03, ece_w=0.4, cross_w=0.0, task_w=(3.0, 0.0, 0.0))
    ref = R.checked_reference("DEERLoss-771", three, cfg, True)
    log = []
    for key, i in (("total_loss", 16), ("nll_loss", 1), ("reg_loss", 2), ("kl_loss", 3), ("ece_loss", 4)):
        R.assert_close(key, got[key].detach().reshape(1), ref.out[i:i + 1], ref.out_scale[i:i + 1], K_NIG_LOSS, log)
    assert got["batch_size"] == B
    print()
    _note("nig K_LOSS", log)
    log = []
    for j, name in enumerate(("gamma", "nu", "alpha", "beta")):
        R.assert_close("d/d" + name, leaves[j].grad.reshape(-1), UP * ref.grads[j].sum(1), UP * ref.grad_scale[j].sum(1), K_NIG_GRAD, log)
    _note("nig K_GRAD", log)
