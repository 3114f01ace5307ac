"""The frame video encoder's backward on the GPU: mmdeer_bn2d_bwd, mmdeer_conv2d_wgrad, mmdeer_conv2d_pack_t and mmdeer_conv2d_dgrad
against the float64 restatement (tests/frames_bwd_ref.py) on their own stored operands, at their edges, in both dtypes; reads and
writes outside the buffers; and the module with ``train_backbone``: the gradients captured from the reference
(tests/golden/frame_grad.npz), the bf16 gradients against the emulation, the switch, frozen parameters, determinism, the downstream
gradients and a few SGD steps."""
import functools
import os

import numpy as np
import pytest
import torch

from mmdeer import frames, synth, video

from . import frames_bwd_ref as RB
from . import frames_ref as R
from .test_cpu_frame_backward import GRAD_CASES, GRAD_GOLDEN, loss_weight, slice_of, state64, tag_of
from .test_gpu_frame_encoder import DEV, GEOMS, SIZES, _bn_inputs, _conv_case, _dt, _filled, _rel

pytestmark = pytest.mark.gpu

C = frames.C
SRCS = {"dense": frames.SRC_DENSE, "pool": frames.SRC_POOL, "avg": frames.SRC_AVG}
# (N, H, W) of the BatchNorm layer: M = 2, 390, 33001 (more than 1024 row blocks' worth), and for the pool an even-sized image, whose
# last row and column sit in one window only
BN_SIZES = [(2, 1, 1), (6, 5, 13), (1, 61, 541)]
BN_CASES = [(*s, src) for s in BN_SIZES for src in ("dense", "pool", "avg")] + [(2, 6, 8, "pool")]
SHARE_CAP = 1e-4          # of a case's elements may be undecided between fp32 and float64 (frames_bwd_ref.undecided)


def bn_bwd_inputs(N, H, W, Cn, compute, src):
    """-> (y, gamma, beta, dout in its source form, running_mean, running_var): seeded, the same on every machine.  The undecided
    share was counted on the CPU for every case, both dtypes and both kinds of statistics, with these seeds: 8.0e-5 at the most
    ((6, 5, 13) pool, C = 64: two elements of 24960), under the cap; with the seed offset 0 one case had four (1.6e-4)."""
    M = N * H * W
    y, gamma, beta = _bn_inputs(M, Cn, compute)
    gen = torch.Generator().manual_seed(31 * M + Cn + len(src) + 2000)
    rows = {"dense": M, "pool": N * R.out_size(H, 3) * R.out_size(W, 3), "avg": N}[src]
    dout = torch.randn(rows, Cn, generator=gen)
    dout = (dout if src == "avg" else dout.to(_dt(compute))).to(DEV)
    rm = (torch.rand(Cn, generator=gen) * 2 - 1).to(DEV)
    rv = (0.5 + 1.5 * torch.rand(Cn, generator=gen)).to(DEV)
    return y, gamma, beta, dout, rm, rv


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
@pytest.mark.parametrize("Cn", [64, 128, 256, 512])
@pytest.mark.parametrize("N,H,W,src", BN_CASES)
def test_bn2d_bwd_matches_float64(N, H, W, src, Cn, compute):
    """dgamma, dbeta: 1e-4 of their norm (test_gpu_video_encoder's bound for the BatchNorm-over-time backward).  dy: 1e-4 in fp32, twice
    the emulation's own distance + 1e-6 in bf16 (dy is stored rounded).  The undecided elements (mask or arg-max within 1e-5 of a tie)
    are left out of the dy comparison, and what they could move widens the vectors' bounds; their share is capped."""
    y, gamma, beta, dout, rm, rv = bn_bwd_inputs(N, H, W, Cn, compute, src)
    y64, g64, b64, d64 = y.double(), gamma.double(), beta.double(), dout.double()
    for running in (False, True):
        if running:
            mean, rstd, stats = rm, rv, (rm.double(), rv.double())
        else:
            (mean, rstd), stats = frames.bn2d_stats(y, N, H, W), (None, None)
        dy, dgamma, dbeta = frames.bn2d_bwd(y, N, H, W, mean, rstd, gamma, beta, dout, SRCS[src], running=running)
        assert dy.shape == y.shape and dy.dtype == y.dtype and dgamma.dtype == dbeta.dtype == torch.float32
        ref_dy, ref_dg, ref_db = RB.bn2d_bwd(y64, g64, b64, d64, N, H, W, SRCS[src], *stats)
        out, slack_b, slack_g = RB.undecided(y64, g64, b64, d64, N, H, W, SRCS[src], *stats)
        share = float(out.double().mean())
        keep = ~out
        d_dy = _rel(dy.double()[keep], ref_dy[keep])
        bound = 1e-4 if compute == "fp32" else 2 * _rel(R.bf16(ref_dy)[keep], ref_dy[keep]) + 1e-6
        e_g, e_b = float((dgamma.double() - ref_dg).norm()), float((dbeta.double() - ref_db).norm())
        print(f"{(N, H, W)} C={Cn} {src} {compute} running={running}: undecided {share:.1e}  dy {d_dy:.2e} (bound {bound:.2e})  "
              f"dgamma {e_g / float(ref_dg.norm()):.2e}  dbeta {e_b / float(ref_db.norm()):.2e}")
        assert share <= SHARE_CAP, share
        assert d_dy <= bound, (d_dy, bound)
        assert e_g <= 1e-4 * float(ref_dg.norm()) + float(slack_g.norm()), (e_g, float(ref_dg.norm()))
        assert e_b <= 1e-4 * float(ref_db.norm()) + float(slack_b.norm()), (e_b, float(ref_db.norm()))
        again = frames.bn2d_bwd(y, N, H, W, mean, rstd, gamma, beta, dout, SRCS[src], running=running)
        assert all(torch.equal(a, b) for a, b in zip(again, (dy, dgamma, dbeta)))                  # fixed order: bit-equal


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_pool_gradient_goes_to_the_first_maximum(compute):
    """Plateaus: small integers, so that a window holds several equal positive maxima, and whole windows of zeros.  Frozen statistics
    (mean 0, variance 1 - eps) keep the values exact on both sides, so nothing is undecided: the gradient must land where torch's
    float64 pool puts it -- the first maximum in (kh, kw) order among the in-image positions -- element for element."""
    N, H, W, Cn = 2, 6, 9, 64
    gen = torch.Generator().manual_seed(5)
    y = torch.tensor([-1.0, 1.0, 2.0])[torch.randint(0, 3, (N, H, W, Cn), generator=gen)]     # no zero: a pre-activation of 0 counts as undecided
    y[0, :3, :4] = -1.0                                                   # windows that hold nothing positive
    y[1, 2:, 5:] = 2.0                                                    # a plateau of maxima
    y = y.reshape(-1, Cn).to(_dt(compute)).to(DEV)
    gamma, beta = torch.ones(Cn, device=DEV), torch.zeros(Cn, device=DEV)
    rm, rv = torch.zeros(Cn, device=DEV), torch.full((Cn,), 1.0 - R.EPS, device=DEV)
    PH, PW = R.out_size(H, 3), R.out_size(W, 3)
    dout = (1 + torch.rand(N * PH * PW, Cn, generator=gen)).to(_dt(compute)).to(DEV)      # every pooled element hands on a non-zero gradient
    dy, dgamma, dbeta = frames.bn2d_bwd(y, N, H, W, rm, rv, gamma, beta, dout, frames.SRC_POOL, running=True)
    ref_dy, ref_dg, ref_db = RB.bn2d_bwd(y.double(), gamma.double(), beta.double(), dout.double(), N, H, W, RB.POOL, rm.double(), rv.double())
    assert not bool(RB.undecided(y.double(), gamma.double(), beta.double(), dout.double(), N, H, W, RB.POOL, rm.double(), rv.double())[0].any())
    assert torch.equal(dy != 0, ref_dy != 0)                              # where the gradient lands
    assert int((ref_dy != 0).sum()) > 0 and int((ref_dy == 0).sum()) > 0
    assert _rel(dy, ref_dy) <= (1e-6 if compute == "fp32" else 2 * _rel(R.bf16(ref_dy), ref_dy) + 1e-6)
    assert _rel(dbeta, ref_db) <= 1e-5 and _rel(dgamma, ref_dg) <= 1e-5


# ------------------------------------------------------------------------------------------------ the convolution's gradients
WGRAD_SIZES = SIZES + [(4, 61, 67)]
DGRAD_SIZES = SIZES + [(2, 6, 8)]


def _dy_case(k, cout, N, H, W, compute, zero_row=False):
    M = N * R.out_size(H, k) * R.out_size(W, k)
    dy = torch.randn(M, cout, generator=torch.Generator().manual_seed(17 * M + cout)).to(_dt(compute))
    if zero_row:
        dy = torch.cat([dy, dy.new_zeros(1, cout)])
    return M, dy.to(DEV)


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
@pytest.mark.parametrize("k,cin,cout", GEOMS)
def test_wgrad_matches_float64(k, cin, cout, compute):
    """dW and dbias within 1e-4 of their norm of float64 on the stored operands, in both dtypes: the products are exact and the
    accumulation is fp32.  Every slice count gives that, the automatic one included, and two runs store the same bits."""
    for N, H, W in WGRAD_SIZES:
        xp, w, b = _conv_case(k, cin, cout, N, H, W, compute)
        M, dy = _dy_case(k, cout, N, H, W, compute)
        ref_dw, ref_db, _ = RB.conv_grads(xp.double(), w.double(), b.double(), dy.double(), N, H, W, k, frames.taps(k))
        for slices in (-1, 1, 2, 5):
            dw, db = frames.conv2d_wgrad(xp, dy, N, H, W, cin, k, slices=slices)
            assert dw.shape == (cout, cin, k, k) and db.shape == (cout,) and dw.dtype == db.dtype == torch.float32
            assert _rel(dw, ref_dw) <= 1e-4 and _rel(db, ref_db) <= 1e-4, (N, H, W, slices, _rel(dw, ref_dw), _rel(db, ref_db))
            dw2, db2 = frames.conv2d_wgrad(xp, dy, N, H, W, cin, k, slices=slices)
            assert torch.equal(dw, dw2) and torch.equal(db, db2)
            dw3, none = frames.conv2d_wgrad(xp, dy, N, H, W, cin, k, bias=False, slices=slices)
            assert none is None and torch.equal(dw3, dw)                  # the bias gradient is a by-product: dW does not depend on it


def _banded(t, G=4096):
    """t between two NaN guard bands of G elements -> (the whole buffer, the view that holds t)"""
    big = torch.full((t.numel() + 2 * G,), float("nan"), dtype=t.dtype, device=DEV)
    big[G:G + t.numel()] = t.reshape(-1)
    inner = big[G:G + t.numel()].view(t.shape)
    assert inner.data_ptr() % 16 == 0
    return big, inner


def _bands_intact(big, numel, G=4096):
    return bool(torch.isnan(big[:G]).all()) and bool(torch.isnan(big[G + numel:]).all())


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
@pytest.mark.parametrize("k,cin,cout", [(7, 3, 64), (3, 64, 128), (3, 8, 64)])
def test_wgrad_reads_and_writes_nothing_outside_its_buffers(k, cin, cout, compute):
    """Both operands between NaN guard bands: the result is finite and equals the result on clean buffers.  The outputs between
    guard bands: nothing is written outside dW, dbias and the scratch the query asked for."""
    N, H, W = 3, 5, 7                                                     # M = 36: one ragged K-tile in both dtypes
    xp, w, b = _conv_case(k, cin, cout, N, H, W, compute, seed=5)
    M, dy = _dy_case(k, cout, N, H, W, compute)
    clean_dw, clean_db = frames.conv2d_wgrad(xp, dy, N, H, W, cin, k, slices=2)
    big_x, in_x = _banded(xp)
    big_dy, in_dy = _banded(dy)
    dw, db = frames.conv2d_wgrad(in_x, in_dy, N, H, W, cin, k, slices=2)
    assert bool(torch.isfinite(dw).all()) and torch.equal(dw, clean_dw) and torch.equal(db, clean_db)
    assert _bands_intact(big_x, xp.numel()) and _bands_intact(big_dy, dy.numel())
    a = frames._lib.Conv2dWgradArgs()
    a.x, a.dy = xp.data_ptr(), dy.data_ptr()
    a.N, a.H, a.W, a.Cin, a.Cout, a.k, a.act_f32, a.slices, a.stream = N, H, W, cin, cout, k, int(compute == "fp32"), 2, frames._lib.current_stream()
    need = frames._lib.load().mmdeer_conv2d_wgrad_scratch(C.byref(a))
    assert need > 0
    big_w, out_w = _banded(torch.zeros(cout * cin * k * k, device=DEV))
    big_b, out_b = _banded(torch.zeros(cout, device=DEV))
    big_s, out_s = _banded(torch.zeros(need, device=DEV))
    a.dw, a.dbias, a.scratch, a.scratch_elems = out_w.data_ptr(), out_b.data_ptr(), out_s.data_ptr(), need
    frames._lib.check(frames._lib.load().mmdeer_conv2d_wgrad(C.byref(a)))
    assert torch.equal(out_w.view(clean_dw.shape), clean_dw) and torch.equal(out_b, clean_db)
    assert _bands_intact(big_w, out_w.numel()) and _bands_intact(big_b, out_b.numel()) and _bands_intact(big_s, need)


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
@pytest.mark.parametrize("k,cin,cout", [g for g in GEOMS if g[0] == 3])
def test_dgrad_matches_float64(k, cin, cout, compute):
    """fp32: 1e-4 of the norm.  bf16: the operands are exact in float64, dx is stored rounded: twice the emulation's own distance +
    1e-6.  The transposed image, element for element, against its index formula."""
    dt = _dt(compute)
    for N, H, W in DGRAD_SIZES:
        xp, w, b = _conv_case(k, cin, cout, N, H, W, compute)
        M, dy = _dy_case(k, cout, N, H, W, compute, zero_row=True)
        wt = frames.conv2d_pack_t(w, dt)
        assert wt.shape == (3, 3, cin, cout) and torch.equal(wt, RB.pack_weight_t(w.double()).to(dt))
        _, _, ref = RB.conv_grads(xp.double(), w.to(dt).double(), b.double(), dy[:M].double(), N, H, W, k, 3)
        dx = frames.conv2d_dgrad(dy, wt, N, H, W)
        assert dx.shape == (N * H * W, cin) and dx.dtype == dt
        bound = 1e-4 if compute == "fp32" else 2 * _rel(R.bf16(ref), ref) + 1e-6
        assert _rel(dx, ref) <= bound, (N, H, W, _rel(dx, ref), bound)
        assert torch.equal(frames.conv2d_dgrad(dy, wt, N, H, W), dx)


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
@pytest.mark.parametrize("cin,cout", [(64, 128), (8, 64)])
def test_dgrad_reads_and_writes_nothing_outside_its_buffers(cin, cout, compute):
    for N, H, W in [(3, 5, 7), (2, 6, 8)]:                                # odd and even sizes: the zero row is read at the far edges
        xp, w, b = _conv_case(3, cin, cout, N, H, W, compute, seed=5)
        M, dy = _dy_case(3, cout, N, H, W, compute, zero_row=True)
        wt = frames.conv2d_pack_t(w, _dt(compute))
        clean = frames.conv2d_dgrad(dy, wt, N, H, W)
        big_dy, in_dy = _banded(dy)
        big_wt, in_wt = _banded(wt)
        dx = frames.conv2d_dgrad(in_dy, in_wt, N, H, W)
        assert bool(torch.isfinite(dx).all()) and torch.equal(dx, clean)
        assert _bands_intact(big_dy, dy.numel()) and _bands_intact(big_wt, wt.numel())
        big_dx, out_dx = _banded(torch.zeros_like(clean))
        a = frames._lib.Conv2dDgradArgs()
        a.dy, a.wt, a.dx = dy.data_ptr(), wt.data_ptr(), out_dx.data_ptr()
        a.N, a.H, a.W, a.Cin, a.Cout, a.k, a.act_f32, a.stream = N, H, W, cin, cout, 3, int(compute == "fp32"), frames._lib.current_stream()
        frames._lib.check(frames._lib.load().mmdeer_conv2d_dgrad(C.byref(a)))
        assert torch.equal(out_dx, clean) and _bands_intact(big_dx, clean.numel())


# ------------------------------------------------------------------------------------------------ the module
def _trainable(i, compute, config=None):
    """The module of gradient case i with its fill, in the case's modes, the frames and the loss weights"""
    idx, B, T, H, W, bb_train = GRAD_CASES[i]
    m = _filled(tag_of(B, T, H, W), compute, True, {"train_backbone": True, **(config or {})})
    m.spatial_backbone.train(bb_train)
    x = torch.from_numpy(R.frames_input(940 + idx, B, T, H, W)).to(DEV)
    return m, x, torch.from_numpy(loss_weight(idx, B)).to(DEV)


def _backbone_grads(m):
    return {n: (None if p.grad is None else p.grad.clone()) for n, p in m.named_parameters() if n.startswith("spatial_backbone.")}


@pytest.mark.parametrize("i", range(len(GRAD_CASES)))
def test_golden_gradients_fp32(i):
    """Against the reference's capture, by the rule of test_oracle_golden.check_side_grads at rtol 3e-3, atol_frac 3e-3: every
    element within rtol |ref| + atol_frac max|ref|; for a tensor stored as a slice, the same slice, the norm and the largest
    magnitude.  The conv biases under batch statistics are analytically zero: noise of at most 1e-4 max|dW| on both sides."""
    idx, B, T, H, W, bb_train = GRAD_CASES[i]
    g, tag = np.load(GRAD_GOLDEN), tag_of(B, T, H, W)
    m, x, w = _trainable(i, "fp32")
    y = m(x)
    assert y.requires_grad
    (y * w).sum().backward()
    np.testing.assert_allclose(y.detach().cpu().numpy(), g[f"{tag}.out"], rtol=1e-3, atol=2e-5)
    grads, seen = _backbone_grads(m), 0
    for key in g:
        if not key.startswith(tag + ".") or key == f"{tag}.out":
            continue
        kind, _, name = key[len(tag) + 1:].partition(".")
        got = grads[name].double().cpu().numpy()
        if kind == "grad":
            np.testing.assert_allclose(got, g[key], rtol=3e-3, atol=3e-3 * float(np.abs(g[key]).max()), err_msg=key)
        elif kind == "gradslice":
            top = float(g[f"{tag}.gradmax.{name}"])
            np.testing.assert_allclose(slice_of(got), g[key], rtol=3e-3, atol=3e-3 * top, err_msg=key)
            assert float(np.linalg.norm(got)) == pytest.approx(float(g[f"{tag}.gradnorm.{name}"]), rel=3e-3), key
            assert float(np.abs(got).max()) == pytest.approx(top, rel=3e-3), key
        elif kind == "gradnoise":
            wname = name[:-len("bias")] + "weight"
            ref_top = float(g[f"{tag}.gradmax.{wname}"]) if f"{tag}.gradmax.{wname}" in g else float(np.abs(g[f"{tag}.grad.{wname}"]).max())
            assert float(np.abs(g[key]).max()) <= 1e-4 * ref_top and float(np.abs(got).max()) <= 1e-4 * float(grads[wname].abs().max()), key
        else:
            continue
        seen += 1
    assert seen == 16, seen


@functools.lru_cache(maxsize=None)
def _restated_grads(i, emulate):
    idx, B, T, H, W, bb_train = GRAD_CASES[i]
    P = {k: v.to(DEV) for k, v in state64(tag_of(B, T, H, W)).items()}
    x = torch.from_numpy(R.frames_input(940 + idx, B, T, H, W)).double().to(DEV)
    w = torch.from_numpy(loss_weight(idx, B)).double().to(DEV)
    return RB.module_grads(P, x, w, bb_train, True, emulate_bf16=emulate, Cp1=8 if emulate else 4)[2]


@pytest.mark.parametrize("i", range(len(GRAD_CASES)))
def test_bf16_gradients_stay_near_the_emulation(i):
    """Coarse by construction: rounding flips ReLU masks and BatchNorm amplifies it, so the emulation itself sits 5 to 25 % from float64.
    Each gradient: within twice the emulation's own distance to float64 + 1e-3 (relative norm); the analytically-zero biases are
    left to the fp32 test.  The per-operator tests above carry the proof."""
    idx, B, T, H, W, bb_train = GRAD_CASES[i]
    m, x, w = _trainable(i, "bf16")
    (m(x) * w).sum().backward()
    f64, emu = _restated_grads(i, False), _restated_grads(i, True)
    for name, got in _backbone_grads(m).items():
        if bb_train and name in (f"{conv}.bias" for conv, _ in R.LAYERS):
            continue
        d, d_emu = _rel(got, f64[name]), _rel(emu[name], f64[name])
        print(f"{name}: bf16 {d:.3e} from float64, the emulation {d_emu:.3e}")
        assert d <= 2 * d_emu + 1e-3, (name, d, d_emu)


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_the_switch_changes_no_feature_and_the_old_path_runs_without_it(compute):
    idx, B, T, H, W, _ = GRAD_CASES[0]
    tag = tag_of(B, T, H, W)
    x = torch.from_numpy(R.frames_input(940 + idx, B, T, H, W)).to(DEV)
    assert not _filled(tag, compute, True).train_backbone             # the default
    for bb_train in (True, False):
        off, on = _filled(tag, compute, True), _filled(tag, compute, True, {"train_backbone": True})
        off.spatial_backbone.train(bb_train)
        on.spatial_backbone.train(bb_train)
        f_off, f_on = off.extract_spatial_features(x), on.extract_spatial_features(x)
        assert f_on.requires_grad and f_on.grad_fn is not None and not f_off.requires_grad
        assert torch.equal(f_on, f_off)                                   # the same launches: bit-equal
        assert all(torch.equal(a, b) for a, b in zip(on.state_dict().values(), off.state_dict().values()))     # the buffers moved alike
        before = {k: v.clone() for k, v in on.state_dict().items() if k in R.BUFFERS}
        with torch.no_grad():
            f_ng = on.extract_spatial_features(x)
        assert f_ng.grad_fn is None and not f_ng.requires_grad and torch.equal(f_ng, f_off)
        moved = [not torch.equal(on.state_dict()[k], before[k]) for k in R.BUFFERS]
        assert all(moved) if bb_train else not any(moved)                 # as before: also under no_grad, never in evaluation mode
        for p in on.spatial_backbone.parameters():
            p.requires_grad_(False)
        f_frozen = on.extract_spatial_features(x)
        assert f_frozen.grad_fn is None and torch.equal(f_frozen, f_off)
        y = on(x)                                                         # the head still trains on detached features
        y.sum().backward()
        assert all(p.grad is None for p in on.spatial_backbone.parameters()) and on.spatial_projection[0].weight.grad is not None
    on = _filled(tag, compute, True, {"train_backbone": True})
    with pytest.raises(ValueError, match="requires_grad"):
        on(x.clone().requires_grad_(True))                                # no gradient with respect to the frames


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_backward_is_deterministic_and_frozen_parameters_get_none(compute):
    m, x, w = _trainable(0, compute)
    (m(x) * w).sum().backward()
    first = _backbone_grads(m)
    assert all(v is not None and v.dtype == torch.float32 and bool(torch.isfinite(v).all()) for v in first.values()) and len(first) == 16
    m.zero_grad(set_to_none=True)
    (m(x) * w).sum().backward()
    second = _backbone_grads(m)
    assert all(torch.equal(first[k], second[k]) for k in first)
    # a partly frozen set: the first layer whole (the backward then stops above it) and one bias higher up
    frozen = {"spatial_backbone.0.weight", "spatial_backbone.0.bias", "spatial_backbone.1.weight", "spatial_backbone.1.bias", "spatial_backbone.7.bias"}
    m.zero_grad(set_to_none=True)
    for n, p in m.named_parameters():
        p.requires_grad_(n not in frozen)
    (m(x) * w).sum().backward()
    for n, v in _backbone_grads(m).items():
        assert (v is None) if n in frozen else torch.equal(v, first[n]), n


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_downstream_gradients_equal_the_parent_on_the_same_features(compute):
    B, T, H, W = 3, 4, 9, 11
    x = torch.from_numpy(R.frames_input(962, B, T, H, W)).to(DEV)
    m = _filled("frm2x3x19x23", compute, True, {"dropout": 0.3, "dropout_seed": 5, "train_backbone": True})
    m.spatial_backbone.eval()
    parent = video.TemporalVideoEncoder({"dropout": 0.3, "dropout_seed": 5}, compute_dtype=compute).to(DEV).train()
    parent.load_state_dict(m.state_dict(), strict=True)
    w = torch.randn(B, 512, device=DEV, generator=torch.Generator(DEV).manual_seed(3))
    feats = m.extract_spatial_features(x)
    assert feats.requires_grad
    (m(x) * w).sum().backward()
    (parent(feats.detach()) * w).sum().backward()
    pg = dict(parent.named_parameters())
    for n, p in m.named_parameters():
        if n.startswith("spatial_backbone."):
            assert p.grad is not None and float(p.grad.abs().max()) > 0, n
        else:
            assert p.grad is not None and torch.equal(p.grad, pg[n].grad), n


def test_sgd_steps_on_the_backbone_lower_a_fixed_loss():
    """fp32, batch statistics, dropout 0: the loss is a fixed function of the backbone's parameters, and a small step against the
    gradient lowers it to first order."""
    m, x, w = _trainable(0, "fp32")
    target = torch.from_numpy(synth.normal(990, w.numel()).reshape(w.shape).astype(np.float32)).to(DEV)
    opt = torch.optim.SGD(m.spatial_backbone.parameters(), lr=1e-3)
    losses = []
    for _ in range(4):
        opt.zero_grad(set_to_none=True)
        loss = ((m(x) - target) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print("losses", losses)
    assert losses[-1] < losses[0] and all(np.isfinite(losses))
