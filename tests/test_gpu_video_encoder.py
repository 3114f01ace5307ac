"""The temporal video encoder (mmdeer.video) on the GPU: the convolution-over-time and BatchNorm operators against the float64
restatement (tests/video_ref.py), the whole encoder against the golden vectors captured from the reference
(tests/golden/video_seq.npz), edges, training and HIP-graph capture."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from mmdeer import _lib, frames, fusions, video

from . import video_ref as R
from .test_oracle_golden import check_side_grads

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "video_seq.npz")
CASES = [(9, 2, False), (3, 17, False), (4, 1, False), (5, 5, True), (2, 17, True)]
NOISE_BIASES = ("temporal_cnn.0.bias", "temporal_cnn.4.bias")
ZERO_BIAS = "temporal_attention.2.bias"
BUFFERS = [f"{l}.{k}" for l in R.BN_LAYERS for k in ("running_mean", "running_var", "num_batches_tracked")]
W = 512


def _dt(compute):
    return torch.float32 if compute == "fp32" else torch.bfloat16


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _filled(tag, compute, train, config=None):
    m = video.TemporalVideoEncoder({"dropout": 0.0, **(config or {})}, compute_dtype=compute)
    sd = R.filled_state(tag, {k: tuple(v.shape) for k, v in m.state_dict().items()})
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return m.to(DEV).train(train)


# ------------------------------------------------------------------------------------------------ the convolution operator
# (1, 2): a one-row shift, every row a sequence end; (5, 1): only the centre tap lives; (37, 7): 259 rows, a ragged last tile;
# (130, 3): the shift exceeds a 128-row tile, so a whole tile reads only padding in one tap.  tile 0 / 2: 64 x 64 / 128 x 128.
CONV_SHAPES = [(1, 2), (1, 33), (5, 1), (37, 7), (130, 3)]


def _conv_inputs(B, T, compute):
    gen = torch.Generator().manual_seed(1000 * T + B)
    dt = _dt(compute)
    x = torch.randn(T * B, W, generator=gen).to(dt).to(DEV)
    gout = torch.randn(T * B, W, generator=gen).to(dt).to(DEV)
    w = (torch.randn(W, W, 3, generator=gen) * 0.03).to(DEV)
    b = (torch.randn(W, generator=gen) * 0.1).to(DEV)
    return x, gout, w, b


def _conv_hip(x, gout, w, b, B, T, compute, tile):
    dt = _dt(compute)
    xp, dyp = video.padded(T, B, dt, DEV), video.padded(T, B, dt, DEV)
    video.interior(xp, B).copy_(x)
    video.interior(dyp, B).copy_(gout)
    img, img_t = video.conv3_pack(w, dt, True)
    y = video.conv3_time(xp, img, b, T, B, tile=tile)
    dx = video.conv3_time(dyp, img_t, None, T, B, tile=tile)
    gw, gb = video.conv3_dw(dyp, xp, T, B, compute)
    return {"y": y.float(), "dx": dx.float(), "dw": gw, "db": gb}, img, img_t


def _conv_ref(x, gout, w, b, B, T, emulate):
    x64, w64, b64 = (t.double().clone().requires_grad_(True) for t in (x, w, b))
    y = R.conv3_time(R.pad_time(x64, B), w64, b64, T, B, emulate_bf16=emulate)
    (y * gout.double()).sum().backward()
    return {"y": y.detach(), "dx": x64.grad, "dw": w64.grad, "db": b64.grad}


@pytest.mark.parametrize("tile", [0, 2])
@pytest.mark.parametrize("compute", ["fp32", "bf16"])
@pytest.mark.parametrize("B,T", CONV_SHAPES)
def test_conv_operator_matches_float64(B, T, compute, tile):
    x, gout, w, b = _conv_inputs(B, T, compute)
    hip, img, img_t = _conv_hip(x, gout, w, b, B, T, compute, tile)
    dt = _dt(compute)
    assert torch.equal(img, w.permute(2, 0, 1).to(dt)) and torch.equal(img_t, w.flip(2).permute(2, 1, 0).to(dt))
    r64 = _conv_ref(x, gout, w, b, B, T, False)
    if compute == "fp32":
        for k, v in r64.items():
            assert _rel(hip[k], v) <= 1e-4, (k, _rel(hip[k], v))
    else:
        emu = _conv_ref(x, gout, w, b, B, T, True)
        for k, v in r64.items():
            assert _rel(hip[k], v) <= 2 * _rel(emu[k], v) + 1e-6, (k, _rel(hip[k], v), _rel(emu[k], v))


@pytest.mark.parametrize("tile", [0, 2])
def test_conv_operator_reads_nothing_outside_the_padded_buffer(tile):
    """The padded buffer sits between NaN rows: a row outside its (T + 2) * B rows that reached a stored output would show."""
    B, T, guard = 37, 7, 256
    x, _, w, b = _conv_inputs(B, T, "fp32")
    big = torch.full((guard + (T + 2) * B + guard, W), float("nan"), device=DEV)
    xp = big[guard:guard + (T + 2) * B]
    xp.zero_()
    video.interior(xp, B).copy_(x)
    img, _ = video.conv3_pack(w, torch.float32, False)
    y = video.conv3_time(xp, img, b, T, B, tile=tile)
    assert torch.isfinite(y).all()
    clean = video.padded(T, B, torch.float32, DEV)
    video.interior(clean, B).copy_(x)
    assert torch.equal(y, video.conv3_time(clean, img, b, T, B, tile=tile))
    assert torch.isnan(big[:guard]).all() and torch.isnan(big[guard + (T + 2) * B:]).all()


def test_conv_operator_empty():
    a = _lib.Conv3TimeArgs()
    a.T, a.B, a.C, a.N, a.act_f32, a.tile, a.stream = 4, 0, 512, 512, 1, -1, _lib.current_stream()
    assert _lib.load().mmdeer_conv3_time(C.byref(a)) == 0


# ------------------------------------------------------------------------------------------------ the BatchNorm operators
def _bn_inputs(Rn, compute, seed=0):
    gen = torch.Generator().manual_seed(77 * Rn + seed)
    dt = _dt(compute)
    x = (torch.randn(Rn, W, generator=gen) * (0.5 + torch.rand(W, generator=gen)) + torch.randn(W, generator=gen)).to(dt).to(DEV)
    gamma = (1 + 0.2 * torch.randn(W, generator=gen)).to(DEV)
    beta = (0.3 * torch.randn(W, generator=gen)).to(DEV)
    dout = torch.randn(Rn, W, generator=gen).to(dt).to(DEV)
    return x, gamma, beta, dout


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
@pytest.mark.parametrize("Rn", [2, 390, 1221, 33001])        # 33001: beyond 1024 blocks of 32 rows, the row blocks grow (34 rows here)
def test_batchnorm_operators_match_float64(Rn, compute):
    """Bounds.  Statistics, dgamma, dbeta are fp32 results of x / dout as stored, in both dtypes: 1e-5 of their norm for the statistics
    (a few fp32 ulps through Welford + Chan), 1e-4 for the two gradient sums (R signed terms each).  `out` and `dx` are stored in the
    activation dtype.  `out`: fp32 1e-5; bf16 twice the distance of the restatement's own bf16 emulation (+ 1e-6), the project's rule.
    `dx`: fp32 1e-5; bf16 one rounding of the stored value, 2^-9 per element, bound 2^-8.  dx under batch statistics is a
    difference of three terms that cancel (completely at R = 2, up to eps), so its error is measured against the norm of the
    uncancelled term gamma rstd g, not against dx itself."""
    x, gamma, beta, dout = _bn_inputs(Rn, compute)
    dt = _dt(compute)
    store = 1e-5 if compute == "fp32" else 2.0 ** -8
    x64, g64, b64 = x.double().clone().requires_grad_(True), gamma.double().clone().requires_grad_(True), beta.double().clone().requires_grad_(True)
    # ---- statistics and the running-buffer update (nn.BatchNorm1d in float64 on the CPU)
    bn = torch.nn.BatchNorm1d(W)
    with torch.no_grad():
        bn.running_mean.copy_(torch.linspace(-1, 1, W)); bn.running_var.copy_(torch.linspace(0.5, 2, W)); bn.num_batches_tracked.fill_(41)
    bn64 = torch.nn.BatchNorm1d(W).double().train()
    bn64.load_state_dict(bn.state_dict())
    bn = bn.to(DEV)
    mean, rstd = video.bn_stats(x, compute, bn)
    bn64(x.double().cpu())
    assert _rel(mean, x64.mean(0)) <= 1e-5 and _rel(rstd, 1 / torch.sqrt(x64.var(0, unbiased=False) + R.EPS)) <= 1e-5
    np.testing.assert_allclose(bn.running_mean.cpu().numpy(), bn64.running_mean.numpy(), rtol=1e-5, atol=1.2e-7)
    np.testing.assert_allclose(bn.running_var.cpu().numpy(), bn64.running_var.numpy(), rtol=1e-5, atol=1.2e-7)
    assert int(bn.num_batches_tracked) == int(bn64.num_batches_tracked) == 42
    m2, r2 = video.bn_stats(x, compute)                                    # without buffers: the same statistics, nothing else moves
    assert torch.equal(m2, mean) and torch.equal(r2, rstd) and int(bn.num_batches_tracked) == 42
    # ---- apply and backward with batch statistics
    out = video.bn_apply(x, mean, rstd, gamma, beta, torch.empty_like(x), compute)
    o64, _, _ = R.batchnorm_rows(x64, g64, b64)
    emu, _, _ = R.batchnorm_rows(x64, g64, b64, emulate_bf16=True)
    assert _rel(out, o64) <= (1e-5 if compute == "fp32" else 2 * _rel(emu, o64) + 1e-6), _rel(out, o64)
    dx, dg, db = video.bn_bwd(dout, out, x, mean, rstd, gamma, torch.empty_like(x), compute)
    mask = (out.double() > 0).double()                 # the kernel's own mask: an element rounded to zero in bf16 carries no gradient
    o64m = (x64 - x64.mean(0)) / torch.sqrt(x64.var(0, unbiased=False) + R.EPS) * g64 + b64
    (o64m * mask * dout.double()).sum().backward()
    term = (gamma.double() / torch.sqrt(x64.detach().var(0, unbiased=False) + R.EPS) * mask * dout.double()).norm()
    assert float((dx.double() - x64.grad).norm()) <= (1e-5 * float(term) + (0 if compute == "fp32" else 2.0 ** -8 * float(x64.grad.norm())))
    assert _rel(dg, g64.grad) <= 1e-4 and _rel(db, b64.grad) <= 1e-4
    # ---- apply and backward with running statistics (evaluation mode): the statistics are constants
    rm, rv = torch.linspace(-1, 1, W, device=DEV), torch.linspace(0.5, 2, W, device=DEV)
    out = video.bn_apply(x, rm, rv, gamma, beta, torch.empty_like(x), compute, running=True)
    x64, g64, b64 = (t.detach().clone().requires_grad_(True) for t in (x64, g64, b64))
    o64, _, _ = R.batchnorm_rows(x64, g64, b64, rm.double(), rv.double(), relu=False)
    emu, _, _ = R.batchnorm_rows(x64, g64, b64, rm.double(), rv.double(), emulate_bf16=True)
    assert _rel(out, torch.relu(o64)) <= (1e-5 if compute == "fp32" else 2 * _rel(emu, torch.relu(o64)) + 1e-6)
    dx, dg, db = video.bn_bwd(dout, out, x, rm, rv, gamma, torch.empty_like(x), compute, running=True, mask_scale=1.25)
    (o64 * (out.double() > 0) * dout.double() * 1.25).sum().backward()
    assert _rel(dx, x64.grad) <= store and _rel(dg, g64.grad) <= 1e-4 and _rel(db, b64.grad) <= 1e-4
    assert dx.dtype == dt


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
@pytest.mark.parametrize("Rn", [2, 390, 33001])       # one row per parity; a ragged last block; the row blocks grow
def test_batchnorm_statistics_are_the_frame_encoders_bit_for_bit(Rn, compute):
    """mmdeer_bn_time_stats and mmdeer_bn2d_stats are one pair of kernels (csrc/bn_rows.h): on the same [R][512] matrix, taken by
    the second as one frame of R x 1 positions, they store the same bits in mean, rstd and the running buffers."""
    x = _bn_inputs(Rn, compute)[0]
    bns = []
    for _ in range(2):
        bn = torch.nn.BatchNorm1d(W)
        with torch.no_grad():
            bn.running_mean.copy_(torch.linspace(-1, 1, W)); bn.running_var.copy_(torch.linspace(0.5, 2, W)); bn.num_batches_tracked.fill_(41)
        bns.append(bn.to(DEV))
    got = (video.bn_stats(x, compute, bns[0]), frames.bn2d_stats(x, 1, Rn, 1, bns[1]))
    for (m, r), bn in zip(got, bns):
        assert torch.isfinite(m).all() and torch.isfinite(r).all() and int(bn.num_batches_tracked) == 42
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])
    assert torch.equal(bns[0].running_mean, bns[1].running_mean) and torch.equal(bns[0].running_var, bns[1].running_var)
    assert torch.equal(bns[0].num_batches_tracked, bns[1].num_batches_tracked)


@pytest.mark.parametrize("Rn", [390, 1221])
def test_batchnorm_statistics_of_an_offset_and_a_constant_channel(Rn):
    """Channel 0 = 100 + 0.05 n: (sum x, sum x^2) in fp32 loses the variance (off by >= 9e-2, negative at R = 390); block-wise Welford
    merged by Chan's formula is within 1e-5.  Channels 1 and 2 are constant: x - mean is an exact zero, the output relu(beta) exactly."""
    x, gamma, beta, _ = _bn_inputs(Rn, "fp32", seed=1)
    x[:, 0] = 100 + 0.05 * torch.arange(Rn, device=DEV)
    x[:, 1], x[:, 2] = 3.25, -7.125
    beta[1], beta[2] = 0.37, -0.2
    mean, rstd = video.bn_stats(x, "fp32")
    ref = 1 / torch.sqrt(x[:, 0].double().var(unbiased=False) + R.EPS)
    assert abs(float(rstd[0]) - float(ref)) <= 1e-3 * float(ref)
    assert float(mean[1]) == 3.25 and float(mean[2]) == -7.125
    out = video.bn_apply(x, mean, rstd, gamma, beta, torch.empty_like(x), "fp32")
    assert torch.equal(out[:, 1], torch.full((Rn,), 0.37, device=DEV)) and torch.equal(out[:, 2], torch.zeros(Rn, device=DEV))


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_batchnorm_dropout_is_the_librarys_mask(compute):
    """Without the ReLU (almost) every element is non-zero, so the zeros of the output are the mask, element for element."""
    B, T, site, p, seed, step = 37, 7, 145, 0.3, 11, 5
    Rn = B * T
    x, gamma, beta, _ = _bn_inputs(Rn, compute, seed=2)
    mean, rstd = video.bn_stats(x, compute)
    plain = video.bn_apply(x, mean, rstd, gamma, beta, torch.empty_like(x), compute, relu=False)
    buf = video.padded(T, B, _dt(compute), DEV)                            # into the interior of a padded buffer
    out = video.bn_apply(x, mean, rstd, gamma, beta, video.interior(buf, B), compute, relu=False, drop=(p, seed, step), site=site)
    keep = torch.empty(Rn, W, dtype=torch.uint8, device=DEV)
    _lib.check(_lib.load().mmdeer_dropout_mask(site, Rn, W, p, seed, step, keep.data_ptr(), _lib.current_stream()))
    live = plain != 0
    assert float(live.float().mean()) > 0.99 and 0.65 < float(keep.float().mean()) < 0.75
    assert torch.equal((out != 0) & live, keep.bool() & live)
    scale = torch.tensor(1.0 / (1.0 - float(np.float32(p))), dtype=torch.float32, device=DEV)
    want = plain.float() * scale * keep.float()
    if compute == "fp32":
        assert torch.equal(out, want)
    else:            # `plain` is already rounded to bf16 and `out` rounds the scaled fp32 value once: two roundings of 2^-9 apart
        assert float(((out.float() - want).abs() - 2.0 ** -7 * want.abs()).max()) <= 0
    assert not buf[:B].any() and not buf[(T + 1) * B:].any()               # the pad rows stay zero
    # a device counter is added to the step (HIP-graph replays): step 2 + counter 3 = step 5
    counter = torch.tensor([3], dtype=torch.int64, device=DEV)
    out2 = video.bn_apply(x, mean, rstd, gamma, beta, torch.empty_like(x), compute, relu=False, drop=(p, seed, 2, counter), site=site)
    assert torch.equal(out2, out)


# ------------------------------------------------------------------------------------------------ golden (reference capture)
# tests/golden/make_golden_video.py prints the distance of the fp32 capture to the float64 restatement: outputs <= 3.5e-6 absolute,
# gradients <= 1.9e-6 of their largest element, buffers <= 1.3e-7 relative -- all below a third of the bounds here, which therefore
# stay the audio encoder's.
@pytest.mark.parametrize("B,T,train", CASES)
def test_golden_fp32_outputs_gradients_and_buffers(B, T, train):
    g = np.load(GOLDEN)
    tag = f"vid{B}x{T}"
    m = _filled(tag, "fp32", train)
    before = {k: v.clone() for k, v in m.state_dict().items() if k in BUFFERS}
    x = torch.from_numpy(g[f"{tag}.input"].astype(np.float32)).to(DEV).requires_grad_(True)
    y = m(x)
    np.testing.assert_allclose(y.detach().cpu().numpy(), g[f"{tag}.out"], rtol=1e-3, atol=2e-5)
    (y * torch.from_numpy(g[f"{tag}.loss_w"]).to(DEV)).sum().backward()
    grads = {n: p.grad for n, p in m.named_parameters()}
    check_side_grads(g, tag, grads, {"video": x.grad}, rtol=3e-3, atol_frac=3e-3)
    after = m.state_dict()
    if T == 1:
        assert all(grads[n] is None for n in grads if n.startswith(("temporal_cnn.", "temporal_attention.")))
        assert all(torch.equal(after[k], before[k]) for k in BUFFERS)
        return
    assert float(grads[ZERO_BIAS].abs().max()) == 0.0                     # written as an exact zero (the reference's value is noise)
    if train:
        for n in NOISE_BIASES:      # analytically zero under batch statistics: rounding noise in the reference and here
            wmax = float(grads[n.replace("bias", "weight")].abs().max())
            assert float(np.abs(g[f"{tag}.gradnoise.{n}"]).max()) <= 1e-4 * wmax and float(grads[n].abs().max()) <= 1e-4 * wmax, n
        for k in BUFFERS:
            if k.endswith("num_batches_tracked"):
                assert int(after[k]) == int(g[f"{tag}.buffer.{k}"]) == 1
            else:   # atol: one fp32 ulp at 1.0, the scale of the values the buffers average (tests/test_cpu_video_encoder.py)
                np.testing.assert_allclose(after[k].cpu().numpy(), g[f"{tag}.buffer.{k}"], rtol=1e-5, atol=1.2e-7, err_msg=k)
    else:
        assert all(torch.equal(after[k], before[k]) for k in BUFFERS)


@pytest.mark.parametrize("B,T,train", CASES)
def test_golden_bf16_outputs_and_gradients_track_fp32(B, T, train):
    g = np.load(GOLDEN)
    tag = f"vid{B}x{T}"
    x = torch.from_numpy(g[f"{tag}.input"].astype(np.float32)).to(DEV)
    w = torch.from_numpy(g[f"{tag}.loss_w"]).to(DEV)
    res = {}
    for compute in ("fp32", "bf16"):
        m = _filled(tag, compute, train)
        y = m(x)
        if compute == "bf16":
            np.testing.assert_allclose(y.detach().cpu().numpy(), g[f"{tag}.out"], rtol=1e-1, atol=8e-2)   # the a14 bf16 tolerance
        (y * w).sum().backward()
        res[compute] = {n: p.grad.double().flatten() for n, p in m.named_parameters() if p.grad is not None}
    assert set(res["fp32"]) == set(res["bf16"])
    for n, a in res["fp32"].items():
        if n == ZERO_BIAS or (train and n in NOISE_BIASES):
            continue
        b = res["bf16"][n]
        assert float((a @ b) / (a.norm() * b.norm())) > 0.97, n


# ------------------------------------------------------------------------------------------------ edges
@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_one_frame_skips_the_temporal_path(compute):
    torch.manual_seed(3)
    m = video.TemporalVideoEncoder({"dropout": 0.0}, compute_dtype=compute).to(DEV).train()
    before = {k: v.clone() for k, v in m.state_dict().items() if k in BUFFERS}
    x = torch.randn(17, 512, device=DEV)
    y = m(x.unsqueeze(1))
    sp, op = m.spatial_projection, m.output_projection
    h = fusions.linear(x, sp[0], compute, relu=True)
    want = fusions._LinActLnFn.apply(h, op[0].weight, op[0].bias, op[3].weight, op[3].bias, compute, None, -1)
    assert torch.equal(y, want) and torch.equal(m(x), want)
    y.sum().backward()
    for n, p in m.named_parameters():
        assert (p.grad is None) == n.startswith(("spatial_backbone.", "temporal_cnn.", "temporal_attention.")), n
    assert all(torch.equal(m.state_dict()[k], before[k]) for k in BUFFERS)


def test_eval_is_deterministic_and_training_under_no_grad_moves_the_buffers():
    torch.manual_seed(4)
    m = video.TemporalVideoEncoder({"dropout": 0.0}).to(DEV)
    x = torch.randn(17, 6, 512, device=DEV)
    m.eval()
    with torch.no_grad():
        y0 = m(x)
        assert torch.equal(m(x), y0)
    assert int(m.temporal_cnn[1].num_batches_tracked) == 0
    m.train()
    rm = m.temporal_cnn[5].running_mean.clone()
    with torch.no_grad():
        y1 = m(x)                                                           # batch statistics, and the buffers move
    assert int(m.temporal_cnn[1].num_batches_tracked) == int(m.temporal_cnn[5].num_batches_tracked) == 1
    assert not torch.equal(m.temporal_cnn[5].running_mean, rm) and not torch.equal(y1, y0)
    m.eval()
    with torch.no_grad():
        assert not torch.equal(m(x), y0)                                    # evaluation now reads the moved buffers


def test_module_edges():
    m = video.TemporalVideoEncoder().to(DEV).eval()
    assert tuple(m(torch.zeros(0, 6, 512, device=DEV)).shape) == (0, 512)
    assert tuple(m(torch.zeros(0, 512, device=DEV)).shape) == (0, 512)
    for shape in ((2, 3, 8, 8), (2, 5, 3, 8, 8)):
        with pytest.raises(NotImplementedError):
            m(torch.zeros(*shape, device=DEV))
    with pytest.raises(RuntimeError):
        m(torch.randn(2, 5, 512))                                          # a CPU tensor: no fallback
    with pytest.raises(RuntimeError):
        video.TemporalVideoEncoder().eval()(torch.randn(2, 5, 512))


# ------------------------------------------------------------------------------------------------ training
def test_training_dropout_gradients_and_sgd():
    torch.manual_seed(5)
    m = video.TemporalVideoEncoder({"dropout_seed": 11}, compute_dtype="fp32").to(DEV).train()
    x = torch.randn(64, 8, 512, device=DEV)
    target = torch.randn(64, 512, device=DEV) * 0.5
    losses = []
    opt = torch.optim.SGD([p for n, p in m.named_parameters() if not n.startswith("spatial_backbone.")], lr=0.05)
    for it in range(10):
        opt.zero_grad()
        loss = (m(x) - target).square().mean()
        loss.backward()
        losses.append(float(loss.detach()))
        for n, p in m.named_parameters():
            if n.startswith("spatial_backbone."):
                assert p.grad is None, n
                continue
            assert p.grad is not None and torch.isfinite(p.grad).all(), n
            if n != ZERO_BIAS and n not in NOISE_BIASES:
                assert float(p.grad.abs().max()) > 0, n
        opt.step()
    assert losses[-1] < losses[0], losses
    assert int(m.temporal_cnn[1].num_batches_tracked) == int(m.temporal_cnn[5].num_batches_tracked) == 10
    with torch.no_grad():
        assert not torch.equal(m(x), m(x))          # the step counter moves the masks


# ------------------------------------------------------------------------------------------------ HIP graph capture
def _capture(step):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()                                        # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_graph_capture_replays_eager_in_eval(compute):
    torch.manual_seed(9)
    m = video.TemporalVideoEncoder(compute_dtype=compute).to(DEV).eval()
    x = torch.randn(64, 8, 512, device=DEV)
    w = torch.randn(64, 512, device=DEV)
    params = [p for n, p in m.named_parameters() if not n.startswith("spatial_backbone.")]

    def step():
        for p in params:
            p.grad = None
        y = m(x)
        (y * w).sum().backward()
        return y.detach().clone(), [p.grad.detach().clone() for p in params]

    y0, g0 = step()
    torch.cuda.synchronize()
    _capture(step)
    for p in params:
        p.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = m(x)
        (y * w).sum().backward()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, y0)
    for p, g in zip(params, g0):
        assert torch.equal(p.grad, g)


def test_graph_capture_keeps_updating_the_running_buffers():
    torch.manual_seed(10)
    eager = video.TemporalVideoEncoder({"dropout": 0.0}).to(DEV).train()
    m = video.TemporalVideoEncoder({"dropout": 0.0}).to(DEV).train()
    m.load_state_dict(eager.state_dict())
    x = torch.randn(64, 8, 512, device=DEV)
    with torch.no_grad():
        y_eager = [eager(x), eager(x)][1]
    state = {k: v.clone() for k, v in m.state_dict().items()}
    with torch.no_grad():
        _capture(lambda: m(x))
        m.load_state_dict(state)                      # the warm-up moved the buffers: back to the start
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            y = m(x)
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, y_eager)
    sd, se = m.state_dict(), eager.state_dict()
    for k in BUFFERS:
        assert torch.equal(sd[k], se[k]), k
    assert int(sd["temporal_cnn.5.num_batches_tracked"]) == 2
