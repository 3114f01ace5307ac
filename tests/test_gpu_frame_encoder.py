"""The frame video encoder on the GPU: the convolution, pack and BatchNorm2d operators against the float64 restatement
(tests/frames_ref.py) at their edges, reads outside the padded buffer, the golden cases captured from the reference
(tests/golden/frame_seq.npz), the module's modes, chunking, gradients and refusals, and HIP-graph capture."""
import functools
import os

import numpy as np
import pytest
import torch

from mmdeer import frames, video

from . import frames_ref as R
from .test_cpu_frame_encoder import CASES, restated, tag_of

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "frame_seq.npz")
# (k, Cin, Cout): the backbone's four layers, and a 3 x 3 layer whose tap row (K = 24) is no whole K-tile in either dtype -- the
# ragged form of the gathered loader, which the backbone's own widths never take
GEOMS = [(7, 3, 64), (3, 64, 128), (3, 128, 256), (3, 256, 512), (3, 8, 64)]
# (N, H, W) of the convolution's input: 1 x 1, 2 x 3, 5 x 7, 19 x 23 (M = 2 * 10 * 12 = 240: three 64-row tiles and a part, one 128-row
# tile and a part), and M = 3 * 120 = 360 (no multiple of 64, more than two 128-row tiles)
SIZES = [(2, 1, 1), (2, 2, 3), (2, 5, 7), (2, 19, 23), (3, 19, 23)]


def _dt(compute):
    return torch.float32 if compute == "fp32" else torch.bfloat16


def _rel(a, b):
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _cp(k, cin, compute):
    return frames.pixel_channels(cin, k, _dt(compute))


def _conv_case(k, cin, cout, N, H, W, compute, seed=0):
    """A convolution's operands as the kernel reads them: the padded buffer and the image in the activation dtype (the values are
    the ones stored, so float64 on them is the exact result), the bias, and the fp32 weight the image was packed from."""
    gen = torch.Generator().manual_seed(seed + 131 * k + 7 * cin + 1000 * H + W + N)
    dt, cp = _dt(compute), _cp(k, cin, compute)
    v = torch.randn(N, H, W, cin, generator=gen)
    w = torch.randn(cout, cin, k, k, generator=gen) / (cin * k * k) ** 0.5
    b = torch.randn(cout, generator=gen).to(DEV)
    xp = R.pad_pixels(v, k // 2, cp, slack=frames.taps(k) - k).to(dt).to(DEV)
    return xp, w.to(DEV), b


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
@pytest.mark.parametrize("k,cin,cout", GEOMS)
def test_conv_operator_matches_float64(k, cin, cout, compute):
    """fp32: relative norm 1e-4 (test_gpu_video_encoder.test_conv_operator_matches_float64's bound at a comparable K).  bf16: the
    operands are exact in float64, the stored output is rounded: twice the restatement's own bf16 emulation + 1e-6."""
    dt = _dt(compute)
    for N, H, W in SIZES:
        xp, w, b = _conv_case(k, cin, cout, N, H, W, compute)
        img = frames.conv2d_pack(w, dt)
        img64 = R.pack_weight(w.double(), xp.shape[1], frames.taps(k))
        assert torch.equal(img, img64.to(dt))                       # the image, element for element, against its index formula
        y64 = R.conv2d_s2(xp.double(), img.double(), b.double(), N, H, W, k)
        emu = R.conv2d_s2(xp.double(), img.double(), b.double(), N, H, W, k, emulate_bf16=True)
        bound = 1e-4 if compute == "fp32" else 2 * _rel(emu, y64) + 1e-6
        outs = [frames.conv2d_s2(xp, img, b, N, H, W, cin, tile=tile) for tile in (-1, 0, 2)]
        for y in outs:
            assert y.shape == y64.shape and _rel(y, y64) <= bound, (N, H, W, _rel(y, y64), bound)
        assert torch.equal(outs[0], outs[1])                        # the automatic choice at these sizes is the 64 x 64 tile
        y0, y064 = frames.conv2d_s2(xp, img, None, N, H, W, cin), R.conv2d_s2(xp.double(), img.double(), None, N, H, W, k)     # no bias
        emu0 = R.conv2d_s2(xp.double(), img.double(), None, N, H, W, k, emulate_bf16=True)
        assert _rel(y0, y064) <= (1e-4 if compute == "fp32" else 2 * _rel(emu0, y064) + 1e-6)


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_frames_pack_matches_its_index_formula(compute):
    dt = _dt(compute)
    for N, H, W in [(2, 1, 1), (3, 5, 7), (2, 19, 23)]:
        f = torch.randn(N, 3, H, W, generator=torch.Generator().manual_seed(H)).to(DEV)
        got = frames.frames_pack(f, dt)
        want = R.pack_frames(f.double(), 4 if compute == "fp32" else 8).to(dt)
        assert got.shape == want.shape and torch.equal(got, want)
        assert float(got[-1].abs().max()) == 0                       # the slack pixel


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
@pytest.mark.parametrize("k,cin,cout,tile", [(7, 3, 64, 0), (7, 3, 64, 2), (3, 64, 128, 0), (3, 64, 128, 2), (3, 8, 64, 0)])
def test_conv_reads_nothing_outside_its_buffer_into_an_output(k, cin, cout, tile, compute):
    """The padded buffer between NaN guard bands: the output is finite and equals the output on a clean buffer, the guards stay."""
    N, H, W = 3, 5, 7                                                # M = 3 * 3 * 4 = 36: every tile has rows beyond M
    xp, w, b = _conv_case(k, cin, cout, N, H, W, compute, seed=5)
    img = frames.conv2d_pack(w, _dt(compute))
    clean = frames.conv2d_s2(xp, img, b, N, H, W, cin, tile=tile)
    G = 4096
    big = torch.full((xp.numel() + 2 * G,), float("nan"), dtype=xp.dtype, device=DEV)
    big[G:G + xp.numel()] = xp.reshape(-1)
    inner = big[G:G + xp.numel()].view(xp.shape)
    assert inner.data_ptr() % 16 == 0
    y = frames.conv2d_s2(inner, img, b, N, H, W, cin, tile=tile)
    assert bool(torch.isfinite(y).all()) and torch.equal(y, clean)
    assert bool(torch.isnan(big[:G]).all()) and bool(torch.isnan(big[G + xp.numel():]).all())
    # the output between guards: nothing is written outside [M][Cout]
    out = torch.full((y.numel() + 2 * G,), float("nan"), dtype=y.dtype, device=DEV)
    a = frames._lib.Conv2dArgs()
    a.x, a.w, a.bias, a.y = xp.data_ptr(), img.data_ptr(), b.data_ptr(), out[G:].data_ptr()
    a.N, a.H, a.W, a.Cin, a.Cout, a.k, a.act_f32, a.tile, a.stream = N, H, W, cin, cout, k, int(compute == "fp32"), tile, frames._lib.current_stream()
    frames._lib.check(frames._lib.load().mmdeer_conv2d_s2(frames.C.byref(a)))
    assert torch.equal(out[G:G + y.numel()].view(y.shape), clean)
    assert bool(torch.isnan(out[:G]).all()) and bool(torch.isnan(out[G + y.numel():]).all())


def _bn_inputs(M, Cn, compute):
    gen = torch.Generator().manual_seed(77 * M + Cn)
    x = torch.randn(M, Cn, generator=gen) * (0.5 + torch.rand(Cn, generator=gen)) + torch.randn(Cn, generator=gen)
    x[:, 1] += 40.0                                                  # an offset of 40 spreads (see the test's docstring)
    x[:, 2] = 0.75                                                   # a constant channel
    gamma = (1 + 0.2 * torch.randn(Cn, generator=gen)).to(DEV)
    beta = (0.3 * torch.randn(Cn, generator=gen)).to(DEV)
    return x.to(_dt(compute)).to(DEV), gamma, beta


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
@pytest.mark.parametrize("Cn", [64, 128, 256, 512])
@pytest.mark.parametrize("N,H,W", [(2, 1, 1), (6, 5, 13), (1, 61, 541)])
def test_batchnorm_operators_match_float64(N, H, W, Cn, compute):
    """M = N H W = 2, 390, 33001 (more than 1024 row blocks' worth: blocks of 34 rows).  The bounds of
    test_gpu_video_encoder.test_batchnorm_operators_match_float64: statistics 1e-5 of their norm, buffers rtol 1e-5 / atol 1.2e-7,
    outputs 1e-5 in fp32 and twice the emulation's own distance + 1e-6 in bf16; the frame means are fp32 in both modes and take the
    fp32 bound.
    The offset channel.  mean is an fp32 vector of the ABI, so a channel of offset mu and spread sigma is normalised with an absolute
    error of k ulp(mu) / sigma, k a few units through Welford + Chan (about 30 to 100 roundings of the mean, half an ulp each, of
    either sign).  For that to stay inside 1e-5 of the output's norm at C = 64 (rms output about 0.5: 1e-5 * 8 * 0.5 = 4e-5) ulp(mu)
    must be about 5e-6 = 2^-18, mu in [32, 64): the offset is 40 spreads, not more.  A variance formed as E[x^2] - mean^2 in fp32
    is then off by about 1600 * eps * (1 .. sqrt(M)) against a spread of one, some 1e-4 and more, relative."""
    M = N * H * W
    x, gamma, beta = _bn_inputs(M, Cn, compute)
    y = x.reshape(M, Cn)
    bn = torch.nn.BatchNorm2d(Cn).to(DEV)
    with torch.no_grad():
        bn.running_mean.uniform_(-1, 1)
        bn.running_var.uniform_(0.5, 2)
    rm0, rv0 = bn.running_mean.double().clone(), bn.running_var.double().clone()
    mean, rstd = frames.bn2d_stats(y, N, H, W, bn)
    x64, g64, b64 = y.double(), gamma.double(), beta.double()
    m64, v64 = x64.mean(0), x64.var(0, unbiased=False)
    assert _rel(mean, m64) <= 1e-5 and _rel(rstd, 1 / torch.sqrt(v64 + R.EPS)) <= 1e-5
    assert float(rstd[2]) == pytest.approx(1 / R.EPS ** 0.5, rel=1e-6)           # the constant channel: variance exactly zero
    # the offset channel on its own (the norms above are carried by the constant channel's rstd = 316).  Welford's M2 is a sum of M
    # non-negative terms, each a few fp32 roundings of a difference of order one, and the rounding of the running mean cancels to first
    # order (the differences sum to zero): sqrt(M) eps = 2e-5 at M = 33001 for the variance, half of it for rstd.  1e-4 leaves a factor
    # of ten.
    assert abs(float(rstd[1]) * float(torch.sqrt(v64[1] + R.EPS)) - 1) <= 1e-4
    rm, rv, nbt = R.running_update(rm0, rv0, 0, m64, v64, M)
    np.testing.assert_allclose(bn.running_mean.cpu().numpy(), rm.cpu().numpy(), rtol=1e-5, atol=1.2e-7)
    np.testing.assert_allclose(bn.running_var.cpu().numpy(), rv.cpu().numpy(), rtol=1e-5, atol=1.2e-7)
    assert int(bn.num_batches_tracked) == nbt == 1
    mean2, rstd2 = frames.bn2d_stats(y, N, H, W)                                  # without buffers: the same statistics, nothing else moves
    assert torch.equal(mean2, mean) and torch.equal(rstd2, rstd) and int(bn.num_batches_tracked) == 1

    def check(out, want, rounded):
        want = want.to(out.device)
        if compute == "fp32" or not rounded:
            assert _rel(out, want) <= 1e-5, _rel(out, want)
        else:
            assert _rel(out, want) <= 2 * _rel(R.bf16(want), want) + 1e-6, _rel(out, want)

    v64_, _, _ = R.batchnorm_relu(x64, g64, b64)
    img = v64_.reshape(N, H, W, Cn).permute(0, 3, 1, 2)
    for running in (False, True):
        if running:                                                             # evaluation mode: the buffers, rstd formed per use
            mean, rstd = bn.running_mean, bn.running_var
            v64_, _, _ = R.batchnorm_relu(x64, g64, b64, mean.double(), rstd.double())
            img = v64_.reshape(N, H, W, Cn).permute(0, 3, 1, 2)
        pad = frames.bn2d_apply(y, N, H, W, mean, rstd, gamma, beta, frames.PAD, running=running)
        assert pad.shape == (N, H + 2, W + 2, Cn)
        check(pad[:, 1:-1, 1:-1], img.permute(0, 2, 3, 1), True)
        for border in (pad[:, 0], pad[:, -1], pad[:, :, 0], pad[:, :, -1]):
            assert float(border.float().abs().max()) == 0                        # exactly zero
        pooled = torch.nn.functional.max_pool2d(img, 3, 2, 1)                    # torch's float64 pool, -inf padded
        pool = frames.bn2d_apply(y, N, H, W, mean, rstd, gamma, beta, frames.POOL, running=running)
        assert pool.shape == (N, pooled.shape[2] + 2, pooled.shape[3] + 2, Cn)
        check(pool[:, 1:-1, 1:-1], pooled.permute(0, 2, 3, 1), True)
        for border in (pool[:, 0], pool[:, -1], pool[:, :, 0], pool[:, :, -1]):
            assert float(border.float().abs().max()) == 0
        avg = frames.bn2d_apply(y, N, H, W, mean, rstd, gamma, beta, frames.AVG, running=running)
        assert avg.dtype == torch.float32 and avg.shape == (N, Cn)
        check(avg, img.mean((2, 3)), False)
        const = pad[:, 1:-1, 1:-1, 2].float()
        assert float((const - const[0, 0, 0]).abs().max()) == 0                  # the constant channel stays constant


# ------------------------------------------------------------------------------------------------ the module
def _filled(tag, compute, train, config=None):
    m = frames.FrameVideoEncoder({"dropout": 0.0, **(config or {})}, compute_dtype=compute)
    sd = R.filled_state(tag, {k: tuple(v.shape) for k, v in m.state_dict().items()})
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return m.to(DEV).train(train)


@functools.lru_cache(maxsize=None)
def _emulated_feats(i):
    """The restatement's bf16-emulating backbone on case i (evaluation and training alike), on the GPU in float64."""
    B, T, H, W, train, _ = CASES[i]
    sd = R.filled_state(tag_of(B, T, H, W), {k: tuple(v.shape) for k, v in frames.FrameVideoEncoder().state_dict().items()})
    P = {k: torch.from_numpy(v.astype(np.int64) if k.endswith("num_batches_tracked") else v).double().to(DEV) for k, v in sd.items()}
    x = torch.from_numpy(R.frames_input(940 + i, B, T, H, W)).double().to(DEV)
    return R.backbone(P, x.reshape(B * T, 3, H, W), train, emulate_bf16=True, Cp1=8)[0].reshape(B, T, 512).cpu()


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
@pytest.mark.parametrize("i", range(len(CASES)))
def test_golden_cases(i, compute):
    """fp32: features and outputs at the module tolerance of test_gpu_video_encoder (rtol 1e-3, atol 2e-5) against the reference's
    capture, the BatchNorm2d buffers at rtol 1e-5 / atol 1.2e-7.  bf16: the features within twice the emulation's own distance to
    float64 (+ 1e-6), the outputs at the existing bf16 module tolerance (rtol 1e-1, atol 8e-2)."""
    B, T, H, W, train, four_d = CASES[i]
    g, tag = np.load(GOLDEN), tag_of(B, T, H, W)
    m = _filled(tag, compute, train)
    x = torch.from_numpy(R.frames_input(940 + i, B, T, H, W)).to(DEV)
    before = {k: v.clone() for k, v in m.state_dict().items() if k in R.BUFFERS}
    feats = m.extract_spatial_features(x)
    assert feats.shape == (B, T, 512) and feats.dtype == torch.float32 and not feats.requires_grad
    if train:                                                       # the second pass below must see the same buffers as the first
        m.load_state_dict({**m.state_dict(), **before})
    with torch.no_grad():
        y = m(x[:, 0] if four_d else x)
    assert y.shape == (B, 512) and y.dtype == torch.float32
    if compute == "fp32":
        np.testing.assert_allclose(feats.cpu().numpy(), g[f"{tag}.feats"], rtol=1e-3, atol=2e-5)
        np.testing.assert_allclose(y.cpu().numpy(), g[f"{tag}.out"], rtol=1e-3, atol=2e-5)
    else:
        f64 = restated(i)[0]
        d_emu, d = _rel(_emulated_feats(i), f64), _rel(feats, f64)
        print(f"{tag}: bf16 features {d:.3e} from float64, the emulation {d_emu:.3e}")
        assert d <= 2 * d_emu + 1e-6, (d, d_emu)
        np.testing.assert_allclose(y.cpu().numpy(), g[f"{tag}.out"], rtol=1e-1, atol=8e-2)
    after = m.state_dict()
    for k in R.BUFFERS:
        if not train:
            assert torch.equal(after[k], before[k]), k
        elif k.endswith("num_batches_tracked"):
            assert int(after[k]) == int(g[f"{tag}.buffer.{k}"]) == 1
        elif compute == "fp32":
            np.testing.assert_allclose(after[k].cpu().numpy(), g[f"{tag}.buffer.{k}"], rtol=1e-5, atol=1.2e-7, err_msg=k)


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_evaluation_is_deterministic_and_chunking_agrees(compute):
    B, T, H, W = 3, 3, 19, 23
    x = torch.from_numpy(R.frames_input(960, B, T, H, W)).to(DEV)
    m = _filled("frm2x3x19x23", compute, False)
    f0 = m.extract_spatial_features(x)
    assert torch.equal(m.extract_spatial_features(x), f0) and torch.equal(m(x), m(x))
    m.frame_chunk = 1
    f1 = m.extract_spatial_features(x)
    m.frame_chunk = 4                                                # 9 frames: chunks of 4, 4 and 1
    f4 = m.extract_spatial_features(x)
    # a frame's features do not depend on its chunk: the same sums in the same order, whichever tile its rows land in
    # (the fp32 operator bound, in both dtypes)
    assert _rel(f1, f0) <= 1e-4 and _rel(f4, f0) <= 1e-4, (_rel(f1, f0), _rel(f4, f0))


def test_training_moves_the_backbone_buffers_and_a_frozen_backbone_keeps_them():
    B, T, H, W = 3, 2, 9, 11
    x = torch.from_numpy(R.frames_input(961, B, T, H, W)).to(DEV)
    m = _filled("frm5x5x16x16", "fp32", True)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    with torch.no_grad():
        y_train = m(x)
    after = {k: v.clone() for k, v in m.state_dict().items()}
    for k in R.BUFFERS:
        assert not torch.equal(after[k], before[k]), k               # also under no_grad
    assert all(int(after[k]) == 1 for k in R.BUFFERS if k.endswith("num_batches_tracked"))
    m.spatial_backbone.eval()                                        # frozen statistics under a training head
    assert m.training and not m.spatial_backbone.training
    y_frozen = m(x)
    now = m.state_dict()
    for k in R.BUFFERS:
        assert torch.equal(now[k], after[k]), k
    assert int(now["temporal_cnn.1.num_batches_tracked"]) == 2       # the head still trains
    assert not torch.equal(y_frozen, y_train)
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        _filled("frm5x5x16x16", "fp32", True)(x[:1, :1, :, :2, :2])


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_downstream_gradients_equal_the_parent_on_the_same_features(compute):
    B, T, H, W = 3, 4, 9, 11
    x = torch.from_numpy(R.frames_input(962, B, T, H, W)).to(DEV)
    m = _filled("frm2x3x19x23", compute, True, {"dropout": 0.3, "dropout_seed": 5})
    m.spatial_backbone.eval()
    parent = video.TemporalVideoEncoder({"dropout": 0.3, "dropout_seed": 5}, compute_dtype=compute).to(DEV).train()
    parent.load_state_dict(m.state_dict(), strict=True)
    w = torch.randn(B, 512, device=DEV, generator=torch.Generator(DEV).manual_seed(3))
    feats = m.extract_spatial_features(x)
    (m(x) * w).sum().backward()
    (parent(feats) * w).sum().backward()
    pg = dict(parent.named_parameters())
    for n, p in m.named_parameters():
        if n.startswith("spatial_backbone."):
            assert p.grad is None, n
        else:
            assert p.grad is not None and torch.equal(p.grad, pg[n].grad), n
    with pytest.raises(ValueError, match="requires_grad"):
        m(x.clone().requires_grad_(True))


def test_empty_batch_feature_inputs_and_refusals():
    m = _filled("frm2x3x19x23", "fp32", False)
    assert m(torch.zeros(0, 2, 3, 8, 8, device=DEV)).shape == (0, 512)
    assert m(torch.zeros(0, 3, 8, 8, device=DEV)).shape == (0, 512)
    assert m.extract_spatial_features(torch.zeros(0, 2, 3, 8, 8, device=DEV)).shape == (0, 2, 512)
    parent = video.TemporalVideoEncoder({"dropout": 0.0}).to(DEV).eval()
    parent.load_state_dict(m.state_dict(), strict=True)
    f = torch.randn(3, 4, 512, device=DEV, generator=torch.Generator(DEV).manual_seed(4))
    assert torch.equal(m(f), parent(f)) and torch.equal(m(f[:, 0]), parent(f[:, 0]))         # features go to the parent unchanged
    z = torch.zeros(1, device=DEV)
    for shape in ((2, 5, 4, 8, 8), (2, 1, 8, 8), (2, 3, 224, 224, 7), (2, 0, 3, 8, 8), (1, 256, 3, 2000, 2000)):
        with pytest.raises(ValueError):
            m(z.expand(*shape))
    # integer and half-precision frames are taken as their fp32 values
    x = torch.randint(0, 255, (2, 2, 3, 8, 8), device=DEV, dtype=torch.uint8)
    assert torch.equal(m(x), m(x.float()))


# ------------------------------------------------------------------------------------------------ HIP graph capture
@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_graph_capture_replays_eager_in_eval(compute):
    B, T, H, W = 2, 3, 19, 23
    m = _filled("frm2x3x19x23", compute, False)
    x = torch.from_numpy(R.frames_input(963, B, T, H, W)).to(DEV)
    with torch.no_grad():
        y0 = m(x).clone()
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            m(x)                                                     # warm-up on a side stream
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            y = m(x)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, y0)
        x.copy_(torch.from_numpy(R.frames_input(964, B, T, H, W)).to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, m(x)) and not torch.equal(y, y0)
