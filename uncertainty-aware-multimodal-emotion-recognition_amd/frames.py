"""Frame video encoder: ``encoders.EnhancedVideoEncoder`` (reference src/models/encoders.py:392-550) from frames, the Conv2d backbone
included: (B, T, 3, H, W) or (B, 3, H, W) -> (B, 512) fp32.

``FrameVideoEncoder`` is ``video.TemporalVideoEncoder`` with its ``spatial_backbone`` run on HIP -- forward only by default, with
its backward as well under ``config['train_backbone']`` (include/mmdeer_frames_bwd.h; the operators are at the end of this list):
``extract_spatial_features`` turns frames into the (B, T, 512) per-frame features that the parent's forward takes.  The backbone is
Conv2d(3, 64, 7, 2, 3) -> BatchNorm2d -> ReLU -> MaxPool2d(3, 2, 1) -> three times Conv2d(C, 2 C, 3, 2, 1) -> BatchNorm2d -> ReLU ->
AdaptiveAvgPool2d(1).

Activations are channels-last rows, one per (n, h, w).  One that feeds a convolution lives in a padded buffer with a zero border
(include/mmdeer_frames.h), so a stride-2 convolution is one implicit-GEMM launch (``mmdeer_conv2d_s2``: one K loop per kernel row
over gathered rows of the buffer, into the same accumulators); BatchNorm2d is ``mmdeer_bn2d_stats`` (Welford partials merged by
Chan's formula, deterministic; the running buffers are updated on the device) and ``mmdeer_bn2d_apply``, which writes the next
convolution's whole padded buffer, border included -- after the max pool in layer 1 -- or, in layer 4, the average over the frame.
Per forward: one pack of the frames, and per layer one weight pack, one convolution and two or three BatchNorm launches.  Torch
does only the fp32 cast of the input and the allocations.  No CPU path: CPU tensors raise."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import torch

from . import _lib, ops
from .video import TemporalVideoEncoder

PAD, POOL, AVG = (_lib.FRAME_CONSTANTS[k] for k in ("BN2D_PAD", "BN2D_POOL", "BN2D_AVG"))
# the forms of the upstream gradient in the backward (include/mmdeer_frames_bwd.h): the mirrors of the three destinations
SRC_DENSE, SRC_POOL, SRC_AVG = (_lib.FRAME_BWD_CONSTANTS[k] for k in ("BN2D_SRC_DENSE", "BN2D_SRC_POOL", "BN2D_SRC_AVG"))
LIMIT = 1 << 31                 # elements of one buffer (include/mmdeer_frames.h)
# frames per backbone pass in evaluation mode: the conv1 output of a chunk of 224 x 224 frames, 112 * 112 * 64 elements a frame,
# stays under 1 GB in fp32 (256 * 3.2 MB = 822 MB)
DEFAULT_FRAME_CHUNK = 256
# (index of the Conv2d in spatial_backbone, of its BatchNorm2d, destination of the normalised output)
LAYERS = ((0, 1, POOL), (4, 5, PAD), (7, 8, PAD), (10, 11, AVG))


def conv_out(size: int, k: int) -> int:
    """Output size of a stride-2 convolution (or pool) of kernel k and padding k // 2."""
    return (size + 2 * (k // 2) - k) // 2 + 1


def pixel_channels(cin: int, k: int, dt) -> int:
    """Cp of the padded input buffer: one 16-byte chunk for the 7 x 7 layer, Cin for the others."""
    return (4 if dt == torch.float32 else 8) if k == 7 else cin


def taps(k: int) -> int:
    """KWe: pixels read per tap row (the 7 x 7 layer reads an eighth with zero weight)."""
    return 8 if k == 7 else k


def plan(n: int, H: int, W: int, dt):
    """The backbone's buffers for n frames of H x W: per layer (k, Cin, Cout, H, W of the conv's input, OH, OW, elements of its
    padded input buffer, slack included), from the header's rules."""
    out, cin, h, w = [], 3, H, W
    for i, cout in enumerate((64, 128, 256, 512)):
        k = 7 if i == 0 else 3
        oh, ow = conv_out(h, k), conv_out(w, k)
        cp = pixel_channels(cin, k, dt)
        out.append((k, cin, cout, h, w, oh, ow, (n * (h + 2 * (k // 2)) * (w + 2 * (k // 2)) + taps(k) - k) * cp))
        h, w, cin = (conv_out(oh, 3), conv_out(ow, 3), cout) if i == 0 else (oh, ow, cout)      # layer 1 is followed by the max pool
    return out


def frames_pack(frames: torch.Tensor, dt) -> torch.Tensor:
    """frames fp32 (N, 3, H, W) -> the padded channels-last buffer of the 7 x 7 convolution, (N (H + 6) (W + 6) + 1, Cp) in dtype ``dt``."""
    N, _, H, W = frames.shape
    out = torch.empty(N * (H + 6) * (W + 6) + 1, pixel_channels(3, 7, dt), dtype=dt, device=frames.device)
    _lib.check(_lib.load().mmdeer_frames_pack(frames.data_ptr(), N, H, W, out.data_ptr(), int(dt == torch.float32), _lib.current_stream()))
    return out


def conv2d_pack(weight: torch.Tensor, dt) -> torch.Tensor:
    """weight (Cout, Cin, k, k) -> image [k][Cout][KWe * Cp] in dtype ``dt``, zeros in the padding positions."""
    w = weight.detach().float().contiguous()
    cout, cin, k, _ = w.shape
    img = torch.empty(k, cout, taps(k) * pixel_channels(cin, k, dt), dtype=dt, device=w.device)
    _lib.check(_lib.load().mmdeer_conv2d_pack(w.data_ptr(), cout, cin, k, img.data_ptr(), int(dt == torch.float32), _lib.current_stream()))
    return img


def conv2d_s2(xp: torch.Tensor, image: torch.Tensor, bias, N: int, H: int, W: int, cin: int, tile: int = -1) -> torch.Tensor:
    """y (N * OH * OW, Cout) = the stride-2 convolution of the padded buffer ``xp`` of N frames of H x W with ``image``."""
    k, cout = image.shape[0], image.shape[1]
    assert xp.dtype == image.dtype
    y = torch.empty(N * conv_out(H, k) * conv_out(W, k), cout, dtype=xp.dtype, device=xp.device)
    a = _lib.Conv2dArgs()
    a.x, a.w, a.bias, a.y = xp.data_ptr(), image.data_ptr(), _lib.ptr(bias), y.data_ptr()
    a.N, a.H, a.W, a.Cin, a.Cout, a.k, a.act_f32, a.tile, a.stream = N, H, W, cin, cout, k, int(xp.dtype == torch.float32), tile, _lib.current_stream()
    _lib.check(_lib.load().mmdeer_conv2d_s2(C.byref(a)))
    return y


def _bn_args(y: torch.Tensor, N: int, H: int, W: int) -> "_lib.Bn2dArgs":
    a = _lib.Bn2dArgs()
    a.x, a.N, a.H, a.W, a.C = y.data_ptr(), N, H, W, y.shape[1]
    a.act_f32, a.stream = int(y.dtype == torch.float32), _lib.current_stream()
    return a


def bn2d_stats(y: torch.Tensor, N: int, H: int, W: int, bn=None, eps: float = 1e-5, scratch: Optional[torch.Tensor] = None):
    """Per-channel (mean, rstd) fp32 of the conv output y (N * H * W, C); with ``bn`` its running buffers are updated on the device.
    ``scratch``: BN2D_SCRATCH fp32 elements the caller keeps for several calls on one stream (allocated here when None)."""
    mean, rstd = torch.empty(y.shape[1], device=y.device), torch.empty(y.shape[1], device=y.device)
    if scratch is None:
        scratch = torch.empty(_lib.BN2D_SCRATCH, device=y.device)
    a = _bn_args(y, N, H, W)
    a.mean, a.rstd, a.scratch, a.eps = mean.data_ptr(), rstd.data_ptr(), scratch.data_ptr(), eps
    if bn is not None:
        _lib.set_bn_buffers(a, bn)
    _lib.check(_lib.load().mmdeer_bn2d_stats(C.byref(a)))
    return mean, rstd


def bn2d_apply(y, N, H, W, mean, rstd, gamma, beta, dest: int, eps: float = 1e-5, running: bool = False) -> torch.Tensor:
    """relu((y - mean) rstd gamma + beta) -> PAD: (N, H + 2, W + 2, C) with a zero border; POOL: the same of the 3 x 3 stride-2 max
    pool; AVG: (N, C) fp32 frame means.  ``running``: (mean, rstd) are (running_mean, running_var)."""
    c = y.shape[1]
    if dest == AVG:
        out = torch.empty(N, c, device=y.device)
    else:
        oh, ow = (conv_out(H, 3), conv_out(W, 3)) if dest == POOL else (H, W)
        out = torch.empty(N, oh + 2, ow + 2, c, dtype=y.dtype, device=y.device)
    a = _bn_args(y, N, H, W)
    a.mean, a.rstd, a.gamma, a.beta, a.eps, a.running = mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), eps, int(running)
    a.out, a.dest = out.data_ptr(), dest
    _lib.check(_lib.load().mmdeer_bn2d_apply(C.byref(a)))
    return out


# ------------------------------------------------------------------------------------------------ the backward operators
def bn2d_bwd(y, N, H, W, mean, rstd, gamma, beta, dout, src: int, eps: float = 1e-5, running: bool = False,
             scratch: Optional[torch.Tensor] = None, zero_row: bool = False):
    """The backward of bn2d_stats + bn2d_apply: ``dout`` is the gradient at the layer's output in the source form ``src`` (SRC_DENSE:
    (N * H * W, C) act; SRC_POOL: (N * PH * PW, C) act; SRC_AVG: (N, C) fp32) -> (dy (N * H * W, C) act, dgamma, dbeta fp32).
    ``zero_row``: dy gets one more row, zero, behind the last -- the form conv2d_dgrad reads."""
    M, c = N * H * W, y.shape[1]
    dy = torch.empty(M + int(zero_row), c, dtype=y.dtype, device=y.device)
    if zero_row:
        dy[M:].zero_()
    dgamma, dbeta = torch.empty(c, device=y.device), torch.empty(c, device=y.device)
    if scratch is None:
        scratch = torch.empty(_lib.BN2D_BWD_SCRATCH, device=y.device)
    idx = torch.empty(N * conv_out(H, 3) * conv_out(W, 3) * c, dtype=torch.uint8, device=y.device) if src == SRC_POOL else None
    a = _lib.Bn2dBwdArgs()
    a.y, a.mean, a.rstd, a.gamma, a.beta = y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), beta.data_ptr()
    a.dout, a.dy, a.dgamma, a.dbeta, a.scratch, a.pool_idx = dout.data_ptr(), dy.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), scratch.data_ptr(), _lib.ptr(idx)
    a.eps, a.src, a.running = eps, src, int(running)
    a.N, a.H, a.W, a.C, a.act_f32, a.stream = N, H, W, c, int(y.dtype == torch.float32), _lib.current_stream()
    _lib.check(_lib.load().mmdeer_bn2d_bwd(C.byref(a)))
    return dy, dgamma, dbeta


def conv2d_wgrad(xp: torch.Tensor, dy: torch.Tensor, N: int, H: int, W: int, cin: int, k: int, bias: bool = True, slices: int = -1):
    """(dw (Cout, Cin, k, k) fp32, dbias (Cout,) fp32 or None) of conv2d_s2 on the padded buffer ``xp`` of N frames of H x W, from
    dy (at least N * OH * OW rows, Cout).  ``slices``: workgroups along the reduction (-1: chosen by the library)."""
    assert xp.dtype == dy.dtype
    cout = dy.shape[1]
    dw = torch.empty(cout, cin, k, k, device=dy.device)
    db = torch.empty(cout, device=dy.device) if bias else None
    a = _lib.Conv2dWgradArgs()
    a.x, a.dy, a.dw, a.dbias = xp.data_ptr(), dy.data_ptr(), dw.data_ptr(), _lib.ptr(db)
    a.N, a.H, a.W, a.Cin, a.Cout, a.k, a.act_f32, a.slices, a.stream = N, H, W, cin, cout, k, int(dy.dtype == torch.float32), slices, _lib.current_stream()
    need = _lib.load().mmdeer_conv2d_wgrad_scratch(C.byref(a))
    _lib.check(-1 if need < 0 else 0)
    scratch = torch.empty(max(need, 1), device=dy.device)
    a.scratch, a.scratch_elems = scratch.data_ptr(), need
    _lib.check(_lib.load().mmdeer_conv2d_wgrad(C.byref(a)))
    return dw, db


def conv2d_pack_t(weight: torch.Tensor, dt) -> torch.Tensor:
    """weight (Cout, Cin, 3, 3) -> the transposed image [3][3][Cin][Cout] in dtype ``dt``."""
    w = weight.detach().float().contiguous()
    cout, cin, k, _ = w.shape
    img = torch.empty(3, 3, cin, cout, dtype=dt, device=w.device)
    _lib.check(_lib.load().mmdeer_conv2d_pack_t(w.data_ptr(), cout, cin, k, img.data_ptr(), int(dt == torch.float32), _lib.current_stream()))
    return img


def conv2d_dgrad(dy: torch.Tensor, wt: torch.Tensor, N: int, H: int, W: int) -> torch.Tensor:
    """dx (N * H * W, Cin): the gradient of the interior of a 3 x 3 convolution's padded input of N frames of H x W, from
    dy (N * OH * OW + 1, Cout) whose last row is zero and the transposed image ``wt``."""
    cin, cout = wt.shape[2], wt.shape[3]
    assert dy.dtype == wt.dtype and dy.shape == (N * conv_out(H, 3) * conv_out(W, 3) + 1, cout)
    dx = torch.empty(N * H * W, cin, dtype=dy.dtype, device=dy.device)
    a = _lib.Conv2dDgradArgs()
    a.dy, a.wt, a.dx = dy.data_ptr(), wt.data_ptr(), dx.data_ptr()
    a.N, a.H, a.W, a.Cin, a.Cout, a.k, a.act_f32, a.stream = N, H, W, cin, cout, 3, int(dy.dtype == torch.float32), _lib.current_stream()
    _lib.check(_lib.load().mmdeer_conv2d_dgrad(C.byref(a)))
    return dx


class _BackboneFn(torch.autograd.Function):
    """The backbone over the whole batch as one autograd node: the forward is ``FrameVideoEncoder._backbone``'s launches and keeps
    per layer the padded input, the convolution's output and the statistics; the backward runs, for layers 4 to 1, bn2d_bwd ->
    conv2d_wgrad -> (above the lowest layer that trains) conv2d_dgrad, and lets go of a layer's buffers as soon as it is through."""

    @staticmethod
    def forward(ctx, enc, frames, dt, training, *params):
        ctx.enc, ctx.dt, ctx.training, ctx.shape = enc, dt, training, tuple(frames.shape)
        f32 = lambda t: t.detach().float().contiguous()                       # noqa: E731
        packed = [(conv2d_pack(params[4 * i], dt), f32(params[4 * i + 1]), f32(params[4 * i + 2]), f32(params[4 * i + 3])) for i in range(4)]
        ctx.kept = []
        feats = enc._backbone(frames, packed, dt, training, ctx.kept)
        ctx.affine = [(g, b) for _, _, g, b in packed]
        ctx.save_for_backward(*params)
        return feats

    @staticmethod
    def backward(ctx, dfeats):
        params, dt, training = ctx.saved_tensors, ctx.dt, ctx.training
        n, _, H, W = ctx.shape
        needs = ctx.needs_input_grad[4:]
        lowest = min(i // 4 for i, need in enumerate(needs) if need)
        grads = [None] * 16
        u, src = dfeats.float().contiguous(), SRC_AVG
        scratch = torch.empty(_lib.BN2D_BWD_SCRATCH, device=u.device)
        layers = plan(n, H, W, dt)
        for li in range(3, lowest - 1, -1):
            k, cin, cout, h, w, oh, ow, _ = layers[li]
            xp, y, mean, rstd = ctx.kept.pop()
            gamma, beta = ctx.affine[li]
            eps = ctx.enc.spatial_backbone[LAYERS[li][1]].eps
            dy, dgamma, dbeta = bn2d_bwd(y, n, oh, ow, mean, rstd, gamma, beta, u, src, eps, not training, scratch, zero_row=li > lowest)
            del y, u
            if needs[4 * li] or needs[4 * li + 1]:
                dw, db = conv2d_wgrad(xp, dy, n, h, w, cin, k, bias=needs[4 * li + 1])
                grads[4 * li], grads[4 * li + 1] = dw, db
            del xp
            grads[4 * li + 2], grads[4 * li + 3] = dgamma, dbeta
            if li > lowest:
                u, src = conv2d_dgrad(dy, conv2d_pack_t(params[4 * li], dt), n, h, w), (SRC_POOL if li == 1 else SRC_DENSE)
            del dy
        ctx.kept.clear()
        out = [g.to(p.dtype) if g is not None and need else None for g, p, need in zip(grads, params, needs)]
        return (None, None, None, None, *out)


class FrameVideoEncoder(TemporalVideoEncoder):
    """``encoders.EnhancedVideoEncoder`` from frames: (B, T, 3, H, W), or (B, 3, H, W) taken as T = 1, -> (B, 512) fp32; (B, T, 512)
    and (B, 512) features go to the parent unchanged.  Same constructor, parameters and 52-entry ``state_dict`` as the parent, so a
    reference checkpoint loads with ``strict=True``.  Any H, W >= 1 is accepted.  ``config['frame_chunk']`` (default 256): frames
    per backbone pass in evaluation mode.

    By default the backbone is FORWARD ONLY, a frozen feature extractor: the features leave ``extract_spatial_features`` detached,
    ``spatial_backbone.*`` parameters receive no gradient (as in the parent), everything downstream trains as in the parent, and a
    frame input with ``requires_grad`` raises ``ValueError``.

    ``config['train_backbone'] = True`` trains it: when grad is enabled and at least one ``spatial_backbone`` parameter requires
    grad, the backbone runs as one autograd node over the whole batch in a single pass, in both modes (``_BackboneFn``: the same
    forward launches, so the features are bit-equal to the default's; the backward is ``mmdeer_bn2d_bwd``, ``mmdeer_conv2d_wgrad``
    and ``mmdeer_conv2d_dgrad`` per layer).  The features then carry the graph, every ``spatial_backbone`` parameter that requires
    grad receives its gradient in its own dtype, and the others none.  Under ``no_grad``, or with every backbone parameter frozen,
    the default path runs, evaluation chunking included.  There is no gradient with respect to the frames: that input stays refused.

    The backbone runs in the mode of ``self.spatial_backbone.training``.  Training mode: batch statistics over all B * T * OH * OW
    positions in the four BatchNorm2d layers, the whole batch in one pass; the running buffers and ``num_batches_tracked`` are
    updated on the device, also under ``no_grad``; one value per channel (B * T * OH * OW = 1 at any layer) raises ``ValueError``
    as in torch.  Evaluation mode: running statistics, frames in chunks.  ``m.train(); m.spatial_backbone.eval()`` gives a
    frozen-statistics backbone under a training head, as in torch.

    Refused with ``ValueError``: a channel count other than 3; a buffer of a backbone pass with 2^31 elements or more (decided on
    the host); a 5-D input with ``shape[1] == 3 and shape[2] == 224`` -- the reference takes that for an averaged frame, makes it a
    6-D tensor and fails; in training mode a BatchNorm2d with ``momentum = None``.

    Every forward packs the four weight images anew (1.6 M elements): nothing is cached, so nothing goes stale when the weights change."""

    def __init__(self, config: Optional[Dict] = None, compute_dtype: str = "fp32"):
        super().__init__(config, compute_dtype)
        self.frame_chunk = int((config or {}).get("frame_chunk", DEFAULT_FRAME_CHUNK))
        if self.frame_chunk < 1:
            raise ValueError(f"frame_chunk must be at least 1 (got {self.frame_chunk})")
        self.train_backbone = bool((config or {}).get("train_backbone", False))

    def _backbone_params(self):
        """the sixteen parameters in the order of _BackboneFn: per layer conv weight, conv bias, BatchNorm weight, BatchNorm bias"""
        sb = self.spatial_backbone
        return [p for ci, bi, _ in LAYERS for p in (sb[ci].weight, sb[ci].bias, sb[bi].weight, sb[bi].bias)]

    def extract_spatial_features(self, video_input: torch.Tensor) -> torch.Tensor:
        """(B, T, 3, H, W) -> (B, T, 512) fp32: ``spatial_backbone`` on every frame.  Detached, unless the backbone trains (the class's
        docstring: ``train_backbone``)."""
        x = video_input
        if x.dim() != 5:
            raise ValueError(f"expected (B, T, 3, H, W), got {tuple(x.shape)}")
        B, T, ch, H, W = x.shape
        if ch != 3:
            raise ValueError(f"expected 3 channels, got {ch}")
        if H < 1 or W < 1:
            raise ValueError(f"expected at least one pixel, got {H} x {W}")
        if x.requires_grad:
            raise ValueError("the backbone is forward only: a frame input with requires_grad is refused")
        training = self.spatial_backbone.training
        if training and any(self.spatial_backbone[bi].momentum is None for _, bi, _ in LAYERS):
            raise ValueError("BatchNorm2d with momentum = None (cumulative averaging) is not supported by the device update of the running buffers")
        dt = ops._act_dtype(self.compute_dtype)
        N = B * T
        grad = self.train_backbone and torch.is_grad_enabled() and any(p.requires_grad for p in self._backbone_params())
        chunk = N if training or grad else min(N, self.frame_chunk)
        for k, _, cout, h, w, oh, ow, elems in plan(chunk, H, W, dt):
            if max(elems, chunk * oh * ow * cout) >= LIMIT:
                raise ValueError(f"{chunk} frames of {H} x {W} need a buffer of 2^31 elements or more")
            if training and N * oh * ow == 1:
                raise ValueError("Expected more than 1 value per channel when training")
        ops._check_dev(x)
        if N == 0:
            return torch.zeros(B, T, 512, device=x.device)
        frames = x.detach().reshape(N, 3, H, W).float().contiguous()
        if grad:
            return _BackboneFn.apply(self, frames, dt, training, *self._backbone_params()).reshape(B, T, 512)
        sb = self.spatial_backbone
        f32 = lambda t: t.detach().float().contiguous()                       # noqa: E731
        params = [(conv2d_pack(sb[ci].weight, dt), f32(sb[ci].bias), f32(sb[bi].weight), f32(sb[bi].bias)) for ci, bi, _ in LAYERS]
        feats = [self._backbone(frames[i:i + chunk], params, dt, training) for i in range(0, N, chunk)]
        return (feats[0] if len(feats) == 1 else torch.cat(feats)).reshape(B, T, 512)

    def _backbone(self, frames: torch.Tensor, params, dt, training: bool, keep: Optional[list] = None) -> torch.Tensor:
        """frames fp32 (n, 3, H, W) -> (n, 512) fp32.  ``keep``: a list that receives, per layer, what the backward reads: (the
        padded input, the convolution's output, mean, rstd -- in evaluation mode copies of running_mean and running_var)."""
        n, _, H, W = frames.shape
        xp = frames_pack(frames, dt)
        scratch = torch.empty(_lib.BN2D_SCRATCH, device=frames.device) if training else None      # one for the four layers: same stream
        for (ci, bi, dest), (img, bias, gamma, beta), (k, cin, cout, h, w, oh, ow, _) in zip(LAYERS, params, plan(n, H, W, dt)):
            bn = self.spatial_backbone[bi]
            y = conv2d_s2(xp, img, bias, n, h, w, cin)
            if training:
                mean, rstd = bn2d_stats(y, n, oh, ow, bn, bn.eps, scratch)
            else:
                mean, rstd = bn.running_mean, bn.running_var
            nxt = bn2d_apply(y, n, oh, ow, mean, rstd, gamma, beta, dest, bn.eps, running=not training)
            if keep is not None:
                keep.append((xp, y, mean, rstd) if training else (xp, y, mean.clone(), rstd.clone()))
            xp = nxt
        return xp

    def forward(self, video_input: torch.Tensor) -> torch.Tensor:
        x = video_input
        if x.dim() in (2, 3):
            return super().forward(x)
        if x.dim() == 5 and x.shape[1] == 3 and x.shape[2] == 224:
            raise ValueError(f"a 5-D input {tuple(x.shape)} with shape[1] == 3 and shape[2] == 224 is ambiguous (the reference takes it "
                             "for an averaged frame and fails): pass (B, 3, 224, W) for single frames")
        if x.dim() == 4:
            x = x.unsqueeze(1)
        if x.dim() != 5:
            raise ValueError(f"expected (B, T, 3, H, W), (B, 3, H, W), (B, T, 512) or (B, 512), got {tuple(video_input.shape)}")
        if x.shape[1] == 0:
            raise ValueError("expected at least one frame")
        if self.hidden_dim != 512:
            raise NotImplementedError(f"the HIP path is built for hidden_dim = 512 (got {self.hidden_dim})")
        return super().forward(self.extract_spatial_features(x))
