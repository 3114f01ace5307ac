"""Temporal video encoder: ``encoders.EnhancedVideoEncoder`` downstream of its spatial CNN (reference src/models/encoders.py:
392-550) on per-frame features (B, T, 512), or (B, 512) taken as T = 1 -> (B, 512) fp32.

``spatial_projection`` (Linear + ReLU + Dropout on every frame, one ``mmdeer_gemm`` over all T * B rows); only for T > 1 the
``temporal_cnn`` -- Conv1d(512, 512, 3, padding = 1) -> BatchNorm1d -> ReLU -> Dropout -> Conv1d -> BatchNorm1d -> ReLU -- and the
``temporal_attention`` pool over time (``temporal.temporal_pool``: the audio encoder's pool at the same widths); then
``output_projection`` = LayerNorm(Dropout(ReLU(Linear))) (``fusions._LinActLnFn``).

Rows are time-major (row t * B + b), so one time step is a shift of B rows.  An activation that feeds a convolution lives in a
padded buffer of (T + 2) * B rows whose first and last B rows are zero: the convolution is then one implicit-GEMM launch
(``mmdeer_conv3_time``: three K loops over row-shifted views into the same accumulators), its input gradient the same kernel on
the padded dY with the reversed, transposed weight image, and its weight gradient three ordinary dW problems on row-shifted
views in one grouped launch.  BatchNorm is ``mmdeer_bn_time_stats / _apply / _bwd`` (Welford partials merged by Chan's formula,
deterministic); the running buffers are updated on the device by the statistics launch.  Torch element-wise kernels do only
this: the transpose of the input to time-major rows, dtype conversions between autograd nodes, the zero fill of the padded
buffers and the copy of the projected features into the first one's interior, and the permutation of the three dW slices to
(N, C, 3).  No CPU path: CPU tensors raise."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import torch
from torch import nn

from . import _lib, fusions, ops, temporal
from .opseq import Exec, set_drop
from .stepcount import StepCounted

W = 512                                           # hidden_dim of the sequence path
_SITE_SP, _SITE_CNN, _SITE_OP = 144, 145, 146     # spatial_projection / temporal_cnn / output_projection dropout


def padded(T: int, B: int, dt, device) -> torch.Tensor:
    """A padded activation buffer ((T + 2) * B, 512) with its pad rows zeroed; ``interior`` is the T * B rows in between."""
    buf = torch.empty((T + 2) * B, W, dtype=dt, device=device)
    buf[:B].zero_()
    buf[(T + 1) * B:].zero_()
    return buf


def interior(buf: torch.Tensor, B: int) -> torch.Tensor:
    return buf[B:buf.shape[0] - B]


def conv3_pack(weight: torch.Tensor, dt, with_rev_t: bool):
    """weight (512, 512, 3) -> (image [3][N][C], image_rev_t [3][C][N] or None) in dtype ``dt``."""
    w = weight.detach().float().contiguous()
    img = torch.empty(3, W, W, dtype=dt, device=w.device)
    img_t = torch.empty(3, W, W, dtype=dt, device=w.device) if with_rev_t else None
    _lib.check(_lib.load().mmdeer_conv3_time_pack(w.data_ptr(), weight.shape[0], weight.shape[1], img.data_ptr(), _lib.ptr(img_t),
                                                  int(dt == torch.float32), _lib.current_stream()))
    return img, img_t


def conv3_time(xp: torch.Tensor, image: torch.Tensor, bias, T: int, B: int, out: Optional[torch.Tensor] = None, tile: int = -1):
    """y (T * B, 512) = bias + sum_j xp[j B : j B + T B] image[j]^T on the padded buffer xp ((T + 2) * B, 512)."""
    assert xp.shape[0] == (T + 2) * B and xp.dtype == image.dtype
    y = torch.empty(T * B, W, dtype=xp.dtype, device=xp.device) if out is None else out
    a = _lib.Conv3TimeArgs()
    a.x, a.ld_x, a.w, a.bias, a.y, a.ld_y = xp.data_ptr(), xp.stride(0), image.data_ptr(), _lib.ptr(bias), y.data_ptr(), y.stride(0)
    a.T, a.B, a.C, a.N, a.act_f32, a.tile, a.stream = T, B, W, W, int(xp.dtype == torch.float32), tile, _lib.current_stream()
    _lib.check(_lib.load().mmdeer_conv3_time(C.byref(a)))
    return y


def conv3_dw(dyp: torch.Tensor, xp: torch.Tensor, T: int, B: int, compute_dtype: str):
    """dW (512, 512, 3) fp32 and the bias gradient (512,) from the padded dY and the padded input: dW[:, :, j] = dY^T xp[j B : j B + T B],
    three weight-gradient problems in one grouped launch (the bias gradient from the first)."""
    ex = Exec(compute_dtype)
    ex.deferred = []
    dy, R = interior(dyp, B), T * B
    gw, gb = torch.zeros(3, W, W, device=dyp.device), torch.zeros(W, device=dyp.device)
    for j in range(3):
        ex.dw(dy, W, xp[j * B:j * B + R], W, gw[j], gb if j == 0 else None, R, W, W)
    ex.flush_dw()
    return gw.permute(1, 2, 0).contiguous(), gb


def _bn_args(x, compute_dtype) -> "_lib.BnTimeArgs":
    a = _lib.BnTimeArgs()
    a.x, a.ld_x, a.R, a.C = x.data_ptr(), x.stride(0), x.shape[0], W
    a.act_f32, a.stream, a.drop_site, a.mask_scale = int(compute_dtype == "fp32"), _lib.current_stream(), -1, 1.0
    return a


def _scratch(device) -> torch.Tensor:
    return torch.empty(_lib.BN_TIME_SCRATCH, device=device)


def bn_stats(x: torch.Tensor, compute_dtype: str, bn: Optional[nn.BatchNorm1d] = None, eps: float = 1e-5):
    """Per-channel (mean, rstd) fp32 of the act matrix x (R, 512); with ``bn`` its running buffers are updated on the device."""
    mean, rstd = torch.empty(W, device=x.device), torch.empty(W, device=x.device)
    scratch = _scratch(x.device)
    a = _bn_args(x, compute_dtype)
    a.mean, a.rstd, a.scratch, a.eps = mean.data_ptr(), rstd.data_ptr(), scratch.data_ptr(), eps
    if bn is not None:
        _lib.set_bn_buffers(a, bn)
    _lib.check(_lib.load().mmdeer_bn_time_stats(C.byref(a)))
    return mean, rstd


def bn_apply(x, mean, rstd, gamma, beta, out, compute_dtype, eps=1e-5, running=False, relu=True, drop=None, site=-1):
    """out = drop(relu((x - mean) rstd gamma + beta)); ``running``: (mean, rstd) are (running_mean, running_var)."""
    a = _bn_args(x, compute_dtype)
    a.mean, a.rstd, a.gamma, a.beta, a.eps, a.running = mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), eps, int(running)
    a.out, a.ld_out, a.relu = out.data_ptr(), out.stride(0), int(relu)
    if drop is not None and drop[0] > 0:
        a.drop_site, a.dropout_p = site, float(drop[0])
        set_drop(a, drop)
    _lib.check(_lib.load().mmdeer_bn_time_apply(C.byref(a)))
    return out


def bn_bwd(dout, out, x, mean, rstd, gamma, dx, compute_dtype, eps=1e-5, running=False, mask_scale=1.0):
    """-> (dx written into ``dx``, dgamma, dbeta) for g = dout (out > 0) mask_scale."""
    dg, db = torch.empty(W, device=x.device), torch.empty(W, device=x.device)
    scratch = _scratch(x.device)
    a = _bn_args(x, compute_dtype)
    a.mean, a.rstd, a.gamma, a.eps, a.running = mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), eps, int(running)
    a.dout, a.ld_dout, a.dx, a.ld_dx = dout.data_ptr(), dout.stride(0), dx.data_ptr(), dx.stride(0)
    if out is not None:
        a.out, a.ld_out = out.data_ptr(), out.stride(0)
    a.mask_scale, a.dgamma, a.dbeta, a.scratch = mask_scale, dg.data_ptr(), db.data_ptr(), scratch.data_ptr()
    _lib.check(_lib.load().mmdeer_bn_time_bwd(C.byref(a)))
    return dx, dg, db


class _TemporalCnnFn(torch.autograd.Function):
    """``temporal_cnn`` on time-major rows h (T * B, 512) -> (T * B, 512) fp32.  ``bns``: the two nn.BatchNorm1d modules (their
    buffers are read in evaluation mode and updated in training mode, also under no_grad)."""

    @staticmethod
    def forward(ctx, h, w0, b0, g0, be0, w1, b1, g1, be1, bns, T, B, compute_dtype, training, drop):
        dt = ops._act_dtype(compute_dtype)
        ops._check_dev(h)
        dev = h.device
        need_grad = any(ctx.needs_input_grad[:9])
        f32 = lambda t: t.detach().float().contiguous()                       # noqa: E731
        xp, saved = padded(T, B, dt, dev), []
        interior(xp, B).copy_(h.detach())
        for i, (w, b, g, be, bn) in enumerate(((w0, b0, g0, be0, bns[0]), (w1, b1, g1, be1, bns[1]))):
            img, img_t = conv3_pack(w, dt, need_grad)
            y = conv3_time(xp, img, f32(b), T, B)
            gamma, beta = f32(g), f32(be)
            if training:
                mean, rstd = bn_stats(y, compute_dtype, bn, bn.eps)
            else:
                mean, rstd = bn.running_mean.detach().clone(), bn.running_var.detach().clone()
            last = i == 1
            nxt = torch.empty(T * B, W, dtype=dt, device=dev) if last else padded(T, B, dt, dev)
            out = nxt if last else interior(nxt, B)
            bn_apply(y, mean, rstd, gamma, beta, out, compute_dtype, bn.eps, running=not training, drop=None if last else drop, site=_SITE_CNN)
            saved += [xp, img_t, y, mean, rstd, gamma, nxt]
            xp = nxt
        if need_grad:
            ctx.save_for_backward(*[t for t in saved if t is not None])
        p = float(drop[0]) if drop is not None else 0.0
        ctx.meta = (T, B, compute_dtype, training, 1.0 / (1.0 - p) if p > 0 else 1.0, bns[0].eps, bns[1].eps, h.dtype, w0.dtype)
        return xp.float()

    @staticmethod
    def backward(ctx, gout):
        T, B, compute_dtype, training, scale0, eps0, eps1, hdt, wdt = ctx.meta
        s = ctx.saved_tensors
        layers = (s[:7], s[7:])
        dt, dev = s[0].dtype, s[0].device
        grads = [None, None]
        dcur = gout.to(dt).contiguous()                                        # gradient at the layer's (post-ReLU, post-dropout) output
        for i in (1, 0):
            xp, img_t, y, mean, rstd, gamma, nxt = layers[i]
            out = nxt if i == 1 else interior(nxt, B)
            dyp = padded(T, B, dt, dev)
            _, dg, db = bn_bwd(dcur, out, y, mean, rstd, gamma, interior(dyp, B), compute_dtype, eps1 if i else eps0,
                               running=not training, mask_scale=1.0 if i else scale0)
            gw, gb = conv3_dw(dyp, xp, T, B, compute_dtype)
            dcur = conv3_time(dyp, img_t, None, T, B)
            grads[i] = (gw.to(wdt), gb.to(wdt), dg.to(wdt), db.to(wdt))
        return (dcur.to(hdt), *grads[0], *grads[1], None, None, None, None, None, None)


class TemporalVideoEncoder(nn.Module, StepCounted):
    """``encoders.EnhancedVideoEncoder`` (reference src/models/encoders.py:392-550) on per-frame features: (B, T, 512) or
    (B, 512) -> (B, 512) fp32.  Submodules carry the reference's names and order, so a reference checkpoint loads with
    ``strict=True``; ``spatial_backbone`` (the Conv2d stack on frames) is held for that and never run: frame tensors raise
    ``NotImplementedError``.  Initialisation is torch's default, as in the reference.

    ``.train()`` uses batch statistics in both BatchNorm layers and updates their running buffers (also under ``no_grad``), and the
    three dropouts are live (the library's counter-hash masks, one step counter tick per training forward); ``.eval()`` uses the
    running statistics.  At T = 1 the temporal CNN and the pool are skipped as in the reference: their parameters receive no
    gradient and the running buffers do not move.  Under data parallelism each rank normalises with the statistics of its own
    batch shard, as torch's unsynchronised BatchNorm does."""

    def __init__(self, config: Optional[Dict] = None, compute_dtype: str = "fp32"):
        super().__init__()
        config = config or {}
        self.hidden_dim = config.get("hidden_dim", 512)
        self.dropout = config.get("dropout", 0.3)
        self.max_frames = config.get("max_frames", 32)
        self.compute_dtype = compute_dtype
        self.dropout_seed, self._train_step = config.get("dropout_seed", 0), 0     # counter-hash dropout: seed + one tick per training forward
        Hd = self.hidden_dim
        self.spatial_backbone = nn.Sequential(
            nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3), nn.BatchNorm2d(64), nn.ReLU(inplace=True),
            nn.MaxPool2d(kernel_size=3, stride=2, padding=1),
            nn.Conv2d(64, 128, kernel_size=3, stride=2, padding=1), nn.BatchNorm2d(128), nn.ReLU(inplace=True),
            nn.Conv2d(128, 256, kernel_size=3, stride=2, padding=1), nn.BatchNorm2d(256), nn.ReLU(inplace=True),
            nn.Conv2d(256, 512, kernel_size=3, stride=2, padding=1), nn.BatchNorm2d(512), nn.ReLU(inplace=True),
            nn.AdaptiveAvgPool2d((1, 1)))
        self.spatial_projection = nn.Sequential(nn.Linear(512, Hd), nn.ReLU(), nn.Dropout(self.dropout))
        self.temporal_cnn = nn.Sequential(
            nn.Conv1d(Hd, Hd, kernel_size=3, padding=1), nn.BatchNorm1d(Hd), nn.ReLU(), nn.Dropout(self.dropout),
            nn.Conv1d(Hd, Hd, kernel_size=3, padding=1), nn.BatchNorm1d(Hd), nn.ReLU())
        self.temporal_attention = nn.Sequential(nn.Linear(Hd, Hd // 2), nn.Tanh(), nn.Linear(Hd // 2, 1), nn.Softmax(dim=1))
        self.output_projection = nn.Sequential(nn.Linear(Hd, Hd), nn.ReLU(), nn.Dropout(self.dropout), nn.LayerNorm(Hd))

    def forward(self, video_input: torch.Tensor) -> torch.Tensor:
        x = video_input
        if x.dim() in (4, 5):
            raise NotImplementedError("frame tensors (the spatial Conv2d backbone) are outside the hot path: pass (B, T, 512) features")
        if self.hidden_dim != W:
            raise NotImplementedError(f"the HIP path is built for hidden_dim = {W} (got {self.hidden_dim})")
        if x.dim() not in (2, 3) or x.shape[-1] != 512:
            raise ValueError(f"expected (B, 512) or (B, T, 512), got {tuple(video_input.shape)}")
        if x.dim() == 2:
            x = x.unsqueeze(1)
        B, T = x.shape[0], x.shape[1]
        if T == 0:
            raise ValueError("expected at least one frame")
        ops._check_dev(x)
        if B == 0:
            return torch.zeros(0, W, device=x.device)
        c = self.compute_dtype
        drop = None
        if self.training and self.dropout > 0:
            drop = self._drop_step(self.dropout, self.dropout_seed)
        h = x.transpose(0, 1).reshape(T * B, 512)                              # time-major rows t * B + b
        h = fusions.linear(h, self.spatial_projection[0], c, relu=True, drop=drop, site=_SITE_SP)
        if T > 1:
            if self.training and T * B < 2:
                raise ValueError("Expected more than 1 value per channel when training")
            cnn = self.temporal_cnn
            h = _TemporalCnnFn.apply(h, cnn[0].weight, cnn[0].bias, cnn[1].weight, cnn[1].bias, cnn[4].weight, cnn[4].bias,
                                     cnn[5].weight, cnn[5].bias, (cnn[1], cnn[5]), T, B, c, self.training, drop)
            h, _ = temporal.temporal_pool(h, self.temporal_attention, T, B, c)
        op = self.output_projection
        return fusions._LinActLnFn.apply(h, op[0].weight, op[0].bias, op[3].weight, op[3].bias, c, drop, _SITE_OP)
