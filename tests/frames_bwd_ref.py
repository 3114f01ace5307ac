"""Float64 restatement of the frame video encoder's BACKWARD (include/mmdeer_frames_bwd.h): gradients by autograd through the
operator functions of tests/frames_ref.py on the kernels' own stored operands, and the module's gradients by autograd through
frames_ref.backbone + video_ref.encoder.  The bf16-emulating form rounds where the backward stores bf16: dy and dx.  Runs on
whatever device its tensors are on.  A helper module, not a test module.

The ReLU mask and the pool's arg-max are decided in fp32 on the device and in float64 here, so an element whose pre-activation is
within TIE of zero, or that is one of the two largest values of a pool window which differ by less than TIE without being equal,
may land on the other side: ``undecided`` marks those elements and bounds what they can move."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import frames_ref as R
from . import video_ref
from .temporal_ref import bf16

TIE = 1e-5
DENSE, POOL, AVG = 0, 1, 2          # the source forms, in the header's numbering
BACKBONE_PARAMS = [f"{layer}.{k}" for pair in R.LAYERS for layer in pair for k in ("weight", "bias")]


def layer_output(y, gamma, beta, N, H, W, src, mean=None, var=None):
    """The output of one BatchNorm2d + ReLU layer in the form its gradient arrives in: DENSE (N H W, C), POOL (N PH PW, C) -- the
    interior of the pooled buffer --, AVG (N, C)."""
    v, _, _ = R.batchnorm_relu(y, gamma, beta, mean, var)
    if src == DENSE:
        return v
    if src == AVG:
        return R.frame_means(v, N)
    return R.maxpool_padded(v, N, H, W)[:, 1:-1, 1:-1].reshape(-1, y.shape[1])


def bn2d_bwd(y, gamma, beta, dout, N, H, W, src, mean=None, var=None, emulate_bf16=False):
    """(dy, dgamma, dbeta) in float64; mean / var given: running statistics (constants)."""
    y, gamma, beta = (t.detach().clone().requires_grad_(True) for t in (y, gamma, beta))
    out = layer_output(y, gamma, beta, N, H, W, src, mean, var)
    dy, dgamma, dbeta = torch.autograd.grad((out * dout).sum(), [y, gamma, beta])
    return (bf16(dy) if emulate_bf16 else dy), dgamma, dbeta


def undecided(y, gamma, beta, dout, N, H, W, src, mean=None, var=None):
    """-> (mask (N H W, C) of the elements left out of the dy comparison, slack_beta, slack_gamma: the sums over them of the
    gradient they could receive, |u| and |u xhat|, which widen the bounds of dbeta and dgamma)."""
    C = y.shape[1]
    m, v = (y.mean(0), y.var(0, unbiased=False)) if mean is None else (mean, var)
    xhat = (y - m) / torch.sqrt(v + R.EPS)
    pre = xhat * gamma + beta
    out = pre.abs() <= TIE
    if src == DENSE:
        u = dout.abs()
    elif src == AVG:
        u = (dout.abs() / (H * W)).repeat_interleave(H * W, 0)
    else:
        img = F.pad(torch.relu(pre).reshape(N, H, W, C).permute(0, 3, 1, 2), (1, 1, 1, 1), value=float("-inf"))
        PH, PW = R.out_size(H, 3), R.out_size(W, 3)
        win = F.unfold(img, 3, stride=2).reshape(N, C, 9, PH * PW)
        top, at = win.topk(2, dim=2)
        near = ((top[:, :, 0] - top[:, :, 1]) < TIE) & (top[:, :, 0] != top[:, :, 1])                 # (N, C, L)
        hit = torch.zeros_like(win).scatter_(2, at, near.unsqueeze(2).expand(-1, -1, 2, -1).to(win.dtype))
        fold = lambda t: F.fold(t.reshape(N, C * 9, PH * PW), (H + 2, W + 2), 3, stride=2)[:, :, 1:-1, 1:-1]      # noqa: E731
        out = out | (fold(hit) > 0).permute(0, 2, 3, 1).reshape(-1, C)
        d = dout.abs().reshape(N, PH * PW, C).permute(0, 2, 1).unsqueeze(2).expand(-1, -1, 9, -1)     # what every window could hand on
        u = fold(d.contiguous()).permute(0, 2, 3, 1).reshape(-1, C)
    return out, (u * out).sum(0), (u * xhat.abs() * out).sum(0)


def conv_grads(xp, weight, bias, dy, N, H, W, k, KWe):
    """(dw (Cout, Cin, k, k), dbias, dx (N H W, Cin) -- the gradient of the interior of the padded buffer) in float64, from the
    stored operands: the padded buffer xp (pixels, Cp), the fp32 weight AS THE IMAGE HOLDS IT (rounded for bf16), dy (M, Cout)."""
    xp, weight, bias = (t.detach().clone().requires_grad_(True) for t in (xp, weight, bias))
    Cp, p = xp.shape[1], k // 2
    y = R.conv2d_s2(xp, R.pack_weight(weight, Cp, KWe), bias, N, H, W, k)
    dxp, dw, db = torch.autograd.grad((y * dy).sum(), [xp, weight, bias])
    pixels = N * (H + 2 * p) * (W + 2 * p)
    dx = dxp[:pixels].reshape(N, H + 2 * p, W + 2 * p, Cp)[:, p:p + H, p:p + W, :weight.shape[1]].reshape(N * H * W, -1)
    return dw, db, dx


def pack_weight_t(weight):
    """weight (Cout, Cin, 3, 3) -> the transposed image (3, 3, Cin, Cout): image[kh][kw][c][co] = weight[co][c][kh][kw]"""
    return weight.permute(2, 3, 1, 0).contiguous()


def module_grads(P: dict, x: torch.Tensor, w: torch.Tensor, backbone_train: bool, head_train: bool, emulate_bf16: bool = False, Cp1: int = 4):
    """x (B, T, 3, H, W), loss = sum(out * w) -> (features (B, T, 512), output (B, 512), {name: gradient} for every floating-point
    entry of P that takes part), by autograd through the restatement.  ``emulate_bf16``: the forward rounding of frames_ref only."""
    B, T = x.shape[0], x.shape[1]
    Q = {k: (v.detach().clone().requires_grad_(True) if v.is_floating_point() and "running_" not in k else v) for k, v in P.items()}
    feats, _ = R.backbone(Q, x.reshape(B * T, *x.shape[2:]), backbone_train, emulate_bf16, Cp1)
    feats = feats.reshape(B, T, -1)
    out, _ = video_ref.encoder(Q, feats, head_train)
    names = [k for k, v in Q.items() if v.requires_grad]
    grads = torch.autograd.grad((out * w).sum(), [Q[k] for k in names], allow_unused=True)
    return feats.detach(), out.detach(), {k: g for k, g in zip(names, grads) if g is not None}
