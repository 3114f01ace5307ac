"""Float64 restatement of the frame video encoder's backbone (encoders.EnhancedVideoEncoder.spatial_backbone on frames), written from
its semantics: four stride-2 convolutions -- cross-correlations with zero padding, 7 x 7 with padding 3, then 3 x 3 with padding 1 --
each followed by BatchNorm2d over all N * OH * OW positions (batch mean and biased variance in training, running statistics in
evaluation; the running update with momentum and the unbiased variance) and ReLU; a 3 x 3 stride-2 max pool padded with -inf behind
the first; the mean over the positions of a frame behind the last.  Downstream of the features it is tests/video_ref.encoder.
Runs on whatever device its tensors are on.  A helper module, not a test module.

The operator functions work on the HIP path's own layouts (include/mmdeer_frames.h) -- the padded channels-last buffer
[N][Hp][Wp][Cp] (+ slack) that feeds a convolution, the weight image [k][Cout][KWe * Cp], the dense output [N * OH * OW][Cout] -- and
have a bf16-emulating form that rounds where the kernels store or feed bf16: the packed frames, the weight image, a stored
convolution output, a stored normalised activation.  The frame means (fp32 on the device) are not rounded."""
from __future__ import annotations

import numpy as np
import torch

from mmdeer import synth

from . import video_ref
from .temporal_ref import bf16

EPS = 1e-5
MOMENTUM = 0.1
LAYERS = (("spatial_backbone.0", "spatial_backbone.1"), ("spatial_backbone.4", "spatial_backbone.5"),
          ("spatial_backbone.7", "spatial_backbone.8"), ("spatial_backbone.10", "spatial_backbone.11"))
BUFFERS = [f"{bn}.{k}" for _, bn in LAYERS for k in ("running_mean", "running_var", "num_batches_tracked")]
filled_state = video_ref.filled_state


def frames_input(stream: int, B: int, T: int, H: int, W: int, scale: float = 1.0) -> np.ndarray:
    """The case's frames (B, T, 3, H, W) fp32 from the counter-based generator."""
    return (synth.normal(stream, B * T * 3 * H * W) * scale).reshape(B, T, 3, H, W).astype(np.float32)


def out_size(size: int, k: int) -> int:
    return (size + 2 * (k // 2) - k) // 2 + 1


def pad_pixels(v: torch.Tensor, p: int, Cp: int, slack: int = 0) -> torch.Tensor:
    """channels-last (N, H, W, C) -> the padded buffer (N * (H + 2p) * (W + 2p) + slack, Cp): zero border, zero channels C .. Cp - 1,
    ``slack`` zero pixels behind the last"""
    N, H, W, C = v.shape
    buf = v.new_zeros(N, H + 2 * p, W + 2 * p, Cp)
    buf[:, p:p + H, p:p + W, :C] = v
    return torch.cat([buf.reshape(-1, Cp), v.new_zeros(slack, Cp)])


def pack_frames(frames: torch.Tensor, Cp: int, emulate_bf16: bool = False) -> torch.Tensor:
    """frames (N, 3, H, W) -> the padded buffer of the 7 x 7 convolution, one slack pixel included"""
    buf = pad_pixels(frames.permute(0, 2, 3, 1), 3, Cp, slack=1)
    return bf16(buf) if emulate_bf16 else buf


def pack_weight(weight: torch.Tensor, Cp: int, KWe: int, emulate_bf16: bool = False) -> torch.Tensor:
    """weight (Cout, Cin, k, k) -> image (k, Cout, KWe * Cp): image[kh][co][kw * Cp + c] = weight[co][c][kh][kw], zero elsewhere"""
    Cout, Cin, k, _ = weight.shape
    img = weight.new_zeros(k, Cout, KWe, Cp)
    img[:, :, :k, :Cin] = weight.permute(2, 0, 3, 1)
    img = img.reshape(k, Cout, KWe * Cp)
    return bf16(img) if emulate_bf16 else img


def conv2d_s2(xp: torch.Tensor, image: torch.Tensor, bias, N: int, H: int, W: int, k: int, emulate_bf16: bool = False) -> torch.Tensor:
    """xp: the padded buffer (pixels, Cp) of N frames of H x W; image (k, Cout, K) -> y (N * OH * OW, Cout):
    y[(n OH + oh) OW + ow] = bias + sum_kh xp.flat[((n Hp + 2 oh + kh) Wp + 2 ow) Cp : + K] image[kh]^T"""
    p, Cp, K = k // 2, xp.shape[1], image.shape[2]
    Hp, Wp, OH, OW = H + 2 * p, W + 2 * p, out_size(H, k), out_size(W, k)
    n, oh, ow = torch.meshgrid(torch.arange(N), torch.arange(OH), torch.arange(OW), indexing="ij")
    origin = (((n * Hp + 2 * oh) * Wp + 2 * ow) * Cp).reshape(-1, 1).to(xp.device)
    flat, e = xp.reshape(-1), torch.arange(K, device=xp.device)
    y = sum(flat[origin + kh * Wp * Cp + e] @ image[kh].t() for kh in range(k))
    if bias is not None:
        y = y + bias
    return bf16(y) if emulate_bf16 else y


def batchnorm_relu(y: torch.Tensor, gamma, beta, mean=None, var=None):
    """y (M, C).  mean / var None: batch statistics.  -> (relu(bn(y)), batch mean, biased batch variance), computed from y as stored"""
    bm, bv = y.mean(0), y.var(0, unbiased=False)
    m, v = (bm, bv) if mean is None else (mean, var)
    return torch.relu((y - m) / torch.sqrt(v + EPS) * gamma + beta), bm, bv


def running_update(rm, rv, nbt, mean, var_biased, M: int):
    """nn.BatchNorm2d's buffer update after one training batch of M positions per channel"""
    return (1 - MOMENTUM) * rm + MOMENTUM * mean, (1 - MOMENTUM) * rv + MOMENTUM * var_biased * (M / (M - 1)), nbt + 1


def to_padded(v: torch.Tensor, N: int, H: int, W: int, emulate_bf16: bool = False) -> torch.Tensor:
    """normalised rows (N * H * W, C) -> the padded buffer of the next 3 x 3 convolution (N, H + 2, W + 2, C)"""
    out = pad_pixels(v.reshape(N, H, W, -1), 1, v.shape[1]).reshape(N, H + 2, W + 2, -1)
    return bf16(out) if emulate_bf16 else out


def maxpool_padded(v: torch.Tensor, N: int, H: int, W: int, emulate_bf16: bool = False) -> torch.Tensor:
    """the same of the 3 x 3 stride-2 max pool, padded with -inf, of the rows (N * H * W, C)"""
    img = torch.nn.functional.pad(v.reshape(N, H, W, -1).permute(0, 3, 1, 2), (1, 1, 1, 1), value=float("-inf"))
    pooled = torch.nn.functional.max_pool2d(img, 3, 2).permute(0, 2, 3, 1)
    return to_padded(pooled.reshape(-1, v.shape[1]), N, pooled.shape[1], pooled.shape[2], emulate_bf16)


def frame_means(v: torch.Tensor, N: int) -> torch.Tensor:
    return v.reshape(N, -1, v.shape[1]).mean(1)


def backbone(P: dict, frames: torch.Tensor, train: bool, emulate_bf16: bool = False, Cp1: int = 4):
    """P: state_dict names -> float64 tensors; frames (N, 3, H, W) -> (features (N, 512), the twelve BatchNorm2d buffers after the
    step -- unchanged in evaluation mode).  ``Cp1``: channels per pixel of the first buffer (4 in fp32, 8 in bf16: zeros either way)."""
    N, _, H, W = frames.shape
    buffers = {k: P[k] for k in BUFFERS}
    xp = pack_frames(frames, Cp1, emulate_bf16)
    for i, (conv, bn) in enumerate(LAYERS):
        w = P[f"{conv}.weight"]
        k = w.shape[2]
        img = pack_weight(w, xp.shape[-1], 8 if k == 7 else 3, emulate_bf16)
        y = conv2d_s2(xp.reshape(-1, xp.shape[-1]), img, P[f"{conv}.bias"], N, H, W, k, emulate_bf16)
        H, W = out_size(H, k), out_size(W, k)
        rm, rv = P[f"{bn}.running_mean"], P[f"{bn}.running_var"]
        v, bm, bv = batchnorm_relu(y, P[f"{bn}.weight"], P[f"{bn}.bias"], None if train else rm, None if train else rv)
        if train:
            buffers[f"{bn}.running_mean"], buffers[f"{bn}.running_var"], buffers[f"{bn}.num_batches_tracked"] = \
                running_update(rm, rv, P[f"{bn}.num_batches_tracked"], bm, bv, N * H * W)
        if i == 0:
            xp = maxpool_padded(v, N, H, W, emulate_bf16)
            H, W = out_size(H, 3), out_size(W, 3)
        elif i < 3:
            xp = to_padded(v, N, H, W, emulate_bf16)
        else:
            return frame_means(v, N), buffers


def encoder(P: dict, x: torch.Tensor, train: bool):
    """x (B, T, 3, H, W) -> (features (B, T, 512), output (B, 512), buffers after the step: BatchNorm2d's and the temporal CNN's)"""
    B, T = x.shape[0], x.shape[1]
    feats, buffers = backbone(P, x.reshape(B * T, *x.shape[2:]), train)
    feats = feats.reshape(B, T, -1)
    y, tbuf = video_ref.encoder(P, feats, train)
    return feats, y, {**buffers, **tbuf}
