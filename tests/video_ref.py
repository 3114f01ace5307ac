"""Float64 restatement of the temporal video encoder (encoders.EnhancedVideoEncoder downstream of its spatial CNN, on (B, T, 512)
per-frame features), written from its semantics: ``spatial_projection`` on every frame; for T > 1 the two 3-tap convolutions over
time (a cross-correlation, y[t] = b + sum_j W[:, :, j] x[t + j - 1] with zeros outside [0, T)) each followed by BatchNorm1d over
all B * T positions (batch mean and biased variance in training, running statistics in evaluation; the running update with
momentum and the unbiased variance) and ReLU, then the attention pool over time; ``output_projection`` = LayerNorm(ReLU(Linear)).
Dropout is off unless ``encoder`` is given the keep masks of a training step (the golden cases use p = 0).  Runs on whatever device its tensors are on.  A helper module, not a test module.

The operator functions ``conv3_time`` and ``batchnorm_rows`` work on the HIP path's own layout -- time-major rows r = t * B + b and,
for the convolution's input, the padded buffer of (T + 2) * B rows -- and have a bf16-emulating form that rounds where the kernels
store or feed bf16: the operands of a product, a stored output, and a gradient handed to the next product."""
from __future__ import annotations

import numpy as np
import torch

from mmdeer import synth

from .temporal_ref import _Round, _RoundGrad, attention_pool, bf16, draw, layer_norm, linear, pool  # noqa: F401  (bf16, draw re-exported for the tests)

W = 512
EPS = 1e-5
MOMENTUM = 0.1
BN_LAYERS = ("temporal_cnn.1", "temporal_cnn.5")


def filled_state(tag: str, shapes) -> "dict[str, np.ndarray]":
    """synth.module_fill, with every ``*.running_var`` replaced by 0.5 + 10 |fill|: module_fill treats that buffer as a bias
    (+-0.05), and a negative variance is a NaN in evaluation mode.  (Its fill of num_batches_tracked casts to 0.)"""
    sd = synth.module_fill(tag, shapes)
    for k in sd:
        if k.endswith(".running_var"):
            sd[k] = (0.5 + np.abs(sd[k]) * 10.0).astype(np.float32)
    return sd


def pad_time(x: torch.Tensor, B: int) -> torch.Tensor:
    """time-major rows (T * B, C) -> the padded buffer ((T + 2) * B, C): B zero rows in front and behind"""
    z = x.new_zeros(B, x.shape[1])
    return torch.cat([z, x, z], dim=0)


def conv3_time(xp: torch.Tensor, weight: torch.Tensor, bias, T: int, B: int, emulate_bf16: bool = False) -> torch.Tensor:
    """xp: padded ((T + 2) * B, C); weight (N, C, 3) -> y (T * B, N): y[r] = bias + sum_j xp[r + j B] W[:, :, j]^T."""
    if emulate_bf16:
        xp, weight = _RoundGrad.apply(_Round.apply(xp)), _Round.apply(weight)
    y = sum(xp[j * B:j * B + T * B] @ weight[:, :, j].t() for j in range(3))
    if bias is not None:
        y = y + bias
    return _Round.apply(y) if emulate_bf16 else y


def batchnorm_rows(x: torch.Tensor, gamma, beta, mean=None, var=None, relu: bool = True, emulate_bf16: bool = False, keep=None):
    """x (R, C).  mean / var None: batch statistics (they take part in the gradient); given: constants (evaluation mode).
    -> (out, batch mean, biased batch variance).  The kernels compute in fp32 from x as stored; the bf16 form rounds the stored output.
    ``keep``: float64 keep * scale of the dropout behind the ReLU (mmdeer_bn_time_apply's drop_site), or None."""
    bm, bv = x.mean(0), x.var(0, unbiased=False)
    m, v = (bm, bv) if mean is None else (mean, var)
    y = (x - m) / torch.sqrt(v + EPS) * gamma + beta
    if relu:
        y = torch.relu(y)
    if keep is not None:
        y = y * keep
    return (_Round.apply(y) if emulate_bf16 else y), bm.detach(), bv.detach()


def running_update(rm, rv, nbt, mean, var_biased, R: int):
    """nn.BatchNorm1d's buffer update after one training batch of R positions"""
    unbiased = var_biased * (R / (R - 1))
    return (1 - MOMENTUM) * rm + MOMENTUM * mean, (1 - MOMENTUM) * rv + MOMENTUM * unbiased, nbt + 1


def sites(B: int, T: int, p: float) -> list:
    """The sites one training forward of TemporalVideoEncoder draws, (name, site, rows, cols, p) (see temporal_ref.draw):
    spatial_projection's on the time-major rows t * B + b, the temporal CNN's ONE nn.Dropout (behind the first BatchNorm-ReLU,
    same rows; T = 1 skips the CNN), output_projection's on B rows."""
    from mmdeer import video
    cnn = [("cnn", video._SITE_CNN, T * B, W, p)] if T > 1 else []
    return [("sp", video._SITE_SP, T * B, W, p)] + cnn + [("op", video._SITE_OP, B, W, p)]


def encoder(P: dict, x: torch.Tensor, train: bool, masks=None, emulate_bf16: bool = False):
    """P: state_dict names -> float64 tensors; x (B, T, 512) or (B, 512).  -> (output (B, 512), buffers after the step: a dict
    with running_mean / running_var / num_batches_tracked of both BatchNorm layers; unchanged in evaluation mode and at T = 1).
    ``masks`` ({"sp", "cnn" (T > 1), "op"}: float64 keep * scale, see ``sites``; "cnn2": a mask on the SECOND BatchNorm layer,
    which the module must not have -- for the sensitivity test): the dropout decisions of a training forward.
    ``emulate_bf16`` rounds where the bf16 path stores bf16 going forward, and the gradients it stores coming back."""
    if x.dim() == 2:
        x = x.unsqueeze(1)
    B, T = x.shape[0], x.shape[1]
    e = emulate_bf16
    k = (lambda n: None) if masks is None else (lambda n: masks[n].to(x.device) if n in masks else None)
    g = (lambda t: _RoundGrad.apply(t)) if e else (lambda t: t)
    buffers = {f"{l}.{k_}": P[f"{l}.{k_}"] for l in BN_LAYERS for k_ in ("running_mean", "running_var", "num_batches_tracked")}
    if e:
        rows = linear(x.transpose(0, 1).reshape(T * B, W), P["spatial_projection.0.weight"], P["spatial_projection.0.bias"], True, k("sp"), e)
    else:
        h = torch.relu(x @ P["spatial_projection.0.weight"].t() + P["spatial_projection.0.bias"])      # (B, T, 512)
        rows = h.transpose(0, 1).reshape(T * B, W)                                                    # time-major
        rows = rows if k("sp") is None else rows * k("sp")
    if T > 1:
        for conv, bn, site in (("temporal_cnn.0", "temporal_cnn.1", "cnn"), ("temporal_cnn.4", "temporal_cnn.5", "cnn2")):
            y = g(conv3_time(pad_time(rows, B), P[f"{conv}.weight"], P[f"{conv}.bias"], T, B, e))     # dY: the stored dx of mmdeer_bn_time_bwd
            rm, rv = P[f"{bn}.running_mean"], P[f"{bn}.running_var"]
            rows, bm, bv = batchnorm_rows(y, P[f"{bn}.weight"], P[f"{bn}.bias"], None if train else rm, None if train else rv,
                                          emulate_bf16=e, keep=k(site))
            if train:
                buffers[f"{bn}.running_mean"], buffers[f"{bn}.running_var"], buffers[f"{bn}.num_batches_tracked"] = \
                    running_update(rm, rv, P[f"{bn}.num_batches_tracked"], bm, bv, T * B)
        feats = g(rows).reshape(T, B, W).transpose(0, 1)                                              # (B, T, 512)
        agg, _ = pool(feats, P, "temporal_attention", e)
    else:
        agg = rows
    # fusions._LinActLnFn: the bf16 form stores y = drop(relu(x W^T + b)) and the LayerNorm rows; coming back dz (masked) and dX
    y = linear(agg, P["output_projection.0.weight"], P["output_projection.0.bias"], True, k("op"), e)
    y = layer_norm(y, P["output_projection.3.weight"], P["output_projection.3.bias"], e, EPS)
    return y, buffers
