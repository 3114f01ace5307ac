"""Float64 restatement of the temporal audio encoder (encoders.EnhancedAudioEncoder on (B, T, 84) features), written from its
semantics: bidirectional LSTM with zero initial state and torch gate order i, f, g, o; the reverse direction reads the steps
backwards and stores its state at the step it consumed; the attention pool s = w2 . tanh(W1 h + b1) + b2 with a softmax over
time; output_projection in evaluation mode.  Runs on whatever device its tensors are on (CPU for the golden checks; the GPU
tests run the same float64 arithmetic on the GPU for speed).  A helper module, not a test module.

``lstm_layer`` also has a bf16-emulating form: it rounds to bf16 where the HIP path stores or feeds bf16 -- the input, the
weights, the input-gate GEMM output, h (the recurrent MFMA operand and the layer output) and the gate gradients that the
backward feeds to its recurrent product -- so a bf16 run can be judged against the rounding it cannot avoid."""
from __future__ import annotations

import numpy as np
import torch

from .rowkernel_ref import drop_keep, drop_threshold

H = 256


def bf16(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.bfloat16).to(x.dtype)


class _RoundGrad(torch.autograd.Function):
    """identity; the gradient passing through is rounded to bf16 (a bf16 operand of the backward's product)"""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return bf16(g)


class _Round(torch.autograd.Function):
    """bf16 rounding of a stored value; the gradient passes unchanged"""

    @staticmethod
    def forward(ctx, x):
        return bf16(x)

    @staticmethod
    def backward(ctx, g):
        return g


def lstm_direction(xg: torch.Tensor, w_hh: torch.Tensor, reverse: bool, emulate_bf16: bool = False):
    """xg (T, B, 4H) = W_ih x + b_ih + b_hh of one direction -> h (T, B, H); h[t] is the state after consuming x_t."""
    T, B = xg.shape[0], xg.shape[1]
    Hd = w_hh.shape[1]
    w = _Round.apply(w_hh) if emulate_bf16 else w_hh
    h = xg.new_zeros(B, Hd)
    c = xg.new_zeros(B, Hd)
    out = [None] * T
    for s in range(T):
        t = T - 1 - s if reverse else s
        rec = h @ w.t()
        if emulate_bf16:
            rec = _RoundGrad.apply(rec)
        g = xg[t] + rec
        i, f, gg, o = torch.sigmoid(g[:, :Hd]), torch.sigmoid(g[:, Hd:2 * Hd]), torch.tanh(g[:, 2 * Hd:3 * Hd]), torch.sigmoid(g[:, 3 * Hd:])
        c = f * c + i * gg
        h = o * torch.tanh(c)
        if emulate_bf16:
            h = _Round.apply(h)
        out[t] = h
    return torch.stack(out, 0)


def lstm_layer(x: torch.Tensor, P: dict, layer: int, emulate_bf16: bool = False, round_dgates: bool = False) -> torch.Tensor:
    """One bidirectional layer on batch-first x (B, T, in) with parameters P (state_dict names of nn.LSTM, prefix-free)
    -> (B, T, 2H) = [forward | reverse].  ``round_dgates`` (with ``emulate_bf16``): the gate gradients are rounded to bf16 on
    their way to the input GEMM's backward too (the stored ``dgates`` matrix of mmdeer_lstm_seq_bwd)."""
    outs = []
    for sfx, rev in (("", False), ("_reverse", True)):
        wih, whh = P[f"weight_ih_l{layer}{sfx}"], P[f"weight_hh_l{layer}{sfx}"]
        b = P[f"bias_ih_l{layer}{sfx}"] + P[f"bias_hh_l{layer}{sfx}"]
        xt = x.transpose(0, 1)                                            # (T, B, in)
        if emulate_bf16:
            xg = _Round.apply(_Round.apply(xt) @ _Round.apply(wih).t() + b)
            if round_dgates:
                xg = _RoundGrad.apply(xg)
        else:
            xg = xt @ wih.t() + b
        outs.append(lstm_direction(xg, whh, rev, emulate_bf16))
    return torch.cat(outs, dim=2).transpose(0, 1)


def attention_pool(h: torch.Tensor, w1, b1, w2, b2):
    """h (B, T, 2H) -> (attended (B, 2H), weights (B, T))"""
    s = (torch.tanh(h @ w1.t() + b1) @ w2.t() + b2)[..., 0]              # (B, T)
    a = torch.softmax(s, dim=1)
    return (a.unsqueeze(-1) * h).sum(1), a


# ----------------------------------------------------------------------------------------------------- the training form
# A dropout site of a module is (name, site number, rows, cols, p): the library draws one decision per (row, column) of that
# matrix from (seed, step, site).  ``draw`` restates the draw on the CPU (rowkernel_ref.drop_keep, tied bit for bit to
# mmdeer_dropout_mask by tests/test_gpu_rowkernels.py) and returns what the references multiply by: float64 keep * scale with
# scale = float32(1 / (1 - float32(p))) (rowkernel_ref.drop_threshold).
def drop_mask(site: int, rows: int, cols: int, p: float, seed: int, step: int, scale=None) -> torch.Tensor:
    keep = drop_keep(site, rows, cols, p, seed, step)
    return torch.from_numpy(keep.astype(np.float64)) * (drop_threshold(p)[1] if scale is None else scale)


def seed_offset(record) -> int:
    """what a site record adds to the module's seed: its optional sixth entry, 0 where a record has five"""
    return record[5] if len(record) > 5 else 0


def draw(sites, seed: int, step: int) -> dict:
    """{name: float64 keep * scale (rows, cols)} of a list of sites at one dropout step; a record is (name, site, rows, cols, p) or
    (name, site, rows, cols, p, seed offset) -- a launch that draws under the module's seed + an offset of its own"""
    return {r[0]: drop_mask(r[1], r[2], r[3], r[4], seed + seed_offset(r), step) for r in sites}


def sites(B: int, T: int, p: float, num_layers: int = 2) -> list:
    """The sites one training forward of TemporalAudioEncoder draws on (B, T, 84): the LSTM's inter-layer dropout on the
    time-major rows t * B + b (T > 1: temporal._SITE_SEQ + layer; T = 1 is the parent's path: side._SITE_LSTM + layer on B
    rows) and the output projection's (side._SITE_OP)."""
    from mmdeer import side, temporal
    base = temporal._SITE_SEQ if T > 1 else side._SITE_LSTM
    return [(f"inter.{l}", base + l, T * B, 2 * H, p) for l in range(num_layers - 1)] + [("op", side._SITE_OP, B, 2 * H, p)]


def linear(x, w, b, relu: bool = False, mask=None, emulate_bf16: bool = False):
    """drop?(relu?(x W^T + b)).  The bf16 form rounds where fusions._LinearFn stores bf16: x, W and the output going forward;
    coming back the incoming gradient, the masked gradient ``ga`` (both GEMMs of the backward read it) and dX."""
    if not emulate_bf16:
        y = x @ w.t() + b
        y = torch.relu(y) if relu else y
        return y if mask is None else y * mask
    y = _RoundGrad.apply(_RoundGrad.apply(_Round.apply(x)) @ _Round.apply(w).t() + b)
    y = torch.relu(y) if relu else y
    y = y if mask is None else y * mask
    return _RoundGrad.apply(_Round.apply(y))


def pool(h, P: dict, prefix: str, emulate_bf16: bool = False):
    """``attention_pool`` under the parameters ``prefix``.{0,2}.*; the bf16 form rounds z = W1 h + b1, the attended row and,
    coming back, dh and dz (the stored outputs of mmdeer_temporal_pool_bwd) and the gradient sum that reaches h."""
    w1, b1, w2, b2 = (P[f"{prefix}.{k}"] for k in ("0.weight", "0.bias", "2.weight", "2.bias"))
    if not emulate_bf16:
        return attention_pool(h, w1, b1, w2, b2)
    h = _RoundGrad.apply(h)
    z = linear(h, w1, b1, emulate_bf16=True)
    hp = _RoundGrad.apply(h)
    s = (torch.tanh(z) @ w2.t() + b2)[..., 0]
    a = torch.softmax(s, dim=1)
    return _RoundGrad.apply(_Round.apply((a.unsqueeze(-1) * hp).sum(1))), a


def layer_norm(y, gamma, beta, emulate_bf16: bool = False, eps: float = 1e-5):
    out = torch.nn.functional.layer_norm(y, (y.shape[1],), gamma, beta, eps)
    return _RoundGrad.apply(_Round.apply(out)) if emulate_bf16 else out      # the stored LayerNorm rows; bf16(g) read back


def encoder(P: dict, x: torch.Tensor, num_layers: int = 2, masks=None, emulate_bf16: bool = False):
    """Forward of encoders.EnhancedAudioEncoder's feature branch on (B, T, 84), parameters under their state_dict names.
    ``masks`` None: evaluation mode.  Given ({"inter.<l>": (T * B, 512) on time-major rows, "op": (B, 512)}, float64
    keep * scale, see ``sites``): the training forward with exactly those dropout decisions.
    Returns (output (B, 512), lstm_out (B, T, 512), attention weights (B, T))."""
    L = {k[len("lstm."):]: v for k, v in P.items() if k.startswith("lstm.")}
    e = emulate_bf16
    B, T = x.shape[0], x.shape[1]
    h = x
    for layer in range(num_layers):
        if e:
            h = _RoundGrad.apply(lstm_layer(_RoundGrad.apply(h), L, layer, True, round_dgates=True))
        else:
            h = lstm_layer(h, L, layer)
        if masks is not None and layer + 1 < num_layers:
            h = h * masks[f"inter.{layer}"].to(h.device).reshape(T, B, -1).transpose(0, 1)       # rows t * B + b
            if e:
                h = _RoundGrad.apply(_Round.apply(h))               # the stored output of side._DropoutFn
    if e and T == 1:
        att, a = h[:, 0], h.new_ones(B, 1)                          # the parent's path runs no pool kernel
    else:
        att, a = pool(h, P, "attention", e)
    y = linear(att, P["output_projection.0.weight"], P["output_projection.0.bias"], True, None if masks is None else masks["op"].to(h.device), e)
    y = linear(y, P["output_projection.3.weight"], P["output_projection.3.bias"], emulate_bf16=e)
    y = layer_norm(y, P["output_projection.4.weight"], P["output_projection.4.bias"], e)
    return y, h, a
