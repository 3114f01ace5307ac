"""Float64 restatement of the temporal audio encoder on a PADDED batch with per-sample lengths, built on tests/temporal_ref.py.  The
definition is the per-sample run: with lengths[b] = n_b, sample b is ``temporal_ref``'s function on x[b:b+1, :n_b] alone, its outputs
zero-padded back to T (what ``pad_packed_sequence(total_length=T)`` returns, and a pool weight of 0 at t >= n_b).  Gradients flow through
the slices, so autograd pads them with zeros too.  n_b = 0: a zero LSTM output, zero weights, a zero attended row -- and the encoder's
output row is what ``output_projection`` makes of zeros.  A dropout mask of a sample is the slice of the full batch's mask at that
sample's rows t * B + b (time-major sites) or b (the output projection's).  A helper module, not a test module."""
from __future__ import annotations

import torch

from . import temporal_ref as R

H = R.H


def _pad_t(v: torch.Tensor, T: int) -> torch.Tensor:
    """(1, n, C) -> (1, T, C), zeros behind"""
    return torch.cat([v, v.new_zeros(1, T - v.shape[1], v.shape[2])], dim=1) if v.shape[1] < T else v


def lstm_layer_with_lengths(x: torch.Tensor, P: dict, layer: int, lengths, emulate_bf16: bool = False, round_dgates: bool = False) -> torch.Tensor:
    """``temporal_ref.lstm_layer`` per sample at its own length on batch-first x (B, T, in) -> (B, T, 2H), zeros at t >= n_b."""
    B, T = x.shape[0], x.shape[1]
    rows = []
    for b in range(B):
        n = int(lengths[b])
        if n == 0:
            rows.append(x.new_zeros(1, T, 2 * P[f"weight_hh_l{layer}"].shape[1]))
        else:
            rows.append(_pad_t(R.lstm_layer(x[b:b + 1, :n], P, layer, emulate_bf16, round_dgates), T))
    return torch.cat(rows, 0)


def scores_pool_with_lengths(h: torch.Tensor, z: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor, lengths):
    """The pool operator from h (B, T, 2H) and z = W1 h + b1 (B, T, H) as given: per sample a softmax of w2 . tanh(z_t) + b2 over
    t < n_b -> (attended (B, 2H), weights (B, T) with zeros at t >= n_b); n_b = 0: zeros."""
    B, T = h.shape[0], h.shape[1]
    att, wts = [], []
    for b in range(B):
        n = int(lengths[b])
        if n == 0:
            att.append(h.new_zeros(1, h.shape[2]))
            wts.append(h.new_zeros(1, T))
            continue
        s = (torch.tanh(z[b:b + 1, :n]) @ w2.t() + b2)[..., 0]
        a = torch.softmax(s, dim=1)
        att.append((a.unsqueeze(-1) * h[b:b + 1, :n]).sum(1))
        wts.append(torch.cat([a, a.new_zeros(1, T - n)], dim=1))
    return torch.cat(att, 0), torch.cat(wts, 0)


def sample_masks(masks, b: int, n: int, B: int):
    """the masks of sample b alone at length n out of the full batch's: time-major sites rows t * B + b for t < n, the others row b"""
    if masks is None:
        return None
    return {k: (v[b:b + 1] if k == "op" else v[[t * B + b for t in range(n)]]) for k, v in masks.items()}


def encoder_with_lengths(P: dict, x: torch.Tensor, lengths, masks=None, emulate_bf16: bool = False, num_layers: int = 2):
    """``temporal_ref.encoder`` on x[b:b+1, :n_b] for every sample -> (output (B, 512), lstm_out (B, T, 512), weights (B, T)), the last two
    zero-padded to T.  ``masks``: the full batch's, as ``temporal_ref.draw(temporal_ref.sites(B, T, p), seed, step)`` with the sites of
    T > 1 draws them (a training forward with lengths runs the sequence path at every T)."""
    B, T = x.shape[0], x.shape[1]
    e = emulate_bf16
    outs, hs, ws = [], [], []
    for b in range(B):
        n = int(lengths[b])
        mb = sample_masks(masks, b, n, B)
        if n == 0:          # an empty utterance: a zero attended row through the projection
            att = x.new_zeros(1, 2 * H)
            y = R.linear(att, P["output_projection.0.weight"], P["output_projection.0.bias"], True, None if mb is None else mb["op"].to(x.device), e)
            y = R.linear(y, P["output_projection.3.weight"], P["output_projection.3.bias"], emulate_bf16=e)
            outs.append(R.layer_norm(y, P["output_projection.4.weight"], P["output_projection.4.bias"], e))
            hs.append(x.new_zeros(1, T, 2 * H))
            ws.append(x.new_zeros(1, T))
            continue
        y, h, a = R.encoder(P, x[b:b + 1, :n], num_layers, mb, e)
        outs.append(y)
        hs.append(_pad_t(h, T))
        ws.append(torch.cat([a, a.new_zeros(1, T - n)], dim=1))
    return torch.cat(outs, 0), torch.cat(hs, 0), torch.cat(ws, 0)
