"""Float64 restatement of the temporal audio encoder (encoders.EnhancedAudioEncoder on (B, T, 84) features), written from its
semantics: bidirectional LSTM with zero initial state and torch gate order i, f, g, o; the reverse direction reads the steps
backwards and stores its state at the step it consumed; the attention pool s = w2 . tanh(W1 h + b1) + b2 with a softmax over
time; output_projection in evaluation mode.  Runs on whatever device its tensors are on (CPU for the golden checks; the GPU
tests run the same float64 arithmetic on the GPU for speed).  A helper module, not a test module.

``lstm_layer`` also has a bf16-emulating form: it rounds to bf16 where the HIP path stores or feeds bf16 -- the input, the
weights, the input-gate GEMM output, h (the recurrent MFMA operand and the layer output) and the gate gradients that the
backward feeds to its recurrent product -- so a bf16 run can be judged against the rounding it cannot avoid."""
from __future__ import annotations

import torch

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


def lstm_layer(x: torch.Tensor, P: dict, layer: int, emulate_bf16: bool = False) -> torch.Tensor:
    """One bidirectional layer on batch-first x (B, T, in) with parameters P (state_dict names of nn.LSTM, prefix-free)
    -> (B, T, 2H) = [forward | reverse]."""
    outs = []
    for sfx, rev in (("", False), ("_reverse", True)):
        wih, whh = P[f"weight_ih_l{layer}{sfx}"], P[f"weight_hh_l{layer}{sfx}"]
        b = P[f"bias_ih_l{layer}{sfx}"] + P[f"bias_hh_l{layer}{sfx}"]
        xt = x.transpose(0, 1)                                            # (T, B, in)
        if emulate_bf16:
            xg = _Round.apply(_Round.apply(xt) @ _Round.apply(wih).t() + b)
        else:
            xg = xt @ wih.t() + b
        outs.append(lstm_direction(xg, whh, rev, emulate_bf16))
    return torch.cat(outs, dim=2).transpose(0, 1)


def attention_pool(h: torch.Tensor, w1, b1, w2, b2):
    """h (B, T, 2H) -> (attended (B, 2H), weights (B, T))"""
    s = (torch.tanh(h @ w1.t() + b1) @ w2.t() + b2)[..., 0]              # (B, T)
    a = torch.softmax(s, dim=1)
    return (a.unsqueeze(-1) * h).sum(1), a


def encoder(P: dict, x: torch.Tensor, num_layers: int = 2):
    """Eval-mode forward of encoders.EnhancedAudioEncoder's feature branch on (B, T, 84), parameters under their state_dict
    names.  Returns (output (B, 512), lstm_out (B, T, 512), attention weights (B, T))."""
    L = {k[len("lstm."):]: v for k, v in P.items() if k.startswith("lstm.")}
    h = x
    for layer in range(num_layers):
        h = lstm_layer(h, L, layer)
    att, a = attention_pool(h, P["attention.0.weight"], P["attention.0.bias"], P["attention.2.weight"], P["attention.2.bias"])
    y = torch.relu(att @ P["output_projection.0.weight"].t() + P["output_projection.0.bias"])
    y = y @ P["output_projection.3.weight"].t() + P["output_projection.3.bias"]
    y = torch.nn.functional.layer_norm(y, (y.shape[1],), P["output_projection.4.weight"], P["output_projection.4.bias"], 1e-5)
    return y, h, a
