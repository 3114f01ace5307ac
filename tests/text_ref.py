"""Float64 restatement of the temporal text encoder (encoders.EnhancedTextEncoder without BERT), written from its semantics:
token gather with clamped ids and positions, the binary mask on the embeddings, the attention pool whose softmax runs over
ALL positions and is then masked and renormalised with + 1e-10, the ten per-sample token statistics, and the three
projections in evaluation mode.  Runs on whatever device its tensors are on.  A helper module, not a test module.

``emulate_bf16`` rounds to bf16 where the HIP path stores bf16 -- the gathered rows x, the GEMM operands and outputs, the
pooled row -- so a bf16 run can be judged against the rounding it cannot avoid."""
from __future__ import annotations

import torch

from .temporal_ref import _Round, _RoundGrad, bf16, draw, layer_norm  # noqa: F401  (bf16, draw: for the tests that import this module)

EPS = 1e-10


def _r(x, emulate):
    return _Round.apply(x) if emulate else x


def gather(ids, mask, emb, pos, emulate_bf16=False):
    """ids (B, L) int64, mask (B, L) -> x (B, L, E) = (emb[clamp(id)] + pos[min(t, P - 1)]) * (mask != 0)."""
    V, P = emb.shape[0], pos.shape[0]
    t = torch.arange(ids.shape[1], device=ids.device).clamp(max=P - 1)
    rows = torch.nn.functional.embedding(ids.clamp(0, V - 1), emb, padding_idx=0)       # row 0 is read, and gets no gradient
    x = (rows + pos[t][None]) * (mask != 0).to(emb.dtype).unsqueeze(-1)
    return _r(x, emulate_bf16)


def table_grads(ids, mask, dx, V, P):
    """float64 index_add: (d_emb (V, E) with row 0 zero, d_pos (P, E)) of ``gather`` for the gradient dx (B, L, E) at x."""
    B, L, E = dx.shape
    g = (dx.double() * (mask != 0).double().unsqueeze(-1)).reshape(B * L, E)
    d_emb = torch.zeros(V, E, dtype=torch.float64, device=dx.device).index_add_(0, ids.clamp(0, V - 1).reshape(-1), g)
    d_emb[0] = 0                                                      # padding_idx = 0
    t = torch.arange(L, device=dx.device).clamp(max=P - 1).repeat(B)
    d_pos = torch.zeros(P, E, dtype=torch.float64, device=dx.device).index_add_(0, t, g)
    return d_emb, d_pos


def masked_pool(x, z, mask, w2, b2):
    """x (B, L, E) already masked, z (B, L, A) = W1 x + b1, mask (B, L), w2 (1, A) or (A,), b2 (1,)
    -> (attended (B, E), weights a (B, L), softmax p (B, L))."""
    m = (mask != 0).to(x.dtype)
    s = torch.tanh(z) @ w2.reshape(-1) + b2.reshape(())
    p = torch.softmax(s, dim=1)
    pm = p * m
    a = pm / (pm.sum(1, keepdim=True) + EPS)
    return (a.unsqueeze(-1) * x).sum(1), a, p


def stats(ids, mask, max_length):
    """ids (B, L) integer, mask (B, L) -> (B, 10) float64 and the exact integer counts (B, 6) = n, u, c_max, id_max, punct, special."""
    B = ids.shape[0]
    out = torch.zeros(B, 10, dtype=torch.float64)
    counts = torch.zeros(B, 6, dtype=torch.int64)
    for b in range(B):
        v = ids[b][mask[b] != 0].cpu().tolist()
        n = len(v)
        if n == 0:
            counts[b, 3] = -1
            continue
        mult = {}
        for t in v:
            mult[t] = mult.get(t, 0) + 1
        u, cmax, idmax = len(mult), max(mult.values()), max(v)
        punct, special = sum(999 <= t <= 1030 for t in v), sum(100 <= t <= 999 for t in v)
        counts[b] = torch.tensor([n, u, cmax, idmax, punct, special])
        out[b, :6] = torch.tensor([n / max_length, u / n, n / (idmax + 1), cmax, punct / n, special / n], dtype=torch.float64)
    return out, counts


def _g(x, emulate):
    """a gradient the HIP path stores in bf16 on its way back (identity going forward)"""
    return _RoundGrad.apply(x) if emulate else x


def _linear(x, P, name, emulate, relu=False, keep=None):
    """drop?(relu?(x W^T + b)); ``keep``: float64 keep * scale or None.  The bf16 form rounds what fusions._LinearFn stores: x, W
    and the output; coming back the incoming gradient, the masked gradient ``ga`` and dX."""
    y = _g(_g(_r(x, emulate), emulate) @ _r(P[name + ".weight"], emulate).t() + P[name + ".bias"], emulate)
    y = torch.relu(y) if relu else y
    if keep is not None:
        y = y * keep.to(y.device)
    return _g(_r(y, emulate), emulate)


def sites(B: int, hidden_dim: int, p: float) -> list:
    """The three sites one training forward of TemporalTextEncoder draws, (name, site, rows, cols, p): the reference's three
    nn.Dropout modules, each on B rows (see temporal_ref.draw)."""
    from mmdeer import text
    return [("bert", text._SITE_BERT, B, hidden_dim, p), ("ling", text._SITE_LING, B, hidden_dim // 4, p), ("out", text._SITE_OUT, B, hidden_dim, p)]


def tail(P, x, ids_stats, mask, max_length=128, emulate_bf16=False, masks=None):
    """From the masked rows x (B, L, E): pool, projections, LayerNorm.  ``masks`` None: evaluation mode; given ({"bert", "ling",
    "out"}: float64 keep * scale, see ``sites``): the training forward with those dropout decisions.
    Returns (output (B, H), weights (B, L), features (B, 10))."""
    e = emulate_bf16
    k = (lambda n: None) if masks is None else (lambda n: masks[n])
    x = _g(x, e)                                                       # dx of mmdeer_token_pool_bwd + dX of the W1 GEMM, summed, as bf16
    z = _linear(x, P, "token_attention.0", e)
    att, a, _ = masked_pool(_g(x, e), z, mask, P["token_attention.2.weight"], P["token_attention.2.bias"])
    pb = _linear(_g(_r(att, e), e), P, "bert_projection.0", e, relu=True, keep=k("bert"))
    f, _ = stats(ids_stats, mask, max_length)
    f = f.to(x.device).to(x.dtype)
    pl = _linear(f, P, "linguistic_projection.0", e, relu=True, keep=k("ling"))
    y = _linear(torch.cat([pb, pl], dim=1), P, "output_projection.0", e, relu=True, keep=k("out"))
    # the bf16 form rounds the LayerNorm rows too: side._LayerNormFn stores them in the compute dtype
    y = layer_norm(y, P["output_projection.3.weight"], P["output_projection.3.bias"], e)
    return y, a, f


def encoder(P, ids, mask, max_length=128, emulate_bf16=False, masks=None):
    """forward(ids, mask) of the no-BERT encoder, parameters under their state_dict names; evaluation mode, or with ``masks`` the
    training forward (see ``tail``)."""
    V = P["embedding.weight"].shape[0]
    x = gather(ids, mask, P["embedding.weight"], P["positional_encoding.weight"], emulate_bf16)
    return tail(P, x, ids.clamp(0, V - 1), mask, max_length, emulate_bf16, masks)


def encoder_embeddings(P, E, ids, mask, max_length=128, emulate_bf16=False, masks=None):
    """BERT branch downstream of last_hidden_state: E (B, L, 768) contextual embeddings, ids unclamped (statistics only);
    evaluation mode, or with ``masks`` the training forward (see ``tail``)."""
    x = _r(E * (mask != 0).to(E.dtype).unsqueeze(-1), emulate_bf16)
    return tail(P, x, ids, mask, max_length, emulate_bf16, masks)
