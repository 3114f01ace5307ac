"""What ``transformers.BertModel.forward`` computes (eval mode, absolute positions, erf GELU), restated in float64 in plain torch
from a ``state_dict``: one function per operator of include/mmdeer_bert.h and one for the whole trunk.  Two departures from the
reference, both the library's own rules: ids are clamped to the vocabulary, and a sample without a valid key gets ZEROS from the
attention (the reference averages V uniformly there, up to rounding).  Masked keys are excluded exactly; for a sample with a valid
key that equals the reference's additive ``finfo.min`` mask (test_cpu_bert compares against a live BertModel).

``rnd``: applied to every tensor the HIP path stores in its compute dtype (the embedding output, qkv, ctx, the GEMM outputs, the
GELU output, the LayerNorm outputs) and to the weight matrices it casts -- the identity for the float64 yardstick, a round trip
through bf16 for the measure of what bf16 storage alone costs."""
import math

import torch

HEAD = 64


def ident(t):
    return t


def bf16_round(t):
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def layer_norm(x, gamma, beta, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * gamma + beta


def add_ln(y, x, gamma, beta, eps):
    return layer_norm(y + x if x is not None else y, gamma, beta, eps)


def embed_ln(word, pos, typ, gamma, beta, eps, ids, type_ids=None):
    """ids (B, L) -> (B, L, H): LayerNorm(word[clamp(id)] + type[tt] + pos[t])"""
    B, L = ids.shape
    idc = ids.long().clamp(0, word.shape[0] - 1)
    tt = torch.zeros_like(idc) if type_ids is None else type_ids.long().clamp(0, typ.shape[0] - 1)
    return layer_norm(word[idc] + typ[tt] + pos[torch.arange(L)].unsqueeze(0), gamma, beta, eps)


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_tanh(x):
    """the OTHER formula (hidden_act = "gelu_new"): what the erf form must not be mistaken for"""
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def attention(qkv, mask, B, L, H):
    """qkv (B * L, >= 3 H) columns [Q | K | V], mask (B * L) -> ctx (B * L, H); heads of 64, scale 1 / 8"""
    heads = H // HEAD
    q, k, v = (qkv[:, i * H:(i + 1) * H].reshape(B, L, heads, HEAD).permute(0, 2, 1, 3) for i in range(3))
    valid = (mask.reshape(B, 1, 1, L) != 0)
    some = valid.any(-1, keepdim=True)
    s = (q @ k.transpose(-1, -2)) / 8.0
    s = torch.where(valid, s, torch.full_like(s, -math.inf))
    p = torch.softmax(torch.where(some, s, torch.zeros_like(s)), dim=-1) * valid * some
    return (p @ v).permute(0, 2, 1, 3).reshape(B * L, H)


def trunk(sd, ids, mask=None, type_ids=None, eps=1e-12, rnd=ident):
    """sd: a BertModel state_dict (any float dtype) -> [embedding output, layer 0's output, ...], each (B, L, H) float64"""
    w = {k: v.double() for k, v in sd.items()}
    B, L = ids.shape
    H = w["embeddings.word_embeddings.weight"].shape[1]
    m = torch.ones(B * L, dtype=torch.float64) if mask is None else (mask.reshape(-1) != 0).double()
    e = "embeddings."
    x = rnd(embed_ln(w[e + "word_embeddings.weight"], w[e + "position_embeddings.weight"], w[e + "token_type_embeddings.weight"],
                     w[e + "LayerNorm.weight"], w[e + "LayerNorm.bias"], eps, ids, type_ids)).reshape(B * L, H)
    states = [x.reshape(B, L, H)]
    n = 0
    while f"encoder.layer.{n}.attention.self.query.weight" in w:
        p = f"encoder.layer.{n}."
        lin = lambda t, name: rnd(t @ rnd(w[p + name + ".weight"]).T + w[p + name + ".bias"])     # noqa: E731
        qkv = torch.cat([lin(x, "attention.self." + r) for r in ("query", "key", "value")], dim=1)
        ctx = rnd(attention(qkv, m, B, L, H))
        x = rnd(add_ln(lin(ctx, "attention.output.dense"), x, w[p + "attention.output.LayerNorm.weight"], w[p + "attention.output.LayerNorm.bias"], eps))
        h = rnd(gelu(lin(x, "intermediate.dense")))
        x = rnd(add_ln(lin(h, "output.dense"), x, w[p + "output.LayerNorm.weight"], w[p + "output.LayerNorm.bias"], eps))
        states.append(x.reshape(B, L, H))
        n += 1
    return states
