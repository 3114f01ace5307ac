"""Float64 restatement of the BERT trunk WITH its dropout (include/mmdeer_bert_drop.h, mmdeer.bert.BertEncoder(dropout=True)): the
operator functions of tests/bert_ref.py and tests/bert_bwd_ref.py with a mask argument, and the trunk's layer sequence with the
masks where transformers.BertModel has them in train().  A helper module, not a test module.

THE MASK, stated once for the tests: a site draws one decision per (row, col) from (seed, step, site) by the library's counter hash,
restated in NumPy by rowkernel_ref.drop_keep; what the references multiply by is m = keep * float32(1 / (1 - float32(p)))
(temporal_ref.drop_mask).  Masks are always drawn here, on the CPU, never by the library.
  hidden sites     row = b * L + t, col = n in [0, H): the embeddings (SITE_EMBED), and per layer the self-output and output sites
  attention site   row = (b * heads + h) * L + i (the query), col = j (the key)
Site ids: mmdeer.bert.SITE_EMBED, and mmdeer.bert.site(layer, place) with place 0 attention, 1 self-output, 2 output.

``rnd``: as in bert_ref / bert_bwd_ref.  The tape is unchanged, so the forward rounding points are bert_ref.trunk's (y and y2 are
stored pre-dropout); the backward has two more stored gradients, dy1 and dy2 (the gradients of the dense outputs, ds o m)."""
import math

import torch

from . import bert_bwd_ref as RB
from . import bert_ref as R
from .temporal_ref import draw, drop_mask  # noqa: F401  (re-exported: the tests draw through this module)


def sites(B, L, H, heads, layers, p_h, p_a):
    """[(name, site id, rows, cols, p)] of one training forward, in transformers' call order; a site of probability 0 is not drawn"""
    from mmdeer import bert
    out = [("embed", bert.SITE_EMBED, B * L, H, p_h)]
    for l in range(layers):
        out += [(f"attn.{l}", bert.site(l, 0), B * heads * L, L, p_a), (f"self_out.{l}", bert.site(l, 1), B * L, H, p_h),
                (f"out.{l}", bert.site(l, 2), B * L, H, p_h)]
    return [s for s in out if s[4] > 0]


def _m(masks, name):
    return None if masks is None else masks.get(name)


def mul(t, m):
    return t if m is None else t * m.reshape(t.shape)


# ------------------------------------------------------------------------------------------------ single operators
def attention(qkv, mask, B, L, H, m=None):
    """bert_ref.attention with ctx = (P o m) V; m (B * heads * L, L) or None"""
    heads = H // R.HEAD
    q, k, v = (qkv[:, i * H:(i + 1) * H].reshape(B, L, heads, R.HEAD).permute(0, 2, 1, 3) for i in range(3))
    valid = (mask.reshape(B, 1, 1, L) != 0)
    some = valid.any(-1, keepdim=True)
    s = (q @ k.transpose(-1, -2)) / 8.0
    s = torch.where(valid, s, torch.full_like(s, -math.inf))
    p = torch.softmax(torch.where(some, s, torch.zeros_like(s)), dim=-1) * valid * some
    return (mul(p, m) @ v).permute(0, 2, 1, 3).reshape(B * L, H)


def add_ln(y, x, gamma, beta, eps, m=None):
    """LayerNorm(y m + x)"""
    s = mul(y, m)
    return R.layer_norm(s + x if x is not None else s, gamma, beta, eps)


def embed_ln(word, pos, typ, gamma, beta, eps, ids, type_ids=None, m=None):
    return mul(R.embed_ln(word, pos, typ, gamma, beta, eps, ids, type_ids), m)


def attention_bwd(qkv, mask, dctx, B, L, H, m=None):
    q = RB.leaf(qkv[:, :3 * H])
    (d,) = torch.autograd.grad((attention(q, mask.double(), B, L, H, m) * dctx.double()).sum(), [q])
    return d


def add_ln_bwd(y, x, g, g2, gamma, beta, eps, m=None):
    """-> (ds, dy, dgamma, dbeta) of out = LayerNorm(y m + x) under the upstream gradient g + g2: ds the gradient of x, dy = ds o m of y"""
    yy, ga, be = RB.leaf(y), RB.leaf(gamma), RB.leaf(beta)
    xx = RB.leaf(x if x is not None else torch.zeros_like(y))
    G = g.double() if g2 is None else g.double() + g2.double()
    dy, ds, dga, dbe = torch.autograd.grad((R.layer_norm(mul(yy, m) + xx, ga, be, eps) * G).sum(), [yy, xx, ga, be])
    return ds, dy, dga, dbe


# ------------------------------------------------------------------------------------------------ the trunk
def trunk(sd, ids, mask=None, type_ids=None, masks=None, eps=1e-12, rnd=R.ident):
    """bert_ref.trunk with ``masks`` = {site name: m} (draw(sites(...), seed, step)) in the places above"""
    w = {k: v.double() for k, v in sd.items()}
    B, L = ids.shape
    H = w["embeddings.word_embeddings.weight"].shape[1]
    m = torch.ones(B * L, dtype=torch.float64) if mask is None else (mask.reshape(-1) != 0).double()
    e = "embeddings."
    x = rnd(embed_ln(w[e + "word_embeddings.weight"], w[e + "position_embeddings.weight"], w[e + "token_type_embeddings.weight"],
                     w[e + "LayerNorm.weight"], w[e + "LayerNorm.bias"], eps, ids, type_ids, _m(masks, "embed"))).reshape(B * L, H)
    states = [x.reshape(B, L, H)]
    n = 0
    while f"encoder.layer.{n}.attention.self.query.weight" in w:
        p = f"encoder.layer.{n}."
        lin = lambda t, name: rnd(t @ rnd(w[p + name + ".weight"]).T + w[p + name + ".bias"])     # noqa: E731
        qkv = torch.cat([lin(x, "attention.self." + r) for r in ("query", "key", "value")], dim=1)
        ctx = rnd(attention(qkv, m, B, L, H, _m(masks, f"attn.{n}")))
        x = rnd(add_ln(lin(ctx, "attention.output.dense"), x, w[p + "attention.output.LayerNorm.weight"], w[p + "attention.output.LayerNorm.bias"],
                       eps, _m(masks, f"self_out.{n}")))
        h = rnd(R.gelu(lin(x, "intermediate.dense")))
        x = rnd(add_ln(lin(h, "output.dense"), x, w[p + "output.LayerNorm.weight"], w[p + "output.LayerNorm.bias"], eps, _m(masks, f"out.{n}")))
        states.append(x.reshape(B, L, H))
        n += 1
    return states


def trunk_grads(sd, ids, mask, type_ids, upstream, masks=None, eps=1e-12, rnd=R.ident):
    """bert_bwd_ref.trunk_grads with the masks; gradient rounding points as there, plus dy1 and dy2"""
    fr, gr = RB._straight(rnd), RB._grad_round(rnd)
    w = {k: RB.leaf(v) for k, v in sd.items()}
    B, L = ids.shape
    H = w["embeddings.word_embeddings.weight"].shape[1]
    m = torch.ones(B * L, dtype=torch.float64) if mask is None else (mask.reshape(-1) != 0).double()
    e = "embeddings."
    x = fr(embed_ln(w[e + "word_embeddings.weight"], w[e + "position_embeddings.weight"], w[e + "token_type_embeddings.weight"],
                    w[e + "LayerNorm.weight"], w[e + "LayerNorm.bias"], eps, ids, type_ids, _m(masks, "embed"))).reshape(B * L, H)
    states = [x.detach().reshape(B, L, H)]
    n = 0
    while f"encoder.layer.{n}.attention.self.query.weight" in w:
        p = f"encoder.layer.{n}."
        lin = lambda t, name: fr(t @ fr(w[p + name + ".weight"]).T + w[p + name + ".bias"])     # noqa: E731
        xl = gr(x)                                                                                   # dx
        qkv = gr(torch.cat([lin(xl, "attention.self." + r) for r in ("query", "key", "value")], dim=1))        # dqkv
        ctx = gr(fr(attention(qkv, m, B, L, H, _m(masks, f"attn.{n}"))))                             # dctx
        y = gr(lin(ctx, "attention.output.dense"))                                                   # dy1
        s1 = gr(mul(y, _m(masks, f"self_out.{n}")) + x)                                              # ds1
        x1 = fr(R.layer_norm(s1, w[p + "attention.output.LayerNorm.weight"], w[p + "attention.output.LayerNorm.bias"], eps))
        h = gr(lin(gr(x1), "intermediate.dense"))                                                    # dh' at h, dx1 at x1
        gh = gr(fr(R.gelu(h)))                                                                       # dh
        y2 = gr(lin(gh, "output.dense"))                                                             # dy2
        s2 = gr(mul(y2, _m(masks, f"out.{n}")) + x1)                                                 # ds2
        x = fr(R.layer_norm(s2, w[p + "output.LayerNorm.weight"], w[p + "output.LayerNorm.bias"], eps))
        states.append(x.detach().reshape(B, L, H))
        n += 1
    out = gr(x).reshape(B, L, H)
    names = list(w)
    grads = torch.autograd.grad((out * upstream.double()).sum(), [w[k] for k in names], allow_unused=True)
    return states, {k: g for k, g in zip(names, grads) if g is not None}
