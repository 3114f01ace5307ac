"""Float64 restatement of the BERT trunk's BACKWARD (include/mmdeer_bert_bwd.h, mmdeer.bert._TailFn): gradients by autograd through
the operator functions of tests/bert_ref.py on the kernels' own stored operands, and the trunk's parameter gradients by autograd
through the same layer sequence as bert_ref.trunk.  A helper module, not a test module.

``rnd``: the identity for the float64 yardstick, ``bert_ref.bf16_round`` for the measure of what bf16 STORAGE alone costs.  It is
applied in two ways.  Forward, where bert_ref.trunk applies it (every tensor the HIP path stores in its compute dtype, and the
weight matrices it casts), with the gradient passed straight through -- a plain ``.to(bfloat16)`` under autograd would round the
gradient too, at points where the HIP path stores none.  Backward, to each gradient tensor the HIP path stores in its compute
dtype: g (the gradient of a layer's output that arrives through the layer above: dx), ds2, dh, dh', dx1, ds1, dctx, dqkv; there the
hook is an identity whose backward rounds."""
import torch

from . import bert_ref as R


def _straight(rnd):
    """x -> rnd(x) with the gradient passed through unchanged"""
    if rnd is R.ident:
        return R.ident

    class Fn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return rnd(x)

        @staticmethod
        def backward(ctx, g):
            return g

    return Fn.apply


def _grad_round(rnd):
    """x -> x with the gradient that arrives rounded by rnd"""
    if rnd is R.ident:
        return R.ident

    class Fn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return x.view_as(x)

        @staticmethod
        def backward(ctx, g):
            return rnd(g)

    return Fn.apply


def leaf(t):
    return t.detach().double().clone().requires_grad_(True)


# ------------------------------------------------------------------------------------------------ single operators
def attention_bwd(qkv, mask, dctx, B, L, H):
    """qkv (B * L, >= 3 H), dctx (B * L, H) -> dqkv (B * L, 3 H), columns [dQ | dK | dV]"""
    q = leaf(qkv[:, :3 * H])
    (d,) = torch.autograd.grad((R.attention(q, mask.double(), B, L, H) * dctx.double()).sum(), [q])
    return d


def add_ln_bwd(y, x, g, g2, gamma, beta, eps):
    """-> (ds, dgamma, dbeta) of out = LayerNorm(y + x; gamma, beta, eps) under the upstream gradient g + g2"""
    s, ga, be = leaf(y if x is None else y.double() + x.double()), leaf(gamma), leaf(beta)
    G = g.double() if g2 is None else g.double() + g2.double()
    return torch.autograd.grad((R.layer_norm(s, ga, be, eps) * G).sum(), [s, ga, be])


def gelu_bwd(x, g):
    xx = leaf(x)
    (d,) = torch.autograd.grad((R.gelu(xx) * g.double()).sum(), [xx])
    return d


def gelu_tanh_bwd(x, g):
    """the derivative of the OTHER formula: what the erf form's must not be mistaken for"""
    xx = leaf(x)
    (d,) = torch.autograd.grad((R.gelu_tanh(xx) * g.double()).sum(), [xx])
    return d


# ------------------------------------------------------------------------------------------------ the trunk
def trunk_grads(sd, ids, mask, type_ids, upstream, eps=1e-12, rnd=R.ident):
    """sd: a BertModel state_dict; loss = sum(last_hidden_state * upstream), upstream (B, L, H) ->
    (last_hidden_state (B, L, H) float64, {name: gradient} for every floating-point entry of sd that takes part).  The layer
    sequence is bert_ref.trunk's, operator for operator."""
    fr, gr = _straight(rnd), _grad_round(rnd)
    w = {k: leaf(v) for k, v in sd.items()}
    B, L = ids.shape
    H = w["embeddings.word_embeddings.weight"].shape[1]
    m = torch.ones(B * L, dtype=torch.float64) if mask is None else (mask.reshape(-1) != 0).double()
    e = "embeddings."
    x = fr(R.embed_ln(w[e + "word_embeddings.weight"], w[e + "position_embeddings.weight"], w[e + "token_type_embeddings.weight"],
                      w[e + "LayerNorm.weight"], w[e + "LayerNorm.bias"], eps, ids, type_ids)).reshape(B * L, H)
    n = 0
    while f"encoder.layer.{n}.attention.self.query.weight" in w:
        p = f"encoder.layer.{n}."
        lin = lambda t, name: fr(t @ fr(w[p + name + ".weight"]).T + w[p + name + ".bias"])     # noqa: E731
        xl = gr(x)                                                                                   # dx: the gradient that arrives through the QKV GEMM
        qkv = gr(torch.cat([lin(xl, "attention.self." + r) for r in ("query", "key", "value")], dim=1))        # dqkv
        ctx = gr(fr(R.attention(qkv, m, B, L, H)))                                                   # dctx
        s1 = gr(lin(ctx, "attention.output.dense") + x)                                              # ds1: of y and of x alike
        x1 = fr(R.layer_norm(s1, w[p + "attention.output.LayerNorm.weight"], w[p + "attention.output.LayerNorm.bias"], eps))
        h = gr(lin(gr(x1), "intermediate.dense"))                                                    # dh' at h, dx1 at x1
        gh = gr(fr(R.gelu(h)))                                                                       # dh
        s2 = gr(lin(gh, "output.dense") + x1)                                                        # ds2
        x = fr(R.layer_norm(s2, w[p + "output.LayerNorm.weight"], w[p + "output.LayerNorm.bias"], eps))
        n += 1
    out = gr(x).reshape(B, L, H)
    names = list(w)
    grads = torch.autograd.grad((out * upstream.double()).sum(), [w[k] for k in names], allow_unused=True)
    return out.detach(), {k: g for k, g in zip(names, grads) if g is not None}
