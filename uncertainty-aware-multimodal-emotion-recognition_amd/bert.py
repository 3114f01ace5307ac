"""The BERT trunk of the text encoder: ``transformers.BertModel`` as the reference's ``EnhancedTextEncoder`` instantiates it
(reference src/models/encoders.py:553-761, ``self.bert``), forward only, on HIP.  ``BertEncoder`` has the parameters of
``BertModel`` under the same names and shapes, so a checkpoint of the reference's ``self.bert`` loads with ``strict=True``;
tokenisation and pretrained weights stay outside this package (no ``from_pretrained`` here: build from a config, load a state dict).

Per forward 1 + 8 * layers launches on the current stream, no host synchronisation and no ``.item()``, so a forward can be
captured with ``torch.cuda.graph`` (run one forward before the capture: it builds the packed operands):

    mmdeer_bert_embed_fwd     x = LayerNorm(word[id] + type[tt] + pos[t])                  (include/mmdeer_bert.h)
    per layer:
      mmdeer_gemm             qkv = x Wqkv^T + bqkv         one GEMM against the packed [3H, H] weight
      mmdeer_bert_attn_fwd    ctx = softmax(Q K^T / 8 over the valid keys) V, per head of 64
      mmdeer_gemm             y = ctx Wo^T + bo
      mmdeer_bert_add_ln_fwd  x = LayerNorm(y + x)
      mmdeer_gemm             h = x Wi^T + bi
      mmdeer_bert_gelu_fwd    h = gelu(h)                   the erf form, in place
      mmdeer_gemm             y = h Wo2^T + bo2
      mmdeer_bert_add_ln_fwd  x = LayerNorm(y + x)

The trunk is FROZEN: every parameter is created with ``requires_grad=False``, a call with grad enabled while a parameter requires
grad raises, and the output carries no graph (its backward -- the reference fine-tunes layers 6-11 -- is not built).  A frozen
trunk is an eval trunk: there is NO dropout inside it in either mode (``.train()`` changes nothing).  The pooler's parameters are
kept for the checkpoint and never read.  One deviation from ``BertModel``: a sample whose mask has no valid token gets zeros
from every attention layer where the reference averages V uniformly (include/mmdeer_bert.h); everything downstream of the trunk
multiplies by the mask.  Masks are binary (nonzero = valid).  No CPU path: CPU tensors raise."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch
from torch import nn

from . import _lib, ops

HEAD_DIM = _lib.BERT_CONSTANTS["BERT_HEAD_DIM"]
MAX_HIDDEN = _lib.BERT_CONSTANTS["BERT_MAX_HIDDEN"]
MAX_TOKENS = _lib.BERT_CONSTANTS["BERT_MAX_TOKENS"]

# bert-base-uncased
DEFAULTS = {"vocab_size": 30522, "hidden_size": 768, "num_hidden_layers": 12, "num_attention_heads": 12, "intermediate_size": 3072,
            "max_position_embeddings": 512, "type_vocab_size": 2, "layer_norm_eps": 1e-12, "hidden_act": "gelu", "initializer_range": 0.02,
            "position_embedding_type": "absolute", "pad_token_id": 0, "add_pooling_layer": True}


def _config(config) -> dict:
    """a dict, or any object with BertConfig's attribute names -> a dict over DEFAULTS"""
    if config is None:
        return dict(DEFAULTS)
    if isinstance(config, dict):
        unknown = set(config) - set(DEFAULTS)
        if unknown:
            raise ValueError(f"BertEncoder: unknown config keys {sorted(unknown)}")
        return {**DEFAULTS, **config}
    return {k: (getattr(config, k) if getattr(config, k, None) is not None else d) for k, d in DEFAULTS.items()}


class BertEncoderOutput:
    """What the reference reads of ``BertModel``'s output: ``last_hidden_state`` (B, L, H) in the compute dtype.  ``hidden_states``
    (the embedding output and every layer's, copies) only with ``output_hidden_states=True``."""

    def __init__(self, last_hidden_state, hidden_states=None):
        self.last_hidden_state, self.hidden_states = last_hidden_state, hidden_states


def _named(**children) -> nn.Module:
    m = nn.Module()
    for name, child in children.items():
        setattr(m, name, child)       # nn.Module.__setattr__ registers it; "self" is BertAttention's own name for its first child
    return m


class BertEncoder(nn.Module):
    """``BertModel(BertConfig(**config))`` forward on HIP (the module docstring has the launch plan and what is not built)."""

    def __init__(self, config=None, compute_dtype: str = "bf16"):
        super().__init__()
        c = self.config = _config(config)
        ops._act_dtype(compute_dtype)
        self.compute_dtype = compute_dtype
        H, I, heads = int(c["hidden_size"]), int(c["intermediate_size"]), int(c["num_attention_heads"])
        if H != HEAD_DIM * heads:
            raise NotImplementedError(f"BertEncoder: hidden_size must be {HEAD_DIM} * num_attention_heads (the head dimension is fixed at "
                                      f"{HEAD_DIM}); got {H} with {heads} heads")
        if H > MAX_HIDDEN or H < HEAD_DIM:
            raise NotImplementedError(f"BertEncoder: hidden_size {H} is outside {HEAD_DIM} .. {MAX_HIDDEN}")
        if c["hidden_act"] != "gelu":
            raise NotImplementedError(f"BertEncoder: hidden_act {c['hidden_act']!r} is not built (only 'gelu', the erf form)")
        if c["position_embedding_type"] != "absolute":
            raise NotImplementedError(f"BertEncoder: position_embedding_type {c['position_embedding_type']!r} is not built (only 'absolute')")
        if I % 8 or I < 8:
            raise NotImplementedError(f"BertEncoder: intermediate_size must be a multiple of 8 (got {I})")
        if min(int(c["vocab_size"]), int(c["max_position_embeddings"]), int(c["type_vocab_size"]), int(c["num_hidden_layers"]) + 1) < 1:
            raise ValueError("BertEncoder: vocab_size, max_position_embeddings and type_vocab_size must be positive")
        self.hidden_size, self.eps = H, float(c["layer_norm_eps"])
        self.embeddings = _named(word_embeddings=nn.Embedding(c["vocab_size"], H, padding_idx=c["pad_token_id"]),
                                 position_embeddings=nn.Embedding(c["max_position_embeddings"], H),
                                 token_type_embeddings=nn.Embedding(c["type_vocab_size"], H), LayerNorm=nn.LayerNorm(H, eps=self.eps))
        self.encoder = _named(layer=nn.ModuleList(
            _named(attention=_named(**{"self": _named(query=nn.Linear(H, H), key=nn.Linear(H, H), value=nn.Linear(H, H)),
                                       "output": _named(dense=nn.Linear(H, H), LayerNorm=nn.LayerNorm(H, eps=self.eps))}),
                   intermediate=_named(dense=nn.Linear(H, I)),
                   output=_named(dense=nn.Linear(I, H), LayerNorm=nn.LayerNorm(H, eps=self.eps)))
            for _ in range(int(c["num_hidden_layers"]))))
        if c["add_pooling_layer"]:
            self.pooler = _named(dense=nn.Linear(H, H))       # kept for the checkpoint, never read
        self._init_weights(float(c["initializer_range"]))
        for p in self.parameters():
            p.requires_grad_(False)
        self._packed, self._packed_key = None, None

    @torch.no_grad()
    def _init_weights(self, std: float):
        """transformers' BertPreTrainedModel._init_weights: normal(0, initializer_range), zero biases, a zero padding row, unit LayerNorm"""
        for m in self.modules():
            if isinstance(m, nn.Linear):
                m.weight.normal_(0.0, std)
                m.bias.zero_()
            elif isinstance(m, nn.Embedding):
                m.weight.normal_(0.0, std)
                if m.padding_idx is not None:
                    m.weight[m.padding_idx].zero_()
            elif isinstance(m, nn.LayerNorm):
                m.weight.fill_(1.0)
                m.bias.zero_()

    # ---------------------------------------------------------------------------------------------------------------------
    def _operands(self):
        """The packed operands: the [3H, H] QKV weight and its bias, compute-dtype copies of the matrices, fp32 vectors.  Built once and
        rebuilt when a parameter changed: the key is every parameter's (_version, data_ptr), which an in-place update
        (load_state_dict, an optimiser step) and a replaced storage (.to(), .data = ...) both move."""
        key = tuple((p._version, p.data_ptr()) for p in self.parameters())
        if self._packed is not None and key == self._packed_key:
            return self._packed
        dt = ops._act_dtype(self.compute_dtype)
        mat = lambda *ws: torch.cat([w.detach() for w in ws], dim=0).to(dt).contiguous()                 # noqa: E731
        vec = lambda *vs: torch.cat([v.detach().reshape(-1) for v in vs], dim=0).float().contiguous()     # noqa: E731
        e = self.embeddings
        packed = {"emb": tuple(t.detach().float().contiguous() for t in (e.word_embeddings.weight, e.position_embeddings.weight, e.token_type_embeddings.weight,
                                                e.LayerNorm.weight, e.LayerNorm.bias)), "layers": []}
        for lyr in self.encoder.layer:
            s, so = getattr(lyr.attention, "self"), lyr.attention.output
            packed["layers"].append({
                "wqkv": mat(s.query.weight, s.key.weight, s.value.weight), "bqkv": vec(s.query.bias, s.key.bias, s.value.bias),
                "wo": mat(so.dense.weight), "bo": vec(so.dense.bias), "g1": vec(so.LayerNorm.weight), "b1": vec(so.LayerNorm.bias),
                "wi": mat(lyr.intermediate.dense.weight), "bi": vec(lyr.intermediate.dense.bias),
                "wo2": mat(lyr.output.dense.weight), "bo2": vec(lyr.output.dense.bias), "g2": vec(lyr.output.LayerNorm.weight),
                "b2": vec(lyr.output.LayerNorm.bias)})
        self._packed, self._packed_key = packed, key
        return packed

    def _add_ln(self, y, x, gamma, beta, out):
        a = _lib.BertAddLnArgs()
        a.y, a.x, a.gamma, a.beta, a.out, a.eps = y.data_ptr(), x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), out.data_ptr(), self.eps
        a.M, a.N, a.ld_y, a.ld_x, a.ld_out = y.shape[0], y.shape[1], y.stride(0), x.stride(0), out.stride(0)
        a.act_f32, a.stream = int(self.compute_dtype == "fp32"), _lib.current_stream()
        _lib.check(_lib.load().mmdeer_bert_add_ln_fwd(C.byref(a)))

    def forward(self, input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor] = None, token_type_ids: Optional[torch.Tensor] = None,
                output_hidden_states: bool = False) -> BertEncoderOutput:
        if input_ids.dim() != 2:
            raise ValueError(f"expected input_ids of shape (B, L), got {tuple(input_ids.shape)}")
        for name, t in (("attention_mask", attention_mask), ("token_type_ids", token_type_ids)):
            if t is not None and tuple(t.shape) != tuple(input_ids.shape):
                raise ValueError(f"expected {name} of the shape of input_ids {tuple(input_ids.shape)}, got {tuple(t.shape)}")
        if input_ids.dtype.is_floating_point or input_ids.dtype == torch.bool:
            raise ValueError(f"input_ids must be an integer tensor (got {input_ids.dtype})")
        B, L = input_ids.shape
        if L < 1:
            raise ValueError("expected at least one token position (L >= 1)")
        if L > self.config["max_position_embeddings"]:
            raise ValueError(f"L = {L} is above max_position_embeddings = {self.config['max_position_embeddings']}")
        if L > MAX_TOKENS:
            raise ValueError(f"L = {L} is above the {MAX_TOKENS} tokens the attention kernel takes")
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise ValueError("the BERT trunk is forward only: its backward is not built.  Keep its parameters at requires_grad=False "
                             "(or call it under torch.no_grad())")
        ops._check_dev(input_ids, attention_mask, token_type_ids, self.embeddings.word_embeddings.weight)
        dt, f32, H = ops._act_dtype(self.compute_dtype), int(self.compute_dtype == "fp32"), self.hidden_size
        dev = input_ids.device
        if B == 0:
            return BertEncoderOutput(torch.empty(0, L, H, dtype=dt, device=dev), () if output_hidden_states else None)
        with torch.no_grad():
            lib, stream, M, I = _lib.load(), _lib.current_stream(), B * L, int(self.config["intermediate_size"])
            w = self._operands()
            ids = input_ids.to(torch.int64).reshape(-1).contiguous()
            tts = None if token_type_ids is None else token_type_ids.to(torch.int64).reshape(-1).contiguous()
            m = (torch.ones(M, device=dev) if attention_mask is None else (attention_mask != 0).float().reshape(-1).contiguous())
            x, y = torch.empty(M, H, dtype=dt, device=dev), torch.empty(M, H, dtype=dt, device=dev)
            qkv, ctx, h = torch.empty(M, 3 * H, dtype=dt, device=dev), torch.empty(M, H, dtype=dt, device=dev), torch.empty(M, I, dtype=dt, device=dev)
            word, pos, typ, g0, b0 = w["emb"]
            a = _lib.BertEmbedArgs()
            a.ids, a.type_ids, a.word, a.pos, a.type = ids.data_ptr(), _lib.ptr(tts), word.data_ptr(), pos.data_ptr(), typ.data_ptr()
            a.gamma, a.beta, a.x, a.eps = g0.data_ptr(), b0.data_ptr(), x.data_ptr(), self.eps
            a.B, a.L, a.H, a.ld_x, a.act_f32, a.stream = B, L, H, H, f32, stream
            a.V, a.P, a.T = self.config["vocab_size"], self.config["max_position_embeddings"], self.config["type_vocab_size"]
            _lib.check(lib.mmdeer_bert_embed_fwd(C.byref(a)))
            states = [x.clone()] if output_hidden_states else None
            at = _lib.BertAttnArgs()
            at.qkv, at.mask, at.ctx = qkv.data_ptr(), m.data_ptr(), ctx.data_ptr()
            at.B, at.L, at.H, at.ld_qkv, at.ld_ctx, at.act_f32, at.stream = B, L, H, 3 * H, H, f32, stream
            ge = _lib.BertGeluArgs()
            ge.x, ge.out, ge.M, ge.N, ge.ld_x, ge.ld_out, ge.act_f32, ge.stream = h.data_ptr(), h.data_ptr(), M, I, I, I, f32, stream
            for p in w["layers"]:
                ops.linear_into(x, p["wqkv"], p["bqkv"], qkv, compute=self.compute_dtype)
                _lib.check(lib.mmdeer_bert_attn_fwd(C.byref(at)))
                ops.linear_into(ctx, p["wo"], p["bo"], y, compute=self.compute_dtype)
                self._add_ln(y, x, p["g1"], p["b1"], y)              # x1 takes y's buffer; x is free from here
                ops.linear_into(y, p["wi"], p["bi"], h, compute=self.compute_dtype)
                _lib.check(lib.mmdeer_bert_gelu_fwd(C.byref(ge)))
                ops.linear_into(h, p["wo2"], p["bo2"], x, compute=self.compute_dtype)
                self._add_ln(x, y, p["g2"], p["b2"], x)              # the layer's output, in x's buffer again
                if output_hidden_states:
                    states.append(x.clone())
            shaped = lambda t: t.reshape(B, L, H)             # noqa: E731
            return BertEncoderOutput(shaped(x), tuple(shaped(s) for s in states) if output_hidden_states else None)
