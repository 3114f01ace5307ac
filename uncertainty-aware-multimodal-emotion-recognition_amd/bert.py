"""The BERT trunk of the text encoder: ``transformers.BertModel`` as the reference's ``EnhancedTextEncoder`` instantiates it
(reference src/models/encoders.py:553-761, ``self.bert``) on HIP: the forward, and with ``finetune_layers=k`` the backward of its last
``k`` layers.  ``BertEncoder`` has the parameters of ``BertModel`` under the same names and shapes, so a checkpoint of the reference's ``self.bert`` loads with ``strict=True``;
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

By default (``finetune_layers=0``) the trunk is FROZEN: every parameter is created with ``requires_grad=False``, a call with grad
enabled while a parameter requires grad raises, and the output carries no graph.  The pooler's parameters are kept for the
checkpoint and never read.

``BertEncoder(config, compute_dtype, finetune_layers=k)``, 1 <= k <= num_hidden_layers, fine-tunes the last ``k`` layers (the
reference's ``_setup_bert_fine_tuning`` freezes the embeddings and layers 0-5 of 12 and trains layers 6-11: k = 6).  Their
parameters are created with ``requires_grad=True``; the embeddings, the layers below and the pooler stay frozen, and a call with
grad enabled raises ``ValueError`` naming the parameter when one of those requires grad.  With grad enabled the layers below the
tail run as ever under ``no_grad`` and the tail is ONE autograd node (``_TailFn``) over all its layers.  A layer's forward is
stated once (``_layer_fwd``): the forward-only path calls it with aliased buffers (x1 takes y's buffer, the GELU is in place, the
output returns to x's) and the tail with fresh ones, so ``last_hidden_state`` is bit-equal to the frozen trunk's.  It keeps per tail layer
x, qkv, ctx, y, x1, the pre-GELU h, gelu(h) and y2 on the tape: 8 H + 2 I elements per token, 100 MB per layer at 4096 tokens of
BERT-base in bf16 (12 288 elements x 4096 x 2 bytes), 600 MB for k = 6; a layer's tape is released as the backward leaves it.
The backward, per tail layer from the top, given g (the gradient of the layer's output) and g2 (None at the top):

    mmdeer_bert_add_ln_bwd   (g, g2; y2, x1, gamma2) -> ds2, dgamma2, dbeta2            (include/mmdeer_bert_bwd.h)
    mmdeer_gemm              dWo2 = ds2^T gelu(h), dbo2 from the same launch (bias_grad)
    mmdeer_gemm              dh = ds2 Wo2
    mmdeer_bert_gelu_bwd     dh' = dh gelu'(h), in place
    mmdeer_gemm              dWi = dh'^T x1, dbi
    mmdeer_gemm              dx1 = dh' Wi
    mmdeer_bert_add_ln_bwd   (dx1, ds2; y, x, gamma1) -> ds1, dgamma1, dbeta1
    mmdeer_gemm              dWo = ds1^T ctx, dbo
    mmdeer_gemm              dctx = ds1 Wo
    mmdeer_bert_attn_bwd     dqkv  (two launches)
    mmdeer_gemm              dWqkv [3H, H] = dqkv^T x, dbqkv: returned as the row slices of query / key / value
    mmdeer_gemm              dx = dqkv Wqkv, only above the lowest tail layer; the next layer starts with g = dx, g2 = ds1

Activation gradients are stored in the compute dtype; parameter gradients are summed in fp32 in a fixed order (no atomics: two
backward runs store the same bits) and returned in the parameters' dtype.  A tail parameter switched back to
``requires_grad=False`` gets no gradient.  There is no gradient with respect to the ids, and ``hidden_states`` are graph-free copies.

DROPOUT is off by default: ``BertEncoder(config, compute_dtype, finetune_layers)`` has none in either mode (``.train()`` changes
nothing), whatever the config's probabilities say -- it fine-tunes as ``BertConfig(hidden_dropout_prob=0, attention_probs_dropout_prob=0)``
does.  ``dropout=True`` is the reference's training configuration (its BERT trains with both probabilities 0.1, BertConfig's
defaults): in ``training`` mode ``hidden_dropout_prob`` is live on the embeddings and behind the dense of BertSelfOutput and BertOutput,
and ``attention_probs_dropout_prob`` on the attention probabilities, in ALL layers, the frozen ones and ``no_grad`` calls included,
whatever ``finetune_layers`` is; ``eval()`` stores the bits of a ``dropout=False`` encoder.  The sites run inside the launches above
(include/mmdeer_bert_drop.h: ``mmdeer_bert_embed_drop_fwd``, ``mmdeer_bert_attn_drop_fwd``, ``mmdeer_bert_drop_add_ln_fwd``, and in the
backward ``mmdeer_bert_drop_add_ln_bwd`` for launches 1 and 7, whose second output dy = ds o m feeds the two GEMMs behind each while ds
goes on by the residual branch, and ``mmdeer_bert_attn_drop_bwd``): no extra launch in either direction, the tape is unchanged (y
and y2 are kept pre-dropout) and no mask is stored -- the library's counter hash regenerates it from (``dropout_seed``, step, site,
row, column), with one site id per (layer, place) from a block that no other module uses (``SITE_EMBED``, ``site(layer, place)``).  A
site whose probability is 0 runs its plain entry.  ``_train_step`` advances by one per forward in which dropout is live; the backward
of a forward uses that forward's step; two runs of the same step store the same bits.

A CAPTURED GRAPH replays the kernel arguments it recorded, so the host's step would freeze.  ``set_step_counter(t)``, ``t`` a one-element
int64 tensor on the module's device, moves the step onto the device: live forward number k = 0, 1, ... since ``take_step_count()``
last returned passes offset = k and the counter's address to the ``_dev`` twins of the five entries (include/mmdeer_bert_drop.h), which
hash step = k + *t, read when the kernel runs; the backward of a forward uses the same pair.  Whoever owns the graph adds
``take_step_count()`` to ``t`` at the end of the captured region (``mmdeer.train_graph.capture_train_step`` does), so that each replay
draws the masks of the next step.  ``set_step_counter(None)`` returns to the host counter; without a counter nothing changes.

One deviation from ``BertModel`` in the forward: a sample whose mask has no valid token gets zeros from every attention layer where
the reference averages V uniformly (include/mmdeer_bert.h), and, mirrored in the backward, zeros in all of its dqkv; everything
downstream of the trunk multiplies by the mask.  Masks are binary (nonzero = valid).  No CPU path: CPU tensors raise."""
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
            "position_embedding_type": "absolute", "pad_token_id": 0, "add_pooling_layer": True,
            "hidden_dropout_prob": 0.1, "attention_probs_dropout_prob": 0.1}       # read only with dropout=True
# dropout site ids (include/mmdeer_bert_drop.h): one for the embeddings, then per layer attention, self-output, output
SITE_EMBED = _lib.BERT_DROP_CONSTANTS["BERT_DROP_SITE_EMBED"]
SITE_LAYER0 = _lib.BERT_DROP_CONSTANTS["BERT_DROP_SITE_LAYER0"]
_ATTN, _SELF_OUT, _OUT = 0, 1, 2


def site(layer: int, place: int) -> int:
    return SITE_LAYER0 + 4 * layer + place


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
    """``BertModel(BertConfig(**config))`` on HIP; ``finetune_layers=k`` trains its last ``k`` layers; ``dropout=True`` makes the config's
    two dropout probabilities live in ``train()``, drawn from ``dropout_seed`` and a step counter (the module docstring has both
    launch plans, the dropout sites and what is not built)."""

    def __init__(self, config=None, compute_dtype: str = "bf16", finetune_layers: int = 0, dropout: bool = False, dropout_seed: int = 0):
        super().__init__()
        c = self.config = _config(config)
        if not isinstance(dropout, bool):
            raise ValueError(f"BertEncoder: dropout must be a bool (got {dropout!r})")
        if isinstance(dropout_seed, bool) or not isinstance(dropout_seed, int) or not 0 <= dropout_seed < 2 ** 64:
            raise ValueError(f"BertEncoder: dropout_seed must be an integer in 0 .. 2^64 - 1 (got {dropout_seed!r})")
        self.dropout, self.dropout_seed, self._train_step = dropout, dropout_seed, 0       # counter-hash dropout: seed + one tick per training forward
        self._step_counter, self._counter_k = None, 0                                      # ... or a device counter + the live forwards since it was read
        self.p_hidden = self.p_attn = 0.0
        if dropout:
            for key in ("hidden_dropout_prob", "attention_probs_dropout_prob"):
                v = c[key]
                if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0.0 <= float(v) < 1.0:       # a NaN fails both comparisons
                    raise ValueError(f"BertEncoder: {key} must be a number in [0, 1) (got {v!r})")
            self.p_hidden, self.p_attn = float(c["hidden_dropout_prob"]), float(c["attention_probs_dropout_prob"])
        if isinstance(finetune_layers, bool) or not isinstance(finetune_layers, int) or not 0 <= finetune_layers <= int(c["num_hidden_layers"]):
            raise ValueError(f"BertEncoder: finetune_layers must be an integer in 0 .. num_hidden_layers = {int(c['num_hidden_layers'])} "
                             f"(got {finetune_layers!r})")
        self.finetune_layers = finetune_layers
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
        for lyr in self.encoder.layer[len(self.encoder.layer) - finetune_layers:]:
            for p in lyr.parameters():
                p.requires_grad_(True)
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
    def _operands_key(self):
        """what the packed operands were built from: the compute dtype and every parameter's (_version, data_ptr), per layer"""
        stamp = lambda m: tuple((p._version, p.data_ptr()) for p in m.parameters())                        # noqa: E731
        return (ops._act_dtype(self.compute_dtype), stamp(self.embeddings), tuple(stamp(lyr) for lyr in self.encoder.layer))

    def operand_mirrors(self):
        """{parameter: the view of the packed operands that holds it} for every trainable parameter of the tail (the operands are
        built first if need be): rows of ``wqkv`` for query / key / value, slices of ``bqkv``, and ``wo``, ``bo``, ``g1``, ... whole.  An
        optimiser that stores each updated parameter into its view too (``optim.ModuleAdamW``: the compute dtype's rounding is
        ``.to(dtype)``'s) and then calls ``operands_current()`` spares the rebuild after its step.  The views are those of the operands
        as they are NOW: a rebuild (a parameter changed by anything else) makes new ones."""
        packed, H = self._operands(), self.hidden_size
        out = {}
        for lyr, w in zip(self.encoder.layer, packed["layers"]):
            s, so = getattr(lyr.attention, "self"), lyr.attention.output
            pairs = [(lin.weight, w["wqkv"][j * H:(j + 1) * H]) for j, lin in enumerate((s.query, s.key, s.value))]
            pairs += [(lin.bias, w["bqkv"][j * H:(j + 1) * H]) for j, lin in enumerate((s.query, s.key, s.value))]
            pairs += [(so.dense.weight, w["wo"]), (so.dense.bias, w["bo"]), (so.LayerNorm.weight, w["g1"]), (so.LayerNorm.bias, w["b1"]),
                      (lyr.intermediate.dense.weight, w["wi"]), (lyr.intermediate.dense.bias, w["bi"]), (lyr.output.dense.weight, w["wo2"]),
                      (lyr.output.dense.bias, w["bo2"]), (lyr.output.LayerNorm.weight, w["g2"]), (lyr.output.LayerNorm.bias, w["b2"])]
            out.update({p: t for p, t in pairs if p.requires_grad})
        return out

    def operands_current(self) -> None:
        """Restamp the fine-tuned tail's packed operands from its parameters as they are: the caller has written every parameter it
        changed into ``operand_mirrors()``'s views, so the next ``_operands()`` returns the same object without rebuilding.  Without
        built operands nothing happens."""
        if self._packed is not None:
            dt, emb, layers = self._packed_key
            first = len(self.encoder.layer) - self.finetune_layers          # only the tail can have been trained: the other stamps stay,
            stamp = lambda m: tuple((p._version, p.data_ptr()) for p in m.parameters())      # noqa: E731  (and still catch a change from elsewhere)
            self._packed_key = (dt, emb, layers[:first] + tuple(stamp(lyr) for lyr in self.encoder.layer[first:]))

    def _operands(self):
        """The packed operands: the [3H, H] QKV weight and its bias, compute-dtype copies of the matrices, fp32 vectors.  Built once and
        rebuilt when a parameter changed: the key is every parameter's (_version, data_ptr), which an in-place update
        (load_state_dict, an optimiser step) and a replaced storage (.to(), .data = ...) both move.  The key is kept per layer and
        for the embeddings, so a step on the tail repacks the tail's layers only: the returned dict is a new object whenever
        anything changed, and holds the SAME entry for every layer (and the embeddings) that did not."""
        key = self._operands_key()
        dt = key[0]
        if self._packed is not None and key == self._packed_key:
            return self._packed
        same = self._packed is not None and self._packed_key[0] == dt
        mat = lambda *ws: torch.cat([w.detach() for w in ws], dim=0).to(dt).contiguous()                 # noqa: E731
        vec = lambda *vs: torch.cat([v.detach().reshape(-1) for v in vs], dim=0).float().contiguous()     # noqa: E731
        e = self.embeddings
        if same and key[1] == self._packed_key[1]:
            emb = self._packed["emb"]
        else:
            emb = tuple(t.detach().float().contiguous() for t in (e.word_embeddings.weight, e.position_embeddings.weight, e.token_type_embeddings.weight,
                                                                  e.LayerNorm.weight, e.LayerNorm.bias))
        packed = {"emb": emb, "layers": []}
        for i, lyr in enumerate(self.encoder.layer):
            if same and key[2][i] == self._packed_key[2][i]:
                packed["layers"].append(self._packed["layers"][i])
                continue
            s, so = getattr(lyr.attention, "self"), lyr.attention.output
            packed["layers"].append({
                "wqkv": mat(s.query.weight, s.key.weight, s.value.weight), "bqkv": vec(s.query.bias, s.key.bias, s.value.bias),
                "wo": mat(so.dense.weight), "bo": vec(so.dense.bias), "g1": vec(so.LayerNorm.weight), "b1": vec(so.LayerNorm.bias),
                "wi": mat(lyr.intermediate.dense.weight), "bi": vec(lyr.intermediate.dense.bias),
                "wo2": mat(lyr.output.dense.weight), "bo2": vec(lyr.output.dense.bias), "g2": vec(lyr.output.LayerNorm.weight),
                "b2": vec(lyr.output.LayerNorm.bias)})
        self._packed, self._packed_key = packed, key
        return packed

    def _add_ln(self, y, x, gamma, beta, out, drop=None, site_id=-1):
        """out = LayerNorm(y + x), or LayerNorm(drop(y) + x) with ``drop`` = (seed, step[, counter]) where the hidden probability is not 0"""
        live = drop is not None and self.p_hidden > 0
        a = _lib.BertDropAddLnArgs() if live else _lib.BertAddLnArgs()
        a.y, a.x, a.gamma, a.beta, a.out, a.eps = y.data_ptr(), x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), out.data_ptr(), self.eps
        a.M, a.N, a.ld_y, a.ld_x, a.ld_out = y.shape[0], y.shape[1], y.stride(0), x.stride(0), out.stride(0)
        a.act_f32, a.stream = int(self.compute_dtype == "fp32"), _lib.current_stream()
        if live:
            a.site, a.dropout_p = site_id, self.p_hidden
            _drop_call("mmdeer_bert_drop_add_ln_fwd", a, drop)
        else:
            _lib.check(_lib.load().mmdeer_bert_add_ln_fwd(C.byref(a)))

    def _drop(self):
        """(seed, step) of this forward where dropout is live -- (seed, step, device counter) with a device counter set --, else None;
        the host counter, or with a device counter the count of live forwards since it was read, advances by one per live forward"""
        if self.dropout and self.training and (self.p_hidden > 0 or self.p_attn > 0):
            if self._step_counter is not None:
                d = (int(self.dropout_seed), self._counter_k, self._step_counter)
                self._counter_k += 1
                return d
            d = (int(self.dropout_seed), self._train_step)
            self._train_step += 1
            return d
        return None

    def set_step_counter(self, t: Optional[torch.Tensor]) -> None:
        """Take the dropout step from the device: ``t`` is a one-element int64 tensor on this module's device (the module docstring
        has the arithmetic), or None to return to the host counter."""
        if t is not None:
            dev = self.embeddings.word_embeddings.weight.device
            if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.numel() != 1 or t.device != dev:
                raise ValueError(f"set_step_counter: expected a one-element int64 tensor on {dev}, got "
                                 f"{(t.dtype, tuple(t.shape), t.device) if isinstance(t, torch.Tensor) else type(t).__name__}")
        self._step_counter, self._counter_k = t, 0

    def take_step_count(self) -> int:
        """How many live forwards ran since the last call (or since the counter was set); the count restarts at 0.  The owner of a
        captured graph adds it to the counter."""
        k, self._counter_k = self._counter_k, 0
        return k

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
        nl = len(self.encoder.layer)
        first_tail = nl - self.finetune_layers
        tail = torch.is_grad_enabled() and self.finetune_layers > 0
        if torch.is_grad_enabled() and self.finetune_layers == 0 and any(p.requires_grad for p in self.parameters()):
            raise ValueError("the BERT trunk is forward only: its backward is not built.  Keep its parameters at requires_grad=False "
                             "(or call it under torch.no_grad()), or build it with finetune_layers=k to train its last k layers")
        if tail:
            below = f"encoder.layer.{first_tail}."
            for name, p in self.named_parameters():
                if p.requires_grad and not (name.startswith("encoder.layer.") and int(name.split(".")[2]) >= first_tail):
                    what = "an embedding parameter" if name.startswith("embeddings.") else f"a parameter outside the fine-tuned tail ({below}* and up)"
                    raise ValueError(f"BertEncoder(finetune_layers={self.finetune_layers}): {name} requires grad, but it is {what}: only the last "
                                     f"{self.finetune_layers} layers have a backward.  Set it to requires_grad=False")
            tail = any(p.requires_grad for lyr in self.encoder.layer[first_tail:] for p in lyr.parameters())
        ops._check_dev(input_ids, attention_mask, token_type_ids, self.embeddings.word_embeddings.weight)
        dt, f32, H = ops._act_dtype(self.compute_dtype), int(self.compute_dtype == "fp32"), self.hidden_size
        dev = input_ids.device
        if B == 0:
            return BertEncoderOutput(torch.empty(0, L, H, dtype=dt, device=dev), () if output_hidden_states else None)
        drop = self._drop()
        with torch.no_grad():
            lib, stream, M, I = _lib.load(), _lib.current_stream(), B * L, int(self.config["intermediate_size"])
            w = self._operands()
            ids = input_ids.to(torch.int64).reshape(-1).contiguous()
            tts = None if token_type_ids is None else token_type_ids.to(torch.int64).reshape(-1).contiguous()
            m = (torch.ones(M, device=dev) if attention_mask is None else (attention_mask != 0).float().reshape(-1).contiguous())
            x, y = torch.empty(M, H, dtype=dt, device=dev), torch.empty(M, H, dtype=dt, device=dev)
            qkv, ctx, h = torch.empty(M, 3 * H, dtype=dt, device=dev), torch.empty(M, H, dtype=dt, device=dev), torch.empty(M, I, dtype=dt, device=dev)
            word, pos, typ, g0, b0 = w["emb"]
            embed_drop = drop is not None and self.p_hidden > 0
            a = _lib.BertEmbedDropArgs() if embed_drop else _lib.BertEmbedArgs()
            a.ids, a.type_ids, a.word, a.pos, a.type = ids.data_ptr(), _lib.ptr(tts), word.data_ptr(), pos.data_ptr(), typ.data_ptr()
            a.gamma, a.beta, a.x, a.eps = g0.data_ptr(), b0.data_ptr(), x.data_ptr(), self.eps
            a.B, a.L, a.H, a.ld_x, a.act_f32, a.stream = B, L, H, H, f32, stream
            a.V, a.P, a.T = self.config["vocab_size"], self.config["max_position_embeddings"], self.config["type_vocab_size"]
            if embed_drop:
                a.site, a.dropout_p = SITE_EMBED, self.p_hidden
                _drop_call("mmdeer_bert_embed_drop_fwd", a, drop)
            else:
                _lib.check(lib.mmdeer_bert_embed_fwd(C.byref(a)))
            states = [x.clone()] if output_hidden_states else None
            for li, p in enumerate(w["layers"][:first_tail if tail else nl]):
                # x1 takes y's buffer (x is free from there), the GELU is in place, and y2 and the layer's output take x's
                _layer_fwd(self, x, p, m, B, L, qkv, ctx, y, x1=y, h=h, gh=h, y2=x, out=x, drop=drop, layer=li)
                if output_hidden_states:
                    states.append(x.clone())
            shaped = lambda t: t.reshape(B, L, H)             # noqa: E731
            if not tail:
                return BertEncoderOutput(shaped(x), tuple(shaped(s) for s in states) if output_hidden_states else None)
        del qkv, ctx, h, y
        params = [p for lyr in self.encoder.layer[first_tail:] for p in lyr.parameters()]
        out = _TailFn.apply(self, x, m, B, L, w["layers"][first_tail:], states, (drop, first_tail), *params)
        return BertEncoderOutput(shaped(out), tuple(shaped(s) for s in states) if output_hidden_states else None)


def _drop_call(entry: str, a, drop) -> None:
    """Dropout entry ``entry`` of the library on ``a`` with ``drop`` = (seed, step): the plain entry at the host's step; or
    (seed, step[, counter]), ``counter`` a one-element int64 device tensor: its ``_dev`` twin, which adds the counter to the step on the
    device."""
    lib = _lib.load()
    a.seed, a.offset = drop[0], drop[1]
    if len(drop) < 3:
        _lib.check(getattr(lib, entry)(C.byref(a)))
    else:
        _lib.check(getattr(lib, entry + "_dev")(C.byref(a), drop[2].data_ptr()))


def _layer_fwd(enc, x, p, m, B, L, qkv, ctx, y, x1, h, gh, y2, out, drop=None, layer=0):
    """One BertLayer's forward on the caller's buffers: the eight launches of the module docstring.  ``p``: the layer's packed
    operands.  Buffers may alias as the frozen path's do (x1 = y, gh = h, y2 = out = x): each is written after its last reader.
    ``drop``: (seed, step[, counter]) where dropout is live: layer ``layer``'s three sites then run their drop entries, in the same launches."""
    lib, c, stream = _lib.load(), enc.compute_dtype, _lib.current_stream()
    f32, (M, H), I = int(c == "fp32"), x.shape, h.shape[1]
    ops.linear_into(x, p["wqkv"], p["bqkv"], qkv, compute=c)
    attn_drop = drop is not None and enc.p_attn > 0
    at = _lib.BertAttnDropArgs() if attn_drop else _lib.BertAttnArgs()
    at.qkv, at.mask, at.ctx = qkv.data_ptr(), m.data_ptr(), ctx.data_ptr()
    at.B, at.L, at.H, at.ld_qkv, at.ld_ctx, at.act_f32, at.stream = B, L, H, 3 * H, H, f32, stream
    if attn_drop:
        at.site, at.dropout_p = site(layer, _ATTN), enc.p_attn
        _drop_call("mmdeer_bert_attn_drop_fwd", at, drop)
    else:
        _lib.check(lib.mmdeer_bert_attn_fwd(C.byref(at)))
    ops.linear_into(ctx, p["wo"], p["bo"], y, compute=c)
    enc._add_ln(y, x, p["g1"], p["b1"], x1, drop, site(layer, _SELF_OUT))
    ops.linear_into(x1, p["wi"], p["bi"], h, compute=c)
    ge = _lib.BertGeluArgs()
    ge.x, ge.out, ge.M, ge.N, ge.ld_x, ge.ld_out, ge.act_f32, ge.stream = h.data_ptr(), gh.data_ptr(), M, I, I, I, f32, stream
    _lib.check(lib.mmdeer_bert_gelu_fwd(C.byref(ge)))
    ops.linear_into(gh, p["wo2"], p["bo2"], y2, compute=c)
    enc._add_ln(y2, x1, p["g2"], p["b2"], out, drop, site(layer, _OUT))


def _ln_bwd(enc, g, g2, y, x, gamma, want_sums: bool, drop=None, site_id=-1):
    """mmdeer_bert_add_ln_bwd -> (ds, dy, dgamma, dbeta); the sums only when wanted.  ds is the gradient of x and dy that of y: one
    tensor, unless ``drop`` = (seed, step[, counter]) makes it mmdeer_bert_drop_add_ln_bwd, whose dy = ds o m."""
    lib, (M, N) = _lib.load(), y.shape
    live = drop is not None and enc.p_hidden > 0
    ds = torch.empty_like(y)
    dy = torch.empty_like(y) if live else ds
    dgamma = dbeta = scratch = None
    a = _lib.BertDropAddLnBwdArgs() if live else _lib.BertAddLnBwdArgs()
    if want_sums:
        dgamma, dbeta = torch.empty(N, device=y.device), torch.empty(N, device=y.device)
        a.scratch_elems = lib.mmdeer_bert_add_ln_bwd_scratch(M, N)
        scratch = torch.empty(a.scratch_elems, device=y.device)
    a.y, a.x, a.g, a.g2, a.gamma, a.ds = y.data_ptr(), x.data_ptr(), g.data_ptr(), _lib.ptr(g2), gamma.data_ptr(), ds.data_ptr()
    a.dgamma, a.dbeta, a.scratch, a.eps = _lib.ptr(dgamma), _lib.ptr(dbeta), _lib.ptr(scratch), enc.eps
    a.M, a.N, a.ld_y, a.ld_x, a.ld_g, a.ld_g2, a.ld_ds = M, N, y.stride(0), x.stride(0), g.stride(0), g2.stride(0) if g2 is not None else 0, N
    a.act_f32, a.stream = int(enc.compute_dtype == "fp32"), _lib.current_stream()
    if live:
        a.dy, a.ld_dy, a.site, a.dropout_p = dy.data_ptr(), N, site_id, enc.p_hidden
        _drop_call("mmdeer_bert_drop_add_ln_bwd", a, drop)
    else:
        _lib.check(lib.mmdeer_bert_add_ln_bwd(C.byref(a)))
    return ds, dy, dgamma, dbeta


# the parameters of one BertLayer in nn.Module.parameters() order, as _TailFn receives them
_Q_W, _Q_B, _K_W, _K_B, _V_W, _V_B, _O_W, _O_B, _LN1_W, _LN1_B, _I_W, _I_B, _O2_W, _O2_B, _LN2_W, _LN2_B = range(16)


class _TailFn(torch.autograd.Function):
    """The fine-tuned tail as one autograd node (the module docstring has both launch plans).  ``packed``: the tail layers' packed
    operands; ``states``: the caller's list of hidden-state copies, or None; ``drop``: ((seed, step[, counter]) or None, the index of the
    tail's first layer): the backward regenerates this forward's masks from it, whatever forwards ran in between."""

    @staticmethod
    def forward(ctx, enc, x, m, B, L, packed, states, drop, *params):
        (M, H), I = x.shape, int(enc.config["intermediate_size"])
        new = lambda n: torch.empty(M, n, dtype=x.dtype, device=x.device)      # noqa: E731
        tape = []
        for li, p in enumerate(packed):
            qkv, cx, y, x1, h, gh, y2, out = new(3 * H), new(H), new(H), new(H), new(I), new(I), new(H), new(H)
            _layer_fwd(enc, x, p, m, B, L, qkv, cx, y, x1, h, gh, y2, out, drop=drop[0], layer=drop[1] + li)
            tape.append((x, qkv, cx, y, x1, h, gh, y2))
            x = out
            if states is not None:
                states.append(x.clone())
        ctx.enc, ctx.mask, ctx.BL, ctx.packed, ctx.tape, ctx.drop = enc, m, (B, L), packed, tape, drop
        ctx.dtypes = [p.dtype for p in params]
        return x

    @staticmethod
    def backward(ctx, g):
        from . import opseq
        enc, m, (B, L), c = ctx.enc, ctx.mask, ctx.BL, ctx.enc.compute_dtype
        needs = ctx.needs_input_grad[8:]
        drop, first = ctx.drop
        lib, f32 = _lib.load(), int(c == "fp32")
        dt = ops._act_dtype(c)
        ex = opseq.Exec(c)
        nl = len(ctx.packed)
        lowest = min(i // 16 for i, need in enumerate(needs) if need)
        grads = [None] * (16 * nl)
        g, g2 = g.reshape(B * L, -1).to(dt).contiguous(), None
        M, H = g.shape
        I = int(enc.config["intermediate_size"])
        dev = g.device

        def dw(li, wi, bi, dy, xin, n, k):
            """dW (n, k) = dy^T xin and its bias gradient, where either is wanted"""
            if needs[16 * li + wi] or needs[16 * li + bi]:
                gw, gb = torch.empty(n, k, device=dev), torch.empty(n, device=dev)
                ex.dw(dy, dy.stride(0), xin, xin.stride(0), gw, gb, M, n, k)
                grads[16 * li + wi], grads[16 * li + bi] = gw, gb
            return None

        ws_bytes = lib.mmdeer_bert_attn_bwd_workspace(B, L, H)
        ws = torch.empty(max(ws_bytes // 4, 4), device=dev)
        for li in range(nl - 1, lowest - 1, -1):
            p = ctx.packed[li]
            x, qkv, cx, y, x1, h, gh, y2 = ctx.tape.pop()
            sums = lambda a, b: needs[16 * li + a] or needs[16 * li + b]      # noqa: E731
            ds2, dy2, grads[16 * li + _LN2_W], grads[16 * li + _LN2_B] = _ln_bwd(enc, g, g2, y2, x1, p["g2"], sums(_LN2_W, _LN2_B), drop,
                                                                                 site(first + li, _OUT))
            del g, g2, y2
            dw(li, _O2_W, _O2_B, dy2, gh, H, I)
            del gh
            dh = torch.empty(M, I, dtype=dt, device=dev)
            ex.dx(dy2, H, p["wo2"], dh, I, M)
            del dy2
            ga = _lib.BertGeluBwdArgs()
            ga.x, ga.g, ga.dx, ga.M, ga.N, ga.ld_x, ga.ld_g, ga.ld_dx = h.data_ptr(), dh.data_ptr(), dh.data_ptr(), M, I, I, I, I
            ga.act_f32, ga.stream = f32, ex.s
            _lib.check(lib.mmdeer_bert_gelu_bwd(C.byref(ga)))
            del h
            dw(li, _I_W, _I_B, dh, x1, I, H)
            dx1 = torch.empty(M, H, dtype=dt, device=dev)
            ex.dx(dh, I, p["wi"], dx1, H, M)
            del dh
            ds1, dy1, grads[16 * li + _LN1_W], grads[16 * li + _LN1_B] = _ln_bwd(enc, dx1, ds2, y, x, p["g1"], sums(_LN1_W, _LN1_B), drop,
                                                                                 site(first + li, _SELF_OUT))
            del dx1, ds2, y, x1
            dw(li, _O_W, _O_B, dy1, cx, H, H)
            dctx = torch.empty(M, H, dtype=dt, device=dev)
            ex.dx(dy1, H, p["wo"], dctx, H, M)
            del dy1
            dqkv = torch.empty(M, 3 * H, dtype=dt, device=dev)
            attn_drop = drop is not None and enc.p_attn > 0
            ab = _lib.BertAttnDropBwdArgs() if attn_drop else _lib.BertAttnBwdArgs()
            ab.qkv, ab.mask, ab.dctx, ab.dqkv = qkv.data_ptr(), m.data_ptr(), dctx.data_ptr(), dqkv.data_ptr()
            ab.workspace, ab.workspace_bytes = ws.data_ptr(), ws_bytes
            ab.B, ab.L, ab.H, ab.ld_qkv, ab.ld_dctx, ab.ld_dqkv, ab.act_f32, ab.stream = B, L, H, 3 * H, H, 3 * H, f32, ex.s
            if attn_drop:
                ab.site, ab.dropout_p = site(first + li, _ATTN), enc.p_attn
                _drop_call("mmdeer_bert_attn_drop_bwd", ab, drop)
            else:
                _lib.check(lib.mmdeer_bert_attn_bwd(C.byref(ab)))
            del dctx, cx, qkv
            if any(needs[16 * li + i] for i in (_Q_W, _Q_B, _K_W, _K_B, _V_W, _V_B)):
                gw, gb = torch.empty(3 * H, H, device=dev), torch.empty(3 * H, device=dev)
                ex.dw(dqkv, 3 * H, x, H, gw, gb, M, 3 * H, H)
                for j, (wi, bi) in enumerate(((_Q_W, _Q_B), (_K_W, _K_B), (_V_W, _V_B))):
                    grads[16 * li + wi], grads[16 * li + bi] = gw[j * H:(j + 1) * H], gb[j * H:(j + 1) * H]
            del x
            if li > lowest:
                g = torch.empty(M, H, dtype=dt, device=dev)
                ex.dx(dqkv, 3 * H, p["wqkv"], g, H, M)
                g2 = ds1
            del dqkv, ds1
        ctx.tape.clear()
        out = [gr.to(d) if gr is not None and need else None for gr, d, need in zip(grads, ctx.dtypes, needs)]
        return (None, None, None, None, None, None, None, None, *out)
