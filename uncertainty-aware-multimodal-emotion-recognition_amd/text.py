"""Temporal text encoder: ``encoders.EnhancedTextEncoder`` (reference src/models/encoders.py:553-761) on token-level text --
ids and a mask (the reference's no-BERT configuration: ``nn.Embedding(30000, 768, padding_idx=0)`` + ``nn.Embedding(128, 768)``),
a (B, L, 768) matrix of contextual embeddings from the caller's own BERT (the reference's BERT branch downstream of
``last_hidden_state``), or -- constructed with ``bert=BertEncoder(...)`` (mmdeer.bert: the trunk on HIP, frozen or with its last layers fine-tuned) -- the
reference's BERT configuration itself: ids and a mask through the trunk, then the same path on its ``last_hidden_state``
-> the (B, 512) block that ``ComposedDEER`` / ``generic_fusion`` take.  Tokenisation and pretrained weights are outside this
package.

Per forward: ``mmdeer_token_embed_fwd`` (gather + position + mask, or mask alone), one ``mmdeer_gemm`` over all B * L rows for
the pool's ``W1 x + b1``, ``mmdeer_token_pool_fwd`` (masked softmax over tokens, renormalisation, weighted sum),
``mmdeer_token_stats`` (the ten "linguistic features", one workgroup per sample instead of the reference's host loop over the
batch), then ``bert_projection``, ``linguistic_projection`` and ``output_projection`` as GEMMs with the ReLU / counter-hash
dropout in their epilogues and ``mmdeer_layernorm_fwd``.  The backward mirrors it; both table gradients are dense, fp32 and
deterministic (``mmdeer_token_embed_bwd``: no floating-point atomics).  Masks are taken as binary (nonzero = valid).  No CPU
path: CPU tensors raise."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import torch
from torch import nn

from . import _lib, fusions, ops, side
from .bert import BertEncoder

_SITE_BERT, _SITE_LING, _SITE_OUT = 136, 137, 138    # the reference's three nn.Dropout sites; the pool has none

E = 768              # bert_hidden_size
A = E // 2           # the score layer of token_attention
STATS = 16           # the ten features + six zero columns (K % 4 == 0 for the GEMM that follows)
MAX_ROWS = 1 << 20   # B * L limit of the table-gradient path (mmdeer_sort_pairs)


def _embed_args(compute_dtype, B, L) -> _lib.TokenEmbedArgs:
    a = _lib.TokenEmbedArgs()
    a.B, a.L, a.width, a.act_f32, a.stream = B, L, E, int(compute_dtype == "fp32"), _lib.current_stream()
    return a


class _TokenEmbedFn(torch.autograd.Function):
    """ids (B, L) int64, m (B * L) fp32 0 / 1 -> x (B * L, 768) in the compute dtype = (emb[clamp(id)] + pos[min(t, P - 1)]) * m,
    and the clamped ids (B * L) int32."""

    @staticmethod
    def forward(ctx, emb, pos, ids, m, B, L, compute_dtype):
        dt = ops._act_dtype(compute_dtype)
        ew, pw = emb.detach().float().contiguous(), pos.detach().float().contiguous()
        x = torch.empty(B * L, E, dtype=dt, device=ids.device)
        ids32 = torch.empty(B * L, dtype=torch.int32, device=ids.device)
        a = _embed_args(compute_dtype, B, L)
        a.ids, a.mask, a.emb, a.pos, a.V, a.P = ids.data_ptr(), m.data_ptr(), ew.data_ptr(), pw.data_ptr(), ew.shape[0], pw.shape[0]
        a.x, a.ld_x, a.ids32 = x.data_ptr(), E, ids32.data_ptr()
        _lib.check(_lib.load().mmdeer_token_embed_fwd(C.byref(a)))
        ctx.save_for_backward(ids32, m)
        ctx.meta = (B, L, compute_dtype, ew.shape[0], pw.shape[0], emb.dtype, pos.dtype)
        ctx.mark_non_differentiable(ids32)
        return x, ids32

    @staticmethod
    def backward(ctx, gx, _gi):
        ids32, m = ctx.saved_tensors
        B, L, compute_dtype, V, P, edt, pdt = ctx.meta
        lib = _lib.load()
        dx = gx.to(ops._act_dtype(compute_dtype)).contiguous()
        d_emb, d_pos = torch.empty(V, E, device=dx.device), torch.empty(P, E, device=dx.device)
        nbytes = lib.mmdeer_token_embed_bwd_scratch(B * L)
        scratch = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dx.device)
        a = _embed_args(compute_dtype, B, L)
        a.mask, a.ids32, a.V, a.P, a.dx, a.ld_dx = m.data_ptr(), ids32.data_ptr(), V, P, dx.data_ptr(), E
        a.d_emb, a.d_pos, a.scratch, a.scratch_bytes = d_emb.data_ptr(), d_pos.data_ptr(), scratch.data_ptr(), nbytes
        _lib.check(lib.mmdeer_token_embed_bwd(C.byref(a)))
        return d_emb.to(edt), d_pos.to(pdt), None, None, None, None, None


class _TokenSrcFn(torch.autograd.Function):
    """src (B * L, 768) precomputed embeddings, m (B * L) -> x = src * m in the compute dtype; backward d_src = dx * m."""

    @staticmethod
    def forward(ctx, src, m, B, L, compute_dtype):
        dt = ops._act_dtype(compute_dtype)
        s = src.detach().float().contiguous()
        x = torch.empty(B * L, E, dtype=dt, device=src.device)
        a = _embed_args(compute_dtype, B, L)
        a.mask, a.src, a.ld_src, a.x, a.ld_x = m.data_ptr(), s.data_ptr(), E, x.data_ptr(), E
        _lib.check(_lib.load().mmdeer_token_embed_fwd(C.byref(a)))
        ctx.save_for_backward(m)
        ctx.meta = (B, L, compute_dtype, src.dtype)
        return x

    @staticmethod
    def backward(ctx, gx):
        (m,) = ctx.saved_tensors
        B, L, compute_dtype, sdt = ctx.meta
        dx = gx.to(ops._act_dtype(compute_dtype)).contiguous()
        d_src = torch.empty(B * L, E, device=dx.device)
        a = _embed_args(compute_dtype, B, L)
        a.mask, a.dx, a.ld_dx, a.d_src, a.ld_dsrc = m.data_ptr(), dx.data_ptr(), E, d_src.data_ptr(), E
        _lib.check(_lib.load().mmdeer_token_embed_bwd(C.byref(a)))
        return d_src.to(sdt), None, None, None, None


def _pool_args(compute_dtype, B, L) -> _lib.TokenPoolArgs:
    a = _lib.TokenPoolArgs()
    a.B, a.L, a.width, a.att_width, a.act_f32, a.stream = B, L, E, A, int(compute_dtype == "fp32"), _lib.current_stream()
    return a


class _TokenPoolFn(torch.autograd.Function):
    """masked attention pool over tokens: x (B * L, 768) already masked, z = W1 x + b1 (B * L, 384), m (B * L)
    -> attended (B, 768) fp32 and the renormalised weights (B, L) fp32."""

    @staticmethod
    def forward(ctx, x, z, m, w2, b2, B, L, compute_dtype):
        dt = ops._act_dtype(compute_dtype)
        xa, za = x.detach().to(dt).contiguous(), z.detach().to(dt).contiguous()
        w2f, b2f = w2.detach().float().reshape(-1).contiguous(), b2.detach().float().reshape(-1).contiguous()
        att = torch.empty(B, E, dtype=dt, device=x.device)
        wts, probs = torch.empty(B, L, device=x.device), torch.empty(B, L, device=x.device)
        a = _pool_args(compute_dtype, B, L)
        a.x, a.ld_x, a.z, a.ld_z, a.mask, a.w2, a.b2 = xa.data_ptr(), E, za.data_ptr(), A, m.data_ptr(), w2f.data_ptr(), b2f.data_ptr()
        a.attended, a.ld_att, a.weights, a.probs = att.data_ptr(), E, wts.data_ptr(), probs.data_ptr()
        _lib.check(_lib.load().mmdeer_token_pool_fwd(C.byref(a)))
        ctx.save_for_backward(xa, za, m, w2f, wts, probs)
        ctx.meta = (B, L, compute_dtype, x.dtype, z.dtype, w2.dtype, w2.shape, b2.dtype, b2.shape)
        ctx.mark_non_differentiable(wts)
        return att.float(), wts

    @staticmethod
    def backward(ctx, gatt, _gw):
        xa, za, m, w2f, wts, probs = ctx.saved_tensors
        B, L, compute_dtype, xdt, zdt, wdt, wshape, bdt, bshape = ctx.meta
        dev, dt = xa.device, xa.dtype
        dout = gatt.to(dt).contiguous()
        dx, dz = torch.empty_like(xa), torch.empty_like(za)
        dw2, db2 = torch.empty(A, device=dev), torch.empty(1, device=dev)
        scratch = torch.empty(_lib.TOKEN_POOL_SCRATCH, device=dev)
        a = _pool_args(compute_dtype, B, L)
        a.x, a.ld_x, a.z, a.ld_z, a.mask, a.w2 = xa.data_ptr(), E, za.data_ptr(), A, m.data_ptr(), w2f.data_ptr()
        a.weights, a.probs, a.dout, a.ld_dout = wts.data_ptr(), probs.data_ptr(), dout.data_ptr(), E
        a.dx, a.ld_dx, a.dz, a.ld_dz = dx.data_ptr(), E, dz.data_ptr(), A
        a.dw2, a.db2, a.scratch = dw2.data_ptr(), db2.data_ptr(), scratch.data_ptr()
        _lib.check(_lib.load().mmdeer_token_pool_bwd(C.byref(a)))
        return dx.to(xdt), dz.to(zdt), None, dw2.reshape(wshape).to(wdt), db2.reshape(bshape).to(bdt), None, None, None


def token_pool(x, m, attention: nn.Sequential, B: int, L: int, compute_dtype: str):
    """``attention`` = Sequential(Linear(768, 384), Tanh, Linear(384, 1), Softmax(dim=1)) over batch-major masked rows
    x (B * L, 768) -> (attended (B, 768) fp32, weights (B, L) fp32)."""
    z = fusions._LinearFn.apply(x, attention[0].weight, attention[0].bias, compute_dtype, False, None, -1)     # (B * L, 384)
    return _TokenPoolFn.apply(x, z, m, attention[2].weight, attention[2].bias, B, L, compute_dtype)


def token_stats(ids32: torch.Tensor, m: torch.Tensor, B: int, L: int, max_length: int) -> torch.Tensor:
    """ids32 (B * L) int32, m (B * L) fp32 -> (B, 16) fp32: the reference's ten "linguistic features" and six zero columns."""
    ops._check_dev(ids32, m)
    out = torch.empty(B, STATS, device=ids32.device)
    a = _lib.TokenStatsArgs()
    a.ids, a.mask, a.out, a.ld_out = ids32.data_ptr(), m.data_ptr(), out.data_ptr(), STATS
    a.B, a.L, a.max_length, a.stream = B, L, int(max_length), _lib.current_stream()
    _lib.check(_lib.load().mmdeer_token_stats(C.byref(a)))
    return out


class TemporalTextEncoder(nn.Module):
    """``encoders.EnhancedTextEncoder`` without BERT: the same parameters, initialisation and ``state_dict`` as the reference's
    no-BERT configuration (14 keys), so its checkpoints load with ``strict=True``.

    ``forward(input_ids, attention_mask)``: (B, L) ids and mask -> (B, 512) fp32, the reference's fallback branch (ids are
    clamped to the vocabulary, positions to ``max_text_length - 1``).
    ``forward_embeddings(token_embeddings, input_ids, attention_mask)``: (B, L, 768) fp32 or bf16 contextual embeddings (what
    the reference takes from ``bert(...).last_hidden_state``) -> (B, 512) fp32; differentiable w.r.t. the embeddings.  The
    ids feed the token statistics only and are NOT clamped, as in the reference; negative valid ids are undefined input (the
    reference's ``bincount`` raises on them; checking here would cost a device sync per call).
    In ``.train()`` the three dropout sites of the reference are live (the library's counter-hash masks).

    ``bert=BertEncoder(...)`` (``hidden_size`` 768) makes it the reference's BERT configuration: the module holds the trunk as
    ``self.bert`` and creates no ``embedding`` / ``positional_encoding`` tables, so its ``state_dict`` keys are the reference's
    (``bert.*``, ``token_attention.*``, ...).  ``forward(input_ids, attention_mask)`` then runs the trunk and ``forward_embeddings`` on its
    ``last_hidden_state`` as it comes, fp32 or bf16; everything behind the trunk trains as without it.  A frozen trunk
    (``finetune_layers == 0``) runs under ``no_grad``, as does any trunk while grad is disabled.  A trunk built with
    ``finetune_layers=k`` is called with grad when grad is enabled: the gradient of the embeddings that ``forward_embeddings``
    produces flows on into the trunk's last ``k`` layers (the reference fine-tunes layers 6-11 of 12: k = 6).  The trunk follows
    this module's ``train()`` / ``eval()``: built with ``dropout=True`` (the reference's training configuration: hidden and attention
    dropout 0.1 in every layer) its dropout is live in ``train()``, with a seed and step counter of its own; by default it has none."""

    def __init__(self, config: Optional[Dict] = None, compute_dtype: str = "fp32", bert: Optional[BertEncoder] = None):
        super().__init__()
        config = config or {}
        self.hidden_dim = config.get("hidden_dim", 512)
        self.dropout = config.get("dropout", 0.3)
        self.max_length = config.get("max_text_length", 128)
        self.compute_dtype = compute_dtype
        ops._act_dtype(compute_dtype)
        self.dropout_seed, self._train_step = config.get("dropout_seed", 0), 0     # counter-hash dropout: seed + one tick per training forward
        self._step_counter, self._counter_k = None, 0                              # ... or a device counter + the live forwards since it was read
        if self.hidden_dim % 32:
            raise NotImplementedError("hidden_dim must be a multiple of 32")
        if bert is not None and not isinstance(bert, BertEncoder):
            raise TypeError(f"bert must be a mmdeer.bert.BertEncoder (got {type(bert).__name__})")
        if bert is not None and bert.hidden_size != E:
            raise ValueError(f"the text encoder takes a BERT trunk of hidden_size {E} (got {bert.hidden_size})")
        self.bert = bert
        self.bert_hidden_size = E
        if bert is None:
            self.vocab_size = 30000
            self.embedding = nn.Embedding(self.vocab_size, E, padding_idx=0)
            self.positional_encoding = nn.Embedding(self.max_length, E)
        self.token_attention = nn.Sequential(nn.Linear(E, A), nn.Tanh(), nn.Linear(A, 1), nn.Softmax(dim=1))
        self.bert_projection = nn.Sequential(nn.Linear(E, self.hidden_dim), nn.ReLU(), nn.Dropout(self.dropout))
        self.linguistic_features_dim = 10
        self.linguistic_projection = nn.Sequential(nn.Linear(10, self.hidden_dim // 4), nn.ReLU(), nn.Dropout(self.dropout))
        self.output_projection = nn.Sequential(nn.Linear(self.hidden_dim + self.hidden_dim // 4, self.hidden_dim), nn.ReLU(),
                                               nn.Dropout(self.dropout), nn.LayerNorm(self.hidden_dim))

    # ---------------------------------------------------------------------------------------------------------------------
    def _check(self, input_ids, attention_mask):
        if input_ids.dim() != 2 or tuple(attention_mask.shape) != tuple(input_ids.shape):
            raise ValueError(f"expected input_ids and attention_mask of one shape (B, L), got {tuple(input_ids.shape)} and "
                             f"{tuple(attention_mask.shape)}")
        if input_ids.shape[1] == 0:
            raise ValueError("expected at least one token position (L >= 1)")
        if input_ids.dtype.is_floating_point or input_ids.dtype == torch.bool:
            raise ValueError(f"input_ids must be an integer tensor (got {input_ids.dtype})")
        return input_ids.shape[0], input_ids.shape[1]

    def _drop(self):
        if self.training and self.dropout > 0:
            if self._step_counter is not None:       # the step on the device: opseq.set_drop forwards the counter as offset_dev
                d = (self.dropout, int(self.dropout_seed), self._counter_k, self._step_counter)
                self._counter_k += 1
                return d
            d = (self.dropout, int(self.dropout_seed), self._train_step)
            self._train_step += 1
            return d
        return None

    def set_step_counter(self, t: Optional[torch.Tensor]) -> None:
        """Take the dropout step from the device, for a captured graph: ``t`` is a one-element int64 tensor on this module's device,
        or None to return to the host counter.  Live forward number k = 0, 1, ... since ``take_step_count()`` last returned hashes
        step k + *t, read when the kernels run; the owner of the graph adds ``take_step_count()`` to ``t`` at the end of the captured
        region (``mmdeer.train_graph.capture_train_step``).  A ``bert=`` trunk gets the same call; give it a counter of its own
        afterwards where its step differs."""
        if t is not None:
            dev = self.token_attention[0].weight.device
            if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.numel() != 1 or t.device != dev:
                raise ValueError(f"set_step_counter: expected a one-element int64 tensor on {dev}, got "
                                 f"{(t.dtype, tuple(t.shape), t.device) if isinstance(t, torch.Tensor) else type(t).__name__}")
        self._step_counter, self._counter_k = t, 0
        if self.bert is not None:
            self.bert.set_step_counter(t)

    def take_step_count(self) -> int:
        """live forwards since the last call (or since the counter was set); restarts at 0"""
        k, self._counter_k = self._counter_k, 0
        return k

    def extract_linguistic_features(self, input_ids: torch.Tensor, attention_mask: torch.Tensor) -> torch.Tensor:
        """(B, L) ids and mask -> (B, 10) fp32, the reference's features (encoders.py:648-699) from one launch."""
        B, L = self._check(input_ids, attention_mask)
        ops._check_dev(input_ids, attention_mask)
        if B == 0:
            return torch.zeros(0, 10, device=input_ids.device)
        m = (attention_mask != 0).float().reshape(-1).contiguous()
        return token_stats(input_ids.to(torch.int32).reshape(-1).contiguous(), m, B, L, self.max_length)[:, :10]

    def _tail(self, x, ids32, m, B, L, drop):
        c = self.compute_dtype
        attended, self.last_attention_weights = token_pool(x, m, self.token_attention, B, L, c)
        pb = fusions.linear(attended, self.bert_projection[0], c, relu=True, drop=drop, site=_SITE_BERT)
        stats = token_stats(ids32, m, B, L, self.max_length)
        lp = self.linguistic_projection[0]
        w = torch.nn.functional.pad(lp.weight, (0, STATS - lp.in_features))       # zero columns under the zero features
        pl = fusions._LinearFn.apply(stats, w, lp.bias, c, True, drop, _SITE_LING)
        op = self.output_projection
        y = fusions.linear(torch.cat([pb, pl], dim=1), op[0], c, relu=True, drop=drop, site=_SITE_OUT)
        return side._LayerNormFn.apply(y, op[3].weight, op[3].bias, c)

    def forward(self, input_ids: torch.Tensor, attention_mask: torch.Tensor) -> torch.Tensor:
        B, L = self._check(input_ids, attention_mask)
        ops._check_dev(input_ids, attention_mask)
        if B == 0:
            return torch.zeros(0, self.hidden_dim, device=input_ids.device)
        if self.bert is not None:
            with torch.set_grad_enabled(torch.is_grad_enabled() and self.bert.finetune_layers > 0):     # the reference: set_grad_enabled(self.training)
                hidden = self.bert(input_ids, attention_mask).last_hidden_state
            return self.forward_embeddings(hidden, input_ids, attention_mask)
        if B * L > MAX_ROWS and torch.is_grad_enabled() and (self.embedding.weight.requires_grad or self.positional_encoding.weight.requires_grad):
            raise ValueError(f"B * L = {B * L} is above the {MAX_ROWS} rows the table gradients take")
        m = (attention_mask != 0).float().reshape(-1).contiguous()
        ids = input_ids.to(torch.int64).reshape(-1).contiguous()
        drop = self._drop()
        x, ids32 = _TokenEmbedFn.apply(self.embedding.weight, self.positional_encoding.weight, ids, m, B, L, self.compute_dtype)
        return self._tail(x, ids32, m, B, L, drop)

    def forward_embeddings(self, token_embeddings: torch.Tensor, input_ids: torch.Tensor, attention_mask: torch.Tensor) -> torch.Tensor:
        B, L = self._check(input_ids, attention_mask)
        if token_embeddings.dim() != 3 or tuple(token_embeddings.shape[:2]) != (B, L) or token_embeddings.shape[2] != E:
            raise ValueError(f"expected token_embeddings of shape ({B}, {L}, {E}), got {tuple(token_embeddings.shape)}")
        if token_embeddings.dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"token_embeddings must be fp32 or bf16 (got {token_embeddings.dtype})")
        ops._check_dev(token_embeddings, input_ids, attention_mask)
        if B == 0:
            return torch.zeros(0, self.hidden_dim, device=input_ids.device)
        m = (attention_mask != 0).float().reshape(-1).contiguous()
        ids32 = input_ids.to(torch.int32).reshape(-1).contiguous()
        drop = self._drop()
        x = _TokenSrcFn.apply(token_embeddings.reshape(B * L, E), m, B, L, self.compute_dtype)
        return self._tail(x, ids32, m, B, L, drop)
