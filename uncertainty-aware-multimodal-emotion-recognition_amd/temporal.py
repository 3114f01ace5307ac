"""Temporal audio encoder: ``encoders.EnhancedAudioEncoder`` on (B, T, 84) pre-extracted features for any T >= 1
(reference src/models/encoders.py:376-389): a bidirectional nn.LSTM over the time steps, the learned attention pool over
time, then ``output_projection``.

``TemporalAudioEncoder`` subclasses ``side.EnhancedAudioEncoder``: the same constructor, parameters, initialisation and
``state_dict``.  T = 1 runs the parent's path.  For T > 1, per LSTM layer: one ``mmdeer_gemm`` over all T * B rows against
the stacked ``[W_ih; W_ih_reverse]`` (bias ``b_ih + b_hh``) and ONE ``mmdeer_lstm_seq_fwd`` launch for all T steps of both
directions; between layers the counter-hash dropout; then the pool's ``W1 h + b1`` GEMM and ``mmdeer_temporal_pool_fwd``.
The backward runs ``mmdeer_lstm_seq_bwd`` once per layer and forms ``dW_hh`` with one GEMM per direction over (T - 1) * B
rows (rows are time-major, so ``h_{t-1}`` of every step is the same matrix shifted by B rows).  No CPU path: CPU tensors
raise.

Padded batches: ``forward(x, lengths)`` with ``lengths[b] = n_b`` valid steps encodes sample b as that sample alone at its own length
(torch's ``pack_padded_sequence`` -> ``nn.LSTM`` -> ``pad_packed_sequence`` per layer, and a pool whose softmax runs over t < n_b),
through the entries of include/mmdeer_seqlen.h: no packing, no sorting and, for lengths already on the device, no host sync, so a
captured training step replays with other lengths.  The LSTM output rows t >= n_b are stored zeros and every gradient there is an
exact zero; the forward does not depend on what the padded positions of x hold (NaN and Inf included).  TRAINING NEEDS FINITE
PADDING: the weight-gradient GEMM multiplies the zero gate gradients of a padded row by that row of x, and 0 * NaN is NaN."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib, fusions, ops, side
from .opseq import Exec

_SITE_SEQ = 128     # the inter-layer dropout of layer l on the (T * B, 512) LSTM output: site 128 + l

H = 256             # hidden units per direction (hidden_dim 512)


def as_lengths(lengths, B: int, T: int, device) -> torch.Tensor:
    """``lengths`` as the (B,) int32 tensor on ``device`` that the kernels read (they clamp each value to [0, T]).  A CUDA int32 /
    int64 tensor is used as it is (int64 converted on the device): no value is looked at and nothing synchronises.  A CPU tensor or a
    Python sequence is range-checked here (``ValueError`` outside [0, T]) and uploaded.  ``TypeError`` for anything but integers."""
    if isinstance(lengths, torch.Tensor) and lengths.is_cuda:
        if lengths.dtype not in (torch.int32, torch.int64):
            raise TypeError(f"lengths must be int32 or int64 (got {lengths.dtype})")
        if tuple(lengths.shape) != (B,):
            raise ValueError(f"lengths must have shape ({B},), got {tuple(lengths.shape)}")
        if lengths.dtype == torch.int64:
            lengths = lengths.clamp(0, T).to(torch.int32)
        return lengths.to(device).contiguous()
    host = lengths if isinstance(lengths, torch.Tensor) else torch.as_tensor(lengths)
    if host.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8):
        raise TypeError(f"lengths must be integers (got {host.dtype})")
    if tuple(host.shape) != (B,):
        raise ValueError(f"lengths must have shape ({B},), got {tuple(host.shape)}")
    if B and (int(host.min()) < 0 or int(host.max()) > T):
        raise ValueError(f"lengths must lie in [0, {T}] (got {int(host.min())} .. {int(host.max())})")
    return host.to(torch.int32).to(device)


def _seq_args(compute_dtype, T, B, lengths=None):
    """mmdeer_lstm_seq_args, or with ``lengths`` its companion mmdeer_lstm_seq_len_args (the same fields + lengths)"""
    a = _lib.LstmSeqArgs() if lengths is None else _lib.LstmSeqLenArgs()
    if lengths is not None:
        a.lengths = lengths.data_ptr()
    a.T, a.B, a.hidden, a.ndir, a.act_f32 = T, B, H, 2, int(compute_dtype == "fp32")
    a.stream = _lib.current_stream()
    return a


class _LstmSeqFn(torch.autograd.Function):
    """One bidirectional LSTM layer over T steps: xg (T * B, 8H) = W_ih x + b_ih + b_hh of both directions (time-major rows)
    -> h (T * B, 2H) in the compute dtype, ``[forward | reverse]``.  ``lengths`` (int32 (B,) on the device, or None): the valid steps of
    each sample, a non-differentiable input; rows t >= n_b of h and of the gradient at xg are stored zeros."""

    @staticmethod
    def forward(ctx, xg, w_hh_f, w_hh_r, T, B, compute_dtype, lengths=None):
        dt = ops._act_dtype(compute_dtype)
        lib, dev = _lib.load(), xg.device
        xga = xg.detach().to(dt).contiguous()
        train = any(ctx.needs_input_grad[:3])         # the tape and W_hh^T only when a backward can follow
        img = torch.empty(2, 4 * H, H, dtype=dt, device=dev)
        img_t = torch.empty(2, H, 4 * H, dtype=dt, device=dev) if train else None
        a = _seq_args(compute_dtype, T, B, lengths)
        _lib.check(lib.mmdeer_lstm_seq_pack(w_hh_f.detach().float().contiguous().data_ptr(), w_hh_r.detach().float().contiguous().data_ptr(),
                                            H, img.data_ptr(), _lib.ptr(img_t), a.act_f32, a.stream))
        h = torch.empty(T * B, 2 * H, dtype=dt, device=dev)
        tg = torch.empty(T * B, 8 * H, device=dev) if train else None
        tc = torch.empty(T * B, 2 * H, device=dev) if train else None
        a.xg, a.ld_xg, a.w_hh, a.h, a.ld_h = xga.data_ptr(), 8 * H, img.data_ptr(), h.data_ptr(), 2 * H
        a.tape_gates, a.tape_c = _lib.ptr(tg), _lib.ptr(tc)
        _lib.check((lib.mmdeer_lstm_seq_fwd if lengths is None else lib.mmdeer_lstm_seq_len_fwd)(C.byref(a)))
        if train:
            ctx.save_for_backward(img_t, tg, tc, h)
        ctx.lengths = lengths
        ctx.meta = (T, B, compute_dtype, xg.dtype, w_hh_f.dtype)
        return h

    @staticmethod
    def backward(ctx, gh):
        img_t, tg, tc, h = ctx.saved_tensors
        T, B, compute_dtype, xdt, wdt = ctx.meta
        ex = Exec(compute_dtype)
        dh = gh.to(h.dtype).contiguous()
        dg = torch.empty(T * B, 8 * H, dtype=h.dtype, device=h.device)
        a = _seq_args(compute_dtype, T, B, ctx.lengths)
        a.w_hh_t, a.tape_gates, a.tape_c = img_t.data_ptr(), tg.data_ptr(), tc.data_ptr()
        a.dh_out, a.ld_dh, a.dgates, a.ld_dg = dh.data_ptr(), 2 * H, dg.data_ptr(), 8 * H
        _lib.check((ex.lib.mmdeer_lstm_seq_bwd if ctx.lengths is None else ex.lib.mmdeer_lstm_seq_len_bwd)(C.byref(a)))
        gw_f, gw_r = torch.zeros(4 * H, H, device=h.device), torch.zeros(4 * H, H, device=h.device)
        if T > 1:
            R = (T - 1) * B
            # forward direction: step t reads h_{t-1}; reverse: step t reads h_{t+1} (with lengths: the stored zero row at t = n_b;
            # the gate gradients of padded rows are stored zeros, so these sums pick up nothing from padding)
            ex.dw(dg[B:, :4 * H], 8 * H, h[:R, :H], 2 * H, gw_f, None, R, 4 * H, H)
            ex.dw(dg[:R, 4 * H:], 8 * H, h[B:, H:], 2 * H, gw_r, None, R, 4 * H, H)
        return dg.to(xdt), gw_f.to(wdt), gw_r.to(wdt), None, None, None, None


def _pool_args(lengths=None):
    """mmdeer_temporal_pool_args, or with ``lengths`` its companion mmdeer_temporal_pool_len_args (the same fields + lengths)"""
    if lengths is None:
        return _lib.TemporalPoolArgs()
    a = _lib.TemporalPoolLenArgs()
    a.lengths = lengths.data_ptr()
    return a


class _TemporalPoolFn(torch.autograd.Function):
    """attention pool over time: h (T * B, 2H), z = W1 h + b1 (T * B, H) -> attended (B, 2H) fp32 and the weights (B, T).
    ``lengths`` (int32 (B,) on the device, or None): the softmax runs over t < n_b, the weights beyond are zeros."""

    @staticmethod
    def forward(ctx, h, z, w2, b2, T, B, compute_dtype, lengths=None):
        dt = ops._act_dtype(compute_dtype)
        ha, za = h.detach().to(dt).contiguous(), z.detach().to(dt).contiguous()
        w2f, b2f = w2.detach().float().reshape(-1).contiguous(), b2.detach().float().reshape(-1).contiguous()
        att = torch.empty(B, 2 * H, dtype=dt, device=h.device)
        wts = torch.empty(B, T, device=h.device)
        a = _pool_args(lengths)
        a.h, a.ld_h, a.z, a.ld_z, a.w2, a.b2 = ha.data_ptr(), 2 * H, za.data_ptr(), H, w2f.data_ptr(), b2f.data_ptr()
        a.attended, a.ld_att, a.weights = att.data_ptr(), 2 * H, wts.data_ptr()
        a.T, a.B, a.hidden, a.act_f32, a.stream = T, B, H, int(dt == torch.float32), _lib.current_stream()
        lib = _lib.load()
        _lib.check((lib.mmdeer_temporal_pool_fwd if lengths is None else lib.mmdeer_temporal_pool_len_fwd)(C.byref(a)))
        ctx.save_for_backward(ha, za, w2f, wts)
        ctx.lengths = lengths
        ctx.meta = (T, B, h.dtype, z.dtype, w2.dtype, w2.shape, b2.dtype, b2.shape)
        ctx.mark_non_differentiable(wts)
        return att.float(), wts

    @staticmethod
    def backward(ctx, gatt, _gw):
        ha, za, w2f, wts = ctx.saved_tensors
        T, B, hdt, zdt, wdt, wshape, bdt, bshape = ctx.meta
        dev, dt = ha.device, ha.dtype
        dout = gatt.to(dt).contiguous()
        dh, dz = torch.empty_like(ha), torch.empty_like(za)
        dw2, db2 = torch.zeros(H, device=dev), torch.zeros(1, device=dev)
        scratch = torch.empty(_lib.TEMPORAL_POOL_SCRATCH, device=dev)
        a = _pool_args(ctx.lengths)
        a.h, a.ld_h, a.z, a.ld_z, a.w2, a.weights = ha.data_ptr(), 2 * H, za.data_ptr(), H, w2f.data_ptr(), wts.data_ptr()
        a.dout, a.ld_dout, a.dh, a.ld_dh, a.dz, a.ld_dz = dout.data_ptr(), 2 * H, dh.data_ptr(), 2 * H, dz.data_ptr(), H
        a.dw2, a.db2, a.scratch = dw2.data_ptr(), db2.data_ptr(), scratch.data_ptr()
        a.T, a.B, a.hidden, a.act_f32, a.stream = T, B, H, int(dt == torch.float32), _lib.current_stream()
        lib = _lib.load()
        _lib.check((lib.mmdeer_temporal_pool_bwd if ctx.lengths is None else lib.mmdeer_temporal_pool_len_bwd)(C.byref(a)))
        return dh.to(hdt), dz.to(zdt), dw2.reshape(wshape).to(wdt), db2.reshape(bshape).to(bdt), None, None, None, None


def lstm_layer(x, lstm: torch.nn.LSTM, layer: int, T: int, B: int, compute_dtype: str, lengths=None) -> torch.Tensor:
    """One bidirectional layer of ``lstm`` on time-major rows x (T * B, in) -> (T * B, 2H) in the compute dtype.  ``lengths``
    (what ``as_lengths`` takes): each sample runs its own n_b steps, as under ``pack_padded_sequence``."""
    P = lambda n: getattr(lstm, f"{n}_l{layer}")                                  # noqa: E731
    R = lambda n: getattr(lstm, f"{n}_l{layer}_reverse")                          # noqa: E731
    w = torch.cat([P("weight_ih"), R("weight_ih")], dim=0)
    b = torch.cat([P("bias_ih") + P("bias_hh"), R("bias_ih") + R("bias_hh")])
    xg = fusions._LinearFn.apply(x, w, b, compute_dtype, False, None, -1)          # (T * B, 2 * 4H)
    if lengths is None:
        return _LstmSeqFn.apply(xg, P("weight_hh"), R("weight_hh"), T, B, compute_dtype)
    return _LstmSeqFn.apply(xg, P("weight_hh"), R("weight_hh"), T, B, compute_dtype, as_lengths(lengths, B, T, xg.device))


def temporal_pool(h, attention: torch.nn.Sequential, T: int, B: int, compute_dtype: str, lengths=None):
    """``attention`` = Sequential(Linear(2H, H), Tanh, Linear(H, 1), Softmax(dim=1)) over time-major h (T * B, 2H)
    -> (attended (B, 2H) fp32, weights (B, T) fp32).  ``lengths``: the softmax runs over each sample's t < n_b."""
    z = fusions._LinearFn.apply(h, attention[0].weight, attention[0].bias, compute_dtype, False, None, -1)   # (T * B, H)
    if lengths is None:
        return _TemporalPoolFn.apply(h, z, attention[2].weight, attention[2].bias, T, B, compute_dtype)
    return _TemporalPoolFn.apply(h, z, attention[2].weight, attention[2].bias, T, B, compute_dtype, as_lengths(lengths, B, T, h.device))


class TemporalAudioEncoder(side.EnhancedAudioEncoder):
    """``encoders.EnhancedAudioEncoder`` (reference src/models/encoders.py:65-126, 356-389) on pre-extracted features:
    (B, 84) or (B, T, 84) for any T >= 1 -> (B, 512) fp32.  Same parameters and ``state_dict`` as the parent, so reference
    checkpoints load with ``strict=True``.  In ``.train()`` the LSTM's inter-layer dropout and the output projection's
    dropout are live (the library's counter-hash masks); the attention pool has none, as in the reference.

    ``forward(x, lengths)``: a batch padded to T steps with ``lengths[b] = n_b`` valid ones (``as_lengths`` says what is taken); row b
    is then ``forward(x[b:b+1, :n_b])`` whatever the padding holds, and n_b = 0 gives what ``output_projection`` makes of zeros.
    With lengths even T = 1 (and a 2-D input) runs the sequence path.  Training needs finite padding (see the module text)."""

    def forward(self, audio_input: torch.Tensor, lengths=None) -> torch.Tensor:
        x = audio_input
        if x.shape[-1] != self.enhanced_features_dim:
            raise NotImplementedError("raw-waveform input (host-side librosa feature extraction) is outside the hot path")
        if x.dim() not in (2, 3):
            raise ValueError(f"expected (B, 84) or (B, T, 84), got {tuple(audio_input.shape)}")
        if lengths is None and (x.dim() == 2 or x.shape[1] == 1):
            return super().forward(x)
        if x.dim() == 2:
            x = x.unsqueeze(1)
        B, T = x.shape[0], x.shape[1]
        if T == 0:
            raise ValueError("expected at least one time step")
        if self.hidden_dim != 2 * H:
            raise NotImplementedError(f"the sequence path is built for hidden_dim = {2 * H} (got {self.hidden_dim})")
        if lengths is not None and not (isinstance(lengths, torch.Tensor) and lengths.is_cuda):
            lengths = as_lengths(lengths, B, T, "cpu")                           # the host checks, before anything runs
        ops._check_dev(x)
        if lengths is not None:
            lengths = as_lengths(lengths, B, T, x.device)
        if B == 0:
            return torch.zeros(0, self.hidden_dim, device=x.device)
        c = self.compute_dtype
        drop = None
        if self.training and self.dropout > 0:
            drop = self._drop_step(self.dropout, self.dropout_seed)
        h = x.transpose(0, 1).reshape(T * B, self.enhanced_features_dim)       # time-major rows t * B + b
        for layer in range(self.num_layers):
            h = lstm_layer(h, self.lstm, layer, T, B, c, lengths)
            if drop is not None and layer + 1 < self.num_layers:                 # nn.LSTM's inter-layer dropout
                h = side._DropoutFn.apply(h, c, drop, _SITE_SEQ + layer)
        attended, _ = temporal_pool(h, self.attention, T, B, c, lengths)
        op = self.output_projection
        y = fusions.linear(attended, op[0], c, relu=True, drop=drop, site=side._SITE_OP)
        y = fusions.linear(y, op[3], c)
        return side._LayerNormFn.apply(y, op[4].weight, op[4].bias, c)
