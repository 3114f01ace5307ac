"""The evidential head as modules of its own: ``deer.DEERLayer`` (reference src/models/deer.py:30-108) and
``deer.MultiDimensionalDEER`` (:198-266) on any feature width -- same constructor arguments, attribute names, ``state_dict``
keys and shapes, initialisation and output dictionaries -- and ``ComposedDEER``, a fusion module + a head as one trainable model.

Host logic only.  Every Linear but the last of an evidence net is an ``mmdeer_gemm`` call (bias + ReLU + counter-hash dropout in
the epilogue; the autograd nodes of ``fusions.py``); the last Linear, the NIG activations and the three uncertainties are ONE
``mmdeer_evidence_tail_fwd`` launch for all heads (csrc/nig_tail.hip), differentiable in all seven outputs through
``mmdeer_evidence_tail_bwd``.  No CPU path: CPU tensors raise.  ``compute_dtype``: 'fp32' (exact-fp32 MFMA, the parity
configuration) or 'bf16' (bf16 storage, fp32 accumulate); inputs and outputs are fp32 tensors either way."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import torch
from torch import nn

from . import _lib, fusions, ops
from .opseq import Exec
from .stepcount import DropOwner

NIG_KEYS = ("mu", "nu", "alpha", "beta", "aleatoric_uncertainty", "epistemic_uncertainty", "uncertainty")
DIM_NAMES = ("valence", "arousal", "dominance")

# dropout sites (none of 1-9, 81-85, 96-97, 112-121, 128+): DEERLayer's two, then MultiDimensionalDEER's shared layers, its heads'
# layer 0 (one stacked GEMM: the column index tells the heads apart) and layer 1 (one site per head)
_SITE_EV0, _SITE_EV1, _SITE_FP0, _SITE_FP1, _SITE_H0, _SITE_H1 = 100, 101, 102, 103, 104, 105


def _tail_args(x, w, G: int, K: int, O: int, evid) -> _lib.EvidenceTailArgs:
    a = _lib.EvidenceTailArgs()
    a.x, a.ld_x, a.w, a.evid = x.data_ptr(), x.stride(0), w.data_ptr(), evid.data_ptr()
    a.B, a.G, a.K, a.O, a.act_f32 = x.shape[0], G, K, O, int(x.dtype == torch.float32)
    a.stream = _lib.current_stream()
    return a


class _TailFn(torch.autograd.Function):
    """x (B, G K): the activations below the last layer of G evidence nets side by side; weight (G, 4 O, K), bias (G, 4 O)
    -> the seven NIG_KEYS outputs, (B, G O) fp32 each.  Outputs the loss does not use reach the backward as ``None`` and the
    operator as NULL planes: their terms are dropped, so a loss on mu, nu, alpha, beta alone has finite gradients where
    alpha - 1 underflows to 0."""

    @staticmethod
    def forward(ctx, x, weight, bias, compute_dtype):
        dt = ops._act_dtype(compute_dtype)
        xa = fusions._act(x, dt)
        G, R, K = weight.shape
        O, B = R // 4, xa.shape[0]
        w, b = weight.detach().to(dt).contiguous(), bias.detach().float().contiguous()
        evid = torch.empty(B, G * O, 4, device=xa.device)
        out = torch.empty(7, B, G * O, device=xa.device)
        a = _tail_args(xa, w, G, K, O, evid)
        a.b, a.nig_out = b.data_ptr(), out.data_ptr()
        _lib.check(_lib.load().mmdeer_evidence_tail_fwd(C.byref(a)))
        ctx.save_for_backward(xa, w, evid)
        ctx.meta = (G, K, O, x.dtype, weight.dtype, bias.dtype)
        ctx.set_materialize_grads(False)
        return tuple(out[i] for i in range(7))

    @staticmethod
    def backward(ctx, *gs):
        xa, w, evid = ctx.saved_tensors
        G, K, O, xdt, wdt, bdt = ctx.meta
        lib, dev, B = _lib.load(), xa.device, xa.shape[0]
        planes = [None if g is None else g.detach().float().contiguous() for g in gs]
        dx = torch.empty_like(xa)
        dw, db = torch.empty(G, 4 * O, K, device=dev), torch.empty(G, 4 * O, device=dev)
        scratch = torch.empty(max(int(lib.mmdeer_evidence_tail_scratch(B, G, K, O)), 4), device=dev)
        a = _tail_args(xa, w, G, K, O, evid)
        for i, p in enumerate(planes):
            a.g_out[i] = _lib.ptr(p)
        a.dx, a.ld_dx, a.dw, a.db, a.scratch = dx.data_ptr(), dx.stride(0), dw.data_ptr(), db.data_ptr(), scratch.data_ptr()
        a.mask_scale = 0.0            # the ReLU / dropout mask of x belongs to the layer below (fusions._LinearFn applies it)
        _lib.check(lib.mmdeer_evidence_tail_bwd(C.byref(a)))
        return dx.to(xdt), dw.to(wdt), db.to(bdt), None


class _HeadsLayer1Fn(torch.autograd.Function):
    """Layer 1 of D evidence nets side by side: x (B, D K), head d reads columns [d K, (d + 1) K) and writes
    drop(relu(x_d W_d^T + b_d)) into columns [d N, (d + 1) N) of the result -- D ``mmdeer_gemm`` calls on column views, no copies.
    Backward: one mask launch for all heads, ``dX`` per head into its column view, the D weight gradients as one grouped launch."""

    @staticmethod
    def forward(ctx, x, compute_dtype, drop, site, *params):
        dt = ops._act_dtype(compute_dtype)
        xa = fusions._act(x, dt)
        ex = Exec(compute_dtype, drop)
        D = len(params) // 2
        N, K = params[0].shape
        B = xa.shape[0]
        ws = [w.detach().to(dt).contiguous() for w in params[0::2]]
        y = torch.empty(B, D * N, dtype=dt, device=xa.device)
        p = ex.p_of(drop[0]) if drop else 0.0
        for d in range(D):
            ex.gemm(xa[:, d * K:], ws[d], y[:, d * N:], B, N, K, D * K, K, D * N, bias=params[2 * d + 1].detach().float().contiguous(),
                    relu=1, drop_site=site + d if p > 0 else -1, p=p)
        ctx.save_for_backward(xa, y, *ws)
        ctx.meta = (compute_dtype, ex.scale_of(drop[0]) if drop else 1.0, x.dtype, [q.dtype for q in params])
        return y.float()

    @staticmethod
    def backward(ctx, g):
        xa, y, *ws = ctx.saved_tensors
        compute_dtype, scale, xdt, pdts = ctx.meta
        ex = Exec(compute_dtype)
        D, (N, K), B, dev = len(ws), ws[0].shape, xa.shape[0], xa.device
        ga = fusions._convert(ex, g, xa.dtype)
        ga = ex.add(torch.empty_like(ga), ga, mask=y, scale=scale)     # (y > 0) / (1 - p): dropped and clipped elements are zeros of y
        dx = torch.empty_like(xa)
        gws, gbs = [torch.zeros(N, K, device=dev) for _ in ws], [torch.zeros(N, device=dev) for _ in ws]
        ex.deferred = []
        for d in range(D):
            ex.dx(ga[:, d * N:], D * N, ws[d], dx[:, d * K:], D * K, B)
            ex.dw(ga[:, d * N:], D * N, xa[:, d * K:], D * K, gws[d], gbs[d], B, N, K)
        ex.flush_dw()
        grads = []
        for d in range(D):
            grads += [gws[d].to(pdts[2 * d]), gbs[d].to(pdts[2 * d + 1])]
        return (dx.to(xdt), None, None, None, *grads)


def evidence_tail(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, compute_dtype: str = "fp32"):
    """The last layer of G evidence nets + NIG activations + uncertainties: x (B, G K), weight (G, 4 O, K), bias (G, 4 O) ->
    seven (B, G O) fp32 tensors in ``NIG_KEYS`` order."""
    return _TailFn.apply(x, weight, bias, compute_dtype)


def _refuse(cond: bool, what: str) -> None:
    if cond:
        raise NotImplementedError(what)


def _check_input(x: torch.Tensor, input_dim: int) -> None:
    if not torch.is_tensor(x) or x.dim() != 2 or x.shape[1] != input_dim:
        raise RuntimeError(f"expected (B, {input_dim}) features, got {tuple(x.shape) if torch.is_tensor(x) else type(x).__name__}")
    ops._check_dev(x)


class DEERLayer(nn.Module, DropOwner):
    """``deer.DEERLayer`` (reference src/models/deer.py:30-108): ``evidence_net`` = Linear(input_dim, hidden_dim), ReLU, Dropout,
    Linear(hidden_dim, hidden_dim // 2), ReLU, Dropout, Linear(hidden_dim // 2, 4 output_dim); Xavier-uniform weights and zero
    biases (drawn from a generator seeded with ``seed``).  ``forward(x[B, input_dim])`` -> the seven (B, output_dim) fp32 tensors of
    ``NIG_KEYS``: two ``mmdeer_gemm`` launches and one ``mmdeer_evidence_tail_fwd``.

    Supported: ``input_dim % 4 == 0``, ``hidden_dim % 16 == 0``, ``hidden_dim <= 1024``, ``1 <= output_dim <= 8``; anything else
    raises ``NotImplementedError``."""

    def __init__(self, input_dim: int, output_dim: int = 1, hidden_dim: int = 256, dropout: float = 0.3,
                 compute_dtype: str = "fp32", seed: int = 0):
        super().__init__()
        ops._act_dtype(compute_dtype)
        _refuse(input_dim <= 0 or input_dim % 4 != 0, f"input_dim = {input_dim}: must be a positive multiple of 4 (16-byte fp32 rows)")
        _refuse(hidden_dim <= 0 or hidden_dim % 16 != 0 or hidden_dim > 1024,
                f"hidden_dim = {hidden_dim}: must be a multiple of 16, at most 1024 (the tail reads hidden_dim // 2 <= 512 columns in 16-byte pieces)")
        _refuse(not 1 <= output_dim <= 8, f"output_dim = {output_dim}: must be in [1, 8]")
        self.input_dim, self.output_dim = input_dim, output_dim
        self.compute_dtype = compute_dtype
        self.evidence_net = nn.Sequential(
            nn.Linear(input_dim, hidden_dim), nn.ReLU(), nn.Dropout(dropout),
            nn.Linear(hidden_dim, hidden_dim // 2), nn.ReLU(), nn.Dropout(dropout),
            nn.Linear(hidden_dim // 2, 4 * output_dim))
        self._init_weights(torch.Generator().manual_seed(seed))
        self._drop = fusions._Drop(seed)

    def _init_weights(self, gen: Optional[torch.Generator] = None) -> None:
        for m in self.evidence_net:                       # deer.py:61-66
            if isinstance(m, nn.Linear):
                with torch.no_grad():
                    bound = (6.0 / (m.in_features + m.out_features)) ** 0.5
                    m.weight.uniform_(-bound, bound, generator=gen)
                    m.bias.zero_()

    def forward(self, x: torch.Tensor) -> Dict[str, torch.Tensor]:
        _check_input(x, self.input_dim)
        if x.shape[0] == 0:
            return {k: torch.zeros(0, self.output_dim, device=x.device) for k in NIG_KEYS}
        net, cd = self.evidence_net, self.compute_dtype
        drop = self._drop.next(self, max(net[2].p, net[5].p))
        d0, d1 = (None if drop is None or p <= 0 else (p,) + drop[1:] for p in (net[2].p, net[5].p))
        h = fusions.linear(x, net[0], cd, relu=True, drop=d0, site=_SITE_EV0)
        h = fusions.linear(h, net[3], cd, relu=True, drop=d1, site=_SITE_EV1)
        outs = _TailFn.apply(h, net[6].weight.unsqueeze(0), net[6].bias.unsqueeze(0), cd)
        return dict(zip(NIG_KEYS, outs))


class MultiDimensionalDEER(nn.Module, DropOwner):
    """``deer.MultiDimensionalDEER`` (reference src/models/deer.py:198-266): the shared ``feature_processor`` (two Linear-ReLU-
    Dropout layers, torch's default ``nn.Linear`` initialisation), one ``DEERLayer(hidden_dim, 1, hidden_dim // 2)`` per
    emotion dimension in ``deer_heads``, ``dimension_names``.  ``forward(x[B, input_dim])`` -> ``{dim}_{key}`` (B, 1) for the
    seven ``NIG_KEYS``, ``mu_all`` and ``uncertainty_all`` (B, emotion_dims).

    Launch plan: two GEMMs for the shared layers, layer 0 of all heads as ONE GEMM against their stacked weights, layer 1 as one
    GEMM per head on column views of its input and output (no copies; the weight gradients as one grouped launch), ONE
    evidence-tail launch for all heads.

    Supported: ``input_dim % 4 == 0``, ``hidden_dim % 32 == 0``, ``hidden_dim <= 2048``, ``1 <= emotion_dims <= 3`` (the
    reference builds the extra heads of ``emotion_dims > 3`` and silently never runs them: it has three names, deer.py:231);
    anything else raises ``NotImplementedError``."""

    def __init__(self, input_dim: int, emotion_dims: int = 3, hidden_dim: int = 256, dropout: float = 0.3,
                 compute_dtype: str = "fp32", seed: int = 0):
        super().__init__()
        ops._act_dtype(compute_dtype)
        _refuse(input_dim <= 0 or input_dim % 4 != 0, f"input_dim = {input_dim}: must be a positive multiple of 4 (16-byte fp32 rows)")
        _refuse(hidden_dim <= 0 or hidden_dim % 32 != 0 or hidden_dim > 2048,
                f"hidden_dim = {hidden_dim}: must be a multiple of 32, at most 2048 (the tail reads hidden_dim // 4 <= 512 columns in 16-byte pieces)")
        _refuse(not 1 <= emotion_dims <= 3, f"emotion_dims = {emotion_dims}: must be in [1, 3] (there are three dimension names)")
        self.input_dim, self.emotion_dims, self.hidden_dim = input_dim, emotion_dims, hidden_dim
        self.compute_dtype = compute_dtype
        self.feature_processor = nn.Sequential(
            nn.Linear(input_dim, hidden_dim), nn.ReLU(), nn.Dropout(dropout),
            nn.Linear(hidden_dim, hidden_dim), nn.ReLU(), nn.Dropout(dropout))
        gen = torch.Generator().manual_seed(seed)
        for m in self.feature_processor:                  # nn.Linear.reset_parameters: both uniform in +-1 / sqrt(fan_in)
            if isinstance(m, nn.Linear):
                with torch.no_grad():
                    bound = 1.0 / m.in_features ** 0.5
                    m.weight.uniform_(-bound, bound, generator=gen)
                    m.bias.uniform_(-bound, bound, generator=gen)
        self.deer_heads = nn.ModuleList([
            DEERLayer(hidden_dim, output_dim=1, hidden_dim=hidden_dim // 2, dropout=dropout, compute_dtype=compute_dtype,
                      seed=seed + 1 + i) for i in range(emotion_dims)])
        self.dimension_names = list(DIM_NAMES[:emotion_dims])
        self.dropout = float(dropout)
        self._drop = fusions._Drop(seed)

    def forward(self, x: torch.Tensor) -> Dict[str, torch.Tensor]:
        _check_input(x, self.input_dim)
        D, names = self.emotion_dims, self.dimension_names
        if x.shape[0] == 0:
            out = {f"{n}_{k}": torch.zeros(0, 1, device=x.device) for n in names for k in NIG_KEYS}
            out["mu_all"], out["uncertainty_all"] = torch.zeros(0, D, device=x.device), torch.zeros(0, D, device=x.device)
            return out
        fp, cd = self.feature_processor, self.compute_dtype
        nets = [h.evidence_net for h in self.deer_heads]
        drop = self._drop.next(self, self.dropout)
        f = fusions.linear(x, fp[0], cd, relu=True, drop=drop, site=_SITE_FP0)
        f = fusions.linear(f, fp[3], cd, relu=True, drop=drop, site=_SITE_FP1)
        w0, b0 = torch.cat([n[0].weight for n in nets], dim=0), torch.cat([n[0].bias for n in nets])
        e1 = fusions._LinearFn.apply(f, w0, b0, cd, True, drop, _SITE_H0)               # (B, D hidden / 2)
        l1 = [q for n in nets for q in (n[3].weight, n[3].bias)]
        e2 = _HeadsLayer1Fn.apply(e1, cd, drop, _SITE_H1, *l1)                           # (B, D hidden / 4)
        w2, b2 = torch.stack([n[6].weight for n in nets]), torch.stack([n[6].bias for n in nets])
        outs = _TailFn.apply(e2, w2, b2, cd)
        predictions: Dict[str, torch.Tensor] = {}
        for d, n in enumerate(names):                    # deer.py:250-255
            for k, v in zip(NIG_KEYS, outs):
                predictions[f"{n}_{k}"] = v[:, d:d + 1]
        predictions["mu_all"], predictions["uncertainty_all"] = outs[0], outs[6]
        return predictions


class ComposedDEER(nn.Module):
    """A fusion module and a head as one model: ``forward(audio, video, text)`` (or one dictionary with those keys) =
    ``head(fusion(audio, video, text)['fused_features'])`` plus the aggregate keys ``MultimodalDEER`` returns (``gamma``, ``nu``,
    ``alpha``, ``beta`` (B, D), ``mu``, ``predictions``, ``uncertainties``, ``total_uncertainty``) and the fusion's extras.  The
    way to a trainable model at another geometry, e.g. ``ComposedDEER(HierarchicalMultimodalFusion(40, 128, 300),
    MultiDimensionalDEER(512))``.  ``compute_loss`` is ``losses.MultiTaskDEERLoss`` unless ``loss`` is given; there is no flat
    gradient buffer, so ``DEERTrainer`` trains it through autograd + ``torch.optim.AdamW``, or with
    ``TrainingConfig(module_optimizer=True)`` + ``optim.ModuleAdamW`` (clip + AdamW as one device-side step)."""

    def __init__(self, fusion: nn.Module, head: MultiDimensionalDEER, loss: Optional[nn.Module] = None):
        super().__init__()
        self.fusion, self.head = fusion, head
        if loss is None:
            from .losses import MultiTaskDEERLoss
            loss = MultiTaskDEERLoss()
        self.loss = loss

    def forward(self, audio_features, video_features=None, text_features=None) -> Dict[str, torch.Tensor]:
        if isinstance(audio_features, dict):
            d = audio_features
            audio_features = d.get("audio", d.get("audio_features"))
            video_features = d.get("video", d.get("video_features"))
            text_features = d.get("text", d.get("text_features"))
        if audio_features is None or video_features is None or text_features is None:
            raise ValueError("audio, video and text features are all required")
        fused = self.fusion(audio_features, video_features, text_features)
        out = dict(self.head(fused["fused_features"]))
        names = self.head.dimension_names
        cat = lambda k: torch.cat([out[f"{n}_{k}"] for n in names], dim=1)              # noqa: E731
        out["gamma"], out["nu"], out["alpha"], out["beta"] = out["mu_all"], cat("nu"), cat("alpha"), cat("beta")
        out["mu"] = out["predictions"] = out["mu_all"]
        out["uncertainties"] = out["total_uncertainty"] = out["uncertainty_all"]
        out["aleatoric_uncertainty"], out["epistemic_uncertainty"] = cat("aleatoric_uncertainty"), cat("epistemic_uncertainty")
        for k, v in fused.items():
            out.setdefault(k, v)
        return out

    def compute_loss(self, predictions: Dict[str, torch.Tensor], targets: torch.Tensor) -> Dict[str, torch.Tensor]:
        return self.loss(predictions, targets)

    def get_predictions_and_uncertainties(self, outputs: Dict[str, torch.Tensor]):
        return outputs["mu_all"], outputs.get("calibrated_uncertainty", outputs["uncertainty_all"])
