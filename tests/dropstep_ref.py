"""The dropout training step of the encoders, the stand-alone DEER heads and the fusion modules on the operator path, stated once
for tests/test_cpu_dropstep_ref.py and tests/test_gpu_dropstep.py.  TEST INFRASTRUCTURE, not a test module.

One ``Adapter`` per module family (audio, text by ids, text by embeddings, video, DEERLayer, MultiDimensionalDEER, and the fusions:
model.HierarchicalMultimodalFusion at a non-default geometry, fusions.AdaptiveFusionGating, fusions.ConcatFusion): its cases, the
closed-form parameters and inputs of a case, the dropout sites a training forward draws (the ``sites`` helpers of the *_ref.py
modules), the float64 reference of the step on given masks, and which mask sits behind each ReLU of that reference.  ``ref_step``
runs the reference step -- loss = sum_k (output_k * w_k) with closed-form weights w over the outputs the module differentiates --
and returns outputs, parameter gradients and input gradients; the masks are always drawn on the CPU (temporal_ref.draw), never by
the library.

A site record is (name, site, rows, cols, p) or (name, site, rows, cols, p, seed offset): the draw is made under DROP_SEED + the
offset (temporal_ref.seed_offset: 0 where the record has five entries).  ``drawn`` lists what a record draws at, the pair
(seed offset, site).  ``zero_grads`` / ``noise_grads`` / ``bf16_exempt`` name whole parameters, or rows of one as "name[lo:hi]"
(``rows_of``).

Case = (geometry..., p).  INPUT_SEED holds the input seed of every case: the first seed (from 0) for which no ReLU input of the
float64 reference that reaches a gradient (a unit its dropout keeps) lies within stackb_ref.RELU_BAND of zero, see
tests/test_cpu_dropstep_ref.py::test_no_relu_input_of_a_case_lies_in_the_band."""
from __future__ import annotations

import contextlib
import functools
import json
import os

import numpy as np
import torch

from mmdeer import synth

from . import fusion_ref, head_ref, temporal_ref, text_ref, video_ref

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
DROP_SEED, STEP = 11, 5            # the modules' dropout_seed and the step counter the tests set
F64 = torch.float64

# ---- the bounds of test A (the modules' own fp32 bounds of their golden tests)
OUT_RTOL, OUT_ATOL = 1e-3, 2e-5
G_RTOL, G_ATOL_FRAC = 3e-3, 3e-3
BUF_RTOL, BUF_ATOL = 1e-5, 1.2e-7


def out_fraction(got, ref):
    """largest |got - ref| / (atol + rtol |ref|): <= 1 is numpy's assert_allclose(rtol=OUT_RTOL, atol=OUT_ATOL)"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float(((got - ref).abs() / (OUT_ATOL + OUT_RTOL * ref.abs())).max())


def grad_fraction(got, ref):
    """largest |got - ref| / (atol_frac max|ref| + rtol |ref|): <= 1 is check_side_grads(rtol=G_RTOL, atol_frac=G_ATOL_FRAC)"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float(((got - ref).abs() / (G_ATOL_FRAC * ref.abs().max() + G_RTOL * ref.abs())).max())


def buffer_fraction(got, ref):
    """largest |got - ref| / (atol + rtol |ref|) of a running buffer: <= 1 is assert_allclose(rtol=BUF_RTOL, atol=BUF_ATOL)"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float(((got - ref).abs() / (BUF_ATOL + BUF_RTOL * ref.abs())).max())


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-300))


@contextlib.contextmanager
def relu_inputs():
    """Every tensor the references hand to ``torch.relu`` inside the block, in call order."""
    seen, orig = [], torch.relu

    def spy(z):
        seen.append(z.detach())
        return orig(z)
    torch.relu = spy
    try:
        yield seen
    finally:
        torch.relu = orig


def _normal(stream, *shape):
    return synth.normal(stream, int(np.prod(shape))).reshape(shape).astype(np.float32)


def _params(sd):
    """state (numpy) -> float64 leaves; the BatchNorm buffers take no gradient"""
    out = {}
    for k, v in sd.items():
        buf = "running_" in k or k.endswith("num_batches_tracked")
        t = torch.from_numpy(np.asarray(v, dtype=np.int64 if k.endswith("num_batches_tracked") else None)).to(F64)
        out[k] = t if buf else t.requires_grad_(True)
    return out


# the closed-form parameter fills (synth.module_fill, as the modules' golden tests use them), one per family
@functools.lru_cache(None)
def _audio_state():
    from mmdeer import temporal
    return synth.module_fill("dropaudio", {k: tuple(v.shape) for k, v in temporal.TemporalAudioEncoder().state_dict().items()})


@functools.lru_cache(None)
def _text_state():
    with open(os.path.join(GOLDEN, "text_state_dict_names.json")) as fh:
        return synth.module_fill("droptext", {k: tuple(s) for k, s in json.load(fh).items()})


@functools.lru_cache(None)
def _video_state():
    with open(os.path.join(GOLDEN, "video_state_dict_names.json")) as fh:
        shapes = {k: tuple(s) for k, s in json.load(fh)}
    return {k: v for k, v in video_ref.filled_state("dropvideo", shapes).items() if not k.startswith("spatial_backbone.")}


@functools.lru_cache(None)
def _head_state(tag):
    with open(os.path.join(GOLDEN, "deer_head_state_dict_names.json")) as fh:
        return synth.module_fill(tag, {k: tuple(v) for k, v in json.load(fh)[tag].items()})


def rows_of(entries) -> dict:
    """("name", "other[lo:hi]", ...) -> {parameter: [row slices]}; a bare name is the whole parameter, slice(None)"""
    out = {}
    for e in entries:
        name, _, rng = e.partition("[")
        lo, hi = (int(v) for v in rng.rstrip("]").split(":")) if rng else (None, None)
        out.setdefault(name, []).append(slice(lo, hi))
    return out


def without_rows(t, slices):
    """a copy of ``t`` with the rows of ``slices`` set to zero"""
    t = t.detach().clone()
    for sl in slices:
        t[sl] = 0
    return t


def drawn(record) -> tuple:
    """what a site record draws at: (seed offset, site)"""
    return (temporal_ref.seed_offset(record), record[1])


class Adapter:
    name = ""
    cases: list = []
    diff_inputs: tuple = ()            # the inputs whose gradient is compared
    loss_outputs = None                # the outputs the loss weighs (None: all); the others are values the module does not differentiate
    zero_grads: tuple = ()             # parameters whose gradient is written as an exact zero
    noise_grads: tuple = ()            # parameters whose gradient is analytically zero and rounding noise on both sides
    bf16_exempt: tuple = ()            # what the modules' own bf16 tests leave out, for the analytic reason they state

    def case_id(self, case):
        return "-".join(str(c) for c in case)

    def seed(self, case):
        return INPUT_SEED[self.name][self.case_id(case)]

    # state(case) -> {name: numpy}; inputs(case, seed) -> {name: numpy}; sites(case) -> [(name, site, rows, cols, p[, seed offset])]
    # ref(P, X, masks, emulate) -> ({output name: tensor}, {buffer name: tensor}); relu_masks(case) -> [mask name or None] per ReLU call

    def masks(self, case, step=STEP, sites=None):
        return temporal_ref.draw(self.sites(case) if sites is None else sites, DROP_SEED, step)

    def weights(self, case, outs):
        return {k: torch.from_numpy(_normal(4200 + i, *v.shape)).to(F64) for i, (k, v) in enumerate(outs.items())
                if self.loss_outputs is None or k in self.loss_outputs}


def ref_step(ad: Adapter, case, masks, emulate=False, seed=None, state=None):
    """The float64 (or bf16-emulating) training step of ``case`` on ``masks`` (None: the evaluation forward) ->
    dict(out={name: tensor}, grads={parameter: gradient or None}, dx={input: gradient}, buffers={...}, relu=[ReLU inputs])."""
    P = _params(ad.state(case) if state is None else state)
    X = {k: torch.from_numpy(v) for k, v in ad.inputs(case, ad.seed(case) if seed is None else seed).items()}
    X = {k: v.to(F64).requires_grad_(True) if k in ad.diff_inputs else v for k, v in X.items()}
    with relu_inputs() as seen:
        outs, buffers = ad.ref(P, X, masks, emulate)
    W = ad.weights(case, outs)
    sum((outs[k] * W[k]).sum() for k in W).backward()
    return dict(out={k: v.detach() for k, v in outs.items()}, grads={k: v.grad for k, v in P.items() if v.requires_grad},
                dx={k: X[k].grad for k in ad.diff_inputs}, buffers=buffers, relu=seen)


def band_count(ad: Adapter, case, seed, band):
    """How many ReLU inputs of the float64 step that reach a gradient (units the dropout behind the ReLU keeps) lie within
    band * max|input| of zero."""
    masks = ad.masks(case)
    r = ref_step(ad, case, masks, seed=seed)
    names = ad.relu_masks(case)
    assert len(names) == len(r["relu"]), (ad.name, len(names), len(r["relu"]))
    n = 0
    for z, name in zip(r["relu"], names):
        near = z.abs() <= band * float(z.abs().max())
        if name is not None:
            near &= (name(masks) if callable(name) else masks[name]).reshape(z.shape) > 0
        n += int(near.sum())
    return n


# ------------------------------------------------------------------------------------------------------------------- audio
class Audio(Adapter):
    name = "audio"
    cases = [(5, 3, 0.3), (37, 3, 0.3), (5, 1, 0.3), (5, 3, 0.5)]          # (B, T, p); 37 x 3 = 111 rows cross a 64-row tile raggedly
    diff_inputs = ("x",)
    zero_grads = ("attention.2.bias",)
    bf16_exempt = ("attention.0.bias", "attention.2.bias")      # tests/test_gpu_temporal_audio.py: a sum of cancelling terms; an exact zero

    def state(self, case):
        return _audio_state()

    def inputs(self, case, seed):
        B, T, _ = case
        return {"x": _normal(5000 + seed, B, T, 84)}

    def sites(self, case):
        B, T, p = case
        return temporal_ref.sites(B, T, p)

    def ref(self, P, X, masks, emulate=False):
        return {"out": temporal_ref.encoder(P, X["x"], masks=masks, emulate_bf16=emulate)[0]}, {}

    def relu_masks(self, case):
        return ["op"]

    def module(self, case, compute, p=None):
        from mmdeer import temporal
        m = temporal.TemporalAudioEncoder({"dropout": case[2] if p is None else p, "dropout_seed": DROP_SEED}, compute_dtype=compute)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in self.state(case).items()}, strict=True)
        return m

    def forward(self, m, X):
        return {"out": m(X["x"])}


# -------------------------------------------------------------------------------------------------------------------- text
class TextEmb(Adapter):
    name = "text_embeddings"
    cases = [(5, 7, 0.3), (37, 9, 0.3), (5, 7, 0.5)]                       # (B, L, p)
    diff_inputs = ("E",)
    zero_grads = ("token_attention.2.bias",)
    bf16_exempt = ("token_attention.0.bias", "token_attention.2.bias")     # tests/test_gpu_text_encoder.py, the same two reasons
    by_ids = False

    def state(self, case):
        return _text_state()

    def inputs(self, case, seed):
        """ids over the whole vocabulary (some in the punctuation / special ranges of the statistics), and a ragged mask: sample
        b has 1 + (3 b) % L leading positions, odd samples with a hole at position 1."""
        B, L, _ = case
        u = synth.uniform01(6000 + seed, B * L).reshape(B, L)
        ids = np.where(u < 0.25, 100 + (u * 4 * 930), 1 + u * 29998).astype(np.int64)
        mask = (np.arange(L)[None, :] < (1 + (3 * np.arange(B)) % L)[:, None]).astype(np.int64)
        mask[1::2, 1] = 0
        X = {"ids": ids, "mask": mask}
        if not self.by_ids:
            X["E"] = _normal(6100 + seed, B, L, 768)
        return X

    def sites(self, case):
        return text_ref.sites(case[0], 512, case[2])

    def ref(self, P, X, masks, emulate=False):
        if self.by_ids:
            return {"out": text_ref.encoder(P, X["ids"], X["mask"], emulate_bf16=emulate, masks=masks)[0]}, {}
        return {"out": text_ref.encoder_embeddings(P, X["E"], X["ids"], X["mask"], emulate_bf16=emulate, masks=masks)[0]}, {}

    def relu_masks(self, case):
        return ["bert", "ling", "out"]

    def module(self, case, compute, p=None):
        from mmdeer import text
        m = text.TemporalTextEncoder({"dropout": case[2] if p is None else p, "dropout_seed": DROP_SEED}, compute_dtype=compute)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in self.state(case).items()}, strict=True)
        return m

    def forward(self, m, X):
        return {"out": m(X["ids"], X["mask"]) if self.by_ids else m.forward_embeddings(X["E"], X["ids"], X["mask"])}


class TextIds(TextEmb):
    name = "text_ids"
    diff_inputs = ()
    by_ids = True


# ------------------------------------------------------------------------------------------------------------------- video
class Video(Adapter):
    name = "video"
    cases = [(5, 3, 0.3), (37, 3, 0.3), (5, 1, 0.3), (5, 3, 0.5)]          # (B, T, p)
    diff_inputs = ("x",)
    zero_grads = ("temporal_attention.2.bias",)                            # tests/test_gpu_video_encoder.py: ZERO_BIAS
    noise_grads = ("temporal_cnn.0.bias", "temporal_cnn.4.bias")           # ... NOISE_BIASES: a bias in front of batch statistics
    bf16_exempt = zero_grads + noise_grads

    def state(self, case):
        return _video_state()

    def inputs(self, case, seed):
        B, T, _ = case
        return {"x": _normal(7000 + seed, B, T, 512)}

    def sites(self, case):
        B, T, p = case
        return video_ref.sites(B, T, p)

    def ref(self, P, X, masks, emulate=False):
        y, buffers = video_ref.encoder(P, X["x"], masks is not None, masks=masks or None, emulate_bf16=emulate)     # {}: training, p = 0
        return {"out": y}, buffers

    def relu_masks(self, case):
        return ["sp", "cnn", None, "op"] if case[1] > 1 else ["sp", "op"]

    def module(self, case, compute, p=None):
        from mmdeer import video
        m = video.TemporalVideoEncoder({"dropout": case[2] if p is None else p, "dropout_seed": DROP_SEED}, compute_dtype=compute)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in self.state(case).items()}, strict=False)
        return m

    def forward(self, m, X):
        return {"out": m(X["x"])}


# -------------------------------------------------------------------------------------------------------------------- head
class Layer(Adapter):
    name = "deer_layer"
    tag = "dl96x3x64"
    cases = [("dl96x3x64", 5, 0.3), ("dl96x3x64", 70, 0.3), ("dl96x3x64", 5, 0.5)]     # (tag, B, p)
    diff_inputs = ("x",)

    def state(self, case):
        return _head_state(case[0])

    def geometry(self, case):
        return (head_ref.DL_CASES if case[0] in head_ref.DL_CASES else head_ref.MD_CASES)[case[0]][:3]

    def inputs(self, case, seed):
        return {"x": _normal(8000 + seed, case[1], self.geometry(case)[0])}

    def sites(self, case):
        return head_ref.sites_layer(case[1], self.geometry(case)[2], case[2])

    def ref(self, P, X, masks, emulate=False):
        return head_ref.deer_layer(P, X["x"], rnd=head_ref.bf16 if emulate else None, masks=masks), {}

    def relu_masks(self, case):
        return ["ev0", "ev1"]

    def module(self, case, compute, p=None):
        from mmdeer import head
        I, O_, Hd = self.geometry(case)
        m = head.DEERLayer(I, output_dim=O_, hidden_dim=Hd, dropout=case[2] if p is None else p, compute_dtype=compute, seed=DROP_SEED)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in self.state(case).items()}, strict=True)
        return m

    def forward(self, m, X):
        return m(X["x"])


class Multi(Layer):
    name = "multi_dim"
    cases = [("md192x3x128", 5, 0.3), ("md192x3x128", 70, 0.3), ("md192x3x128", 5, 0.5)]

    def sites(self, case):
        _, D, Hd = self.geometry(case)
        return head_ref.sites_multi(case[1], Hd, D, case[2])

    def ref(self, P, X, masks, emulate=False):
        D = len({k.split(".")[1] for k in P if k.startswith("deer_heads.")})
        return head_ref.multi_dim(P, X["x"], D, rnd=head_ref.bf16 if emulate else None, masks=masks), {}

    def relu_masks(self, case, geometry=None):
        _, D, Hd = geometry or self.geometry(case)
        w = Hd // 2
        out = ["fp0", "fp1"]
        for d in range(D):
            out += [lambda m, d=d: m["h0"][:, d * w:(d + 1) * w], f"h1.{d}"]
        return out

    def module(self, case, compute, p=None):
        from mmdeer import head
        I, D, Hd = self.geometry(case)
        m = head.MultiDimensionalDEER(I, emotion_dims=D, hidden_dim=Hd, dropout=case[2] if p is None else p, compute_dtype=compute, seed=DROP_SEED)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in self.state(case).items()}, strict=True)
        return m


# ------------------------------------------------------------------------------------------------------------------ fusions
@functools.lru_cache(None)
def _fusion_state(dims):
    from mmdeer.model import HierarchicalMultimodalFusion
    return synth.module_fill("dropfusion", {k: tuple(v.shape) for k, v in HierarchicalMultimodalFusion(*dims).state_dict().items()})


@functools.lru_cache(None)
def _adaptive_state():
    from mmdeer import fusions
    m = fusions.AdaptiveFusionGating(list(synth.FUSION_ALT_DIMS), list(Adaptive.strategies), Adaptive.hidden)
    return synth.module_fill("dropadaptive", {k: tuple(v.shape) for k, v in m.state_dict().items()})


@functools.lru_cache(None)
def _concat_state():
    from mmdeer import fusions
    m = fusions.ConcatFusion(sum(synth.FUSION_ALT_DIMS), Concat.width)
    return synth.module_fill("dropconcat", {k: tuple(v.shape) for k, v in m.state_dict().items()})


def _load_strict(m, state):
    m.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    return m


class Fusion(Adapter):
    """model.HierarchicalMultimodalFusion on the operator path (generic_fusion.GenericHierarchicalFusion behind the wrapper)."""
    name = "fusion"
    # (audio_dim, video_dim, text_dim, B, p): B = 1 -- the stacked AV GEMM has two rows, every dW a one-row reduction; B = 37 -- ragged
    # against every row tile, 2B = 74; a second probability; the geometry of the end-to-end step
    cases = [(40, 128, 300, 1, 0.3), (40, 128, 300, 37, 0.3), (40, 128, 300, 5, 0.1), (512, 512, 512, 5, 0.5)]
    diff_inputs = ("audio", "video", "text")
    loss_outputs = ("fused_features", "audiovisual_features", "trimodal_features")
    _E, _F = fusion_ref.E, fusion_ref.F
    # one key per query: the softmax is 1 whatever q and k are, their rows are written as exact zeros
    zero_grads = (f"audio_visual_fusion.cross_attention.in_proj_weight[0:{2 * _E}]", f"audio_visual_fusion.cross_attention.in_proj_bias[0:{2 * _E}]")
    # a key bias shifts both scores of a query alike, and the softmax does not see a common shift
    noise_grads = (f"trimodal_fusion.modality_attention.in_proj_bias[{_F}:{2 * _F}]",)
    bf16_exempt = noise_grads          # a sum of cancelling terms: rounding noise on every side

    def state(self, case):
        return _fusion_state(tuple(case[:3]))

    def inputs(self, case, seed):
        B = case[3]
        return {k: _normal(9000 + 3 * seed + i, B, d) for i, (k, d) in enumerate(zip(self.diff_inputs, case[:3]))}

    def sites(self, case):
        return fusion_ref.sites_fusion(case[3], case[4])

    def ref(self, P, X, masks, emulate=False):
        return (fusion_ref.fusion_bf16 if emulate else fusion_ref.fusion)(P, X["audio"], X["video"], X["text"], masks), {}

    def relu_masks(self, case):
        return ["av_fuse", "tri_fuse", "out_proj"]

    def module(self, case, compute, p=None):
        from mmdeer.model import HierarchicalMultimodalFusion
        m = HierarchicalMultimodalFusion(*case[:3], dropout=case[4] if p is None else p, compute_dtype=compute, seed=DROP_SEED)
        return _load_strict(m, self.state(case))

    def forward(self, m, X):
        o = m(X["audio"], X["video"], X["text"])
        assert o["uncertainty_weights"] is None
        out = {k: o[k] for k in fusion_ref.FUSION_OUTS[:4]}
        out.update({f"av_attention_{k}": o["av_attention_weights"][k] for k in ("audio_to_video", "video_to_audio")})
        return out


class Adaptive(Adapter):
    """fusions.AdaptiveFusionGating over 'attention' and 'bilinear': its feature encoder's nn.Dropout(0.3) is the one site, and it
    reaches the loss only through the strategy weights."""
    name = "adaptive"
    strategies, hidden = ("attention", "bilinear"), 256
    cases = [(1, 0.3), (37, 0.3)]                                              # (B, the fixed p of the encoder's nn.Dropout)
    diff_inputs = ("x0", "x1", "x2")
    loss_outputs = ("fused_features",)
    # the softmax over the modalities does not see a common shift of its scores (tests/test_gpu_fusions.py treats it the same way)
    noise_grads = ("fusion_modules.attention.attention.bias",)
    bf16_exempt = noise_grads

    def state(self, case):
        return _adaptive_state()

    def inputs(self, case, seed):
        return {k: _normal(9300 + 3 * seed + i, case[0], d) for i, (k, d) in enumerate(zip(self.diff_inputs, synth.FUSION_ALT_DIMS))}

    def sites(self, case):
        return fusion_ref.sites_adaptive(case[0], case[1], self.hidden)

    def ref(self, P, X, masks, emulate=False):
        feats = [X[k] for k in self.diff_inputs]
        return (fusion_ref.adaptive_bf16 if emulate else fusion_ref.adaptive)(P, feats, self.strategies, masks), {}

    def relu_masks(self, case):
        return ["enc", None]

    def module(self, case, compute, p=None):
        from mmdeer import fusions
        m = fusions.AdaptiveFusionGating(list(synth.FUSION_ALT_DIMS), list(self.strategies), self.hidden, compute_dtype=compute, dropout_seed=DROP_SEED)
        assert m.feature_encoder[2].p == case[1]
        if p is not None:
            m.feature_encoder[2].p = p
        return _load_strict(m, self.state(case))

    def forward(self, m, X):
        return dict(m(*[X[k] for k in self.diff_inputs]))


class Concat(Adapter):
    """fusions.ConcatFusion, the Linear-ReLU-Dropout-LayerNorm block on its own."""
    name = "concat"
    width = 512
    cases = [(1, 0.3), (37, 0.3), (5, 0.5)]                                    # (B, p)
    diff_inputs = ("x",)

    def state(self, case):
        return _concat_state()

    def inputs(self, case, seed):
        return {"x": _normal(9600 + seed, case[0], sum(synth.FUSION_ALT_DIMS))}

    def sites(self, case):
        return fusion_ref.sites_concat(case[0], case[1], self.width)

    def ref(self, P, X, masks, emulate=False):
        return (fusion_ref.concat_bf16 if emulate else fusion_ref.concat)(P, X["x"], masks), {}

    def relu_masks(self, case):
        return ["concat"]

    def module(self, case, compute, p=None):
        from mmdeer import fusions
        m = fusions.ConcatFusion(sum(synth.FUSION_ALT_DIMS), self.width, case[1] if p is None else p, compute_dtype=compute, dropout_seed=DROP_SEED)
        return _load_strict(m, self.state(case))

    def forward(self, m, X):
        return {"out": m(X["x"])}


ADAPTERS = {a.name: a for a in (Audio(), TextEmb(), TextIds(), Video(), Layer(), Multi(), Fusion(), Adaptive(), Concat())}
ALL_CASES = [(a.name, c) for a in ADAPTERS.values() for c in a.cases]
CASE_IDS = [f"{n}-{ADAPTERS[n].case_id(c)}" for n, c in ALL_CASES]

# chosen by tests/test_cpu_dropstep_ref.py's search (band_count == 0 at the first such seed from 0); asserted there
INPUT_SEED = {
    "audio": {"5-3-0.3": 0, "37-3-0.3": 0, "5-1-0.3": 0, "5-3-0.5": 0},
    "text_embeddings": {"5-7-0.3": 0, "37-9-0.3": 1, "5-7-0.5": 0},
    "text_ids": {"5-7-0.3": 0, "37-9-0.3": 0, "5-7-0.5": 0},
    "video": {"5-3-0.3": 1, "37-3-0.3": 35, "5-1-0.3": 1, "5-3-0.5": 0},       # 37 x 3: 150 k units that reach a gradient; seeds 0 .. 34 have 3 .. 11 in the band
    "deer_layer": {"dl96x3x64-5-0.3": 0, "dl96x3x64-70-0.3": 1, "dl96x3x64-5-0.5": 0},
    "multi_dim": {"md192x3x128-5-0.3": 0, "md192x3x128-70-0.3": 0, "md192x3x128-5-0.5": 0},
    "fusion": {"40-128-300-1-0.3": 0, "40-128-300-37-0.3": 8, "40-128-300-5-0.1": 1, "512-512-512-5-0.5": 0},   # B = 37: 47 k units, 1 .. 3 in the band at seeds 0 .. 7
    "adaptive": {"1-0.3": 0, "37-0.3": 0},
    "concat": {"1-0.3": 0, "37-0.3": 0, "5-0.5": 0},
}


# --------------------------------------------------------------------------------------------------------------------- the seam
# head.ComposedDEER(HierarchicalMultimodalFusion(40, 128, 300), MultiDimensionalDEER(512)) with both modules' dropout live: the one
# place where a fusion gradient arrives through a head's backward and not from a test's cotangent.  Both modules draw under DROP_SEED
# (their sites are disjoint), each at its own step.
SEAM_CASE = (40, 128, 300, 5, 0.3)
SEAM_HEAD = (512, 3, 256)                                  # MultiDimensionalDEER(512): input_dim, emotion_dims, hidden_dim
SEAM_STEPS = (STEP, STEP + 3)                              # the fusion's step, the head's step
SEAM_INPUT_SEED = 1                                        # the first seed with no kept ReLU input of fusion or head in the band (asserted on the CPU)


@functools.lru_cache(None)
def _seam_head_state():
    from mmdeer import head
    I, Dm, Hd = SEAM_HEAD
    sd = head.MultiDimensionalDEER(I, emotion_dims=Dm, hidden_dim=Hd).state_dict()
    return synth.module_fill("dropseam", {k: tuple(v.shape) for k, v in sd.items()})


def seam_masks(steps=SEAM_STEPS):
    fu = ADAPTERS["fusion"]
    return fu.masks(SEAM_CASE, step=steps[0]), temporal_ref.draw(head_ref.sites_multi(SEAM_CASE[3], SEAM_HEAD[2], SEAM_HEAD[1], SEAM_CASE[4]), DROP_SEED, steps[1])


def seam_weights(outs):
    return {k: torch.from_numpy(_normal(4600 + i, *v.shape)).to(F64) for i, (k, v) in enumerate(outs.items())}


def seam_ref(seed=SEAM_INPUT_SEED, steps=SEAM_STEPS):
    """fusion_forward followed by the multi_dim reference, float64, each on its own masks -> dict(out = the head's outputs,
    grads = the FUSION parameters' gradients, head_grads, dx, relu = [(ReLU input, its mask)])."""
    fu = ADAPTERS["fusion"]
    fm, hm = seam_masks(steps)
    P, H = _params(fu.state(SEAM_CASE)), _params(_seam_head_state())
    X = {k: torch.from_numpy(v).to(F64).requires_grad_(True) for k, v in fu.inputs(SEAM_CASE, seed).items()}
    with relu_inputs() as seen:
        fused = fusion_ref.fusion(P, X["audio"], X["video"], X["text"], fm)["fused_features"]
        outs = head_ref.multi_dim(H, fused, SEAM_HEAD[1], masks=hm)
    W = seam_weights(outs)
    sum((outs[k] * W[k]).sum() for k in outs).backward()
    names = fu.relu_masks(SEAM_CASE) + ADAPTERS["multi_dim"].relu_masks(("seam", SEAM_CASE[3], SEAM_CASE[4]), geometry=SEAM_HEAD)
    both = dict(fm, **hm)
    assert len(names) == len(seen)
    relu = [(z, (n(both) if callable(n) else both[n]).reshape(z.shape)) for z, n in zip(seen, names)]
    return dict(out={k: v.detach() for k, v in outs.items()}, grads={k: v.grad for k, v in P.items()},
                head_grads={k: v.grad for k, v in H.items()}, dx={k: v.grad for k, v in X.items()}, relu=relu)
