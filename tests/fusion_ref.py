"""The training step of the fusion modules on the operator path -- model.HierarchicalMultimodalFusion at a non-default geometry
(mmdeer/generic_fusion.py), fusions.AdaptiveFusionGating and fusions.ConcatFusion -- for tests/dropstep_ref.py: the dropout sites
a training forward draws, the float64 reference (oracle.deer_oracle, on given masks) and its bf16-emulating form.  A helper module,
not a test module.

``masks``: float64 keep * scale per site (temporal_ref.draw), None = evaluation mode.  The oracle multiplies by mask / (1 - p), so
it is called with p = 0: the scale the library applies (float32(1 / (1 - float32(p)))) is the one inside the mask.

The bf16 forms are the float64 computation with a rounding to bf16 wherever the modules store bf16 (generic_fusion.py, fusions.py):
every autograd Function stores its output, its saved activations and its weight matrices in the compute dtype and returns
``.float()``; an incoming gradient is converted to the compute dtype first; every dX / dz is stored in the compute dtype; ``probs``,
the softmax weights, LayerNorm statistics, biases, LayerNorm vectors and all weight / bias gradients stay fp32 (here: float64)."""
from __future__ import annotations

import math

import torch

from oracle import deer_oracle as O

from .temporal_ref import _Round, _RoundGrad, linear

E, F, HEADS = 256, 512, 8          # intermediate_dim, fusion_dim, heads: the sizes the operator path is built for
FUSION_OUTS = ("fused_features", "audiovisual_features", "trimodal_features", "trimodal_attention_weights",
               "av_attention_audio_to_video", "av_attention_video_to_audio")


# ------------------------------------------------------------------------------------------------------------------- sites
def sites_fusion(B: int, p: float) -> list:
    """What one training forward of generic_fusion.GenericHierarchicalFusion draws, in launch order.  ``av``: ONE (2B, 8) draw, one
    decision per (row, head) of the stacked value projection (drop_shift = log2(E / heads) on its E columns), rows [0, B) key video
    (the audio query's call), rows [B, 2B) key audio.  ``tri_attn``: the trimodal attention draws inside its kernel at the library's
    own site (csrc/common.h SITE_TRI_ATTN), column 4 h + 2 t + u, under the module's seed + generic_fusion._TRI_SEED_OFFSET."""
    from mmdeer import generic_fusion as G

    from .rowkernel_ref import SITE_TRI_ATTN
    return [("av", G._SITE_AV, 2 * B, HEADS, p), ("av_fuse", G._SITE_AVF, B, E, p),
            ("tri_attn", SITE_TRI_ATTN, B, 4 * HEADS, p, G._TRI_SEED_OFFSET),
            ("tri_fuse", G._SITE_TRIF, B, F, p), ("out_proj", G._SITE_OUT, B, F, p)]


def sites_adaptive(B: int, p: float, hidden_dim: int = 256) -> list:
    from mmdeer import fusions
    return [("enc", fusions._SITE_ENC, B, hidden_dim, p)]


def sites_concat(B: int, p: float, fusion_dim: int = 512) -> list:
    from mmdeer import fusions
    return [("concat", fusions._SITE_CONCAT, B, fusion_dim, p)]


def oracle_masks(masks):
    """the masks of ``sites_fusion`` under the names oracle.fusion_forward reads"""
    if masks is None:
        return None
    B = masks["av"].shape[0] // 2
    return {"av_attn_a2v": masks["av"][:B], "av_attn_v2a": masks["av"][B:], "av_fuse": masks["av_fuse"],
            "tri_attn": masks["tri_attn"].reshape(B, HEADS, 2, 2), "tri_fuse": masks["tri_fuse"], "out_proj": masks["out_proj"]}


def _flat(o):
    return {"fused_features": o["fused_features"], "audiovisual_features": o["audiovisual_features"],
            "trimodal_features": o["trimodal_features"], "trimodal_attention_weights": o["trimodal_attention_weights"].detach(),
            "av_attention_audio_to_video": o["av_attention_weights"]["audio_to_video"].detach(),
            "av_attention_video_to_audio": o["av_attention_weights"]["video_to_audio"].detach()}


# -------------------------------------------------------------------------------------------------------------- float64 forms
def fusion(P, audio, video, text, masks=None):
    """HierarchicalMultimodalFusion; P under the module's state_dict names -> FUSION_OUTS (the reported weights detached: the module
    marks them non-differentiable)."""
    Pf = {"fusion." + k: v for k, v in P.items()}
    om = oracle_masks(masks)
    if masks is None or masks["av"].shape[1] == HEADS:
        return _flat(O.fusion_forward(Pf, audio, video, text, masks=om, p=0.0, heads=HEADS))
    # only the sensitivity test's per-column mistake comes here: an AV mask with one decision per column is the oracle's 1-key
    # attention with as many "heads" as columns; the rest is fusion_forward's own composition
    av = O.av_fusion(Pf, audio, video, om, 0.0, heads=masks["av"].shape[1])
    tri = O.trimodal_fusion(Pf, av["fused_features"], text, om, 0.0, HEADS)
    final, _ = O._relu_drop_ln(tri["fused_features"], Pf, "fusion.output_projection", om["out_proj"], 0.0)
    return _flat({"fused_features": final, "audiovisual_features": av["fused_features"], "trimodal_features": tri["fused_features"],
                  "av_attention_weights": av["attention_weights"], "trimodal_attention_weights": tri["attention_weights"]})


def adaptive(P, feats, strategies, masks=None):
    y, w = O.adaptive_fusion(P, feats, strategies, mask=None if masks is None else masks["enc"], p=0.0)
    return {"fused_features": y, "strategy_weights": w.detach()}


def concat(P, x, masks=None):
    return {"out": O.concat_fusion(P, x, mask=None if masks is None else masks["concat"], p=0.0)}


# ----------------------------------------------------------------------------------------------------------------- bf16 forms
def _rg(x):
    return _RoundGrad.apply(x)


def _r(x):
    return _Round.apply(x)


def _lin(x, P, name, relu=False, mask=None):
    """fusions._LinearFn (``fusions.linear``, generic_fusion._LinearRaw): temporal_ref.linear's bf16 form"""
    return linear(x, P[name + ".weight"], P[name + ".bias"], relu=relu, mask=mask, emulate_bf16=True)


def _block(x, P, prefix, mask):
    """fusions._LinActLnFn under the parameters ``prefix``{0,3}.*: y = bf16(drop(relu(bf16(x) bf16(W)^T + b))) is stored, the
    statistics are fp32 over it, the output is bf16; coming back the gradient is rounded on entry, dz = bf16(LayerNorm'(g) (y > 0)
    scale) feeds both GEMMs, dX is bf16."""
    pre = _rg(_rg(_r(x)) @ _r(P[prefix + "0.weight"]).t() + P[prefix + "0.bias"])
    y = torch.relu(pre)
    y = _r(y if mask is None else y * mask)
    return _rg(_r(O._layer_norm(y, P[prefix + "3.weight"], P[prefix + "3.bias"])))


def fusion_bf16(P, audio, video, text, masks=None):
    """GenericHierarchicalFusion.forward launch by launch, compute_dtype = 'bf16'."""
    m = masks or {}
    B = audio.shape[0]
    av = "audio_visual_fusion."
    ap, vp = _lin(audio, P, av + "audio_projection"), _lin(video, P, av + "video_projection")
    # _AVAttnFn on the stacked rows: v = bf16((x Wv^T + bv) * keep factor of (row, head)) and out = bf16(v Wo^T + bo) are stored;
    # backward: bf16(g); dv = bf16((g Wo) * factor) in ONE rounding (no rounding of g Wo on its own); d kv = bf16(dv Wv)
    kv = _rg(_r(torch.cat([vp, ap], dim=0)))
    w_in, b_in = P[av + "cross_attention.in_proj_weight"], P[av + "cross_attention.in_proj_bias"]
    pre = _rg(kv @ _r(w_in[2 * E:]).t() + b_in[2 * E:])
    wgt = torch.ones(2 * B, HEADS, dtype=pre.dtype) if masks is None else m["av"]
    v = _r((pre.view(2 * B, HEADS, E // HEADS) * wgt[:, :, None]).reshape(2 * B, E))
    att = _rg(_r(v @ _r(P[av + "cross_attention.out_proj.weight"]).t() + P[av + "cross_attention.out_proj.bias"]))
    avf = _block(torch.cat([att[:B], att[B:]], dim=1), P, av + "fusion_layers.", m.get("av_fuse"))
    tri = "trimodal_fusion."
    x0, x1 = _lin(avf, P, tri + "audiovisual_projection"), _lin(text, P, tri + "text_projection")
    xtok = torch.stack([x0, x1], dim=1).reshape(2 * B, F)
    qkv = linear(xtok, P[tri + "modality_attention.in_proj_weight"], P[tri + "modality_attention.in_proj_bias"], emulate_bf16=True)
    # _TriAttnFn: q, k, v are read from the stored bf16 rows, everything inside the kernel is fp32, probs stay fp32, the token-pooled
    # context is stored bf16; coming back bf16(g) in, bf16 dqkv out (the rounding of qkv's gradient above)
    hd = F // HEADS
    q, k, vv = (u.reshape(B, 2, HEADS, hd).transpose(1, 2) for u in qkv.split(F, dim=-1))
    prob = torch.softmax((q @ k.transpose(-1, -2)) * math.sqrt(1.0 / hd), dim=-1)
    probd = prob if masks is None else prob * m["tri_attn"].reshape(B, HEADS, 2, 2)
    obar = _rg(_r((probd @ vv).transpose(1, 2).reshape(B, 2, F).mean(dim=1)))
    pooled = _lin(obar, P, tri + "modality_attention.out_proj")
    trif = _block(pooled, P, tri + "final_fusion.", m.get("tri_fuse"))
    fused = _block(trif, P, "output_projection.", m.get("out_proj"))
    w = wgt.mean(dim=1, keepdim=True)
    return _flat({"fused_features": fused, "audiovisual_features": avf, "trimodal_features": trif,
                  "trimodal_attention_weights": probd.mean(dim=1), "av_attention_weights": {"audio_to_video": w[:B], "video_to_audio": w[B:]}})


def _mix(stacked, logits=None, w_att=None, b_att=None):
    """fusions._MixFn: the rows are read as bf16, the logits (given, or rows . w_att + b_att with the fp32 vector) and the softmax
    weights are fp32, the mixed row is stored bf16.  Coming back: bf16(g); dP is ONE rounding of w_s g + ds_s w_att with the fp32 ds;
    the logits' gradient is stored bf16 (dlogits8), and d w_att / d b_att are sums over THAT."""
    st = _rg(_r(stacked))
    if logits is None:
        toward_rows = st @ w_att.detach().t()
        s = _rg(st.detach() @ w_att.t() + b_att) + (toward_rows - toward_rows.detach())
        s = s.squeeze(-1)
    else:
        s = _rg(logits)
    w = torch.softmax(s, dim=-1)
    return _rg(_r((w.unsqueeze(-1) * st).sum(dim=1))), w


def adaptive_bf16(P, feats, strategies, masks=None):
    """AdaptiveFusionGating.forward with AttentionFusion / BilinearFusion inside, compute_dtype = 'bf16'."""
    cat = torch.cat(list(feats), dim=-1)
    h = _lin(cat, P, "feature_encoder.0", relu=True, mask=None if masks is None else masks["enc"])
    h = _lin(h, P, "feature_encoder.3", relu=True)
    logits = _lin(h, P, "strategy_selector.0")
    outs = []
    for name in strategies:
        pre = f"fusion_modules.{name}."
        if name == "attention":
            st = torch.stack([_lin(f, P, f"{pre}projections.{i}") for i, f in enumerate(feats)], dim=1)
            outs.append(_mix(st, w_att=P[pre + "attention.weight"], b_att=P[pre + "attention.bias"])[0])
        else:
            # _BilinearFn: bf16 inputs, the outer product z stored bf16, the weight bf16, the RESULT fp32; coming back bf16(g),
            # dz = bf16(g W) stored, dx1 / dx2 bf16.  The additional Linear is added to the fp32 result by torch.
            a1, a2 = _rg(_r(feats[0])), _rg(_r(feats[1]))
            Wb = P[pre + "bilinear.weight"]
            z = _rg(_r(a1[:, :, None] * a2[:, None, :])).reshape(a1.shape[0], -1)
            y = _rg(z @ _r(Wb).reshape(Wb.shape[0], -1).t() + P[pre + "bilinear.bias"])
            outs.append(y + _lin(torch.cat(list(feats[2:]), dim=-1), P, pre + "additional_linear"))
    y, w = _mix(torch.stack(outs, dim=1), logits=logits)
    return {"fused_features": y, "strategy_weights": w.detach()}


def concat_bf16(P, x, masks=None):
    return {"out": _block(x, P, "", None if masks is None else masks["concat"])}
