"""The ``nn.Linear`` layers on Stack B's training path, stated once: one record per layer (``Lin``), created per model from the
module tree (``Layers``), and everything that used to enumerate the tree again derived from the records -- the per-step operand
accessors (``Params``), the fragment-major images the layer chains stream (``frag_images``), and the table of transposed copies
the optimiser step maintains (``Layers.transposed_table``).  ``stackb_train.py`` states the runs of these layers and executes them.

Host logic only.  The ORDER of ``Layers.all`` is the order of the path; the derived tables are walked in it, and their order is what
``mmdeer_repack`` / ``mmdeer_pack_transposed_batch`` see."""
from __future__ import annotations

from dataclasses import dataclass
from types import SimpleNamespace
from typing import Optional, Tuple

import torch
from torch import nn

from .chainops import K_OK, FragImages

ENC, FUS, HID = 256, 512, 256
SITE_RES, SITE_ATTN_S, SITE_ATTN_C, SITE_EST, SITE_WN, SITE_AV, SITE_TRI, SITE_H0, SITE_H3 = 32, 64, 65, 66, 67, 68, 69, 70, 71     # H3: 71..73
ENCODERS = ("audio_encoder", "video_encoder", "text_encoder")
HEADS = ("valence", "arousal", "dominance")


@dataclass(eq=False)
class Lin:
    """One nn.Linear of the path.  ``name``: key of its images; ``prefix``: its state-dict prefix (gradient names, flat views)."""
    name: str
    prefix: str
    mod: nn.Linear
    N: int                              # (N, K) = the weight's shape
    K: int
    relu: int = 0
    site: int = -1                      # dropout site of the epilogue (-1: none)
    p: Optional[float] = None           # None: the config's dropout; the estimator's is 0.2 whatever the config says
    shift: int = 0                      # one dropout decision per 2^shift columns (the attention heads)
    ln: Optional[str] = None            # state-dict prefix of the LayerNorm that follows
    ln_mod: Optional[nn.LayerNorm] = None
    residual: int = 0                   # x + LayerNorm(...): a residual block
    img: bool = False                   # derived operands: fragment-major W (columns zero-padded to a multiple of 64),
    imgT: bool = False                  # fragment-major W^T,
    wt: bool = False                    # row-major transposed copy (at the parameter's own offset),
    area: Optional[Tuple[str, int]] = None    # (stacked / sliced area of the transposed buffer, its column there)

    @property
    def weight(self):
        return self.mod.weight


class Layers:
    """The records of one model, by role (``enc[m].stem / .res[l] / .out``, ``vs vc os oc``, ``e1 e2 e3``, ``wn0 wn3``, ``av tri``
    = [first, last] of a fusion stage, ``gate``, ``h0 h3 h6`` per head) and in path order (``all``)."""

    def __init__(self, model):
        self.cfg, self.all = model.config, []

        def lin(name, prefix, **kw):
            mod = model.get_submodule(prefix)
            r = Lin(name, prefix, mod, *mod.weight.shape, ln_mod=model.get_submodule(kw["ln"]) if "ln" in kw else None, **kw)
            self.all.append(r)
            return r
        both = dict(img=True, imgT=True, wt=True)
        self.enc = []
        for m, e in enumerate(ENCODERS):
            stem = lin(f"enc{m}.w0", e + ".input_projection.0", relu=1, ln=e + ".input_projection.2", img=True)
            res = [lin(f"enc{m}.res{l}", f"{e}.encoder_layers.{l}.layers.0", relu=1, site=SITE_RES + 3 * l + m, ln=f"{e}.encoder_layers.{l}.layers.3",
                       residual=1, **both) for l in range(self.cfg.encoder_layers)]
            self.enc.append(SimpleNamespace(name=e, stem=stem, res=res, out=lin(f"enc{m}.wo", e + ".output_projection", **both)))
        a, f = "attention_module", "fusion_module"
        self.vs = lin("wv_s", a + ".self_attention.value_proj", site=SITE_ATTN_S, shift=5, img=True, area=("wv", 0))
        self.vc = lin("wv_c", a + ".cross_attention.value_proj", site=SITE_ATTN_C, shift=5, img=True, area=("wv", ENC))
        self.os, self.oc = lin("wos", a + ".self_attention.output_proj", **both), lin("woc", a + ".cross_attention.output_proj", **both)
        est = a + ".uncertainty_estimator.estimator"
        self.e1, self.e2 = lin("we1", est + ".0", relu=1, site=SITE_EST, p=0.2, **both), lin("we2", est + ".3", relu=1, **both)
        self.e3 = lin("we3", est + ".5")                                   # 64 -> 1: inside the attention row kernel
        self.wn0 = lin("wn1", a + ".weight_network.0", area=("wn1", 0))    # its 768 feature columns are a GEMM, the rest the row kernel's
        self.wn3 = lin("wn2", a + ".weight_network.3")
        stage = lambda k, pre, site: [lin(k + ".w0", pre + ".0", relu=1, site=site, ln=pre + ".3", **both), lin(k + ".w4", pre + ".4", relu=1, **both)]
        self.av, self.tri = stage("av", f + ".av_fusion", SITE_AV), stage("tri", f + ".trimodal_fusion", SITE_TRI)
        self.gate = lin("wg", f + ".fusion_gate.0", wt=True)
        self.h0, self.h3, self.h6 = [], [], []
        for d, nm in enumerate(HEADS):
            pre = f"prediction_heads.{nm}.evidence_network"
            self.h0.append(lin(f"wh0.{d}", pre + ".0", relu=1, site=SITE_H0, img=True, area=("wh0", d * HID)))
            self.h3.append(lin(f"wh3.{d}", pre + ".3", relu=1, site=SITE_H3 + d, **both))
            self.h6.append(lin(f"wh6.{d}", pre + ".6"))                    # 128 -> 4: row-major images wh6p.d / wh6bd
        self.areas = {}                       # area -> its members, in path order
        for r in self.all:
            if r.area:
                self.areas.setdefault(r.area[0], []).append(r)

    def area_shape(self, key):
        """(rows, columns) of a transposed area: the members' W^T side by side."""
        rs = self.areas[key]
        return rs[0].K, sum(r.N for r in rs)

    def transposed_table(self, offset_of, end):
        """What ``mmdeer_pack_transposed_batch`` writes: [(parameter, destination offset, ld, column)], the areas' offsets behind ``end``
        and the buffer's length.  The copies of the encoders' output projections come first, then those of their residual blocks, then
        the rest in path order, then the areas' members."""
        extra, tab = {}, []
        for key in self.areas:
            extra[key] = end
            rows, cols = self.area_shape(key)
            end += (rows * cols + 63) // 64 * 64
        enc = [e.out for e in self.enc] + [r for e in self.enc for r in e.res]
        plain = enc + [r for r in self.all if r.wt and all(r is not q for q in enc)]
        tab += [(r.weight, offset_of(r.weight), 0, 0) for r in plain]
        for key, rs in self.areas.items():
            tab += [(r.weight, extra[key], self.area_shape(key)[1] if len(rs) > 1 else 0, r.area[1]) for r in rs]
        return tab, extra, end

    def chains_take(self) -> bool:
        """Whether the chain kernel instantiates this geometry (otherwise the step runs launch by launch)."""
        c = self.cfg
        return (c.encoder_dim == ENC and c.fusion_dim == FUS and c.encoder_layers <= 4 and c.audio_dim <= 128 and c.audio_dim % 2 == 0
                and c.video_dim in K_OK and c.text_dim in K_OK and c.attention_heads == 8 and c.emotion_dims == 3)


def layers_of(model, flat=None) -> Layers:
    """The records: those the flat state was built with (``CompleteDEERModel._flat`` rebuilds it, and them, whenever a parameter of
    the model was moved or replaced), or, without one, read from the module tree now."""
    return flat["layers"] if flat is not None else Layers(model)


def frag_images(model, st) -> Optional[FragImages]:
    """Fragment-major images of every matrix the layer chains of the bf16 training step stream (W for the forward runs, W^T for
    the dX runs), sourced from the flat bf16 copy / the transposed copies the optimiser step maintains.  None when the model's
    geometry is outside what the chain kernel instantiates (the step then runs launch by launch)."""
    L = st["layers"]
    if not L.chains_take():
        return None
    packed, packed_t, by_id, extra = st["packed"], st["packed_t"], st["by_id"], st["extra_t"]
    F = FragImages(st["dev"])

    def W(r):
        off, n = by_id[id(r.weight)]
        return packed[off:off + n].view(r.N, r.K)
    for r in L.all:
        if r.img:
            F.add(r.name, W(r), r.N, (r.K + 63) // 64 * 64, ld_src=r.K, cols_valid=r.K)
        if r.imgT:
            F.add(r.name + ".T", W(r), r.N, r.K, transpose=1)
    for key, rs in L.areas.items():      # W^T of the stacked operands, from the transposed row-major copies (their areas behind the last parameter)
        if len(rs) > 1:
            rows, cols = L.area_shape(key)
            F.add(key + ".T", packed_t[extra[key]:extra[key] + rows * cols].view(rows, cols), rows, cols)
    # row-major restatements the remaining GEMM launches read: the feature columns of weight_network.0 (a column slice of a
    # 771-wide matrix), the heads' last layers zero-padded from 4 to 8 rows
    F.area("wn1", ENC, 3 * ENC)
    F.place("wn1", W(L.wn0), ENC, 3 * ENC, ld_src=L.wn0.K)
    F.area("wh6bd", 24, 3 * HID // 2)          # the three last head layers block-diagonally: d H3 of all heads in one dX launch
    for d, r in enumerate(L.h6):
        F.area(f"wh6p.{d}", 8, HID // 2)
        F.place(f"wh6p.{d}", W(r), 4, HID // 2)
        F.place("wh6bd", W(r), 4, HID // 2, row0=8 * d, col0=d * (HID // 2))
    F.finish()
    return F


class Params:
    """One step's operands by record: compute-dtype matrices and fp32 vectors.  Default: a cast per matrix per step (torch here is
    memory plumbing).  With ``flat`` (CompleteDEERModel._flat: the fused training step) the matrices are VIEWS of the flat
    compute-dtype copy the optimiser step maintains; with ``Fg`` (the chain plan) the operands that are slices / concatenations /
    paddings of parameters are images the optimiser step maintains too -- no per-step copies at all."""

    def __init__(self, L: Layers, dt, flat=None, Fg=None):
        self.L, self.dt, self.flat, self.Fg = L, dt, flat, Fg
        self.packed_t = flat.get("packed_t") if flat is not None else None
        self._copies = {}               # per step: casts, concatenations, paddings -- they hold this step's values
        # views of the flat buffers hold no values of their own: they are kept with the flat state, like the records
        self._views = flat["views"] if flat is not None else self._copies

    @staticmethod
    def _get(store, key, make, *args):  # keys: (kind, record name | area)
        v = store.get(key)
        if v is None:
            v = store[key] = make(*args)
        return v

    def _flat_view(self, buf, r, rows, cols):
        off, n = self.flat["by_id"][id(r.weight)]
        return buf[off:off + n].view(rows, cols)

    def _f32(self, *ts):
        v = tuple(t.detach().float().contiguous() for t in ts)
        return v if len(v) > 1 else v[0]

    def w(self, r):                     # (N, K), compute dtype
        if self.flat is not None:
            return self._get(self._views, ("w", r.name), self._flat_view, self.flat["packed"], r, r.N, r.K)
        return self._get(self._copies, ("w", r.name), lambda: r.weight.detach().to(self.dt).contiguous())

    def wt(self, r):                    # (K, N) transposed copy: dX = dY W then runs as an NT GEMM on the LDS-DMA kernel; None without one
        if self.packed_t is None or not r.wt:
            return None
        return self._get(self._views, ("t", r.name), self._flat_view, self.packed_t, r, r.K, r.N)

    def b(self, r):
        return self._get(self._views, ("b", r.name), self._f32, r.mod.bias)

    def ln(self, r):                    # (gamma, beta) of the LayerNorm behind r
        return self._get(self._views, ("ln", r.name), self._f32, r.ln_mod.weight, r.ln_mod.bias)

    def vecw(self, r):                  # a matrix the row kernels read as fp32
        return self._get(self._views, ("v", r.name), self._f32, r.weight)

    def img(self, r, T=False, row0=0):
        return self.Fg(r.name + (".T" if T else ""), row0)

    def stack(self, key):               # launch-by-launch plan: [members' W ; ...], [members' bias ; ...] -- a per-step copy
        rs = self.L.areas[key]
        return self._get(self._copies, ("stack", key), lambda: (torch.cat([self.w(r) for r in rs], 0), torch.cat([self.b(r) for r in rs], 0)))

    def stack_t(self, key):             # the area of the transposed buffer (rows x columns of Layers.area_shape), or None
        if self.packed_t is None:
            return None
        rows, cols = self.L.area_shape(key)
        off = self.flat["extra_t"][key]
        return self.packed_t[off:off + rows * cols].view(rows, cols)

    def wn1(self):                      # the 768 feature columns of weight_network.0, row-major
        D3 = 3 * ENC
        return self.Fg.mat("wn1") if self.Fg is not None else self._get(self._copies, ("features", "wn1"), lambda: self.w(self.L.wn0)[:, :D3].contiguous())

    def wn1_t(self):
        t = self.stack_t("wn1")
        return None if t is None else t[:3 * ENC]

    def wn1u(self):                     # its three uncertainty columns, (256, 3) fp32
        w = self.L.wn0.weight.detach()[:, 3 * ENC:]
        return w if self.Fg is not None else self._get(self._copies, ("uncertainty", "wn1"), lambda: w.float().contiguous())

    def wh6p(self, d):                  # (8, 128): a head's last layer, rows 4..7 zero (8-column gradient blocks)
        if self.Fg is not None:
            return self.Fg.mat(f"wh6p.{d}")
        return self._get(self._copies, ("padded", self.L.h6[d].name), lambda: torch.nn.functional.pad(self.w(self.L.h6[d]), (0, 0, 0, 4)))
