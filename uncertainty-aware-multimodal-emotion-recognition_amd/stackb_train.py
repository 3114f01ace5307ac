"""Stack B training path: forward with dropout and backward of ``complete_project.CompleteDEERModel``
(reference src/models/complete_project.py:462-602) as a sequence of C-ABI operator calls.

This file is host logic only -- it owns buffers and the ORDER of the launches; every number is produced by
``libmmdeer_hip.so``: the Linear layers by ``mmdeer_gemm`` (forward with bias / ReLU / hash dropout in the epilogue;
``dX = dY W`` with the ``(Y > 0) / (1 - p)`` mask of the layer below in the epilogue; ``dW = dY^T X`` with the bias gradient
from the same launch), LayerNorm by ``mmdeer_layernorm_fwd`` / ``_bwd`` (the backward folds the ReLU + dropout mask of the
``Linear-ReLU-Dropout-LayerNorm`` blocks, complete_project.py:65-70, 315-333), and the row operators of
``csrc/stackb_train.hip`` (attention tail forward / backward, gate mix backward, softplus backward, masked adds).

Dropout sites (all ``nn.Dropout``; masks are the library's counter hash keyed by (seed, step, site, row, column), so the
backward regenerates them): ResidualBlock (:68), MultiHeadAttention attention weights (:141, 172 -- one decision per (row,
head) because every softmax is over a single key), UncertaintyEstimator (:186, p = 0.2 whatever the config says),
weight_network (:237), the two fusion stages (:318, 328) and the prediction heads (:379, 382).

How it is written.  ``stackb_layers.py`` holds one record per ``nn.Linear`` of the path and derives every operand table from the
records.  Here every sample-local run of layers -- the three encoders, the attention blocks' value / output projections, the
estimator, the two fusion stages, the heads' first two layers, and the dX run of each of them -- is stated ONCE, as a list of
``Layer`` s made of ``Part`` s, inside ``forward_train`` / ``backward``; ``Runner`` executes a run by one of two launch plans that
write the same tape and the same gradients, bit for bit (tests/test_gpu_stackb.py): launch by launch (``model.train_plan = 'ops'``;
fp32; geometries the chain kernel does not instantiate), or -- the default of the bf16 fused step -- as ONE launch of the layer-chain
kernel (``mmdeer_chain``, csrc/chain.hip; host side ``chainops.py``): 16 chain launches, 49 launches per step instead of ~170.  Where
the plans differ in more than that, the difference is a field of ``Part`` / ``Layer`` or a branch of ``Runner``, with its reason.
The row kernels between the runs, the 128 -> 4 head layers and the weight-gradient records around them are written out in order:
the order of the ``dw`` / fold / copy records decides the composition of the grouped launches and hence the bits.

``model.keep_backward_tape`` (default off; tests/test_gpu_stackb_step.py) keeps references to what the backward leaves in memory: ``T["bwd"]``, by
name, the activation-gradient matrices both plans store, and ``T["ops"]``, launch by launch only, the three kinds of matrix a chain keeps in LDS
(``lnr.``: LayerNorm rows before a residual block's bypass is added; ``dln.``: the gradient a LayerNorm backward reads; ``dxr.``: dz W before the bypass
gradient is added; each followed by the ``Lin`` name).  References only: no launch, copy or allocation more, and the same order.

Layout conventions are those of the inference executor (csrc/stackb.hip): encoder outputs in column blocks of one (B, 768)
matrix whose (3B, 256) reading is the row set of the shared-weight attention layers; heads stacked along N.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from functools import partial
from typing import Callable, Dict, List, Optional, Sequence

import torch

from . import _lib
from .chainops import Chain, FragImages
from .opseq import Exec, set_drop
from .stackb_layers import ENC, FUS, HID, SITE_WN, Lin, Params, layers_of


def chain_plan(model, flat, dt) -> Optional[FragImages]:
    """The fragment-major weight images when this step runs its sample-local layer runs as chains: the fused bf16 step on a
    geometry the chain kernel instantiates, unless ``model.train_plan == 'ops'`` (the launch-by-launch sequence, kept as the
    reference the chains are tested against bit for bit)."""
    if flat is None or dt != torch.bfloat16 or getattr(model, "train_plan", "auto") == "ops":
        return None
    return flat.get("frag")


@dataclass
class Part:
    """One Linear inside a layer of a run: columns [kin, kin + K) of the layer's input -> columns [nout_off, ...) of its output
    (forward: x W^T + b with the record's epilogue; dX run: dy W)."""
    lin: Lin
    kin: int = 0
    nout_off: int = 0
    dcol: int = 0                            # forward: column of this part in the dropout site's mask (parts of one stacked layer share a site)
    x: Optional[torch.Tensor] = None         # launch by launch: this part's input where that is a matrix of its own, not columns of a panel
    mask: Optional[torch.Tensor] = None      # dX: times (mask[:, mcol:] > 0) * mscale -- ReLU + dropout of the layer below
    mcol: int = 0
    mscale: float = 1.0
    regen: Optional[Lin] = None              # dX: times the dropout factor of this layer's forward epilogue, regenerated
    res_add: int = 0                         # dX: the output is added to the bypass gradient of a residual block,
    res_dup: int = 0                         # ... which the layer above it keeps a copy of
    dw: Optional[tuple] = None               # (dy, x, Lin | (gw, gb)): the weight-gradient record that follows this part
    before: Optional[Callable] = None        # launches that make this part's input: both plans, in this place
    after: Optional[Callable] = None         # launches that read its output: launch by launch right after it, else after the chain launch


@dataclass
class Layer:
    """Parts that fill one output panel, and its end: ``out`` (``out2``: the columns from ``split`` on) is where the panel is kept;
    ``ln`` = (xln, mean, rstd): the LayerNorm behind the layer's Linear (a residual block's adds the layer's input);
    ``lnb`` = (Lin the LayerNorm is behind, y, mean, rstd, dz, mask_scale): its backward (gamma / beta gradients to that LayerNorm's)."""
    parts: Sequence[Part]
    out: Optional[torch.Tensor] = None
    out2: Optional[torch.Tensor] = None
    split: int = 0
    ln: Optional[tuple] = None
    lnb: Optional[tuple] = None
    stacked: Optional[str] = None            # the parts are the members of this stacked operand.  Forward, launch by launch: each reads its
    one: bool = False                        # rows of the stacked copy, or (one) the layer is ONE GEMM on it; dX (no parts): the stacked matrix
    dw: Sequence[tuple] = ()                 # weight-gradient records that follow the layer's end


def _cols(t, c0, n=None):
    """Columns [c0, c0 + n) of a row-major matrix as the launches see them (an address and the row stride): the matrix itself where
    they start at its first column."""
    return t if c0 == 0 else t[:, c0:] if n is None else t[:, c0:c0 + n]


class Runner:
    """Executes runs by one of the two plans.  ``dw(dy, x, target)`` / ``vec(name, n)``: the backward's gradient destinations."""

    def __init__(self, ex: Exec, Q: Params, chain: bool, pc: float, tape: Optional[dict] = None):
        self.ex, self.Q, self.chain, self.pc = ex, Q, chain, pc
        self.dw = self.vec = None
        self.tape = tape           # model.keep_backward_tape, launch by launch: the matrices between two launches that no tape entry names

    def p_of(self, r: Lin) -> float:
        return self.pc if r.p is None else r.p

    def fwd(self, x, rows, layers, ts=0):
        self._chain(x, rows, layers, ts, False) if self.chain else self._ops_fwd(x, rows, layers)

    def bwd(self, x, rows, layers, ts=0):
        self._chain(x, rows, layers, ts, True) if self.chain else self._ops_bwd(x, rows, layers)

    # ---- one launch of the layer-chain kernel.  ts: samples per workgroup (16 where a layer is wider than 512; 0: the kernel's choice)
    def _chain(self, x, rows, layers, ts, T):
        ex, Q = self.ex, self.Q
        sited = [pt.regen if T else pt.lin for ly in layers for pt in ly.parts]
        p = next((self.p_of(r) for r in sited if r is not None and r.site >= 0), 0.0 if T else self.pc)
        K0 = max(pt.kin + (pt.lin.N if T else Q.Fg.shape[pt.lin.name][1]) for pt in layers[0].parts)
        ch = Chain(ex, x, x.stride(0), K0, rows, p=ex.p_of(p), ts=ts)
        nwg, folds = None, []
        for ly in layers:
            nout = 0
            if T and ly.stacked:                                   # [W_0 ; W_1 ; ...]^T: one segment
                n, k = Q.Fg.shape[ly.stacked + ".T"]
                ch.seg(Q.Fg(ly.stacked + ".T"), n, k)
                nout = n
            for pt in ly.parts:
                r = pt.lin
                if pt.before:
                    pt.before()
                if T:
                    n, k = Q.Fg.shape[r.name + ".T"]
                    step = 384 if n > 512 else n                   # W^T is [n][k]: at most four 128-column tiles per segment
                    for c0 in range(0, n, step):
                        ch.seg(Q.img(r, True, c0), min(step, n - c0), k, kin=pt.kin, nout_off=pt.nout_off + c0, mask=pt.mask,
                               ldm=pt.mask.stride(0) if pt.mask is not None else 0, mcol=pt.mcol, mscale=pt.mscale, res_add=pt.res_add, res_dup=pt.res_dup,
                               site=pt.regen.site if pt.regen else -1, shift=pt.regen.shift if pt.regen else 0)
                else:
                    n, k = Q.Fg.shape[r.name]
                    ch.seg(Q.img(r), n, k, bias=Q.b(r), relu=r.relu, site=r.site, shift=r.shift, dcol=pt.dcol, kin=pt.kin, nout_off=pt.nout_off)
                nout += n
                if pt.dw:
                    self.dw(*pt.dw)
            ln = lnb = None
            if ly.ln is not None:
                ln = (*Q.ln(ly.parts[0].lin), *ly.ln)
            if ly.lnb is not None:                                 # gamma / beta partials per workgroup, folded in the step's one fold launch
                r, y, mean, rstd, dz, ms = ly.lnb
                nwg = nwg or ch.workgroups()
                part = torch.empty(nwg * 2 * nout, dtype=torch.float32, device=y.device)
                lnb = (Q.ln(r)[0], y, mean, rstd, dz, part, ms)
                folds += [(part, self.vec(r.ln + ".weight", nout), nwg, nout, 2 * nout), (part[nout:], self.vec(r.ln + ".bias", nout), nwg, nout, 2 * nout)]
            ch.end(nout, stash=ly.out, ld_stash=ly.out.stride(0) if ly.out is not None else 0, stash2=ly.out2, split=ly.split, ln=ln,
                   residual=int(ly.ln is not None and ly.parts[0].lin.residual), lnb=lnb)
            for rec in ly.dw:
                self.dw(*rec)
        ch.launch()
        if folds:
            ex.folds += folds
        for ly in layers:
            for pt in ly.parts:
                if pt.after:
                    pt.after()

    # ---- launch by launch, forward
    def _ops_fwd(self, x, rows, layers):
        ex, Q = self.ex, self.Q
        src = x
        for ly in layers:
            if ly.one:
                r = ly.parts[0].lin
                W, b = Q.stack(ly.stacked)
                ex.linear(src, src.stride(0), W, b, ly.out, ly.out.stride(0), rows, relu=r.relu, site=r.site, p=self.p_of(r) if r.site >= 0 else 0.0, shift=r.shift)
            for pt in ly.parts:
                r = pt.lin
                if not ly.one:
                    if ly.stacked:
                        W, b = (t[r.area[1]:r.area[1] + r.N] for t in Q.stack(ly.stacked))
                    else:
                        W, b = Q.w(r), Q.b(r)
                    xin = _cols(src, pt.kin, r.K)
                    out = _cols(ly.out2, pt.nout_off - ly.split) if ly.out2 is not None and pt.nout_off >= ly.split else _cols(ly.out, pt.nout_off)
                    ex.linear(xin, xin.stride(0), W, b, out, out.stride(0), rows, relu=r.relu, site=r.site, p=self.p_of(r) if r.site >= 0 else 0.0, shift=r.shift)
                if pt.after:
                    pt.after()
            if ly.ln is not None:
                r = ly.parts[0].lin
                xln, mean, rstd = ly.ln
                if r.residual:                                     # x + LayerNorm(...) (:73): to a temporary, then the sum (the chain's residual=1)
                    tmp = ex.ln_fwd(ly.out, *Q.ln(r), None, mean, rstd)[0]
                    if self.tape is not None:
                        self.tape["lnr." + r.name] = tmp               # LayerNorm(...) before the bypass is added
                    ex.add(xln, src, tmp)
                else:
                    ex.ln_fwd(ly.out, *Q.ln(r), xln, mean, rstd)
                src = xln
            else:
                src = ly.out

    # ---- launch by launch, dX run
    def _ops_bwd(self, x, rows, layers):
        ex, Q = self.ex, self.Q
        src, bypass = x, None
        for ly in layers:
            cur = ly.out
            if ly.stacked:
                ex.dx(src, src.stride(0), Q.stack(ly.stacked)[0], cur, cur.stride(0), rows, wt=Q.stack_t(ly.stacked))
            for pt in ly.parts:
                r = pt.lin
                if pt.before:
                    pt.before()
                dy = pt.x if pt.x is not None else _cols(src, pt.kin, r.N)
                out = _cols(ly.out, pt.nout_off) if ly.out is not None else torch.empty(rows, r.K, dtype=ex.dt, device=dy.device)
                g = pt.regen
                ex.dx(dy, dy.stride(0), Q.w(r), out, out.stride(0), rows, mask=None if pt.mask is None else _cols(pt.mask, pt.mcol),
                      ldm=0 if pt.mask is None else pt.mask.stride(0), mask_scale=pt.mscale, regen_site=g.site if g else -1, shift=g.shift if g else 0,
                      p=self.p_of(g) if g else 0.0, wt=Q.wt(r))
                if pt.dw:
                    self.dw(*pt.dw)
                if pt.res_add:                                     # (the chain keeps the bypass gradient in columns [256, 512) of its panel)
                    if self.tape is not None:
                        self.tape["dxr." + r.name] = out               # dz W before the bypass gradient is added
                    out = ex.add(torch.empty_like(out), bypass, out)
                if ly.out is None:
                    cur = out
                if pt.after:
                    pt.after()
            if ly.lnb is not None:
                r, y, mean, rstd, dz, ms = ly.lnb
                if self.tape is not None:
                    self.tape["dln." + r.name] = cur                   # the gradient the LayerNorm backward reads
                ex.ln_bwd(cur, y, mean, rstd, Q.ln(r)[0], self.vec(r.ln + ".weight", y.shape[1]), self.vec(r.ln + ".bias", y.shape[1]), ms, dz=dz)
                bypass, cur = cur, dz
            for rec in ly.dw:
                self.dw(*rec)
            src = cur


def forward_train(model, xs: List[torch.Tensor], drop, flat=None) -> Dict:
    """Forward with every intermediate the backward needs kept on a tape.  Returns the tape (incl. planes (8, B, 3))."""
    ex = Exec(model.compute_dtype, drop)
    dt, f32, dev = ex.dt, ex.f32, xs[0].device
    pc = model.config.dropout
    B = xs[0].shape[0]
    L = layers_of(model, flat)
    # bf16 fused step: the sample-local runs of layers go through the layer-chain kernel (mmdeer_chain), ONE launch per run
    Fg = chain_plan(model, flat, dt)
    Q = Params(L, dt, flat, Fg)
    # model.keep_backward_tape (tests/test_gpu_stackb_step.py): references to what the launches leave in memory and no tape entry names --
    # no launch, copy or allocation more, and the same order
    ops_tape = {} if getattr(model, "keep_backward_tape", False) else None
    run = Runner(ex, Q, Fg is not None, pc, ops_tape)
    new = lambda *s, d=None: torch.empty(*s, dtype=d or dt, device=dev)
    stat = lambda n: (torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev))
    T: Dict = {"P": Q, "B": B, "xs": xs, "ex": ex, "enc": [], "chain": Fg is not None, "ops": ops_tape}
    E = new(B, 3 * ENC)
    for m, (x, e) in enumerate(zip(xs, L.enc)):
        # encoder m: Linear-ReLU-LayerNorm stem, the residual blocks x + LayerNorm(Dropout(ReLU(Linear x))), output projection
        # (complete_project.py:77-118) -- L + 2 layers.  Inputs are read in the loader's dtype and converted while staging.
        K = x.shape[1]
        K0 = (K + 63) // 64 * 64
        if run.chain and x.stride(0) != K0:                              # the 84-wide audio rows: zero-padded copy (memory plumbing;
            xin = torch.zeros(B, K0, dtype=dt, device=dev)               # train_step_fused hands over rows that are padded already)
            xin[:, :K].copy_(x)
            x = xin[:, :K]
        t = {"xin": x, "y0": new(B, ENC), "y": [], "st": [], "h": [new(B, ENC)]}
        t["m0"], t["r0"] = stat(B)
        layers = [Layer([Part(e.stem)], out=t["y0"], ln=(t["h"][0], t["m0"], t["r0"]))]
        for r in e.res:
            y, hn, st = new(B, ENC), new(B, ENC), stat(B)
            layers.append(Layer([Part(r)], out=y, ln=(hn, *st)))
            t["y"].append(y); t["st"].append(st); t["h"].append(hn)
        layers.append(Layer([Part(e.out)], out=E[:, m * ENC:(m + 1) * ENC]))
        run.fwd(x, B, layers, ts=16 if K0 > 512 else 0)
        T["enc"].append(t)
    T["E"] = E
    E3 = E.view(3 * B, ENC)
    # attention: every softmax is over ONE key, so a block is output_proj(drop(value_proj(x))) with one dropout decision per
    # (row, 32-column head) (:141, 172); every one of the 3 B (sample, modality) rows is a sample of its own.  Value projections of
    # both blocks: one layer, two column ranges of one (3B, 512) matrix; both output projections: one layer, each reading its half
    VV = new(3 * B, 2 * ENC)
    S, X = new(3 * B, ENC), new(3 * B, ENC)
    H1, H2 = new(3 * B, ENC // 2), new(3 * B, ENC // 4)
    run.fwd(E3, 3 * B, [Layer([Part(L.vs), Part(L.vc, nout_off=ENC)], out=VV, stacked="wv"),
                        Layer([Part(L.os), Part(L.oc, kin=ENC, nout_off=ENC)], out=S, out2=X, split=ENC)])
    run.fwd(E3, 3 * B, [Layer([Part(L.e1)], out=H1), Layer([Part(L.e2)], out=H2)])       # the estimator's two layers (:186)
    pre = new(B, ENC)
    ex.linear(S.view(B, 3 * ENC), 3 * ENC, Q.wn1(), Q.b(L.wn0), pre, ENC, B)
    AV, Tt = new(B, 2 * ENC), new(B, FUS + ENC)
    r, w4, u4 = new(B, ENC), new(B, 4, d=torch.float32), new(B, 4, d=torch.float32)
    a = _lib.StackBAttnTrainArgs()
    a.h2, a.pre, a.self_out, a.cross_out = H2.data_ptr(), pre.data_ptr(), S.data_ptr(), X.data_ptr()
    wn1u = Q.wn1u()
    a.est_w3, a.est_b3, a.wn_w1_unc, a.wn_w2, a.wn_b2 = (t.data_ptr() for t in (Q.vecw(L.e3), Q.b(L.e3), wn1u, Q.vecw(L.wn3), Q.b(L.wn3)))
    a.out_av, a.out_text = AV.data_ptr(), Tt[:, FUS:].data_ptr()
    a.r, a.weights4, a.unc4 = r.data_ptr(), w4.data_ptr(), u4.data_ptr()
    a.ld_w1_unc, a.ld_av, a.ld_text, a.B, a.act_f32 = wn1u.stride(0), 2 * ENC, FUS + ENC, B, f32
    a.training, a.drop_site, a.dropout_p = int(drop is not None), SITE_WN, ex.p_of(pc)
    set_drop(a, drop)
    a.stream = ex.s
    if B:
        _lib.check(ex.lib.mmdeer_stackb_attn_mix_train_fwd(C.byref(a)))
    T.update(VV=VV, S=S, X=X, H1=H1, H2=H2, pre=pre, AV=AV, T=Tt, r=r, w4=w4, u4=u4, attn_args=a)

    # fusion
    def stage(recs, inp, out):
        # Linear-ReLU-Dropout-LayerNorm-Linear-ReLU (complete_project.py:315-333)
        a1, n1, st = new(B, FUS), new(B, FUS), stat(B)
        run.fwd(inp, B, [Layer([Part(recs[0])], out=a1, ln=(n1, *st)), Layer([Part(recs[1])], out=out)], ts=16 if recs[0].K > 512 else 0)
        return (a1, n1, *st)
    R2 = new(B, FUS)
    T["av"] = stage(L.av, AV, Tt[:, :FUS])
    T["tri"] = stage(L.tri, Tt, R2)
    G = new(B, FUS)
    ex.linear(Tt, FUS + ENC, Q.w(L.gate), Q.b(L.gate), G, FUS, B)
    fused = new(B, FUS)
    fused32 = new(B, FUS, d=torch.float32)
    if B:
        _lib.check(ex.lib.mmdeer_stackb_gate_mix(G.data_ptr(), FUS, R2.data_ptr(), FUS, Tt.data_ptr(), FUS + ENC, fused.data_ptr(), FUS,
                                                 fused32.data_ptr(), B, FUS, f32, ex.s))
    T.update(R2=R2, G=G, fused=fused, fused32=fused32)
    # heads: the first two layers of the three evidence networks (complete_project.py:376-384), 512 -> 3 x 256 -> 3 x 128, are a run
    # (launch by launch the first is ONE N = 768 GEMM on the stacked copy); each head's 128 -> 4 layer reads its block of the second
    H0, H3 = new(B, 3 * HID), new(B, 3 * HID // 2)
    ev = new(B, 12, d=torch.float32)

    def last(d):
        ex.linear(H3[:, d * 128:(d + 1) * 128], 3 * HID // 2, Q.w(L.h6[d]), Q.b(L.h6[d]), ev[:, 4 * d:4 * d + 4], 12, B)
    run.fwd(fused, B, [Layer([Part(h, dcol=d * HID, nout_off=d * HID) for d, h in enumerate(L.h0)], out=H0, stacked="wh0", one=True),
                       Layer([Part(h, kin=d * HID, nout_off=d * (HID // 2), after=partial(last, d)) for d, h in enumerate(L.h3)], out=H3)], ts=16)
    planes = new(8, B, 3, d=torch.float32)
    cal = model.calibration_layer
    cn = cal.calibration_network
    cps = [t.detach().float().reshape(-1).contiguous() for t in (cal.temperature, cn[0].weight, cn[0].bias, cn[2].weight, cn[2].bias, cn[4].weight, cn[4].bias)]
    if B:
        _lib.check(ex.lib.mmdeer_stackb_head(ev.data_ptr(), 12, *[t.data_ptr() for t in cps], planes.data_ptr(), B, ex.s))
    T.update(H0=H0, H3=H3, ev=ev, planes=planes, cal_keep=cps)
    return T


def backward(model, T: Dict, g4: torch.Tensor, flat=None) -> Dict[str, torch.Tensor]:
    """Gradients of every parameter on the path from d (mu, nu, alpha, beta) = g4 (4, B, 3) fp32.  Returns
    {state_dict key: fp32 gradient}; the calibration layer (not on the path of mu / nu / alpha / beta) gets none.

    With ``flat`` (the fused training step) every gradient is written straight into its slice of the model's flat gradient
    buffer (``.grad`` of each parameter is a view of it), the weight-gradient GEMMs are recorded and run as grouped launches
    with one slab fold per group at the end (``Exec.flush_dw`` -> ``mmdeer_gemm_batch``), and nothing is returned through
    autograd; the query / key projections keep the zeros the buffer was created with."""
    ex: Exec = T["ex"]
    Q, B, dt, f32 = T["P"], T["B"], ex.dt, ex.f32
    L = Q.L
    pc = model.config.dropout
    dev = g4.device
    new = lambda *s, d=None: torch.empty(*s, dtype=d or dt, device=dev)
    # every fp32 gradient / scratch matrix of the pass is a slice of ONE zeroed buffer (one memset instead of ~100)
    pool = torch.zeros((0 if flat is not None else sum(p.numel() for p in model.parameters())) + (1 << 20), dtype=torch.float32, device=dev)
    cursor = [0]

    def z32(*shape):
        n = 1
        for d in shape:
            n *= d
        lo = cursor[0]
        cursor[0] = (lo + n + 63) // 64 * 64                       # 256-byte aligned slices
        if cursor[0] > pool.numel():
            return torch.zeros(*shape, dtype=torch.float32, device=dev)
        return pool[lo:lo + n].view(*shape)

    G: Dict[str, torch.Tensor] = {}
    sc = ex.scale_of(pc)
    chain = flat is not None and bool(T.get("chain"))               # the layer-chain plan (see forward_train)
    Fg = Q.Fg if chain else None
    run = Runner(ex, Q, chain, pc, T.get("ops"))
    keep = T.get("ops") is not None                                 # model.keep_backward_tape: T["bwd"], by name, at the end
    late = []                      # flat mode: (destination view, source) copies that must wait for the grouped dW launches
    if flat is not None:
        ex.deferred, ex.folds = [], []
        fview = lambda name: flat["gview"][name]

    def grads(r: Lin):
        if flat is not None:
            return fview(r.prefix + ".weight"), fview(r.prefix + ".bias")
        G[r.prefix + ".weight"], G[r.prefix + ".bias"] = z32(r.N, r.K), z32(r.N)
        return G[r.prefix + ".weight"], G[r.prefix + ".bias"]

    def vec(name, n):              # a vector gradient the row kernels write directly (LayerNorm gamma / beta)
        if flat is not None:
            return fview(name)
        G[name] = z32(n)
        return G[name]

    def dw(dy, x, tgt):            # gw (N, K) = dy^T x, gb = column sums of dy; tgt: the Linear they belong to, or (gw, gb) scratch
        gw, gb = grads(tgt) if isinstance(tgt, Lin) else tgt
        ex.dw(dy, dy.stride(0), x, x.stride(0), gw, gb, dy.shape[0], gw.shape[0], gw.shape[1])
    run.dw, run.vec = dw, vec

    def put(name, src, pad_from=None):            # a gradient that is a slice of a wider scratch matrix
        # pad_from (flat mode): `src` is the head of that zero-tailed scratch vector (the rows behind it are exact zeros: the products of the
        # zero columns the row kernels pad their 8-column outputs with) and has fewer than 4 elements -- four are copied, so that the copy
        # rides in the one batched fold launch; the extra zeros land in the parameter's alignment gap of the flat buffer (64-element slots)
        if flat is not None:
            n = src.numel()
            if pad_from is not None and n % 4:
                off = flat["offs"][name]
                late.append((flat["g"][off:off + (n + 3) // 4 * 4], pad_from.reshape(-1)[:(n + 3) // 4 * 4]))
            else:
                late.append((fview(name), src))
        else:
            G[name] = src

    # ---- heads
    dev_ = new(B, 24)                                                   # head d in columns 8 d .. 8 d + 3, zeros in 8 d + 4 .. 8 d + 7
    _lib.check(ex.lib.mmdeer_stackb_head_bwd(T["ev"].data_ptr(), 12, g4.contiguous().data_ptr(), dev_.data_ptr(), 24, B, f32, ex.s))
    H0, H3 = T["H0"], T["H3"]
    dH3, dH0, dfused = new(B, 3 * HID // 2), new(B, 3 * HID), new(B, FUS)

    def last_bwd(d):               # d H3 through a head's 128 -> 4 layer, and that layer's gradients (8-row blocks, rows 4..7 zero)
        h3, ev_d = H3[:, d * 128:(d + 1) * 128], dev_[:, 8 * d:8 * d + 8]
        if not chain:
            ex.dx(ev_d, 24, Q.wh6p(d), dH3[:, d * 128:(d + 1) * 128], 3 * HID // 2, B, mask=h3, ldm=3 * HID // 2, mask_scale=sc)
        elif d == 0:               # chain plan: one launch for the three heads (the block-diagonal image of their last layers)
            ex.dx(dev_, 24, Fg.mat("wh6bd"), dH3, 3 * HID // 2, B, mask=H3, ldm=3 * HID // 2, mask_scale=sc)
        w8, b8 = z32(8, 128), z32(8)
        dw(ev_d, h3, (w8, b8))
        put(L.h6[d].prefix + ".weight", w8[:4]); put(L.h6[d].prefix + ".bias", b8[:4])
    # d H0 = d H3 W3 (masked by H0) per head, d fused = d H0 W0 (the stacked first layers)
    run.bwd(dH3, B, [Layer([Part(h, kin=d * (HID // 2), nout_off=d * HID, mask=H0, mcol=d * HID, mscale=sc, before=partial(last_bwd, d),
                                 dw=(dH3[:, d * 128:(d + 1) * 128], H0[:, d * HID:(d + 1) * HID], h)) for d, h in enumerate(L.h3)], out=dH0),
                     Layer((), out=dfused, stacked="wh0")], ts=16)
    gw0, gb0 = z32(3 * HID, FUS), z32(3 * HID)
    dw(dH0, T["fused"], (gw0, gb0))
    for d, h in enumerate(L.h0):
        put(h.prefix + ".weight", gw0[d * HID:(d + 1) * HID]); put(h.prefix + ".bias", gb0[d * HID:(d + 1) * HID])
    # ---- fusion: gate mix, trimodal stage, gate, audio-visual stage
    Tt, R2, Gt = T["T"], T["R2"], T["G"]
    dG, dZ4, dav_a = new(B, FUS), new(B, FUS), new(B, FUS)
    _lib.check(ex.lib.mmdeer_stackb_gate_mix_bwd(dfused.data_ptr(), FUS, Gt.data_ptr(), FUS, R2.data_ptr(), FUS, Tt.data_ptr(), FUS + ENC,
                                                 dG.data_ptr(), FUS, dZ4.data_ptr(), FUS, dav_a.data_ptr(), FUS, B, FUS, f32, ex.s))

    def stage_bwd(recs, dz4, st, inp):
        # d n1 = d z4 W4, LayerNorm backward (masked) -> d z0, d input = d z0 W0 (the weight gradients read dz4 / dz0)
        a1, n1, mean, rstd = st
        r0, r4 = recs
        dz0, din = new(B, FUS), new(B, r0.K)
        run.bwd(dz4, B, [Layer([Part(r4, dw=(dz4, n1, r4))], lnb=(r0, a1, mean, rstd, dz0, sc), dw=[(dz0, inp, r0)]),
                         Layer([Part(r0)], out=din)], ts=16 if r0.K > 512 else 0)
        return din, dz0

    dT, dz0_tri = stage_bwd(L.tri, dZ4, T["tri"], Tt)
    dT2 = ex.dx(dG, FUS, Q.w(L.gate), new(B, FUS + ENC), FUS + ENC, B, wt=Q.wt(L.gate))
    dw(dG, Tt, L.gate)
    dtext = ex.add(new(B, ENC), dT[:, FUS:], dT2[:, FUS:])
    # d av_fused: through the trimodal input, the gate input and the gate mix; av_fused = relu(.)
    tmp = ex.add(new(B, FUS), dT[:, :FUS], dT2[:, :FUS])
    dz4_av = ex.add(new(B, FUS), tmp, dav_a, mask=Tt[:, :FUS], scale=1.0)
    dAV, dz0_av = stage_bwd(L.av, dz4_av, T["av"], T["AV"])
    # ---- attention tail
    a = T["attn_args"]
    dS, dpre = new(3 * B, ENC), new(B, ENC)
    dSX = new(3 * B, 2 * ENC) if chain else None                 # chain plan: [d self | d cross], the input rows of the attention dX run;
    dX = dSX[:, ENC:] if chain else new(3 * B, ENC)              # launch by launch: two dense matrices
    a.ld_dcross = 2 * ENC if chain else 0
    unc8 = new(B, 8) if (flat is not None and not f32 and B >= 2) else None     # the uncertainties as a bf16 GEMM operand (a by-product of the kernel below; both plans of the bf16 fused step)
    a.unc8 = _lib.ptr(unc8)
    dlog8, dz8e, dh2 = new(B, 8), new(3 * B, 8), new(3 * B, ENC // 4)
    a.d_av, a.d_text = dAV.data_ptr(), dtext.data_ptr()
    a.ld_text = ENC                                  # the text gradient is a dense (B, 256) matrix here
    a.d_self, a.d_cross, a.d_pre = dS.data_ptr(), dX.data_ptr(), dpre.data_ptr()
    a.d_logits8, a.d_z8, a.d_h2 = dlog8.data_ptr(), dz8e.data_ptr(), dh2.data_ptr()
    if B:
        _lib.check(ex.lib.mmdeer_stackb_attn_mix_bwd(C.byref(a)))
    t4w, t4b = z32(8, ENC), z32(8)
    dw(dlog8, T["r"], (t4w, t4b))                                                           # weight_network.3 (3 x 256)
    put(L.wn3.prefix + ".weight", t4w[:3]); put(L.wn3.prefix + ".bias", t4b[:3], pad_from=t4b)
    gwn, gbn = grads(L.wn0)
    feat = z32(ENC, 3 * ENC)
    dw(dpre, T["S"].view(B, 3 * ENC), (feat, gbn))
    unc = z32(ENC, 8 if unc8 is not None else 4)
    if unc8 is not None:
        dw(dpre, unc8, (unc, None))
    elif B >= 2:
        dw(dpre, T["u4"], (unc, None))
    else:           # a (1, 4) operand is below the GEMM's 8-element minimum: the same product over two rows, the second zero
        d2, u2 = torch.zeros(2, ENC, dtype=dt, device=dev), z32(2, 4)
        d2[:1].copy_(dpre); u2[:1].copy_(T["u4"])
        dw(d2, u2, (unc, None))
    if flat is not None:
        late.append((gwn[:, :3 * ENC], feat)); late.append((gwn[:, 3 * ENC:], unc[:, :3]))
    else:
        gwn[:, :3 * ENC].copy_(feat); gwn[:, 3 * ENC:].copy_(unc[:, :3])                   # (memory plumbing: two column blocks of one parameter)
    dS_b = ex.dx(dpre, ENC, Q.wn1(), new(B, 3 * ENC), 3 * ENC, B, wt=Q.wn1_t())
    dS_a = dS                                                    # the row kernel's part of d self
    dS = ex.add(dSX[:, :ENC] if chain else new(3 * B, ENC), dS, dS_b.view(3 * B, ENC))
    # uncertainty estimator: its 64 -> 1 layer's gradients, then the two dX products on the 3 B rows
    t4w2, t4b2 = z32(8, ENC // 4), z32(8)
    dw(dz8e, T["H2"], (t4w2, t4b2))
    put(L.e3.prefix + ".weight", t4w2[:1]); put(L.e3.prefix + ".bias", t4b2[:1], pad_from=t4b2)
    E3 = T["E"].view(3 * B, ENC)
    dH1, dE_est = new(3 * B, ENC // 2), new(3 * B, ENC)
    run.bwd(dh2, 3 * B, [Layer([Part(L.e2, mask=T["H1"], mscale=ex.scale_of(run.p_of(L.e1)))], out=dH1), Layer([Part(L.e1)], out=dE_est)])
    dw(dh2, T["H1"], L.e2)
    dw(dH1, E3, L.e1)
    # the two attention blocks: both output-projection dX products (each on its half of the [d self | d cross] rows, the
    # attention-dropout factor of the forward regenerated per (row, head)), then the stacked value projections' dX
    VV = T["VV"]
    dVV, dE_v = new(3 * B, 2 * ENC), new(3 * B, ENC)
    gwv, gbv = z32(2 * ENC, ENC), z32(2 * ENC)
    run.bwd(dSX, 3 * B, [Layer([Part(L.os, x=dS, regen=L.vs), Part(L.oc, x=dX, regen=L.vc, kin=ENC, nout_off=ENC)], out=dVV,
                               dw=[(dS, VV[:, :ENC], L.os), (dX, VV[:, ENC:], L.oc), (dVV, E3, (gwv, gbv))]),
                         Layer((), out=dE_v, stacked="wv")])
    for i, v in enumerate((L.vs, L.vc)):
        put(v.prefix + ".weight", gwv[i * ENC:(i + 1) * ENC]); put(v.prefix + ".bias", gbv[i * ENC:(i + 1) * ENC])
        # one key per query: the softmax is the constant 1, so query / key projections get exact zeros (as autograd gives;
        # in flat mode their slices of the gradient buffer are never written and keep the zeros it was created with)
        if flat is None:
            for q in ("query_proj", "key_proj"):
                blk = v.prefix.rsplit(".", 1)[0]
                G[f"{blk}.{q}.weight"], G[f"{blk}.{q}.bias"] = z32(ENC, ENC), z32(ENC)
    dE = ex.add(new(3 * B, ENC), dE_v, dE_est).view(B, 3 * ENC)
    # ---- encoders: dh = dE W_out, then per residual block (top down) dz = LayerNorm'(dh) masked, dh += dz W, and the stem's
    # LayerNorm backward at the end; the weight gradients read the stored dz / h rows
    denc = []
    for m, (t, e) in enumerate(zip(T["enc"], L.enc)):
        dEm = dE[:, m * ENC:(m + 1) * ENC]
        hs, nres = t["h"], len(e.res)
        layers, part, dzs = [], Part(e.out, dw=(dEm, hs[-1], e.out), res_dup=int(nres > 0)), []
        for l in reversed(range(nres)):
            dz = new(B, ENC)
            layers.append(Layer([part], lnb=(e.res[l], t["y"][l], *t["st"][l], dz, sc), dw=[(dz, hs[l], e.res[l])]))
            dzs.append(dz)
            part = Part(e.res[l], res_add=1, res_dup=int(l > 0))
        dz0 = new(B, ENC)
        layers.append(Layer([part], lnb=(e.stem, t["y0"], t["m0"], t["r0"], dz0, 1.0), dw=[(dz0, t["xin"], e.stem)]))
        run.bwd(dEm, B, layers)
        denc.append({"dz": dzs[::-1], "dz0": dz0})               # dz[l]: of residual block l
    if keep:
        T["bwd"] = dict(dev_=dev_, dH3=dH3, dH0=dH0, dfused=dfused, dG=dG, dZ4=dZ4, dav_a=dav_a, dz0_tri=dz0_tri, dT=dT, dT2=dT2, dtext=dtext,
                        tmp=tmp, dz4_av=dz4_av, dz0_av=dz0_av, dAV=dAV, dS_a=dS_a, dX=dX, dpre=dpre, dlog8=dlog8, dz8e=dz8e, dh2=dh2, unc8=unc8,
                        dS_b=dS_b, dS=dS, dH1=dH1, dE_est=dE_est, dVV=dVV, dE_v=dE_v, dE=dE, enc=denc)
    if flat is not None:
        ex.flush_dw()
        ex.deferred = None
        for dst, src in late:      # after the weight-gradient launches; dense runs ride in the one fold launch below
            ex.copy1d(dst, src)
        ex.flush_folds()
        ex.folds = None
    return G
