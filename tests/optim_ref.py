"""float64 restatement of the fused optimiser step (mmdeer_adamw_step) and numpy decoders of the packed-parameter buffer it shares
with mmdeer_pack_weights, written from the formulas alone: the mmdeer_adamw_args comment of include/mmdeer.h, torch.optim.AdamW and
clip_grad_norm_ for the arithmetic; include/mmdeer.h, the comments of csrc/layout.inc and the index formulas of csrc/chain.h for the
images.  Nothing here reads the library's tables: the geometry (rows, columns, flat offsets, field offsets) comes in through the
public look-ups, the list of which parameter has which image is stated below from the layer structure.

The comparison: |got - ref| <= K * U * magnitude per element, U = 2^-24, magnitude = the sum of the |terms| the
value is made of.  An element of magnitude 0 must match exactly.  K per family is twice the worst ratio of adamw_step_f32 -- the same
operation order in numpy float32 -- against adamw_step_ref over the cases below (tests/test_cpu_optim_ref.py measures it).
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
F64 = torch.float64
POW_ULPS = 1.0          # allowance for the host's powf(beta, step): this many ulps of beta^step (glibc documents 1 ulp)
CLIP_EPS = float(np.float32(1e-6))

# twice the worst float32 CPU ratio per family (test_cpu_optim_ref.py asserts the tie; DESIGN.md section 16 has the measured figures)
K = {"norm": 1.93, "p": 10.45, "exp_avg": 5.22, "exp_avg_sq": 8.88}


# ============================================================================ geometry
class Geometry:
    """The canonical parameter table as the public look-ups give it."""

    def __init__(self, lib):
        n = lib.mmdeer_num_params()
        self.names = [lib.mmdeer_param_name(i).decode() for i in range(n)]
        self.rows = [lib.mmdeer_param_rows(i) for i in range(n)]
        self.cols = [lib.mmdeer_param_cols(i) for i in range(n)]
        self.off = [lib.mmdeer_param_offset(i) for i in range(n)]
        self.flat = lib.mmdeer_flat_elems()
        self.n = n
        self.numel = [r * c for r, c in zip(self.rows, self.cols)]
        self.is_matrix = [c > 1 for c in self.cols]
        mask = np.zeros(self.flat, dtype=bool)
        pid = np.full(self.flat, -1, dtype=np.int64)
        for i in range(n):
            assert not mask[self.off[i]:self.off[i] + self.numel[i]].any()
            mask[self.off[i]:self.off[i] + self.numel[i]] = True
            pid[self.off[i]:self.off[i] + self.numel[i]] = i
        self.mask, self.pid = mask, pid

    def index(self, name):
        return self.names.index(name)

    def sl(self, i):
        return slice(self.off[i], self.off[i] + self.numel[i])

    def per_element(self, values):
        """one value per parameter -> one per flat element (0 in the gaps)"""
        v = np.asarray(values, dtype=np.float64)
        assert v.shape == (self.n,)
        return np.where(self.mask, v[np.maximum(self.pid, 0)], 0.0)

    def weights_fields(self, lib, f32):
        """field -> byte offset, and the buffer's size under 'bytes'"""
        W = {f: lib.mmdeer_weights_offset(f32, f.encode()) for f in FIELDS}
        assert all(o >= 0 for o in W.values())
        W["bytes"] = lib.mmdeer_weights_bytes(f32)
        return W


FIELDS = ("wpack", "wtpack", "vpack", "wa_pad", "wqkv_hm", "wscratch", "wfpack", "wtfpack", "wa_frag")


def f32(x):
    return float(np.float32(x))


# ============================================================================ the step in float64
def adamw_step_ref(G, p, g, m, v, lr_per_param, step, beta1, beta2, eps, wd, max_norm, grad_scale, norm=None):
    """clip_grad_norm_(max_norm) of grad_scale * g over the parameters, then torch.optim.AdamW (decoupled decay).  p, g, m, v: flat
    tensors of G.flat elements (any device / float dtype); elements in the gaps between parameters are neither read nor changed.
    Scalars enter as the float32 values the library receives; bias corrections exactly in float64.  norm: None, or the norm to
    derive the clip factor from (teacher forcing with the kernel's own norm).  Returns p, exp_avg, exp_avg_sq, norm and the
    magnitudes mag_p, mag_exp_avg, mag_exp_avg_sq (float64)."""
    dev = p.device
    p, g, m, v = (t.to(F64) for t in (p, g, m, v))
    mask = torch.from_numpy(G.mask).to(dev)
    lr = torch.from_numpy(G.per_element([f32(x) for x in lr_per_param])).to(dev)
    b1, b2, eps, wd, gs, mx = f32(beta1), f32(beta2), f32(eps), f32(wd), f32(grad_scale), f32(max_norm)
    omb1, omb2 = float(np.float32(1) - np.float32(beta1)), float(np.float32(1) - np.float32(beta2))    # exact for beta in [0.5, 1)
    pw1, pw2 = b1 ** step, b2 ** step
    bc1, bc2 = 1.0 - pw1, 1.0 - pw2
    gz = torch.where(mask, g, torch.zeros_like(g))
    norm_ref = abs(gs) * math.sqrt(float((gz * gz).sum()))
    n = norm_ref if norm is None else float(norm)
    clip = min(1.0, mx / (n + CLIP_EPS)) if mx > 0 else 1.0
    g1 = gz * (gs * clip)
    t_m, t_g = b1 * m, omb1 * g1
    m1 = t_m + t_g
    v1 = b2 * v + omb2 * g1 * g1
    den = v1.sqrt() / math.sqrt(bc2) + eps
    decay = 1.0 - lr * wd
    p1 = p * decay - (lr / bc1) * m1 / den
    mag_m = t_m.abs() + t_g.abs()
    # the fp32 bias corrections: POW_ULPS ulps (2 U relative each) of beta^step, divided by the correction; sqrt halves the second
    extra = 2.0 * POW_ULPS * (pw1 / bc1 + 0.5 * pw2 / bc2)
    mag_p = (p * decay).abs() + (lr / bc1) * mag_m / den * (1.0 + extra)
    z = torch.zeros_like(p)
    return {"p": torch.where(mask, p1, p), "exp_avg": torch.where(mask, m1, m), "exp_avg_sq": torch.where(mask, v1, v),
            "norm": norm_ref, "mag_p": torch.where(mask, mag_p, z), "mag_exp_avg": torch.where(mask, mag_m, z),
            "mag_exp_avg_sq": torch.where(mask, v1, z)}


def ratio(got, ref, mag):
    """worst |got - ref| / (U * magnitude); inf where a value of magnitude 0 is not matched exactly, or is not finite"""
    got, ref, mag = (torch.as_tensor(t, dtype=F64) for t in (got, ref, mag))
    err = (got.to(ref.device) - ref).abs()
    r = torch.where(mag > 0, err / (U * mag), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf)))
    r = torch.where(torch.isnan(r), torch.full_like(r, math.inf), r)
    return float(r.max())


def ratios(got, ref):
    """got: p, exp_avg, exp_avg_sq (flat), norm; ref: what adamw_step_ref returned.  The norm is compared with ref's own norm."""
    out = {f: ratio(got[f], ref[f], ref["mag_" + f]) for f in ("p", "exp_avg", "exp_avg_sq")}
    out["norm"] = ratio(float(got["norm"]), ref["norm"], ref["norm"])
    return out


def rejects(got, ref, k=None):
    k = K if k is None else k
    return any(r > k[f] for f, r in ratios(got, ref).items())


# ============================================================================ the same operation order in numpy float32
VARIANTS = ("lr0_all", "lr_stack_first", "norm_no_scale", "sign_lost", "clip_no_1e6", "l2_decay", "eps_in_sqrt", "eps_not_bc2",
            "bc_swapped", "step_minus_1", "m_unscaled")
STACKED_HEADS = tuple(f"head.deer_heads.{h}.evidence_net.0.weight" for h in range(3))


def sumsq_f32(g, mask):
    """sum of squares in float32 in the shape of the library's pass: 4-element chunks, 65536 strided serial accumulators, a pairwise tree"""
    f = np.float32
    x = np.where(mask, g, f(0)).astype(f).reshape(-1, 4)
    s = (x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + (x[:, 2] * x[:, 2] + x[:, 3] * x[:, 3])
    nthr = 65536
    s = np.concatenate([s, np.zeros(-len(s) % nthr, dtype=f)]).reshape(-1, nthr)
    acc = np.zeros(nthr, dtype=f)
    for row in s:
        acc = acc + row
    while len(acc) > 1:
        acc = acc[0::2] + acc[1::2]
    return acc[0]


def adamw_step_f32(G, p, g, m, v, lr_per_param, step, beta1, beta2, eps, wd, max_norm, grad_scale, variant=None):
    """The update as adamw_update4 (csrc/optim.hip) states it: separate float32 operations, no contraction; the norm in the shape of the
    library's two-level sum.  Measures the rounding constants and carries the seeded errors (variant) -- never the expected value."""
    f = np.float32
    assert variant is None or variant in VARIANTS
    p, g, m, v = (np.asarray(t, dtype=f) for t in (p, g, m, v))
    lrp = np.asarray(lr_per_param, dtype=f).copy()
    if variant == "lr0_all":
        lrp[:] = lrp[0]
    if variant == "lr_stack_first":
        for name in STACKED_HEADS[1:]:
            lrp[G.index(name)] = lrp[G.index(STACKED_HEADS[0])]
    lr = np.where(G.mask, lrp[np.maximum(G.pid, 0)], f(0)).astype(f)
    b1, b2, eps, wd, gs, mx = f(beta1), f(beta2), f(eps), f(wd), f(grad_scale), f(max_norm)
    t = step - 1 if variant == "step_minus_1" else step
    bc1, bc2 = f(1) - f(float(b1) ** t), f(1) - f(float(b2) ** t)          # powf correctly rounded; the bound allows POW_ULPS
    if variant == "bc_swapped":
        bc1, bc2 = bc2, bc1
    with np.errstate(all="ignore"):
        norm = np.sqrt(sumsq_f32(g, G.mask)) * (f(1) if variant == "norm_no_scale" else np.abs(gs))
        den_c = norm if variant == "clip_no_1e6" else norm + f(1e-6)
        clip = np.minimum(f(1), mx / den_c) if mx > 0 else f(1)
        kgs = clip * (np.abs(gs) if variant == "sign_lost" else gs)
        ibc1, isbc2 = f(1) / bc1, f(1) / np.sqrt(bc2)
        g0 = np.where(G.mask, g, f(0)).astype(f)
        g1 = g0 * kgs
        if variant == "l2_decay":
            g1 = g1 + wd * p
            p1 = p.copy()
        else:
            p1 = p * (f(1) - lr * wd)
        m1 = m * b1 + (g0 if variant == "m_unscaled" else g1) * (f(1) - b1)
        v1 = v * b2 + g1 * g1 * (f(1) - b2)
        st = lr * ibc1
        if variant == "eps_in_sqrt":
            den = np.sqrt(v1 * isbc2 * isbc2 + eps)
        elif variant == "eps_not_bc2":
            den = (np.sqrt(v1) + eps) * isbc2
        else:
            den = np.sqrt(v1) * isbc2 + eps
        p1 = p1 - st * m1 / den
    for a in (p1, m1, v1):
        assert a.dtype == f
    return {"p": np.where(G.mask, p1, p), "exp_avg": np.where(G.mask, m1, m), "exp_avg_sq": np.where(G.mask, v1, v), "norm": float(norm)}


# ============================================================================ the cases of tests/test_gpu_optim_step.py
BETA1, BETA2, EPS = 0.9, 0.999, 1e-8
# name, step, weight_decay, grad_scale, clipping (max_norm as a multiple of the reference norm; 0 and -1: off), gradient draw
CASES = (
    ("s1", 1, 0.01, 1.0, 0.5, "wide"),
    ("s2", 2, 0.0, 0.25, 4.0, "wide"),
    ("s1000", 1000, 0.01, -0.5, 0.0, "wide"),
    ("s100000", 100000, 0.0, 1.0, 0.5, "wide"),
    ("s2b", 2, 0.01, -0.5, 0.5, "wide"),
    ("s1000b", 1000, 0.0, 0.25, -1.0, "wide"),
    ("s100000b", 100000, 0.01, -0.5, 4.0, "wide"),
    # a norm near the 1e-6 of the clip factor: only here does that constant show
    ("tiny", 3, 0.01, 0.25, 0.5, "tiny"),
    # all-zero gradient at step 1: norm exactly 0, clip factor min(1, max / 1e-6) = 1, the parameters only decay
    ("zero", 1, 0.01, 1.0, 1.0, "zero"),
)
CASE_NAMES = tuple(c[0] for c in CASES)
AV_IN_PROJ = "fusion.audio_visual_fusion.cross_attention.in_proj_weight"
GAP_M, GAP_V = 5.0, 6.0          # what the gaps of the flat moment buffers hold: nobody may write there


def learning_rates(G):
    return [f32(1e-3 * (1 + i / 64)) for i in range(G.n)]


def case_inputs(G, name):
    """Flat float32 p, g, exp_avg, exp_avg_sq of a case and its hyper-parameters.  Parameters O(1) with exact zeros; gradient
    magnitudes log-uniform over 1e-10 .. 1e2 (tiny: 1e-12 .. 1e-7), so eps = 1e-8 matters in a visible share of the elements; the q/k
    rows of the AV in_proj gradient exactly zero, as the backward leaves them; moments zero at step 1, else drawn (v >= 0)."""
    i = CASE_NAMES.index(name)
    _, step, wd, gs, clip, draw = CASES[i]
    rng = np.random.default_rng(1000 + i)
    n = G.flat
    p = rng.standard_normal(n).astype(np.float32)
    p[rng.random(n) < 0.01] = 0.0
    lo, hi = {"wide": (-10.0, 2.0), "tiny": (-12.0, -7.0), "zero": (-10.0, 2.0)}[draw]
    mag = lambda: (10.0 ** rng.uniform(lo, hi, n)) * np.where(rng.random(n) < 0.5, -1.0, 1.0)
    g = mag().astype(np.float32)
    if draw == "zero":
        g[:] = 0.0
    a = G.index(AV_IN_PROJ)
    g[G.off[a]:G.off[a] + 2 * (G.rows[a] // 3) * G.cols[a]] = 0.0
    if step == 1:
        m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    else:
        m = mag().astype(np.float32)
        v = (mag() ** 2).astype(np.float32)
    for t, gap in ((p, 0.0), (g, 0.0), (m, GAP_M), (v, GAP_V)):
        t[~G.mask] = gap
    norm = abs(gs) * math.sqrt(float((g.astype(np.float64)[G.mask] ** 2).sum()))
    hyper = dict(step=step, beta1=BETA1, beta2=BETA2, eps=EPS, wd=wd, max_norm=f32(clip * norm) if clip > 0 and norm > 0 else clip, grad_scale=gs)
    return p, g, m, v, hyper


# ============================================================================ the weights buffer
def bf16_rne(x):
    """float32 -> bf16 bits (uint16), round to nearest even (finite inputs)"""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def frag(M):
    """fragment-major order (csrc/chain.h) of a [16 a][64 b] matrix: 16-byte granule ((wt * (K / 64) + kt) * 2 + c) * 64 + lane holds
    M[16 wt + (lane & 15)][64 kt + 32 c + 8 (lane >> 4) .. + 8)"""
    R, Kc = M.shape
    assert R % 16 == 0 and Kc % 64 == 0
    out = np.zeros(R * Kc, dtype=M.dtype)
    for wt in range(R // 16):
        for kt in range(Kc // 64):
            for c in range(2):
                for lane in range(64):
                    l = ((wt * (Kc // 64) + kt) * 2 + c) * 64 + lane
                    r, k0 = 16 * wt + (lane & 15), 64 * kt + 32 * c + 8 * (lane >> 4)
                    out[8 * l:8 * l + 8] = M[r, k0:k0 + 8]
    return out


def frag_fast(M):
    """frag() as one transpose: [wt][r][kt][c][q][e] -> [wt][kt][c][q][r][e], lane = 16 q + r"""
    R, Kc = M.shape
    assert R % 16 == 0 and Kc % 64 == 0
    return np.ascontiguousarray(M.reshape(R // 16, 16, Kc // 64, 2, 4, 8).transpose(0, 2, 3, 4, 1, 5)).reshape(-1)


def unfrag(flat, R, Kc):
    return np.ascontiguousarray(np.asarray(flat).reshape(R // 16, Kc // 64, 2, 4, 16, 8).transpose(0, 4, 1, 2, 3, 5)).reshape(R, Kc)


def head_major_rows():
    """wqkv_hm: row 192 h + 96 wn + 32 part + dd takes row 512 part + 64 h + 32 wn + dd of the [1536][512] in_proj; returns src[dst]"""
    src = np.empty(1536, dtype=np.int64)
    for part in range(3):
        for h in range(8):
            for wn in range(2):
                for dd in range(32):
                    src[192 * h + 96 * wn + 32 * part + dd] = 512 * part + 64 * h + 32 * wn + dd
    return src


# Which images each parameter has, from the layer structure (the comment above the image table of csrc/stackc.hip):
#   every matrix: row-major in wpack; every vector: vpack.  Besides that
#   frag   the forward chains stream the matrix: fragment-major image of S in wfpack at S's flat offset
#   fragT  a dX chain runs through it: fragment-major image of S^T in wtfpack at S's flat offset
#   wt     a dX GEMM multiplies by W^T: [cols][wt_ld] in wtpack at the flat offset of the matrix the rows belong to
#   pad    the 84-wide audio weight as [256][128] (wa_pad) and the fragment-major image of that (wa_frag)
#   hm     the trimodal in_proj in head-major row order (wqkv_hm)
# rows: (first, count) or None = all; S: (first parameter, first row, rows) the kernels read as one matrix; wt: (parameter, ld).
_AV, _TRI, _HD = "fusion.audio_visual_fusion.", "fusion.trimodal_fusion.", "head."
_CHAIN = ("frag", "fragT", "wt")


def image_table(variant=None):
    """variant: a seeded wrong table for the round-trip test ('v_at_row_0', 'stack_reversed', 'wt_col_dropped')"""
    T = []

    def add(name, kinds, rows=None, S=None, wt=None, s_row=None, wt_col=None):       # s_row / wt_col: None = where the flat offsets put the range
        T.append(dict(name=name, kinds=tuple(kinds), rows=rows, S=S, wt=wt, s_row=s_row, wt_col=wt_col))
    add(_AV + "audio_projection.weight", ("pad",))                                  # an input projection: no dX
    add(_AV + "video_projection.weight", ("frag",))
    # the AV in_proj [q; k; v] with one key per query: only the value rows are multiplied by -- a [256][256] chain matrix of their own;
    # the q / k rows exist in W^T [256][768] alone
    inp = _AV + "cross_attention.in_proj_weight"
    add(inp, ("wt",), rows=(0, 512), wt=(inp, 768))
    add(inp, _CHAIN, rows=(0 if variant == "v_at_row_0" else 512, 256), S=(inp, 0 if variant == "v_at_row_0" else 512, 256), wt=(inp, 768),
        wt_col=0 if variant == "wt_col_dropped" else None)
    for n in ("cross_attention.out_proj.weight", "fusion_layers.0.weight"):
        add(_AV + n, _CHAIN)
    add(_TRI + "audiovisual_projection.weight", _CHAIN)
    add(_TRI + "text_projection.weight", ("frag",))
    add(_TRI + "modality_attention.in_proj_weight", ("hm", "wt"))
    for n in (_TRI + "modality_attention.out_proj.weight", _TRI + "final_fusion.0.weight", "fusion.output_projection.0.weight",
              _HD + "feature_processor.0.weight", _HD + "feature_processor.3.weight"):
        add(n, _CHAIN)
    first = _HD + "deer_heads.0.evidence_net.0.weight"                              # the three first head layers: one [384][256] S
    order = (2, 1, 0) if variant == "stack_reversed" else (0, 1, 2)
    for slot, h in enumerate(order):
        wrong = dict(s_row=128 * slot, wt_col=128 * slot) if variant == "stack_reversed" else {}
        add(_HD + f"deer_heads.{h}.evidence_net.0.weight", _CHAIN, S=(first, 0, 384), wt=(first, 384), **wrong)
    for h in range(3):
        add(_HD + f"deer_heads.{h}.evidence_net.3.weight", _CHAIN)                  # each on its own; evidence_net.6: wpack only
    return T


def _resolve(G, e):
    """-> pid, row0, rows, cols, S flat offset, the range's first row in S, S rows, W^T flat offset, ld, first column"""
    i = G.index(e["name"])
    row0, rows = e["rows"] or (0, G.rows[i])
    cols = G.cols[i]
    off = G.off[i] + row0 * cols
    sname, srow0, srows = e["S"] or (e["name"], 0, G.rows[i])
    s_off = G.off[G.index(sname)] + srow0 * cols
    wname, ld = e["wt"] or (e["name"], G.rows[i])
    w_off = G.off[G.index(wname)]
    wt_col = e["wt_col"] if e["wt_col"] is not None else (off - w_off) // cols
    s_row = e["s_row"] if e["s_row"] is not None else (off - s_off) // cols
    return i, row0, rows, cols, s_off, s_row, srows, w_off, ld, wt_col


def expected_weights(G, W, params, compute_f32, background, pack_transposed=True, table=None):
    """The bytes of the weights buffer after a pack of `params` (flat float32, G.flat elements) over `background` (uint8, at least
    W['bytes'] long; a copy is returned).  pack_transposed = False: the wtpack / wtfpack fields are left alone.  wscratch is not
    written here: compare it separately."""
    out = np.array(background, dtype=np.uint8, copy=True)
    es = 4 if compute_f32 else 2
    P = np.ascontiguousarray(params, dtype=np.float32)
    Q = P.view(np.uint32) if compute_f32 else bf16_rne(P)                           # the matrices in the compute dtype

    def put(field, elem, arr, size=es):
        b = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        lo = W[field] + elem * size
        out[lo:lo + b.size] = b

    for i in range(G.n):
        if G.is_matrix[i]:
            put("wpack", G.off[i], Q[G.sl(i)])
        else:
            put("vpack", G.off[i], P[G.sl(i)], 4)
    stacks = {}
    for e in (image_table() if table is None else table):
        i, row0, rows, cols, s_off, s_row, srows, w_off, ld, wt_col = _resolve(G, e)
        M = Q[G.off[i] + row0 * cols:G.off[i] + (row0 + rows) * cols].reshape(rows, cols)
        if "wt" in e["kinds"] and pack_transposed:                                  # [cols][ld], this range's rows as columns wt_col ..
            lo = W["wtpack"] + w_off * es
            view = out[lo:lo + cols * ld * es].view(Q.dtype).reshape(cols, ld)
            view[:, wt_col:wt_col + rows] = M.T
        if compute_f32:
            continue
        if "frag" in e["kinds"] or "fragT" in e["kinds"]:
            S = stacks.setdefault(s_off, (np.zeros((srows, cols), dtype=Q.dtype), e["kinds"]))[0]
            S[s_row:s_row + rows] = M
        if "pad" in e["kinds"]:
            Pd = np.zeros((rows, 128), dtype=Q.dtype)
            Pd[:, :cols] = M
            put("wa_pad", 0, Pd)
            put("wa_frag", 0, frag_fast(Pd))
        if "hm" in e["kinds"]:
            put("wqkv_hm", 0, M[head_major_rows()])
    for s_off, (S, kinds) in stacks.items():
        if "frag" in kinds:
            put("wfpack", s_off, frag_fast(S))
        if "fragT" in kinds and pack_transposed:
            put("wtfpack", s_off, frag_fast(np.ascontiguousarray(S.T)))
    return out


def decode_weights(G, W, buf, compute_f32, table=None):
    """Every image of every parameter read back out of the buffer, in W's own orientation and the compute dtype's bits:
    {(kind, parameter name, first row): [rows][cols]}; vectors under ('vpack', name, 0) as float32 bits."""
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    es, dt = (4, np.uint32) if compute_f32 else (2, np.uint16)

    def get(field, elem, count, size=es, dtype=dt):
        lo = W[field] + elem * size
        return buf[lo:lo + count * size].view(dtype)

    out = {}
    for i in range(G.n):
        if G.is_matrix[i]:
            out[("wpack", G.names[i], 0)] = get("wpack", G.off[i], G.numel[i]).reshape(G.rows[i], G.cols[i])
        else:
            out[("vpack", G.names[i], 0)] = get("vpack", G.off[i], G.numel[i], 4, np.uint32).reshape(G.rows[i], 1)
    for e in (image_table() if table is None else table):
        i, row0, rows, cols, s_off, s_row, srows, w_off, ld, wt_col = _resolve(G, e)
        key = lambda kind: (kind, e["name"], row0)
        if "wt" in e["kinds"]:
            out[key("wt")] = get("wtpack", w_off, cols * ld).reshape(cols, ld)[:, wt_col:wt_col + rows].T
        if compute_f32:
            continue
        if "frag" in e["kinds"]:
            out[key("frag")] = unfrag(get("wfpack", s_off, srows * cols), srows, cols)[s_row:s_row + rows]
        if "fragT" in e["kinds"]:
            out[key("fragT")] = unfrag(get("wtfpack", s_off, srows * cols), cols, srows).T[s_row:s_row + rows]
        if "pad" in e["kinds"]:
            out[key("pad")] = get("wa_pad", 0, rows * 128).reshape(rows, 128)
            out[key("pad_frag")] = unfrag(get("wa_frag", 0, rows * 128), rows, 128)
        if "hm" in e["kinds"]:
            inv = np.empty(1536, dtype=np.int64)
            inv[head_major_rows()] = np.arange(1536)
            out[key("hm")] = get("wqkv_hm", 0, rows * cols).reshape(rows, cols)[inv]
    return out


def expected_images(G, params, compute_f32, table=None):
    """what decode_weights must return after a pack of params: the rows of each range, rounded to the compute dtype"""
    P = np.ascontiguousarray(params, dtype=np.float32)
    Q = P.view(np.uint32) if compute_f32 else bf16_rne(P)
    want = {}
    for i in range(G.n):
        if G.is_matrix[i]:
            want[("wpack", G.names[i], 0)] = Q[G.sl(i)].reshape(G.rows[i], G.cols[i])
        else:
            want[("vpack", G.names[i], 0)] = P.view(np.uint32)[G.sl(i)].reshape(G.rows[i], 1)
    for e in image_table():                                    # always the true table: a seeded wrong decoder is judged against it
        i = G.index(e["name"])
        row0, rows = e["rows"] or (0, G.rows[i])
        M = Q[G.off[i] + row0 * G.cols[i]:G.off[i] + (row0 + rows) * G.cols[i]].reshape(rows, G.cols[i])
        for kind in e["kinds"]:
            if kind != "wt" and compute_f32:
                continue
            if kind == "pad":
                Pd = np.zeros((rows, 128), dtype=Q.dtype)
                Pd[:, :G.cols[i]] = M
                want[("pad", e["name"], row0)] = want[("pad_frag", e["name"], row0)] = Pd
            else:
                want[(kind, e["name"], row0)] = M
    return want


def crafted_parameters(G, seed=5):
    """random values, fp32 values exactly halfway between two bf16 neighbours (even and odd upper halves), +-0, fp32 denormals and the
    largest finite fp32, spread over every parameter"""
    rng = np.random.default_rng(seed)
    bits = rng.standard_normal(G.flat).astype(np.float32).view(np.uint32).copy()
    kind = rng.integers(0, 16, G.flat)
    hi = rng.integers(0x3000, 0x4800, G.flat).astype(np.uint32)                     # upper halves of ordinary magnitudes
    sign = (rng.integers(0, 2, G.flat).astype(np.uint32) << 31)
    bits = np.where(kind == 0, ((hi & ~np.uint32(1)) << 16) | 0x8000 | sign, bits)  # a tie under an even upper half: rounds down
    bits = np.where(kind == 1, ((hi | np.uint32(1)) << 16) | 0x8000 | sign, bits)   # ... under an odd one: rounds up
    bits = np.where(kind == 2, sign, bits)                                          # +-0
    bits = np.where(kind == 3, rng.integers(1, 0x800000, G.flat).astype(np.uint32) | sign, bits)   # fp32 denormals
    bits = np.where(kind == 4, np.uint32(0x7F7FFFFF) | sign, bits)                  # the largest finite fp32
    bits = np.where(kind == 5, ((hi << 16) | 0x8001 | sign), bits)                  # just above a tie
    p = bits.astype(np.uint32).view(np.float32).copy()
    p[~G.mask] = 0.0
    return p


def background(nbytes):
    """a byte pattern that is no plausible bf16 / fp32 value of the data: 0xA5 0x5A ... (bf16 0x5AA5 ~ 2.3e16, 0xA55A ~ -1.9e-16)"""
    b = np.empty(nbytes, dtype=np.uint8)
    b[0::2], b[1::2] = 0xA5, 0x5A
    return b
