"""float64 restatements of the row kernels: LayerNorm (csrc/rowops.hip, csrc/ln_rows.h), the trimodal 2-token attention
(csrc/attention.hip), the side rows (csrc/side.hip: CrossModalAttention core, the T = 1 LSTM cell), mmdeer_convert and the dropout draw
(csrc/common.h, make_drop of csrc/api.hip), and the in_proj + attention of csrc/tri_fused.hip in stages (projection, clamped softmax of
the stored q and k, context, backward).  Written from the formulas in plain torch / numpy: nothing here calls the library or oracle/.

Every value comes with a *scale* (DESIGN.md section 13): the sum of the absolute values of the pieces that are added to form it,
carried through the formula by the class SV below -- a sum's scale is the sum of its pieces' scales plus the sum of their absolute
values, a product's is |a| scale(b) + scale(a) |b| + |a b|, a function's is |f'| scale(a) + |f(a)|; an input is exact (scale 0).
So a value that is a small difference of large pieces (a row of mean 1000 and spread 1) has the scale of the pieces, and a value
that is exactly zero by construction (a masked dz, the LSTM's forget block) has scale 0 and must be matched exactly.  Each operation
also adds TINY = 2^-102 (2^-24 TINY = 2^-126, the smallest normal float32: below it float32 has absolute precision only).

Comparison (assert_close):  fp32 outputs |got - ref| <= K 2^-24 scale;  bf16-stored outputs that bound and one rounding to bf16, stated
exactly: the reference must lie within K 2^-24 scale (+ 2^-126) of the interval of reals that round to the stored bf16 number.  The formulas are written once, for a dtype: float64 is the reference, float32 on the CPU measures K (tests/test_cpu_rowkernel_ref.py).
`variant` seeds one deliberate error (the CPU test shows that the comparison rejects each)."""
import numpy as np
import torch

EPS24 = 2.0 ** -24
TINY = 2.0 ** -102
F64 = torch.float64


# =========================================================================== values with scales
class SV:
    """value v and scale s (same shape)."""
    __slots__ = ("v", "s")

    def __init__(self, v, s=None):
        self.v = v
        self.s = torch.zeros_like(v) if s is None else s

    @staticmethod
    def _own(v):
        return v.abs() + TINY

    def __add__(self, o):
        v = self.v + o.v
        return SV(v, self.s + o.s + SV._own(v))

    def __sub__(self, o):
        v = self.v - o.v
        return SV(v, self.s + o.s + SV._own(v))

    def __mul__(self, o):
        v = self.v * o.v
        return SV(v, self.v.abs() * o.s + self.s * o.v.abs() + SV._own(v))

    def __truediv__(self, o):
        v = self.v / o.v
        return SV(v, self.s / o.v.abs() + self.v.abs() * o.s / (o.v * o.v) + SV._own(v))

    def mulc(self, c):          # times a constant
        v = self.v * c
        return SV(v, self.s * abs(c) + SV._own(v))

    def addc(self, c):
        v = self.v + c
        return SV(v, self.s + SV._own(v))

    def rsubc(self, c):         # c - self
        v = c - self.v
        return SV(v, self.s + SV._own(v))

    def sum(self, dim, keepdim=False):
        return SV(self.v.sum(dim, keepdim), self.s.sum(dim, keepdim) + self.v.abs().sum(dim, keepdim) + TINY)

    def max(self, dim):         # keepdim; the scale of the element that is the maximum
        v, i = self.v.max(dim, keepdim=True)
        return SV(v, self.s.gather(dim, i))

    def fn(self, f, df):
        v = f(self.v)
        return SV(v, df(self.v, v).abs() * self.s + SV._own(v))

    def exp(self):
        return self.fn(torch.exp, lambda x, y: y)

    def tanh(self):
        return self.fn(torch.tanh, lambda x, y: 1 - y * y)

    def sigmoid(self):
        return self.fn(torch.sigmoid, lambda x, y: y * (1 - y))

    def rsqrt(self):
        return self.fn(lambda x: 1.0 / torch.sqrt(x), lambda x, y: -0.5 * y / x)

    def where(self, cond):      # cond ? self : exact 0
        z = torch.zeros_like(self.v)
        return SV(torch.where(cond, self.v, z), torch.where(cond, self.s, z))

    def reshape(self, *shape):
        return SV(self.v.reshape(*shape), self.s.reshape(*shape))

    def __getitem__(self, idx):
        return SV(self.v[idx], self.s[idx])


def leaf(x, dt=F64):
    return SV(torch.as_tensor(x).to(dt))


def cat(svs, dim):
    return SV(torch.cat([a.v for a in svs], dim), torch.cat([a.s for a in svs], dim))


def stack(svs, dim):
    return SV(torch.stack([a.v for a in svs], dim), torch.stack([a.s for a in svs], dim))


def bf16_round(x):
    return x.to(torch.bfloat16).to(torch.float32)


# =========================================================================== comparison
def bf16_cell(got):
    """[lo, hi] (float64): the reals that round to nearest to the bf16 number `got` -- half way to its two bf16 neighbours."""
    b = got.to(torch.bfloat16).view(torch.int16).to(torch.int32) & 0xFFFF
    key = torch.where(b < 0x8000, b, 0x8000 - b)                       # monotone in the value; -0 and +0 coincide

    def value(k):
        bits = torch.where(k >= 0, k, 0x8000 - k)
        return torch.where(bits >= 0x8000, bits - 0x10000, bits).to(torch.int16).view(torch.bfloat16).to(F64)
    g = got.to(F64)
    return (g + value(key - 1)) / 2, (g + value(key + 1)) / 2


def assert_close(name, got, ref: SV, K, bf16=False, log=None):
    """fp32 output: |got - ref| <= K 2^-24 scale.  bf16-stored output: that bound and ONE rounding to bf16 -- some real x with
    |x - ref| <= K 2^-24 scale + 2^-126 rounds to `got`, i.e. ref is no farther than that from the cell of reals that round to
    `got` (bf16 keeps 8 significant bits: the cell reaches up to 2^-8 |got| to either side).  Returns, and appends to `log`, the
    worst ratio of the excess to 2^-24 scale."""
    got = torch.as_tensor(got).detach().cpu()
    rv, rs = ref.v.detach().to(F64), ref.s.detach().to(F64)
    got = got.reshape(rv.shape)
    assert bool(torch.isfinite(rv).all()), f"{name}: the reference is not finite"
    assert bool(torch.isfinite(got).all()), f"{name}: {int((~torch.isfinite(got)).sum())} values are not finite"
    if bf16:
        assert bool((got.to(torch.bfloat16).to(F64) == got.to(F64)).all()), f"{name}: not bf16 values"
        lo, hi = bf16_cell(got)
        excess = (torch.maximum(lo - rv, rv - hi) - 2.0 ** -126).clamp_min(0.0)
    else:
        excess = (got.to(F64) - rv).abs()
    exact = rs == 0
    if bool(exact.any()):
        bad = got.to(F64)[exact] != rv[exact]
        assert not bool(bad.any()), f"{name}: {int(bad.sum())} values that are exact by construction differ"
    ratio = torch.where(exact, torch.zeros_like(excess), excess / (EPS24 * rs.clamp_min(1e-300)))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if log is not None:
        log.append((name, worst))
    if worst > K:
        i = int(ratio.reshape(-1).argmax())
        raise AssertionError(f"{name}: worst excess / (2^-24 scale) = {worst:.3g} > K = {K} at flat index {i}: got "
                             f"{float(got.reshape(-1)[i])!r}, ref {float(rv.reshape(-1)[i])!r}, scale {float(rs.reshape(-1)[i]):.3g}")
    return worst


def rejects(name, got, ref: SV, K, bf16=False):
    try:
        assert_close(name, got, ref, K, bf16)
    except AssertionError:
        return True
    return False


# =========================================================================== LayerNorm
def ln_fwd(y, gamma, beta, dt=F64, variant=None):
    """nn.LayerNorm, biased variance, eps 1e-5 -> dict of SV: out [M, N], mean [M], rstd [M]."""
    Y, G, Bt = leaf(y, dt), leaf(gamma, dt), leaf(beta, dt)
    N = Y.v.shape[-1]
    mean = Y.sum(-1, True).mulc(1.0 / N)
    d = Y - mean
    var = (d * d).sum(-1, True).mulc(1.0 / ((N - 1) if variant == "unbiased" else N))
    rstd = (var if variant == "no_eps" else var.addc(1e-5)).rsqrt()
    out = d * rstd * G + Bt
    return {"out": out, "mean": mean.reshape(-1), "rstd": rstd.reshape(-1)}


def ln_bwd(dout, y, mean, rstd, gamma, mask_scale, dt=F64, variant=None):
    """dz = mask * rstd (g - mean(g) - xhat mean(g xhat)), g = dout gamma, xhat = (y - mean) rstd; mask = (y > 0) * mask_scale for
    mask_scale > 0, absent otherwise.  dgamma = sum_rows dout xhat, dbeta = sum_rows dout, slab [ceil(M/16)][2][N]: the same sums
    over 16 consecutive rows.  -> dict of SV."""
    D, Y, G = leaf(dout, dt), leaf(y, dt), leaf(gamma, dt)
    Mu, Rs = leaf(mean, dt).reshape(-1, 1), leaf(rstd, dt).reshape(-1, 1)
    M, N = Y.v.shape
    xhat = (Y - Mu) * Rs
    gd = D * G
    m1 = gd.sum(-1, True).mulc(1.0 / N)
    dy = gd - m1
    if variant != "no_xhat_term":
        dy = dy - xhat * (gd * xhat).sum(-1, True).mulc(1.0 / N)
    dy = dy * Rs
    dz = ln_mask(dy, Y.v, mask_scale, variant)
    dg = D * xhat
    G16 = (M + 15) // 16 if M > 0 else 1
    pad = G16 * 16 - M

    def groups(a):
        z = torch.zeros(pad, N, dtype=a.v.dtype)
        a = SV(torch.cat([a.v, z]), torch.cat([a.s, z])).reshape(G16, 16, N)
        return (a[:, :15] if variant == "slab15" else a).sum(1)
    slab = stack([groups(dg), groups(D)], 1)                   # [G16][2][N]
    return {"dz": dz, "dgamma": dg.sum(0), "dbeta": D.sum(0), "slab": slab, "_dy": dy}


def ln_mask(dy, y, mask_scale, variant=None):
    """the ReLU / dropout mask folded into the LayerNorm backward: dy (y > 0) mask_scale for mask_scale > 0, dy itself otherwise."""
    if mask_scale > 0:
        y = torch.as_tensor(y)
        return dy.mulc(float(mask_scale)).where((y >= 0) if variant == "mask_ge" else (y > 0))
    return dy


# =========================================================================== dropout draw
_M32 = np.uint64(0xFFFFFFFF)


def _u32(x):
    return np.asarray(x, dtype=np.uint64) & _M32


def mix32(x):
    """the 'lowbias32' finaliser in uint32 arithmetic (held in uint64, masked after every multiply)."""
    x = _u32(x)
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & _M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & _M32
    x = x ^ (x >> np.uint64(16))
    return x


def drop_threshold(p):
    """make_drop: (thresh, scale).  p arrives as a C float; keep = 1 - p in double, clamped at 0; thresh = floor(keep 2^32), saturated at
    2^32 - 1; scale = float32(1 / keep), 0 when keep = 0."""
    keep = max(1.0 - float(np.float32(p)), 0.0)
    t = keep * 4294967296.0
    thresh = 0xFFFFFFFF if t >= 4294967295.0 else int(t)
    return thresh, (float(np.float32(1.0 / keep)) if keep > 0 else 0.0)


def drop_key(site, seed, offset):
    seed, offset = int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1)
    k = mix32((seed & 0xFFFFFFFF) ^ 0x9E3779B9)
    k = mix32(int(k) ^ (seed >> 32))
    k = mix32(int(k) ^ (offset & 0xFFFFFFFF))
    k = mix32(int(k) ^ (offset >> 32) ^ ((site * 0x85EBCA6B) & 0xFFFFFFFF))
    return int(k)


def drop_rand(site, rows, cols, seed, offset, row0=0):
    """the 32-bit draw of every element of rows [row0, row0 + rows) x cols: mix32((row * 0x9E3779B1) ^ (col * 0x85EBCA77) ^ key)."""
    r = (np.arange(row0, row0 + rows, dtype=np.uint64) * np.uint64(0x9E3779B1)) & _M32
    c = (np.arange(cols, dtype=np.uint64) * np.uint64(0x85EBCA77)) & _M32
    return mix32(r[:, None] ^ c[None, :] ^ np.uint64(drop_key(site, seed, offset)))


def drop_keep(site, rows, cols, p, seed, offset, row0=0):
    """keep mask (bool [rows, cols]) of a dropout site: draw < thresh."""
    return drop_rand(site, rows, cols, seed, offset, row0) < np.uint64(drop_threshold(p)[0])


SITE_AV_ATTN, SITE_TRI_ATTN = 1, 3


def tri_keep(B, p, seed, offset):
    """the attention-dropout masks of the trimodal block: keep [B, 8, 2, 2] (site 3, col = head 4 + t 2 + u) and the kept-head counts
    [B, 2] of the two AV calls (site 1, rows [0, B) and [B, 2B), col = head)."""
    keep = torch.from_numpy(drop_keep(SITE_TRI_ATTN, B, 32, p, seed, offset)).reshape(B, 8, 2, 2)
    av = torch.from_numpy(drop_keep(SITE_AV_ATTN, 2 * B, 8, p, seed, offset)).reshape(2, B, 8).sum(-1).t().contiguous()
    return keep, av


# =========================================================================== trimodal attention
def _tri_split(qkv, dt):
    """qkv [2B, 1536]: a tensor (an exact input) or an SV (values that carry a scale, e.g. the float64 projection of fused_proj)."""
    X = SV(qkv.v.to(dt), qkv.s.to(dt)) if isinstance(qkv, SV) else leaf(qkv, dt)
    B = X.v.shape[0] // 2
    X = X.reshape(B, 2, 3, 8, 64)
    return B, X[:, :, 0], X[:, :, 1], X[:, :, 2]            # q, k, v: [B, t, h, d]


def _tri_scores(q, k):
    return stack([stack([(q[:, t] * k[:, u]).sum(-1) for u in range(2)], -1) for t in range(2)], -2)      # [B, 8, t, u]


def tri_attn(qkv, keep=None, p=0.0, av_kept=None, dt=F64, variant=None, probs=None):
    """2-token, 8-head self-attention on rows (2b + t) of [2B, 1536] = [q | k | v]: scores q.k / 8, softmax over the 2 keys, dropout
    AFTER the softmax (keep [B, 8, 2, 2], scale float32(1 / (1 - p))), PV, mean over the two tokens.  -> dict of SV: obar [B, 512],
    probs [B, 8, 2, 2] (before dropout), attn_w [B, 2, 2] (head mean after dropout), av_w [B, 2].  qkv: a tensor or an SV; with
    `probs` (SV [B, 8, 2, 2]) given, the softmax stage is skipped and only v is taken from qkv (the staged reference of the fused kernel)."""
    B, q, k, v = _tri_split(qkv, dt)
    scale = drop_threshold(p)[1] if keep is not None else 1.0
    kf = None if keep is None else torch.as_tensor(keep).to(dt) * scale           # [B, 8, 2, 2], exact
    if kf is not None and variant == "keep_swap":                                 # columns 4 h + 1 and 4 h + 2 exchanged
        kf = kf.transpose(-1, -2)
    if probs is None:
        s = _tri_scores(q, k)
        if variant != "no_scale":
            s = s.mulc(0.125)
        if variant == "drop_before" and kf is not None:
            s = s * SV(kf)
        e = (s - s.max(-1)).exp()
        prob = e / e.sum(-1, True)
    else:
        prob = SV(probs.v.to(dt), probs.s.to(dt))
    d = prob if (kf is None or variant == "drop_before") else prob * SV(kf)
    # o_t = sum_u d[t, u] v_u ; obar = (o_0 + o_1) / 2
    w = d.sum(-2)                                                                   # [B, 8, u]
    o = SV(w.v[..., 0:1], w.s[..., 0:1]) * v[:, 0] + SV(w.v[..., 1:2], w.s[..., 1:2]) * v[:, 1]      # [B, 8, 64]
    out = {"obar": (o if variant == "no_half" else o.mulc(0.5)).reshape(B, 512), "probs": prob, "attn_w": d.sum(1).mulc(0.125)}
    if keep is None:
        out["av_w"] = SV(torch.ones(B, 2, dtype=dt))
    else:
        kept = torch.as_tensor(av_kept).to(dt)
        if variant == "av_swap":
            kept = kept.flip(-1)
        out["av_w"] = SV(kept).mulc(scale).mulc(0.125)
    return out


def tri_attn_bwd(qkv, dobar, probs, keep=None, p=0.0, dt=F64, variant=None):
    """backward of tri_attn from the SAVED probabilities, the keep mask fixed -> SV dqkv [2B, 1536].  qkv: a tensor or an SV."""
    B, q, k, v = _tri_split(qkv, dt)
    scale = drop_threshold(p)[1] if keep is not None else 1.0
    kf = SV(torch.ones(B, 8, 2, 2, dtype=dt) if keep is None else torch.as_tensor(keep).to(dt) * scale)
    P = leaf(probs, dt).reshape(B, 8, 2, 2)
    go = leaf(dobar, dt).reshape(B, 8, 64).mulc(0.5)                                # d o_t = d obar / 2, both tokens
    d = P if variant == "dv_no_keep" else P * kf
    Dv = [(go * v[:, u]).sum(-1, True) for u in range(2)]                           # [B, 8, 1]
    dp = stack([cat([Dv[0], Dv[1]], -1)] * 2, -2) * kf                              # [B, 8, t, u]
    T = (P * dp).sum(-1, True)
    ds = P * (dp - SV(T.v.expand(-1, -1, -1, 2), T.s.expand(-1, -1, -1, 2)))
    if variant != "ds_no_scale":
        ds = ds.mulc(0.125)
    el = lambda a, t, u: SV(a.v[:, :, t, u, None], a.s[:, :, t, u, None])           # [B, 8, 1]
    dq = [el(ds, t, 0) * k[:, 0] + el(ds, t, 1) * k[:, 1] for t in range(2)]
    if variant == "dk_transposed":                                                  # ds[t][u] where ds[u][t] belongs
        dk = [el(ds, u, 0) * q[:, 0] + el(ds, u, 1) * q[:, 1] for u in range(2)]
    else:
        dk = [el(ds, 0, u) * q[:, 0] + el(ds, 1, u) * q[:, 1] for u in range(2)]
    dv = [(el(d, 0, u) + el(d, 1, u)) * go for u in range(2)]
    rows = [cat([dq[t].reshape(B, 512), dk[t].reshape(B, 512), dv[t].reshape(B, 512)], -1) for t in range(2)]
    return stack(rows, 1).reshape(2 * B, 1536)


# =========================================================================== in_proj + attention in one kernel (csrc/tri_fused.hip)
# The kernel rounds q and k to bf16 in front of the scores and nothing else in front of P V or in the backward, so the reference is
# staged, every stage taking the kernel's own earlier OUTPUT as an exact input:
#   projection     qkv_out  against  sum_k x w + bias                                         (fused_proj)
#   probabilities  probs    against  the clamped 2-key softmax of the STORED q, k             (fused_probs: 64 exact products a score)
#   context        obar, attn_w, av_w  against  tri_attn(projection, probs = those reference probabilities)
#   backward       dqkv     against  tri_attn_bwd(projection, dobar, the kernel's saved probs)
LOG2E = 1.4426950408889634
EXP2_CLAMP = 115.0


def fused_weight_image(w_bits32):
    """in_proj_weight as float32 bit patterns [1536][512] -> the head-major bf16 image (uint16 [1536][512]):
    row 192 h + 96 wn + 32 part + dd  <-  row 512 part + 64 h + 32 wn + dd, every element through convert()."""
    b = convert(np.asarray(w_bits32, dtype=np.uint32).reshape(1536, 512))
    img = np.empty_like(b)
    for h in range(8):
        for wn in range(2):
            for part in range(3):
                src = 512 * part + 64 * h + 32 * wn
                dst = 192 * h + 96 * wn + 32 * part
                img[dst:dst + 32] = b[src:src + 32]
    return img


def fused_proj(x, w, bias, dt=F64, variant=None):
    """x [2B, 512] (bf16 values), w [1536, 512] fp32 master weights (the kernel reads their bf16 image), bias [1536] fp32 -> SV [2B, 1536]
    = sum_k x w + bias with the sum rule's scale sum_k |x w| + |bias| (+ |value|).  float32: the kernel's order as far as a CPU can
    state it -- the accumulator starts at the bias and takes 16 steps of 32 exact products (a product of two bf16 numbers is exact
    in float32; a step's sum is formed in float64 and rounded once)."""
    X, W, b = torch.as_tensor(x).to(F64), bf16_round(torch.as_tensor(w).float()).to(F64), torch.as_tensor(bias).to(F64)
    if variant == "no_bias":
        b = torch.zeros_like(b)
    elif variant == "bias_qk_swap":
        b = torch.cat([b[512:1024], b[:512], b[1024:]])
    elif variant == "wn_swap":                                                      # the two 32-dim halves of every head exchanged
        W = W.reshape(3, 8, 2, 32, 512).flip(2).reshape(1536, 512)
    if dt == F64:
        v = X @ W.t() + b
    else:
        acc = b.to(dt).expand(X.shape[0], -1)
        for c in range(0, 512, 32):
            acc = (acc.to(F64) + X[:, c:c + 32] @ W[:, c:c + 32].t()).to(dt)
        v = acc.to(F64)
    s = X.abs() @ W.abs().t() + b.abs() + v.abs() + TINY
    return SV(v.to(dt), s.to(dt))


def fused_probs(tile, keep=None, p=0.0, dt=F64, variant=None):
    """the kernel's softmax over two keys from the STORED q | k tile [2B, 1536] (bf16 values, exact):
        p[t][t] = 1 / (1 + 2^min((s[t][1-t] - s[t][t]) log2(e) / 8, 115)),   p[t][1-t] = 1 - p[t][t], formed as 2^min(..) p[t][t]
    (the difference from 1 would cancel in any precision once p[t][1-t] < 2^-53).  At the clamp the exponent is the constant 115.
    -> SV [B, 8, 2, 2] and the largest |score gap| after the 1/8."""
    B, q, k, _ = _tri_split(tile, dt)
    s = _tri_scores(q, k)
    if variant == "drop_before" and keep is not None:
        s = s * SV(torch.as_tensor(keep).to(dt) * drop_threshold(p)[1])
    own = stack([s[..., 0, 0], s[..., 1, 1]], -1)                                   # [B, 8, t]
    oth = stack([s[..., 0, 1], s[..., 1, 0]], -1)
    d = (oth - own).mulc(LOG2E if variant == "no_scale" else 0.125 * LOG2E)
    gap = float(d.v.abs().max()) / LOG2E if d.v.numel() else 0.0
    if variant != "no_clamp":
        at = d.v >= EXP2_CLAMP
        d = SV(torch.where(at, torch.full_like(d.v, EXP2_CLAMP), d.v), torch.where(at, torch.zeros_like(d.s), d.s))
    ex = d.fn(torch.exp2, lambda x, y: y * 0.6931471805599453)
    p_own = SV(torch.ones_like(ex.v)) / ex.addc(1.0)
    p_oth = ex * p_own
    row0, row1 = stack([p_own[..., 0], p_oth[..., 0]], -1), stack([p_oth[..., 1], p_own[..., 1]], -1)
    return stack([row0, row1], -2), gap


# =========================================================================== CrossModalAttention core
INV_SQRT32 = 0.17677669529663687


def _softmax(s, dim):
    e = (s - s.max(dim)).exp()
    return e / e.sum(dim, True)


def cross_modal_attn(q, ka, va, kv, vv, gate_logits, dt=F64, variant=None):
    """q, k_*, v_* [B, 256] = 8 heads x 32; score_h = q_h . k_h / sqrt(32); softmax over the HEAD axis; c = sum_h p_h v_h [B, 32];
    out_m = softmax(gate_logits)[m] c_m.  -> dict of SV: out_a, out_v [B, 32] (+ the pieces the backward restatement reuses)."""
    Q = leaf(q, dt).reshape(-1, 8, 32)
    g = _softmax(leaf(gate_logits, dt), -1)                                         # [B, 2]
    res = {}
    for m, (kk, vw, name) in enumerate(((ka, va, "out_a"), (kv, vv, "out_v"))):
        Kk, Vw = leaf(kk, dt).reshape(-1, 8, 32), leaf(vw, dt).reshape(-1, 8, 32)
        if variant == "softmax_dims":
            pr = _softmax((Q * Kk).mulc(INV_SQRT32), -1)                            # [B, 8, 32]: over the 32 dims
            c = (pr * Vw).sum(1)
        else:
            pr = _softmax((Q * Kk).sum(-1, True).mulc(INV_SQRT32), 1)               # [B, 8, 1]: over the heads
            c = (pr * Vw).sum(1)                                                    # [B, 32]
        gm = 1 - m if variant == "gate_swap" else m
        res[name] = c * SV(g.v[:, gm:gm + 1], g.s[:, gm:gm + 1])
        res["_p%d" % m], res["_c%d" % m] = pr, c
    res["_gate"] = g
    return res


def cross_modal_attn_bwd(q, ka, va, kv, vv, gate_logits, g_a, g_v, dt=F64):
    """-> dict of SV: dq, dka, dva, dkv, dvv [B, 256], dgl [B, 2]."""
    f = cross_modal_attn(q, ka, va, kv, vv, gate_logits, dt)
    Q = leaf(q, dt).reshape(-1, 8, 32)
    gate = f["_gate"]
    out, dgate, dq = {}, [], None
    for m, (kk, vw, gg, nk, nv) in enumerate(((ka, va, g_a, "dka", "dva"), (kv, vv, g_v, "dkv", "dvv"))):
        Kk, Vw, Gm = leaf(kk, dt).reshape(-1, 8, 32), leaf(vw, dt).reshape(-1, 8, 32), leaf(gg, dt)
        pr, c = f["_p%d" % m], f["_c%d" % m]
        dgate.append((Gm * c).sum(-1, True))                                        # [B, 1]
        dc = (Gm * SV(gate.v[:, m:m + 1], gate.s[:, m:m + 1])).reshape(-1, 1, 32)
        out[nv] = (pr * dc).reshape(-1, 256)                                        # d v_h = p_h dc
        dpp = (dc * Vw).sum(-1, True)                                               # [B, 8, 1]
        ds = (pr * (dpp - (pr * dpp).sum(1, True))).mulc(INV_SQRT32)
        out[nk] = (Q * ds).reshape(-1, 256)
        dq = Kk * ds if dq is None else dq + Kk * ds
    out["dq"] = dq.reshape(-1, 256)
    dg = cat(dgate, -1)                                                             # [B, 2]
    out["dgl"] = gate * (dg - (gate * dg).sum(-1, True))
    return out


# =========================================================================== LSTM cell at T = 1, zero state
def _gates(gates, hidden, ndir, dt):
    Gt = leaf(gates, dt).reshape(-1, ndir, 4, hidden)
    return Gt[:, :, 0], Gt[:, :, 2], Gt[:, :, 3]                                    # i, g, o (f multiplies c0 = 0)


def lstm_cell_t1(gates, hidden, ndir, dt=F64, variant=None):
    """gates [B, ndir 4 hidden] (i, f, g, o per direction) -> SV h [B, ndir hidden] = sigmoid(o) tanh(sigmoid(i) tanh(g))."""
    gi, gg, go = _gates(gates, hidden, ndir, dt)
    c = gi.sigmoid() * gg.tanh()
    return (go.sigmoid() * (c if variant == "no_tanh_c" else c.tanh())).reshape(-1, ndir * hidden)


def lstm_cell_t1_bwd(gates, dout, hidden, ndir, dt=F64):
    """-> SV dgates [B, ndir 4 hidden]; the forget block is exactly 0."""
    gi, gg, go = _gates(gates, hidden, ndir, dt)
    dh = leaf(dout, dt).reshape(-1, ndir, hidden)
    si, tg, so = gi.sigmoid(), gg.tanh(), go.sigmoid()
    tc = (si * tg).tanh()
    dc = dh * so * (tc * tc).rsubc(1.0)
    di = dc * tg * si * si.rsubc(1.0)
    dg = dc * si * (tg * tg).rsubc(1.0)
    do = dh * tc * so * so.rsubc(1.0)
    return stack([di, SV(torch.zeros_like(di.v)), dg, do], 2).reshape(-1, ndir * 4 * hidden)


# =========================================================================== convert
def convert(bits32):
    """float32 bit patterns (uint32 array) -> bf16 bit patterns (uint16), round to nearest even; a NaN stays a NaN."""
    u = np.asarray(bits32, dtype=np.uint64) & _M32
    r = ((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)) & np.uint64(0xFFFF)
    nan = (u & np.uint64(0x7FFFFFFF)) > np.uint64(0x7F800000)
    return np.where(nan, (u >> np.uint64(16)) | np.uint64(0x40), r).astype(np.uint16)


def convert_values():
    """float32 bit patterns with the edges of the conversion: ties to even both ways, +-0, inf, NaN, bf16 denormals, the largest finite
    float32 (rounds to inf) and the largest finite bf16."""
    return np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001, 0x7F800001, 0x7FFFFFFF,
                     0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0xBF808000, 0xBF818000,       # ties: to even down / up
                     0x00010000, 0x00008000, 0x00018000, 0x00007FFF, 0x807F0000, 0x007F8000, 0x00000001,   # bf16 denormals
                     0x7F7FFFFF, 0x7F7F0000, 0x7F7F8000, 0x7F7F7FFF, 0xFF7FFFFF,                   # largest finite values
                     0x3F800000, 0x40490FDB, 0xC2F6E979, 0x3EAAAAAB], dtype=np.uint32)


# =========================================================================== the cases of section 3 (shared by the CPU and GPU tests)
def _gen(*key):
    """a generator seeded by the case (integers and names)."""
    seed = 0
    for k in key:
        seed = (seed * 1000003 + (k if isinstance(k, int) else sum((i + 1) * ord(ch) for i, ch in enumerate(str(k))))) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


# K per output family: twice the worst ratio of the float32 CPU evaluation over the cases below, rounded up -- measured and asserted by
# tests/test_cpu_rowkernel_ref.py (float32 worst: 2.07, 3.41, 0.47, 0.63, 0.39, 0.44, 1.49), recorded in DESIGN.md section 15 next to
# what an MI355X shows.  The ratios are small because the scale charges every operation of the formula one rounding of its result.
K = {"ln_fwd": 4.5, "ln_bwd": 7.5, "tri_fwd": 1.0, "tri_bwd": 1.5, "cross_fwd": 1.0, "cross_bwd": 1.0, "lstm": 3.5}

LN_N = (4, 8, 252, 256, 260, 512, 768, 1020, 1024)
LN_M_ALL = (1, 2, 3, 7, 8, 9, 15, 16, 17, 33, 1027)
LN_M_FEW = (1, 17, 1027)
LN_MASK_SCALES = (float(np.float32(1 / 0.7)), 1.0, 0.0)
LN_CLASSES = ("relu_normal", "mean_1000", "constant", "nonpositive", "tiny_1e-4", "zeros_and_smallest")


def ln_shapes():
    return [(M, N) for N in LN_N for M in (LN_M_ALL if N in (256, 512) else LN_M_FEW)]


def ln_row_class(i, M, N):
    return (i + M + N // 4) % len(LN_CLASSES)


def ln_inputs(M, N, bf16):
    """y (the stored ReLU'd / dropped rows in front of the LayerNorm; row i is of class ln_row_class(i, M, N)), dout, gamma, beta as
    float32 CPU tensors; y and dout hold bf16-representable values when bf16."""
    g = _gen(M, N, 11)
    y = torch.relu(torch.randn(M, N, generator=g))
    smallest = (2.0 ** -133, 2.0 ** -126) if bf16 else (2.0 ** -149, 2.0 ** -126)    # smallest subnormal and normal of the dtype
    for i in range(M):
        c = ln_row_class(i, M, N)
        if c == 1:
            y[i] = 1000.0 + torch.randn(N, generator=g)
        elif c == 2:
            y[i] = 0.75
        elif c == 3:
            y[i] = -torch.relu(torch.randn(N, generator=g))
        elif c == 4:
            y[i] = y[i] * 1e-4
        elif c == 5:
            y[i, 0::4] = 0.0
            y[i, 1::4] = smallest[0]
            y[i, 3::4] = smallest[1]
    dout = torch.randn(M, N, generator=g)
    gamma = 1 + 0.1 * torch.randn(N, generator=g)
    beta = 0.05 * torch.randn(N, generator=g)
    if bf16:
        y, dout = bf16_round(y), bf16_round(dout)
    return y, dout, gamma, beta


TRI_B = (1, 2, 3, 4, 5, 1027)
TRI_CLASSES = ("normal", "saturated", "identical_tokens", "zeros")
TRI_P = (0.0, 0.3, 0.9)
TRI_SEED, TRI_OFFSET = 2 ** 40 + 7, 2 ** 33 + 1


def tri_inputs(B, cls, bf16):
    """qkv [2B, 1536], dobar [B, 512]."""
    g = _gen(B, cls, 12)
    qkv = torch.randn(2 * B, 1536, generator=g)
    if cls == "saturated":
        # q_0 = k_0 = u, q_1 = k_1 = -u with |u|^2 = 1024: the scores are +128 (t == u) and -128, 256 apart: exp underflows to exactly 0
        x = qkv.view(B, 2, 3, 8, 64)
        u = torch.randn(B, 8, 64, generator=g).sign() * 4.0
        x[:, 0, 0], x[:, 1, 0] = u, -u
        x[:, 0, 1], x[:, 1, 1] = u, -u
    elif cls == "identical_tokens":
        x = qkv.view(B, 2, 1536)
        x[:, 1] = x[:, 0]
    elif cls == "zeros":
        qkv.zero_()
    dobar = torch.randn(B, 512, generator=g)
    if bf16:
        qkv, dobar = bf16_round(qkv), bf16_round(dobar)
    return qkv.contiguous(), dobar


# ---- the fused kernel (tests/test_gpu_fused_attention.py).  One workgroup = 128 samples x one head: 127 / 128 / 129 sit either side of
# one row tile, 641 = 6 tiles (48 workgroups), 1025 = 9 tiles, the last holding ONE sample (72 workgroups: 9 per XCD).
FUSED_B = (1, 2, 127, 128, 129, 300, 641, 1025)
FUSED_B_ALL_CLASSES = (1, 2, 129)
FUSED_CLASSES = ("normal", "identical_tokens", "x_zero", "bias_zero", "bias_ramp", "saturated", "clamp_x4", "clamp_qbias40")
FUSED_CLASSES_EVERY_B = ("normal", "clamp_x4")
FUSED_DROPS = ((91, 5), (0, 0), (2 ** 40 + 7, 2 ** 33 + 1))                         # (seed, offset)
FUSED_P = (0.0, 0.3, 0.9)
# K per family.  tile, ctx (obar / attn_w / av_w) and bwd contain the projection, whose summation inside the MFMA a CPU cannot restate:
# at least 8, the constant accepted for bf16 MFMA accumulation over sum |a w| (C_BOUND of tests/test_gpu_gemm_routes.py); else twice the
# float32 CPU evaluation's worst ratio, rounded up to the next half (tests/test_cpu_rowkernel_ref.py measures and asserts: tile 0.95, probs 0.87, ctx 0.57, bwd 0.39).
K.update({"fused_tile": 8.0, "fused_probs": 2.0, "fused_ctx": 8.0, "fused_bwd": 8.0})


def fused_cases(B):
    """(class, p, seed, offset) of batch B: every class at the small batches, two at every batch; eval and p = 0.3 / 0.9 each, the
    (seed, offset) pairs in rotation so that every pair meets every p."""
    classes = FUSED_CLASSES if B in FUSED_B_ALL_CLASSES else FUSED_CLASSES_EVERY_B
    out = []
    for ci, cls in enumerate(classes):
        for pi, p in enumerate(FUSED_P):
            seed, offset = FUSED_DROPS[(ci + pi + FUSED_B.index(B)) % 3]
            out.append((cls, p, seed, offset))
    return out


_FUSED_MEMO = {}


def fused_weights():
    """fp32 master in_proj_weight [1536, 512] (std 0.06) and bias [1536] (std 0.2): one set for every case."""
    if "w" not in _FUSED_MEMO:
        g = _gen("fused weights", 15)
        _FUSED_MEMO["w"] = (torch.randn(1536, 512, generator=g) * 0.06, torch.randn(1536, generator=g) * 0.2)
    return _FUSED_MEMO["w"]


def fused_inputs(B, cls):
    """x [2B, 512] (bf16 values), bias [1536] fp32, dobar [B, 512] (bf16 values); the weights are fused_weights()[0].
    With x of unit normals a score gap (after the 1/8) has a spread of about 2.6; x scaled by 2.5 puts the gaps at 20 .. 79 (saturated,
    p down to 1e-34, below the clamp at 79.7), x scaled by 4 or +40 on head 0's q bias beyond 80 (the clamp)."""
    if (B, cls) in _FUSED_MEMO:
        return _FUSED_MEMO[(B, cls)]
    g = _gen(B, cls, 16)
    x = torch.randn(2 * B, 512, generator=g)
    bias = fused_weights()[1].clone()
    if cls == "identical_tokens":
        x.view(B, 2, 512)[:, 1] = x.view(B, 2, 512)[:, 0]
    elif cls == "x_zero":
        x.zero_()
    elif cls == "bias_zero":
        bias.zero_()
    elif cls == "bias_ramp":
        bias = torch.arange(1536, dtype=torch.float32) / 64.0
    elif cls == "saturated":
        x *= 2.5
    elif cls == "clamp_x4":
        x *= 4.0
    elif cls == "clamp_qbias40":
        bias[:64] += 40.0
    dobar = torch.randn(B, 512, generator=g)
    _FUSED_MEMO[(B, cls)] = (bf16_round(x).contiguous(), bias.contiguous(), bf16_round(dobar))
    return _FUSED_MEMO[(B, cls)]


def fused_proj_of(B, cls, dt=F64):
    """fused_proj of a case's inputs, computed once per (B, class, dtype) and left unchanged."""
    key = (B, cls, dt, "proj")
    if key not in _FUSED_MEMO:
        x, bias, _ = fused_inputs(B, cls)
        _FUSED_MEMO[key] = fused_proj(x, fused_weights()[0], bias, dt)
    return _FUSED_MEMO[key]


CROSS_B = (1, 3, 4, 5, 1027)
CROSS_LD = (256, 264, 768)
CROSS_CLASSES = ("normal", "dominant_head", "equal_scores", "gate_equal", "gate_apart")


def cross_inputs(B, cls, bf16):
    """q, ka, va, kv, vv [B, 256], gate_logits [B, 2], g_a, g_v [B, 32]."""
    g = _gen(B, cls, 13)
    q, ka, va, kv, vv = (torch.randn(B, 256, generator=g) for _ in range(5))
    gl = torch.randn(B, 2, generator=g)
    if cls == "dominant_head":                       # head (b % 8): score larger than every other by more than 100
        for t in (ka, kv):
            k3, q3 = t.view(B, 8, 32), q.view(B, 8, 32)
            k3 *= 0.05
            for b in range(B):
                h = b % 8
                k3[b, h] = q3[b, h] * (120.0 / INV_SQRT32 / float((q3[b, h] ** 2).sum()))
    elif cls == "equal_scores":                      # q and k the same in every head: the 8 scores are equal bit for bit; v_h = unit h
        q = q.view(B, 8, 32)[:, :1].expand(B, 8, 32).reshape(B, 256).clone()
        ka = ka.view(B, 8, 32)[:, :1].expand(B, 8, 32).reshape(B, 256).clone()
        kv = kv.view(B, 8, 32)[:, :1].expand(B, 8, 32).reshape(B, 256).clone()
        eye = torch.zeros(8, 32)
        eye[torch.arange(8), torch.arange(8)] = 1.0
        va = eye.reshape(1, 256).expand(B, 256).clone()
        vv = va.clone()
        gl[:, 1] = gl[:, 0]
    elif cls == "gate_equal":
        gl[:, 1] = gl[:, 0]
    elif cls == "gate_apart":
        gl[:, 1] = gl[:, 0] + torch.where(torch.arange(B) % 2 == 0, 50.0, -50.0)
    g_a, g_v = torch.randn(B, 32, generator=g), torch.randn(B, 32, generator=g)
    if bf16:
        q, ka, va, kv, vv = (bf16_round(t) for t in (q, ka, va, kv, vv))
    return q, ka, va, kv, vv, gl, g_a, g_v


LSTM_SHAPES = [(B, H, nd) for H in (1, 3, 64, 128) for nd in (1, 2) for B in (1, 37)] + [(4100, 128, 2)]
LSTM_CLASSES = ("normal_x3", "saturated_40", "zeros")


def lstm_cases():
    """(B, hidden, ndir, class): every class at the small shapes; the large one (B ndir hidden > 4096 * 256: the second grid-stride
    trip) once, its rows cycling through the classes."""
    return [(B, H, nd, cls) for B, H, nd in LSTM_SHAPES for cls in (LSTM_CLASSES if B < 4100 else ("mixed",))]


def lstm_inputs(B, H, ndir, cls, bf16):
    """gates [B, ndir 4 H], dout [B, ndir H]."""
    g = _gen(B, H, ndir, cls, 14)
    gates = torch.randn(B, ndir * 4 * H, generator=g) * 3.0
    if cls == "saturated_40":
        gates = gates.sign() * 40.0
    elif cls == "zeros":
        gates.zero_()
    elif cls == "mixed":
        gates[1::3] = gates[1::3].sign() * 40.0
        gates[2::3] = 0.0
    dout = torch.randn(B, ndir * H, generator=g)
    if bf16:
        gates, dout = bf16_round(gates), bf16_round(dout)
    return gates, dout
