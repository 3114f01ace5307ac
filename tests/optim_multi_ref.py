"""float64 restatement of mmdeer_adamw_multi (include/mmdeer_optim.h), written from that header's comment, clip_grad_norm_ and
torch.optim.AdamW alone: global-norm clipping of grad_scale * g over the LISTED tensors, then the decoupled AdamW update per tensor
with its class's lr, weight decay and step count.  A tensor marked ``skip`` (torch: grad is None) is not listed: untouched, not in
the norm.

The comparison is tests/optim_ref.py's: |got - ref| <= K * U * magnitude per element, U = 2^-24, magnitude = the sum of the |terms|
the value is made of; magnitude 0 must match exactly.  The element update is adamw_update4's operation order, so p, exp_avg and
exp_avg_sq take optim_ref.K; the norm's K belongs to the new fold (chunks of 1024 elements dealt to at most 2048 blocks, serial over
a block's chunks, pairwise over lanes, waves, blocks) and is twice the worst ratio of adamw_multi_f32 -- the kernel's operation and
fold order in numpy float32 -- against adamw_multi_ref over the cases below (tests/test_cpu_module_adamw.py asserts the tie).
"""
import math

import numpy as np

from .optim_ref import CLIP_EPS, POW_ULPS, U, f32, ratio  # noqa: F401  (U, ratio, POW_ULPS re-exported to the tests)
from .optim_ref import K as _K_UPDATE

CHUNK = 1024          # MMDEER_ADAMW_MULTI_CHUNK: the tests assert it is the header's
NPART = 2048          # MMDEER_ADAMW_MULTI_SCRATCH
K = {"p": _K_UPDATE["p"], "exp_avg": _K_UPDATE["exp_avg"], "exp_avg_sq": _K_UPDATE["exp_avg_sq"], "norm": 2.06}
BETA1, BETA2, EPS = 0.9, 0.999, 1e-8
FAMILIES = ("p", "exp_avg", "exp_avg_sq")


# ============================================================================ the step in float64
def adamw_multi_ref(tensors, classes, beta1, beta2, eps, max_norm, grad_scale, norm=None):
    """tensors: dicts with p, g, m, v (1-D arrays), cls, skip; classes: (lr, weight_decay, step) per class.  Scalars enter as the
    float32 values the library receives; bias corrections exactly in float64.  norm: None, or the norm to derive the clip factor from
    (teacher forcing with the kernel's own).  Returns {'norm', 'tensors': [p, exp_avg, exp_avg_sq, mag_p, mag_exp_avg,
    mag_exp_avg_sq per tensor]}; a skipped tensor comes back as it went in, with magnitudes 0 (it must match exactly)."""
    b1, b2, eps, gs, mx = f32(beta1), f32(beta2), f32(eps), f32(grad_scale), f32(max_norm)
    omb1, omb2 = float(np.float32(1) - np.float32(beta1)), float(np.float32(1) - np.float32(beta2))
    ss = 0.0
    for t in tensors:
        if not t["skip"]:
            g = np.asarray(t["g"], dtype=np.float64)
            ss += float((g * g).sum())
    norm_ref = abs(gs) * math.sqrt(ss)
    n = norm_ref if norm is None else float(norm)
    clip = min(1.0, mx / (n + CLIP_EPS)) if mx > 0 else 1.0
    out = []
    for t in tensors:
        p, g, m, v = (np.asarray(t[k], dtype=np.float64) for k in ("p", "g", "m", "v"))
        if t["skip"]:
            z = np.zeros_like(p)
            out.append({"p": p, "exp_avg": m, "exp_avg_sq": v, "mag_p": z, "mag_exp_avg": z, "mag_exp_avg_sq": z})
            continue
        lr, wd, step = classes[t["cls"]]
        lr, wd = f32(lr), f32(wd)
        pw1, pw2 = b1 ** step, b2 ** step
        bc1, bc2 = 1.0 - pw1, 1.0 - pw2
        g1 = g * (gs * clip)
        t_m, t_g = b1 * m, omb1 * g1
        m1 = t_m + t_g
        v1 = b2 * v + omb2 * g1 * g1
        den = np.sqrt(v1) / math.sqrt(bc2) + eps
        decay = 1.0 - lr * wd
        p1 = p * decay - (lr / bc1) * m1 / den
        mag_m = np.abs(t_m) + np.abs(t_g)
        extra = 2.0 * POW_ULPS * (pw1 / bc1 + 0.5 * pw2 / bc2)      # the fp32 bias corrections from the host's powf
        mag_p = np.abs(p * decay) + (lr / bc1) * mag_m / den * (1.0 + extra)
        out.append({"p": p1, "exp_avg": m1, "exp_avg_sq": v1, "mag_p": mag_p, "mag_exp_avg": mag_m, "mag_exp_avg_sq": v1})
    return {"norm": norm_ref, "tensors": out}


def ratios(got, ref):
    """got: {'norm', 'tensors': [{p, exp_avg, exp_avg_sq}]}; ref: what adamw_multi_ref returned -> the worst ratio per family"""
    out = {f: 0.0 for f in FAMILIES}
    for gt, rt in zip(got["tensors"], ref["tensors"]):
        for f in FAMILIES:
            if rt[f].size:
                out[f] = max(out[f], ratio(np.asarray(gt[f], dtype=np.float64), rt[f], rt["mag_" + f]))
    out["norm"] = ratio(float(got["norm"]), ref["norm"], ref["norm"])
    return out


def rejects(got, ref):
    return any(r > K[f] for f, r in ratios(got, ref).items())


# ============================================================================ the kernel's operation and fold order in numpy float32
VARIANTS = ("l2_decay", "eps_in_sqrt", "bc_swapped", "step_minus_1", "clip_no_1e6", "skipped_in_norm", "lr_class0")


def sumsq_f32(tensors, count_skipped=False):
    """The two launches' sum of squares: groups of 4 counted from the 16-byte boundary below each tensor's first element (``head``
    elements below it), 256 groups per chunk, chunk c to block c mod grid with grid = min(chunks, 2048); a lane sums its group of the
    block's chunks serially, then pairwise trees over the 256 lanes, and over the partials padded to 2048."""
    f = np.float32
    chunks = []
    for t in tensors:
        n = len(t["g"])
        if (t["skip"] and not count_skipped) or n == 0:
            continue
        h = t.get("head", 0)
        nch = (n + h + CHUNK - 1) // CHUNK
        x = np.zeros(nch * CHUNK, dtype=f)
        x[h:h + n] = np.asarray(t["g"], dtype=f)
        x = x.reshape(nch, 256, 4)
        chunks.append((x[..., 0] * x[..., 0] + x[..., 1] * x[..., 1]) + (x[..., 2] * x[..., 2] + x[..., 3] * x[..., 3]))
    if not chunks:
        return f(0)
    s = np.concatenate(chunks, axis=0)
    grid = min(len(s), NPART)
    s = np.concatenate([s, np.zeros((-len(s) % grid, 256), dtype=f)]).reshape(-1, grid, 256)
    acc = np.zeros((grid, 256), dtype=f)
    for row in s:
        acc = acc + row
    while acc.shape[1] > 1:
        acc = acc[:, 0::2] + acc[:, 1::2]
    part = np.concatenate([acc[:, 0], np.zeros(NPART - grid, dtype=f)])
    while len(part) > 1:
        part = part[0::2] + part[1::2]
    assert part.dtype == f
    return part[0]


def adamw_multi_f32(tensors, classes, beta1, beta2, eps, max_norm, grad_scale, variant=None):
    """adamw_update4's operation order (separate float32 operations, no contraction) per tensor, the norm in the kernel's fold order.
    Measures the rounding constants and carries the seeded errors (variant) -- never the expected value."""
    f = np.float32
    assert variant is None or variant in VARIANTS
    b1, b2, eps, gs, mx = f(beta1), f(beta2), f(eps), f(grad_scale), f(max_norm)
    out = []
    with np.errstate(all="ignore"):
        norm = np.sqrt(sumsq_f32(tensors, count_skipped=variant == "skipped_in_norm")) * np.abs(gs)
        den_c = norm if variant == "clip_no_1e6" else norm + f(1e-6)
        clip = np.minimum(f(1), mx / den_c) if mx > 0 else f(1)
        kgs = clip * gs
        for t in tensors:
            p, g, m, v = (np.asarray(t[k], dtype=f) for k in ("p", "g", "m", "v"))
            if t["skip"]:
                out.append({"p": p, "exp_avg": m, "exp_avg_sq": v})
                continue
            lr, wd, step = classes[0 if variant == "lr_class0" else t["cls"]][0], classes[t["cls"]][1], classes[t["cls"]][2]
            lr, wd = f(lr), f(wd)
            s = step - 1 if variant == "step_minus_1" else step
            bc1, bc2 = f(1) - f(float(b1) ** s), f(1) - f(float(b2) ** s)      # powf correctly rounded; the bound allows POW_ULPS
            if variant == "bc_swapped":
                bc1, bc2 = bc2, bc1
            ibc1, isbc2 = f(1) / bc1, f(1) / np.sqrt(bc2)
            g1 = g * kgs
            if variant == "l2_decay":
                g1 = g1 + wd * p
                p1 = p.copy()
            else:
                p1 = p * (f(1) - lr * wd)
            m1 = m * b1 + g1 * (f(1) - b1)
            v1 = v * b2 + g1 * g1 * (f(1) - b2)
            st = lr * ibc1
            den = np.sqrt(v1 * isbc2 * isbc2 + eps) if variant == "eps_in_sqrt" else np.sqrt(v1) * isbc2 + eps
            p1 = p1 - st * m1 / den
            for a in (p1, m1, v1):
                assert a.dtype == f
            out.append({"p": p1, "exp_avg": m1, "exp_avg_sq": v1})
    return {"norm": float(norm), "tensors": out}


# ============================================================================ the cases of tests/test_gpu_module_adamw.py
C = CHUNK
# layout -> (count, head, grad_head, skip) per tensor.  head: elements between the 16-byte boundary and the tensor's first element, for
# the parameter, its moments and its mirror (1: the tensor starts one element into a larger buffer); grad_head: the same for the
# gradient -- where it differs from head the tensor takes the element-by-element path.
EDGES = [(1, 0, 0, False), (3, 0, 0, False), (4, 0, 0, False), (5, 0, 0, False), (C - 1, 0, 0, False), (C, 0, 0, False), (C + 1, 0, 0, False),
         (2 * C + 3, 0, 0, False),
         (2 * C + 5, 1, 1, False),         # parameter and gradient one element into a larger buffer: 4-byte, not 16-byte aligned
         (C + 7, 0, 2, False),             # an aligned parameter whose gradient is not: element by element
         (5, 3, 3, False), (1, 1, 1, False), (3, 1, 1, False),      # odd starts at sizes below one group
         (77, 0, 0, True), (C + 2, 1, 1, True),                     # skipped: grad is None
         (300000, 0, 0, False)]            # 293 chunks of this tensor alone
# both grids wrap: more chunks than the 2048 blocks of either launch, from an odd start
WRAP = [(2200000 + 3, 1, 1, False), (5, 0, 0, False)]
MANY = [(1 + (37 * i) % 70, i % 4 if i % 3 == 0 else 0, i % 4 if i % 3 == 0 else 0, i % 17 == 5) for i in range(130)]
LAYOUTS = {"edges": EDGES, "many": MANY, "wrap": WRAP}
# name, layout, (step of class 0, step of class 1), max_norm as a multiple of the reference norm (0 and -1: off), grad_scale, mirrors
# ('bf16' / 'f32' for every tensor; every fourth tensor has none), gradient draw
CASES = (
    ("e1", "edges", (1, 1), 0.5, 1.0, "bf16", "wide"),
    ("e2", "edges", (2, 2), 4.0, 0.5, "f32", "wide"),
    ("e1000", "edges", (1000, 1000), 0.0, 1.0, "bf16", "wide"),
    ("m1", "many", (1, 1), 0.5, 0.5, "bf16", "wide"),
    ("m2", "many", (2, 5), -1.0, 1.0, "f32", "wide"),
    ("m1000", "many", (1000, 1000), 4.0, 1.0, "bf16", "wide"),
    ("w2", "wrap", (2, 2), 0.5, 1.0, "bf16", "wide"),
    # a norm near the 1e-6 of the clip factor: only here does that constant show
    ("tiny", "many", (3, 3), 0.5, 0.5, "f32", "tiny"),
)
CASE_NAMES = tuple(c[0] for c in CASES)
LR = (1e-3, 2.5e-4)
WD = (0.01, 0.0)


def case_inputs(name):
    """-> (tensors, classes, hyper, mirror kind).  Parameters O(1) with exact zeros; gradient magnitudes log-uniform over 1e-10 .. 1e2
    (tiny: 1e-12 .. 1e-7) so that eps = 1e-8 matters in a visible share of the elements; moments zero where the class is at step 1,
    else drawn (v >= 0); tensor i belongs to class i mod 2."""
    i = CASE_NAMES.index(name)
    _, layout, steps, clip, gs, mirror, draw = CASES[i]
    rng = np.random.default_rng(4000 + i)
    lo, hi = {"wide": (-10.0, 2.0), "tiny": (-12.0, -7.0)}[draw]
    tensors = []
    for j, (n, head, ghead, skip) in enumerate(LAYOUTS[layout]):
        mag = lambda: (10.0 ** rng.uniform(lo, hi, n)) * np.where(rng.random(n) < 0.5, -1.0, 1.0)      # noqa: E731
        p = rng.standard_normal(n).astype(np.float32)
        p[rng.random(n) < 0.01] = 0.0
        g = mag().astype(np.float32)
        cls = j % 2
        if steps[cls] == 1:
            m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
        else:
            m, v = mag().astype(np.float32), (mag() ** 2).astype(np.float32)
        tensors.append({"p": p, "g": g, "m": m, "v": v, "cls": cls, "skip": skip, "head": head, "ghead": ghead,
                        "mirror": None if j % 4 == 3 else mirror})
    classes = [(f32(LR[c]), f32(WD[c]), steps[c]) for c in range(2)]
    ss = sum(float((t["g"].astype(np.float64) ** 2).sum()) for t in tensors if not t["skip"])
    norm = abs(gs) * math.sqrt(ss)
    hyper = dict(beta1=BETA1, beta2=BETA2, eps=EPS, max_norm=f32(clip * norm) if clip > 0 else clip, grad_scale=gs)
    return tensors, classes, hyper, mirror


def bf16_rne(x):
    """float32 -> bf16 bits (uint16), round to nearest even (finite inputs)"""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)
