"""mmdeer_chain on every kernel behind it, called through the C ABI (include/mmdeer.h; host side mmdeer/chainops.py).

One call runs one of four kernels (csrc/chain.hip: launch_chain).  KERNELS below names each with the arguments and options that
select it.  Every case runs on every kernel where its table is legal (K = 768 and panels wider than 512 columns: 16-sample
workgroups only) and is checked four ways:

1. bit for bit against the same layers run one by one (mmdeer_gemm with tile = -1, mmdeer_layernorm_fwd / _bwd,
   mmdeer_add_masked: the rounding points of the launch-by-launch plan of mmdeer/stackb_train.py), including the
   LayerNorm-backward partial slabs of the 16-sample kernels slab for slab (the 32-sample kernel folds 32 rows per slab: its
   folded sums are compared within an fp32 bound).  A segment with dcol_off != 0 has no single-GEMM equivalent: such cases
   take check 2 only;
2. element-wise against float64, teacher-forced per layer (each layer's reference starts from the chain's own stored bf16 input
   panel), under bounds derived from the accumulation (C_BOUND as in test_gpu_gemm_routes.py) and the bf16 rounding of the
   stored value; dropout against the exact keep mask of mmdeer_dropout_mask;
3. NaN canaries: every output sits inside a canary buffer (a row above, a row below, pad columns up to its leading dimension,
   one partial slab on either side); inputs carry canaries in their pad columns and in rows past `rows`.  After the call the
   canaries must be intact and no stored value may be a NaN;
4. determinism: the call runs twice and must store the same bits.

The LayerNorm-backward rows / statistics are far from zero, so that a read before its load has landed (registers start at zero)
gives a visibly wrong dz."""
import math

import numpy as np
import pytest
import torch

from mmdeer import _lib
from mmdeer.chainops import Chain, FragImages
from mmdeer.opseq import Exec

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CANARY32 = 0x7FA5A5A5          # a NaN no kernel produces (payload), as int32 / float32 bits
CANARY16 = 0x7FA5              # the same for bf16 storage
U = 2.0 ** -24                 # unit roundoff of the fp32 accumulators
UB = 2.0 ** -8                 # unit roundoff of bf16 storage (half an ulp, relative)
C_BOUND = 8.0                  # |acc - ref| <= C_BOUND * U * sum_k |a w| for bf16 operands (test_gpu_gemm_routes.py)

# kernel -> samples per workgroup and the options that select it (launch_chain: option chain_depth picks the 16-sample variant)
KERNELS = {
    "s16": dict(ts=16, opts=dict(chain_depth=4)),
    "s16_d2": dict(ts=16, opts=dict(chain_depth=2)),
    "s16_d8": dict(ts=16, opts=dict(chain_depth=8)),
    "s32": dict(ts=32, opts=dict(chain_depth=4)),
}


def _canary(n, f32):
    if f32:
        return torch.full((max(n, 1),), CANARY32, dtype=torch.int32, device=DEV).view(torch.float32)
    return torch.full((max(n, 1),), CANARY16, dtype=torch.int16, device=DEV).view(torch.bfloat16)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16)


class Inp:
    """An input matrix of `rows` rows at row stride `ld` in a canary buffer with two canary rows behind it; columns [c0, c1) hold
    `vals`, every other element is a canary.  `m`: the [rows][ld] view (the pointer the chain gets), `val`: the stored values."""

    def __init__(self, rows, c0, c1, ld, vals, f32=False):
        self.buf = _canary((rows + 2) * ld, f32)
        self.m = self.buf[:rows * ld].view(rows, ld)
        self.m[:, c0:c1] = vals if f32 else vals.to(torch.bfloat16)
        self.val = self.m[:, c0:c1].double()


class Out:
    """An output of `rows` x `width` at row stride `ld` in a canary buffer with `pad` canary elements (at least a row) on either side."""

    def __init__(self, rows, width, ld, f32=False, pad=None):
        pad = pad if pad is not None else ld
        self.buf = _canary(rows * ld + 2 * pad, f32)
        self.m = self.buf[pad:pad + rows * ld].view(rows, ld)
        self.width = width
        self.written = torch.zeros(self.buf.numel(), dtype=torch.bool, device=DEV)
        self.written[pad:pad + rows * ld].view(rows, ld)[:, :width] = True

    @property
    def val(self):
        return self.m[:, :self.width]

    def check(self, name):
        c = CANARY32 if self.buf.dtype == torch.float32 else CANARY16
        broken = int(((_bits(self.buf) != c) & ~self.written).sum())
        assert broken == 0, f"{name}: {broken} canaries overwritten"
        assert not bool(torch.isnan(self.val.float()).any()), f"{name}: NaN stored (a canary reached an output)"


# ------------------------------------------------------------------------------------------------------------------ tables
def S(N, K, **kw):
    """One segment: N output columns from K input columns.  kin / nout_off: panel windows; bias (default on), relu; site / shift /
    dcol: dropout; mask = (ld_mask, mask_col0, mask_scale); res_add / res_dup: residual backward."""
    return dict(N=N, K=K, **kw)


def L(segs, nout=None, kind="plain", stash=True, ld_stash=None, split=0, residual=0, ms=0.0):
    """One layer: its segments and what its end does -- 'plain' (stash, optionally split), 'ln' (LayerNorm forward) or 'lnb'
    (LayerNorm backward with lnb_mask_scale = ms)."""
    nout = nout if nout is not None else max(s.get("nout_off", 0) + s["N"] for s in segs)
    return dict(segs=segs, nout=nout, kind=kind, stash=stash, ld_stash=ld_stash, split=split, residual=residual, ms=ms)


def _legal(case, ts):
    if ts == 16:
        return True
    wide = [case["K0"]] + [lay["nout"] for lay in case["layers"]] + [s["K"] for lay in case["layers"] for s in lay["segs"]]
    return max(wide) <= 512 and all(s["K"] != 768 for lay in case["layers"] for s in lay["segs"])


def _bitwise_ok(case):
    return all(s.get("dcol", 0) == 0 for lay in case["layers"] for s in lay["segs"])


class Table:
    """The operands of a case: input rows, weight images, vectors, masks, LayerNorm-backward rows and statistics."""

    def __init__(self, case, rows, seed):
        g = torch.Generator(device=DEV).manual_seed(seed)
        rn = lambda *s: torch.randn(*s, generator=g, device=DEV)
        self.case, self.rows = case, rows
        self.K0 = case["K0"]
        self.ldx = case.get("ldx", self.K0 + 8)
        self.X = Inp(rows, 0, self.K0, self.ldx, rn(rows, self.K0))
        self.F = FragImages(DEV)
        self.layers = []
        for li, lay in enumerate(case["layers"]):
            segs = []
            for si, s in enumerate(lay["segs"]):
                W = (rn(s["N"], s["K"]) / math.sqrt(s["K"])).to(torch.bfloat16)
                key = f"{li}.{si}"
                self.F.add(key, W, s["N"], s["K"])
                b = rn(s["N"]) * 0.2 if s.get("bias", True) else None
                mk = None
                if s.get("mask"):
                    ldm, col0, _ = s["mask"]
                    mk = Inp(rows, col0, col0 + s["N"], ldm, rn(rows, s["N"]))
                segs.append(dict(s, key=key, W=W, b=b, mk=mk))
            e = dict(lay, segs=segs)
            n = lay["nout"]
            if lay["kind"] == "ln":
                e["g"], e["be"] = 1 + 0.1 * rn(n), 0.1 * rn(n)
            elif lay["kind"] == "lnb":
                e["g"] = 1 + 0.1 * rn(n)
                y = Inp(rows, 0, n, n, 1.5 + rn(rows, n))            # far from zero: so are the statistics
                y64 = y.val
                mu = y64.mean(1, keepdim=True)
                rs = 1.0 / torch.sqrt(((y64 - mu) ** 2).mean(1, keepdim=True) + 1e-5)
                e["y"], e["mu"], e["rs"] = y, Inp(rows, 0, 1, 1, mu.float(), f32=True), Inp(rows, 0, 1, 1, rs.float(), f32=True)
            self.layers.append(e)
        self.F.finish()
        self.F.refresh()
        p = case.get("p", 0.0)
        self.dev_ctr = torch.tensor([case["dev"]], dtype=torch.int64, device=DEV) if case.get("dev") is not None else None
        self.drop = (p, case.get("seed", 1234), case.get("offset", 0), self.dev_ctr) if p > 0 else None


def _run_chain(T, ts, opts):
    """One mmdeer_chain call into fresh canary buffers; returns {name: Out}."""
    rows = T.rows
    ex = Exec("bf16", T.drop)
    ch = Chain(ex, T.X.m, T.ldx, T.K0, rows, p=T.case.get("p", 0.0), ts=ts)
    nwg = ch.workgroups()
    outs = {}
    for li, lay in enumerate(T.layers):
        for s in lay["segs"]:
            mk = s["mk"]
            ldm, col0, ms = s["mask"] if s.get("mask") else (0, 0, 1.0)
            ch.seg(T.F(s["key"]), s["N"], s["K"], bias=s["b"], relu=s.get("relu", 0), site=s.get("site", -1), shift=s.get("shift", 0),
                   dcol=s.get("dcol", 0), kin=s.get("kin", 0), nout_off=s.get("nout_off", 0), mask=None if mk is None else mk.buf,
                   ldm=ldm, mcol=col0, mscale=ms, res_add=s.get("res_add", 0), res_dup=s.get("res_dup", 0))
        n, split = lay["nout"], lay["split"]
        st = st2 = None
        if lay["stash"]:
            w = split or n
            ld = lay["ld_stash"] or w
            st = outs[f"L{li}.stash"] = Out(rows, w, ld)
            if split:
                st2 = outs[f"L{li}.stash2"] = Out(rows, n - split, ld)
        kw = dict(stash=st and st.m, ld_stash=st.m.stride(0) if st else 0, stash2=st2 and st2.m, split=split)
        if lay["kind"] == "ln":
            xln, mean, rstd = Out(rows, n, n), Out(rows, 1, 1, True, pad=8), Out(rows, 1, 1, True, pad=8)
            outs.update({f"L{li}.xln": xln, f"L{li}.mean": mean, f"L{li}.rstd": rstd})
            ch.end(n, ln=(lay["g"], lay["be"], xln.m, mean.m, rstd.m), residual=lay["residual"], **kw)
        elif lay["kind"] == "lnb":
            dz, part = Out(rows, n, n), Out(nwg, 2 * n, 2 * n, True)
            outs.update({f"L{li}.dz": dz, f"L{li}.part": part})
            ch.end(n, lnb=(lay["g"], lay["y"].buf, lay["mu"].buf, lay["rs"].buf, dz.m, part.m, lay["ms"]), **kw)
        else:
            ch.end(n, **kw)
    with _lib.options(**opts):
        ch.launch()
    torch.cuda.synchronize()
    for name, o in outs.items():
        o.check(name)
    return outs, nwg


def _run_sequence(T):
    """The same layers launch by launch (the rounding points of stackb_train.py's 'ops' plan); returns {name: tensor}."""
    rows = T.rows
    ex = Exec("bf16", T.drop)
    ex.folds = []
    p = T.case.get("p", 0.0)
    new = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device=DEV)
    cur = T.X.m
    res = {}
    for li, lay in enumerate(T.layers):
        n = lay["nout"]
        dup = any(s.get("res_dup", 0) for s in lay["segs"])
        pan = new(rows, n + 256 if dup else n)
        for s in lay["segs"]:
            N, K, kin, no = s["N"], s["K"], s.get("kin", 0), s.get("nout_off", 0)
            ldm, col0, ms = s["mask"] if s.get("mask") else (0, 0, 1.0)
            mk = s["mk"]
            dst = new(rows, N) if s.get("res_add", 0) else pan[:, no:]
            ex.gemm(cur[:, kin:], s["W"], dst, rows, N, K, cur.stride(0), K, dst.stride(0), bias=s["b"], relu=s.get("relu", 0),
                    Y=None if mk is None else mk.m[:, col0:], ldy=ldm, mask_scale=ms, drop_site=s.get("site", -1) if p > 0 else -1,
                    drop_shift=s.get("shift", 0), p=p)
            if s.get("res_add", 0):
                ex.add(pan[:, no:no + N], dst, cur[:, 256:512])
        if dup:
            pan[:, 256:].copy_(pan[:, :256])
        raw = pan[:, :n].contiguous()
        if lay["stash"]:
            sp = lay["split"] or n
            res[f"L{li}.stash"] = raw[:, :sp]
            if lay["split"]:
                res[f"L{li}.stash2"] = raw[:, sp:]
        if lay["kind"] == "ln":
            xln, mean, rstd = ex.ln_fwd(raw, lay["g"], lay["be"])
            if lay["residual"]:
                xln = ex.add(new(rows, n), xln, cur[:, :n])
            res.update({f"L{li}.xln": xln, f"L{li}.mean": mean, f"L{li}.rstd": rstd})
            cur = xln
        elif lay["kind"] == "lnb":
            gg, gb = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
            dz = ex.ln_bwd(raw, lay["y"].m, lay["mu"].m.view(-1), lay["rs"].m.view(-1), lay["g"], gg, gb, lay["ms"])
            res[f"L{li}.dz"] = dz
            res[f"L{li}.part"] = ex.folds[-2][0].view(-1, 2 * n)
            cur = torch.cat([dz, pan[:, 256:]], 1) if dup else dz
        else:
            cur = pan
    torch.cuda.synchronize()
    return res


def _keep(T, site, shift, dcol, N):
    """float64 keep factor [rows][N] of a dropout site: mmdeer_dropout_mask at column (dcol + n) >> shift."""
    p, seed, off, ctr = T.drop
    off += int(ctr.item()) if ctr is not None else 0
    cols = ((dcol + N - 1) >> shift) + 1
    m = torch.empty(T.rows * cols, dtype=torch.uint8, device=DEV)
    _lib.check(_lib.load().mmdeer_dropout_mask(site, T.rows, cols, p, seed, off, m.data_ptr(), _lib.current_stream()))
    idx = (torch.arange(N, device=DEV) + dcol) >> shift
    return m.view(T.rows, cols)[:, idx].double() / (1.0 - p)


def _close(name, got, ref, bound):
    err = (got.double() - ref).abs()
    bad = err > bound
    if bool(bad.any()):
        i = int(torch.argmax((err - bound).flatten()))
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} elements out of bound; worst at {np.unravel_index(i, tuple(err.shape))}: "
                             f"got {float(got.flatten()[i])}, ref {float(ref.flatten()[i])}, bound {float(bound.flatten()[i])}")


def _check_f64(T, outs, ms_rows):
    """Float64, teacher-forced: each layer starts from the chain's own stored input panel.  Returns, per LayerNorm-backward
    layer, the column sums of |d xhat| and |d| (the scale of its gamma / beta gradients)."""
    rows = T.rows
    absums = {}
    cur = T.X.val
    byp = None
    for li, lay in enumerate(T.layers):
        n = lay["nout"]
        pan = torch.zeros(rows, n, dtype=torch.float64, device=DEV)
        tol = torch.zeros_like(pan)
        for s in lay["segs"]:
            N, K, kin, no = s["N"], s["K"], s.get("kin", 0), s.get("nout_off", 0)
            a, w = cur[:, kin:kin + K], s["W"].double()
            v = a @ w.T
            acc = C_BOUND * U * (a.abs() @ w.abs().T)
            if s["b"] is not None:
                v = v + s["b"].double()
            acc = acc + U * v.abs()
            if s.get("relu", 0):
                v = v.clamp_min(0)
            if T.drop is not None and s.get("site", -1) >= 0:
                f = _keep(T, s["site"], s.get("shift", 0), s.get("dcol", 0), N)
                v, acc = v * f, acc * f
            if s.get("mask"):
                f = (s["mk"].val > 0).double() * s["mask"][2]
                v, acc = v * f, acc * f
            if s.get("res_add", 0):
                acc = acc + UB * v.abs()            # the product is stored as bf16 before the bypass is added
                v = v + byp
            pan[:, no:no + N] = v
            tol[:, no:no + N] = acc + UB * v.abs()
        raw = None
        if lay["stash"]:
            sp = lay["split"] or n
            got = outs[f"L{li}.stash"].val
            if lay["split"]:
                got = torch.cat([got, outs[f"L{li}.stash2"].val], 1)
            _close(f"L{li} raw panel", got, pan, tol)
            raw = got.double()
        if lay["kind"] == "ln":
            y = raw
            mu = y.mean(1, keepdim=True)
            rs = 1.0 / torch.sqrt(((y - mu) ** 2).mean(1, keepdim=True) + 1e-5)
            xh = (y - mu) * rs
            g, be = lay["g"].double(), lay["be"].double()
            o = xh * g + be
            t = 256 * U * (g.abs() * (xh.abs() + rs * mu.abs() + 1) + be.abs()) + UB * o.abs()
            if lay["residual"]:
                o = o + cur[:, :n]
            _close(f"L{li} mean", outs[f"L{li}.mean"].val, mu, 64 * U * y.abs().amax(1, keepdim=True) + 1e-30)
            _close(f"L{li} rstd", outs[f"L{li}.rstd"].val, rs, 64 * U * rs)
            _close(f"L{li} xln", outs[f"L{li}.xln"].val, o, t + UB * o.abs())
            cur, byp = outs[f"L{li}.xln"].val.double(), None
        elif lay["kind"] == "lnb":
            d = raw if raw is not None else pan
            y, mu, rs = lay["y"].val, lay["mu"].val, lay["rs"].val
            xh = (y - mu) * rs
            gd = d * lay["g"].double()
            m1, m2 = gd.mean(1, keepdim=True), (gd * xh).mean(1, keepdim=True)
            dz = (gd - m1 - xh * m2) * rs
            scale = rs * (gd.abs() + gd.abs().mean(1, keepdim=True) + xh.abs() * (gd * xh).abs().mean(1, keepdim=True))
            t = 32 * U * scale + (0 if raw is not None else 4 * UB * scale)
            if lay["ms"] > 0:
                f = (y > 0).double() * lay["ms"]
                dz, t = dz * f, t * f
            _close(f"L{li} dz", outs[f"L{li}.dz"].val, dz, t + UB * dz.abs())
            # partial slabs: workgroup w sums its ms_rows rows
            part = outs[f"L{li}.part"].val.double()
            nwg = part.shape[0]
            dx, aa, ab = d * xh, (d * xh).abs(), d.abs()
            pad = nwg * ms_rows - rows
            fold = lambda z: torch.cat([z, torch.zeros(pad, n, dtype=z.dtype, device=DEV)]).view(nwg, ms_rows, n).sum(1)
            c = 32 * U + (0 if raw is not None else 2 * UB)     # without a stash, d is the float64 panel: add its bf16 rounding
            _close(f"L{li} dgamma partials", part[:, :n], fold(dx), c * fold(aa) + 1e-30)
            _close(f"L{li} dbeta partials", part[:, n:], fold(d), c * fold(ab) + 1e-30)
            absums[f"L{li}.part"] = torch.cat([aa.sum(0), ab.sum(0)])
            byp = raw
            dzv = outs[f"L{li}.dz"].val.double()
            dup = any(s.get("res_dup", 0) for s in lay["segs"])
            cur = torch.cat([dzv, raw], 1) if dup else dzv
        else:
            dup = any(s.get("res_dup", 0) for s in lay["segs"])
            byp = raw
            cur = torch.cat([raw, raw], 1) if dup else raw
    return absums


def _run_case(case, kernel, rows, seed=0):
    K = KERNELS[kernel] if isinstance(kernel, str) else kernel
    ts = K["ts"]
    T = Table(case, rows, seed)
    outs, nwg = _run_chain(T, ts, K["opts"])
    assert nwg == _lib.load().mmdeer_chain_workgroups(rows, ts)
    ms_rows = 16 if (ts == 16 or (ts == 0 and rows <= 4096)) else 32
    # 4. determinism
    again, _ = _run_chain(T, ts, K["opts"])
    for name in outs:
        assert torch.equal(_bits(outs[name].val), _bits(again[name].val)), f"{name}: a second run stored different bits"
    # 2. float64, teacher-forced
    absums = _check_f64(T, outs, ms_rows)
    # 1. bit for bit against the launch-by-launch sequence
    if _bitwise_ok(case):
        ref = _run_sequence(T)
        for name, r in ref.items():
            got = outs[name].val
            if name.endswith(".part") and ms_rows == 32:
                fg, fr = got.double().sum(0), r.double().sum(0)
                assert bool(((fg - fr).abs() <= 64 * U * absums[name] + 1e-30).all()), f"{name}: folded gamma / beta gradients"
                continue
            if name.endswith(".mean") or name.endswith(".rstd"):
                got = got.reshape(-1)
            assert got.shape == r.shape, (name, got.shape, r.shape)
            eq = _bits(got.contiguous()) == _bits(r.contiguous())
            assert bool(eq.all()), f"{name}: {int((~eq).sum())} of {eq.numel()} elements differ from the launch-by-launch sequence"


# --------------------------------------------------------------------------------------------------------------- the cases
def _cases():
    c = {}
    c["bias_relu"] = dict(K0=256, layers=[L([S(256, 256, relu=1)]), L([S(128, 256, bias=False)])])
    for K in (64, 128, 256, 384, 512, 768):
        c[f"k{K}_t128"] = dict(K0=K, layers=[L([S(256, K, relu=1)]), L([S(128, 128, kin=128)])])
        c[f"k{K}_t128x4"] = dict(K0=K, layers=[L([S(512, K)])])
    for K in (128, 256):
        c[f"k{K}_t64"] = dict(K0=K, layers=[L([S(192, K, relu=1)]), L([S(64, 128, kin=64)])])
    c["windows_3seg"] = dict(K0=512, layers=[
        L([S(128, 256, kin=256), S(256, 128, kin=128, nout_off=128), S(128, 64, nout_off=384, relu=1)]),
        L([S(64, 128, kin=384), S(128, 256, kin=128, nout_off=64)]), L([S(128, 192 - 64, kin=64)])])
    c["windows_2seg_64"] = dict(K0=384, layers=[L([S(64, 256, kin=128), S(192, 128, nout_off=64)])])
    for p in (0.1, 0.5):
        for sh in (0, 5):
            c[f"drop_p{p}_shift{sh}"] = dict(K0=256, p=p, offset=11, layers=[
                L([S(256, 256, relu=1, site=3, shift=sh)]), L([S(192, 256, site=4, shift=sh)])])
    c["drop_offset_dev"] = dict(K0=256, p=0.5, offset=5, dev=7, layers=[L([S(256, 256, relu=1, site=2)]), L([S(128, 256, site=6)])])
    c["drop_dcol"] = dict(K0=256, p=0.1, offset=3, layers=[L([S(128, 256, site=1, dcol=384), S(128, 256, site=1, dcol=96, nout_off=128)])])
    c["drop_dcol_shift"] = dict(K0=256, p=0.5, dev=9, layers=[L([S(192, 256, site=1, shift=5, dcol=200)])])
    c["mask"] = dict(K0=256, layers=[L([S(256, 256, mask=(456, 64, 1.25))]), L([S(192, 128, mask=(200, 8, 0.5))])])
    c["mask_drop"] = dict(K0=256, p=0.5, offset=1, layers=[L([S(256, 256, relu=1, site=5, mask=(328, 72, 2.0))])])
    for n in (256, 512):
        for r in (0, 1):
            c[f"ln{n}_res{r}"] = dict(K0=n, layers=[L([S(n, n if n == 256 else 512, relu=1)], kind="ln", residual=r, ld_stash=n + 64),
                                                     L([S(128, 256, kin=n - 256)])])
        for ms in (0.0, -1.0, 1.25):
            c[f"lnb{n}_ms{ms}"] = dict(K0=256, layers=[L([S(n, 256)], kind="lnb", ms=ms), L([S(128, 256, kin=n - 256)])])
    c["lnb_nostash"] = dict(K0=256, layers=[L([S(256, 256)], kind="lnb", ms=1.25, stash=False)])
    c["lnb_last_seg_one_tile"] = dict(K0=256, layers=[L([S(128, 256), S(128, 256, nout_off=128)], kind="lnb", ms=2.0)])
    c["lnb_last_seg_one_tile_k64"] = dict(K0=256, layers=[L([S(128, 256), S(128, 64, kin=64, nout_off=128)], kind="lnb", ms=1.25)])
    c["lnb_last_seg_k64"] = dict(K0=256, layers=[L([S(256, 256), S(256, 64, kin=192, nout_off=256)], kind="lnb", ms=1.0)])
    c["lnb_masked_seg"] = dict(K0=256, layers=[L([S(256, 256, mask=(264, 0, 1.25))], kind="lnb", ms=1.25)])
    c["residual_bwd"] = dict(K0=256, layers=[
        L([S(256, 256, bias=False, res_dup=1)], kind="lnb", ms=1.25),
        L([S(256, 256, bias=False, res_add=1, res_dup=1)], kind="lnb", ms=1.25),
        L([S(256, 256, bias=False, res_add=1)], kind="lnb", ms=0.0)])
    c["residual_bwd_plain"] = dict(K0=256, layers=[L([S(256, 256, res_dup=1)]), L([S(256, 256, res_add=1)])])
    for sp in (8, 40, 64, 200, 448):
        c[f"split{sp}"] = dict(K0=256, layers=[L([S(512, 256)], split=sp, ld_stash=max(sp, 512 - sp) + 24)])
    c["split_ld_eq"] = dict(K0=256, layers=[L([S(256, 256), S(128, 128, nout_off=256)], split=128, ld_stash=256)])
    c["ldx_eq_K0"] = dict(K0=256, ldx=256, layers=[L([S(128, 256)])])
    c["ldx_wide"] = dict(K0=128, ldx=128 + 200, layers=[L([S(256, 128, relu=1)])])
    c["segs12"] = dict(K0=256, layers=[L([S(128, 128, relu=1), S(128, 128, kin=128, nout_off=128)]) for _ in range(6)])
    c["layers12"] = dict(K0=128, layers=[L([S(128, 128, relu=i & 1, bias=i % 3 != 0)]) for i in range(12)])
    c["vec_floats_4864"] = dict(K0=512, layers=[L([S(512, 512, relu=1)], kind="ln") for _ in range(3)] + [L([S(256, 512)])])
    c["vecs16"] = dict(K0=256, layers=[L([S(256, 256, relu=1)], kind="ln") for _ in range(5)] + [L([S(128, 256)])])
    return c


CASES = _cases()
FEATURE_PARAMS = [pytest.param(name, k, id=f"{name}-{k}") for name, case in CASES.items() for k in KERNELS if _legal(case, KERNELS[k]["ts"])]


@pytest.mark.parametrize("name,kernel", FEATURE_PARAMS)
def test_chain_feature(name, kernel):
    _run_case(CASES[name], kernel, rows=47, seed=len(name))


MIXED = dict(K0=256, p=0.5, offset=2, dev=3, layers=[
    L([S(256, 256, relu=1, site=1)], kind="ln"),
    L([S(256, 256, mask=(264, 8, 1.25), res_dup=1)], kind="lnb", ms=1.25),
    L([S(128, 256, site=2, shift=5), S(128, 128, kin=128, nout_off=128)], kind="lnb", ms=0.0),
    L([S(192, 256, relu=1)], split=64, ld_stash=136)])


@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("rows", [1, 15, 16, 17, 31, 32, 33, 47])
def test_chain_row_counts(rows, kernel):
    _run_case(MIXED, kernel, rows=rows, seed=rows)


@pytest.mark.parametrize("rows", [4096, 4097])
def test_chain_workgroup_switch_point(rows):
    """samples_per_workgroup = 0: 16-sample workgroups up to 4096 rows, 32-sample ones above."""
    assert _lib.load().mmdeer_chain_workgroups(rows, 0) == (256 if rows == 4096 else 129)
    _run_case(MIXED, dict(ts=0, opts=dict(chain_depth=4)), rows=rows, seed=rows)


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_chain_large_ragged_grid(kernel):
    """10001 rows: more workgroups than one round of the chip holds, a ragged last one."""
    _run_case(MIXED, kernel, rows=10001, seed=5)


def _random_case(rng, ts):
    cap = 768 if ts == 16 else 512
    K0 = int(rng.choice([64, 128, 256, 384, 512] + ([768] if ts == 16 else [])))
    p = float(rng.choice([0.0, 0.1, 0.5]))
    layers, width, dup = [], K0, False
    for li in range(int(rng.integers(2, 5))):
        kind = str(rng.choice(["plain", "ln", "lnb"]))
        segs, nout = [], 0
        nseg = 1 if kind == "ln" else int(rng.integers(1, 4))
        target = int(rng.choice([256, 512])) if kind != "plain" else cap
        for si in range(nseg):
            ks = [k for k in (64, 128, 256, 384, 512, 768) if k <= width and (k != 768 or ts == 16)]
            K = int(rng.choice(ks))
            kin = int(rng.integers(0, (width - K) // 64 + 1)) * 64
            rest = target - nout if kind != "plain" else cap - nout
            ns = [n for n in (64, 128, 192, 256, 384, 512) if n <= rest and (n % 128 == 0 or K in (128, 256)) and n // (128 if n % 128 == 0 else 64) <= 4]
            if kind != "plain" and si == nseg - 1:
                ns = [n for n in ns if n == rest]
            if not ns:
                break
            N = int(rng.choice(ns))
            s = S(N, K, kin=kin, nout_off=nout, relu=int(rng.integers(0, 2)), bias=bool(rng.integers(0, 2)))
            if p > 0 and rng.integers(0, 2):
                s.update(site=int(rng.integers(0, 8)), shift=int(rng.choice([0, 5])))
            if rng.integers(0, 3) == 0:
                s["mask"] = (N + 8 * int(rng.integers(0, 3)), 0, float(rng.choice([1.0, 1.25])))
            segs.append(s)
            nout += N
        if not segs or (kind != "plain" and nout != target):
            kind = "plain"
        if not segs:
            break
        residual = int(kind == "ln" and nout == width and not dup and rng.integers(0, 2))
        layers.append(L(segs, nout=nout, kind=kind, residual=residual, ms=float(rng.choice([0.0, 1.25])), ld_stash=nout + 8 * int(rng.integers(0, 3))))
        width = nout
    return dict(K0=K0, p=p, offset=int(rng.integers(0, 100)), layers=layers)


@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("seed", range(6))
def test_chain_random_tables(seed, kernel):
    """Seeded random tables mixing segment windows, 64- and 128-column tiles, every K, dropout, masks, LayerNorm forward and backward."""
    ts = KERNELS[kernel]["ts"]
    rng = np.random.default_rng(1000 * seed + ts)
    case = _random_case(rng, ts)
    rows = int(rng.integers(1, 6 * ts))
    _run_case(case, kernel, rows=rows, seed=seed)


def test_chain_kernel_table_is_complete():
    """Every kernel of KERNELS takes part in the feature cases, and K = 768 and 768-wide panels run on 16-sample workgroups only."""
    kernels = {k for _, k in (p.values for p in FEATURE_PARAMS)}
    assert kernels == set(KERNELS)
    assert not any(k == "s32" and n.startswith("k768") for n, k in (p.values for p in FEATURE_PARAMS))


# ------------------------------------------------------------------------------------------------------- mmdeer_repack
def test_repack_many_jobs_with_canaries():
    """mmdeer_repack with 150 jobs (three launches of at most 64): row-major and fragment-major, plain and transposed, with
    cols_valid < cols; every destination image sits between canaries, which must stay intact."""
    lib = _lib.load()
    g = torch.Generator(device=DEV).manual_seed(3)
    jobs = (_lib.RepackJob * 150)()
    keep, expect = [], []
    for j in range(150):
        tr, layout = j % 2, (j // 2) % 2
        rows, cols = (64, 32 + 16 * (j % 3)) if tr else (16 * (1 + j % 3), 64 * (1 + j % 2))
        cv = cols - 8 * (j % 3) if j % 5 else cols
        ld_src = cols + 8
        src = torch.randn(rows, ld_src, generator=g, device=DEV).to(torch.bfloat16)
        S_ = src[:, :cols].clone()
        S_[:, cv:] = 0
        img = S_.T.contiguous() if tr else S_
        R, Cn = img.shape
        if layout == 1:
            # fragment-major: granule ((wt * (Cn / 64) + kt) * 2 + c) * 64 + lane = img[16 wt + (lane & 15)][64 kt + 32 c + 8 (lane >> 4) ...]
            ref = img.view(R // 16, 16, Cn // 64, 2, 4, 8).permute(0, 2, 3, 4, 1, 5).reshape(-1)
            ld_dst, dst_col, n = 0, 0, R * Cn
        else:
            ld_dst, dst_col = Cn + 16, 8
            n = R * ld_dst
            ref = None
        buf = _canary(n + 128, False)
        dst = buf[64:64 + n]
        jb = jobs[j]
        jb.src, jb.dst, jb.ld_src, jb.rows, jb.cols, jb.cols_valid = src.data_ptr(), dst.data_ptr(), ld_src, rows, cols, cv
        jb.transpose, jb.layout, jb.ld_dst, jb.dst_col = tr, layout, ld_dst, dst_col
        keep.append((src, buf))
        expect.append((buf, img, ref, layout, ld_dst, dst_col, n))
    _lib.check(lib.mmdeer_repack(jobs, 150, _lib.current_stream()))
    torch.cuda.synchronize()
    for j, (buf, img, ref, layout, ld_dst, dst_col, n) in enumerate(expect):
        written = torch.zeros(buf.numel(), dtype=torch.bool, device=DEV)
        if layout == 1:
            written[64:64 + n] = True
            assert torch.equal(_bits(buf[64:64 + n]), _bits(ref)), f"job {j}: fragment-major image"
        else:
            R, Cn = img.shape
            m = buf[64:64 + n].view(R, ld_dst)
            written[64:64 + n].view(R, ld_dst)[:, dst_col:dst_col + Cn] = True
            assert torch.equal(_bits(m[:, dst_col:dst_col + Cn]), _bits(img)), f"job {j}: row-major image"
        assert int(((_bits(buf) != CANARY16) & ~written).sum()) == 0, f"job {j}: canaries overwritten"
