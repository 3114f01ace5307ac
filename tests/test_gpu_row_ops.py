"""The row operators of Stack B (csrc/stackb.hip, csrc/stackb_train.hip) and of the alternative fusion modules
(csrc/fusions.hip) on their own, called through the C ABI (include/mmdeer.h): residual_ln, attn_mix (eval, training forward,
backward), gate_mix / _bwd, head / _bwd, add_masked, softmax_mix_fwd / _bwd, outer_fwd / _bwd.

Every operator, in fp32 and in bf16 storage, gets
1. a float64 reference written here from the header's formulas, on the stored inputs (bf16 upcast), backward references from
   torch.autograd on that float64 forward; a mask a backward reads from stored data (r > 0, h2 > 0, tri > 0, add_masked's mask)
   is taken from those same stored bits;
2. NaN canaries: every output sits in a canary buffer (a row above, a row below, pad columns up to its leading dimension),
   inputs carry canaries in their pad columns; afterwards all canaries are intact and no stored value is a NaN;
3. determinism: two runs store the same bits;
4. B == 0 / M == 0: returns 0 with every pointer NULL;
5. refusals (-1, a message that names the problem, nothing written), the misaligned pointers among them.

Bounds: |got - ref| <= K * U * scale (+ UB * |ref| for a bf16 output, + TINY), scale = the float64 sum of the absolute values of
the terms that form the output, an earlier value's scale carried on times the absolute derivative.  K per operator and output
is four times the largest ratio |got - ref| / (U * scale) measured on an MI355X, rounded up to a power of two, at least C_BOUND;
the measured ratio stands next to each K below and K * U stays below 2**-12, so that a wrong term, lane or index (an error of
the order of scale) is at least 4096 bounds away.  TINY = 2**-126, the smallest normal fp32: a term below it (exp(-100) of an
underflowing softmax weight or sigmoid) is zero or a denormal as the kernel's denormal mode has it, which these tests do not
pin.  No element is excused, except the calibrated plane of the head on rows whose total uncertainty is not finite."""
import ctypes as C

import numpy as np
import pytest
import torch

from mmdeer import _lib

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CANARY32 = 0x7FA5A5A5          # a NaN no kernel produces (payload), as int32 / float32 bits
CANARY16 = 0x7FA5              # the same for bf16 storage
U = 2.0 ** -24                 # unit roundoff of the fp32 arithmetic
UB = 2.0 ** -8                 # unit roundoff of bf16 storage (half an ulp, relative)
TINY = 2.0 ** -126             # smallest normal fp32
C_BOUND = 8.0                  # the project's floor for K (test_gpu_gemm_routes.py)
WAVE_B = (1, 3, 4, 5, 7, 130)  # wave-per-sample kernels: 4 samples per workgroup, partial last workgroups, many workgroups

# operator.output -> K;  the comment is the largest |got - ref| / (U * scale) measured on an MI355X (fp32 and bf16 storage)
K = {
    "residual_ln.out": 8.0,                # measured 1.178
    "attn_mix.unc": 8.0,                   # measured 1.34
    "attn_mix.weights": 8.0,               # measured 1.704
    "attn_mix.out": 16.0,                  # measured 2.186
    "attn_mix.r": 16.0,                    # measured 2.763
    "attn_mix_bwd.d_self": 8.0,            # measured 1.257
    "attn_mix_bwd.d_cross": 8.0,           # measured 1.41
    "attn_mix_bwd.d_logits8": 8.0,         # measured 0.1569
    "attn_mix_bwd.d_pre": 8.0,             # measured 0.1665
    "attn_mix_bwd.d_z8": 8.0,              # measured 1.232
    "attn_mix_bwd.d_h2": 8.0,              # measured 1.233
    "gate_mix.out": 16.0,                  # measured 2.372
    "gate_mix_bwd.dg": 32.0,               # measured 4.253
    "gate_mix_bwd.dtri": 16.0,             # measured 2.902
    "gate_mix_bwd.dav": 8.0,               # measured 1.888
    "add_masked.out": 8.0,                 # measured 1
    "head.nu_alpha_beta": 8.0,             # measured 1.999
    "head.uncertainties": 8.0,             # measured 1.842
    "head.calibrated": 8.0,                # measured 0.1379
    "head_bwd.dev": 16.0,                  # measured 2.336
    "softmax_mix.weights8": 16.0,          # measured 2.374
    "softmax_mix.out": 8.0,                # measured 1.023
    "softmax_mix_bwd.dlogits8": 8.0,       # measured 0.9045
    "softmax_mix_bwd.dP": 8.0,             # measured 1.584
    "outer_fwd.z": 8.0,                    # measured 0.9999
    "outer_bwd.dx1": 8.0,                  # measured 1.904
    "outer_bwd.dx2": 16.0,                 # measured 2.224
}
assert all(C_BOUND <= k and k * U < 2.0 ** -12 for k in K.values())
RATIOS = {}


# ---------------------------------------------------------------------------------------------------------------- plumbing
def _stream():
    return torch.cuda.current_stream().cuda_stream


def _lib_err():
    return _lib.load().mmdeer_last_error().decode()


def _canary(n, f32):
    if f32:
        return torch.full((max(n, 1),), CANARY32, dtype=torch.int32, device=DEV).view(torch.float32)
    return torch.full((max(n, 1),), CANARY16, dtype=torch.int16, device=DEV).view(torch.bfloat16)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16)


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, device=DEV)


def _store(v, f32):
    """The values as the operator's storage holds them."""
    return v.float() if f32 else v.to(torch.bfloat16)


class Mat:
    """`rows` rows at row stride `ld` in a canary buffer, a canary row above and one below.  The column windows `wins`
    ((c0, c1) pairs, default (0, width)) hold values -- `vals`, stored in the buffer's type, for an input, or what the operator
    writes for an output -- and every other element is a canary."""

    def __init__(self, rows, width, ld, f32, vals=None, wins=None):
        self.f32, self.rows, self.ld = bool(f32), rows, ld
        self.wins = wins if wins is not None else [(0, width)]
        self.buf = _canary((rows + 2) * ld, f32)
        self.m = self.buf[ld:ld + rows * ld].reshape(rows, ld)
        self.written = torch.zeros(self.buf.numel(), dtype=torch.bool, device=DEV)
        for c0, c1 in self.wins:
            self.written[ld:ld + rows * ld].reshape(rows, ld)[:, c0:c1] = True
        if vals is not None:
            c0, c1 = self.wins[0]
            self.m[:, c0:c1] = _store(vals, f32)

    def ptr(self, col=None):
        col = self.wins[0][0] if col is None else col
        return self.m.data_ptr() + col * self.m.element_size()

    def win(self, i=0):
        c0, c1 = self.wins[i]
        return self.m[:, c0:c1]

    @property
    def val(self):
        return self.win(0)

    @property
    def d(self):
        return self.val.double()

    def snap(self):
        return _bits(self.buf).clone()

    def check(self, name, nan_ok=False):
        c = CANARY32 if self.f32 else CANARY16
        broken = int(((_bits(self.buf) != c) & ~self.written).sum())
        assert broken == 0, f"{name}: {broken} canaries overwritten"
        if not nan_ok:
            for i in range(len(self.wins)):
                assert not bool(torch.isnan(self.win(i).float()).any()), f"{name}: NaN stored (a canary reached an output)"

    def untouched(self, name):
        c = CANARY32 if self.f32 else CANARY16
        assert bool((_bits(self.buf) == c).all()), f"{name}: written by a refused call"


def _close(name, got, ref, bound):
    err = (got.double() - ref).abs()
    bad = ~(err <= bound)
    if bool(bad.any()):
        i = int(torch.argmax(torch.where(bad, err - bound, torch.full_like(err, -1.0)).flatten()))
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} elements out of bound; worst at {np.unravel_index(i, tuple(err.shape))}: "
                             f"got {float(got.flatten()[i])}, ref {float(ref.flatten()[i])}, bound {float(bound.flatten()[i])}")


def _check(key, name, got, ref, scale, bf16_out=False, inf_ok=False):
    """|got - ref| <= K[key] * U * scale + TINY (+ UB * |ref|).  Where the float64 reference is not finite (inf_ok: the head's
    constructed rows) the stored value must be the same infinity / a NaN for a NaN.  Prints the measured ratio first."""
    got, ref, scale = got.detach().double().reshape(-1), ref.detach().double().reshape(-1), scale.detach().double().reshape(-1)
    fin = torch.isfinite(ref)
    if not inf_ok:
        assert bool(fin.all()), f"{name}: the float64 reference is not finite"
    elif not bool(fin.all()):
        same = (got == ref) | (torch.isnan(got) & torch.isnan(ref))
        assert bool(same[~fin].all()), f"{name}: {int((~same[~fin]).sum())} elements differ from a non-finite reference"
    got, ref, scale = got[fin], ref[fin], scale[fin]
    assert bool(torch.isfinite(scale).all()) and bool((scale >= 0).all()), f"{name}: bad scale"
    fixed = TINY + (UB * ref.abs() if bf16_out else 0.0)
    excess = ((got - ref).abs() - fixed).clamp_min(0.0)
    ratio = torch.where(scale > 0, excess / (U * scale.clamp_min(1e-300)), torch.where(excess > 0, torch.full_like(excess, float("inf")), torch.zeros_like(excess)))
    r = float(ratio.max()) if ratio.numel() else 0.0
    RATIOS[key] = max(RATIOS.get(key, 0.0), r)
    print(f"RATIO {key} {r:.4g}  ({name})")
    _close(name, got, ref, K[key] * U * scale + fixed)


def _same_bits(name, a, b):
    assert torch.equal(a, b), f"{name}: two runs differ in {int((a != b).sum())} stored elements"


def _zero_bits(name, t):
    """Exact (positive) zeros."""
    n = int((_bits(t.contiguous()) != 0).sum())
    assert n == 0, f"{name}: {n} elements are not exact zeros"


def _refused(name, rc, word, outs):
    assert rc == -1, f"{name}: accepted (rc {rc})"
    msg = _lib_err()
    assert word in msg, f"{name}: the message '{msg}' does not name '{word}'"
    for i, o in enumerate(outs):
        o.untouched(f"{name} output {i}")


def _off(ptr, f32):
    """A pointer one element past `ptr`: not on 4 elements."""
    return ptr + (4 if f32 else 2)


def _softmax_scale(w, lg, slg):
    """Scale of w = softmax(lg): w_k + sum_j |w_k (delta_kj - w_j)| e_j, where e_j = slg_j (the scale of lg_j) + |lg_j - max lg|
    (the subtraction in front of the exponential)."""
    e = slg + (lg - lg.max(-1, keepdim=True).values).abs()
    return w + w * ((1.0 - w) * e + (w * e).sum(-1, keepdim=True) - w * e)


def _softmax_bwd_scale(w, sw, dw, sdw):
    """Scale of ds = w (dw - sum_j w_j dw_j) with w and dw known to sw and sdw."""
    dot = (w * dw).sum(-1, keepdim=True)
    return w * (sdw + (w * sdw).sum(-1, keepdim=True)) + sw * (dw - dot).abs() + w * (sw * dw.abs()).sum(-1, keepdim=True)


# ============================================================================================================ residual_ln
def _ln_call(y, x, gamma, beta, out, M, N, f32, ld_y=None, ld_x=None, ld_out=None):
    rc = _lib.load().mmdeer_stackb_residual_ln(y.ptr(), ld_y or y.ld, x.ptr() if x is not None else None, (ld_x or x.ld) if x is not None else 0,
                                               gamma.data_ptr(), beta.data_ptr(), out.ptr(), ld_out or out.ld, M, N, f32, _stream())
    torch.cuda.synchronize()
    return rc


def _ln_inputs(M, N, f32, seed):
    g = _gen(seed)
    y = _randn(g, M, N) * (1.0 + torch.arange(M, device=DEV).float()[:, None])
    y[0] = 100.0 + 0.01 * _randn(g, N)              # mean 100, spread 0.01: the kernel centres before it squares
    if M >= 3:
        y[2] = -3.25                                # a constant row: variance 0
    return y, _randn(g, M, N), 1.0 + 0.5 * _randn(g, N), 0.3 * _randn(g, N)


def _ln_ref(y, x, gamma, beta):
    N = y.shape[1]
    mean = y.mean(1, keepdim=True)
    v = y - mean
    sv = y.abs() + y.abs().mean(1, keepdim=True)
    var = (v * v).mean(1, keepdim=True)
    svar = (2.0 * v.abs() * sv + v * v).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    srstd = rstd + 0.5 * rstd ** 3 * (svar + 1e-5)
    ref = v * rstd * gamma + beta
    scale = (v * rstd * gamma).abs() + beta.abs() + gamma.abs() * (sv * rstd + v.abs() * srstd)
    if x is not None:
        ref, scale = ref + x, scale + x.abs()
    return ref, scale


@pytest.mark.parametrize("f32", [1, 0])
def test_residual_ln(f32):
    """M in {1, 3, 4, 5, 7, 130} x N in {256, 512}, x NULL and given, every leading dimension its own and > N, a row of mean 100
    and spread 0.01, a constant row, out aliasing x."""
    for i, M in enumerate(WAVE_B):
        for N in (256, 512):
            for with_x in (0, 1, 2):            # 2: out aliases x
                yv, xv, gamma, beta = _ln_inputs(M, N, f32, 100 + i)
                y = Mat(M, N, N + 8, f32, yv)
                x = Mat(M, N, N + 12, f32, xv) if with_x else None
                ref, scale = _ln_ref(y.d, x.d if x is not None else None, gamma.double(), beta.double())
                name = f"residual_ln f32={f32} M={M} N={N} x={with_x}"
                snaps = []
                for _ in range(2):
                    if with_x == 2:
                        x = Mat(M, N, N + 12, f32, xv)
                        out = x
                    else:
                        out = Mat(M, N, N + 4, f32)
                    assert _ln_call(y, x, gamma, beta, out, M, N, f32) == 0, f"{name}: {_lib_err()}"
                    out.check(name)
                    snaps.append(out.snap())
                y.check(name + " (y)")
                _same_bits(name, *snaps)
                _check("residual_ln.out", name, out.val, ref, scale, not f32)


@pytest.mark.parametrize("f32", [1, 0])
def test_residual_ln_refusals(f32):
    lib = _lib.load()
    assert lib.mmdeer_stackb_residual_ln(None, 0, None, 0, None, None, None, 0, 0, 256, f32, _stream()) == 0, _lib_err()
    yv, xv, gamma, beta = _ln_inputs(1, 256, f32, 7)
    y, x, out = Mat(1, 256, 264, f32, yv), Mat(1, 256, 264, f32, xv), Mat(1, 256, 264, f32)
    _refused("N=128", _ln_call(y, x, gamma, beta, out, 1, 128, f32), "N=128", [out])
    _refused("ld_y < N", _ln_call(y, x, gamma, beta, out, 1, 256, f32, ld_y=252), "leading dimension", [out])
    _refused("ld_out % 4", _ln_call(y, x, gamma, beta, out, 1, 256, f32, ld_out=258), "leading dimension", [out])
    _refused("ld_x < N", _ln_call(y, x, gamma, beta, out, 1, 256, f32, ld_x=128), "leading dimension", [out])
    for who in ("y", "x", "out"):
        p = {"y": y.ptr(), "x": x.ptr(), "out": out.ptr()}
        p[who] = _off(p[who], f32)
        rc = lib.mmdeer_stackb_residual_ln(p["y"], 264, p["x"], 264, gamma.data_ptr(), beta.data_ptr(), p["out"], 264, 1, 256, f32, _stream())
        torch.cuda.synchronize()
        _refused(f"misaligned {who}", rc, "misaligned", [out])


# ====================================================================================== attn_mix: eval, training forward, backward
def _attn_params(variant, ld_w1, seed):
    g = _gen(seed)
    w3, b3 = 0.3 * _randn(g, 64), torch.tensor([0.2], device=DEV)
    w1u = 0.5 * _randn(g, 256, 3)
    w2 = 0.5 * _randn(g, 3, 256)                      # distinct rows
    b2 = torch.tensor([0.3, -0.2, 0.1], device=DEV)
    if variant == "equal":                            # three equal logits in every row
        w2 = w2[:1].repeat(3, 1)
        b2 = torch.full((3,), 0.3, device=DEV)
    # weight_network.0.weight [256][771]: canaries around the three columns wn_w1_unc addresses
    W1 = Mat(256, 3, ld_w1, 1, w1u, wins=[(ld_w1 - 3, ld_w1)])
    return dict(w3=w3, b3=b3, W1=W1, w1u=W1.d, w2=w2.contiguous(), b2=b2, ld_w1=ld_w1)


def _attn_inputs(B, f32, variant, P, seed):
    g = _gen(seed)
    mod = (1.0 + torch.arange(3, device=DEV).float())[None, :, None]       # modality m scaled by 1 + m
    h2 = _randn(g, B, 3, 64) * mod
    idx = torch.arange(B * 3 * 64, device=DEV).reshape(B, 3, 64)
    h2[idx % 7 == 0] = 0.0
    h2[idx % 7 == 1] = -0.0
    pre = _randn(g, B, 256)
    if variant == "spread":                           # rows 0, 2, ..: logit 0 exceeds logit 1 by far more than 100
        pre[0::2] = 4.0 * (P["w2"][0] - P["w2"][1])
    s, c = _randn(g, B, 3, 256) * mod, _randn(g, B, 3, 256) * mod
    return dict(h2=Mat(3 * B, 64, 64, f32, h2.reshape(3 * B, 64)), pre=Mat(B, 256, 256, f32, pre), s=Mat(B, 768, 768, f32, s.reshape(B, 768)),
                c=Mat(B, 768, 768, f32, c.reshape(B, 768)))


def _attn_forward64(I, P, B, fac, forced):
    """float64 forward.  fac [B][256]: the dropout keep factor (forced False: hidden = relu(.) * fac) or the stored mask
    (r > 0) * mask_scale (forced True: hidden = (.) * fac, the teacher-forced form the backward differentiates)."""
    h2, pre, s, c = I["h2"], I["pre"], I["s"], I["c"]
    w3, b3, w1u, w2, b2 = P["w3"].double(), P["b3"].double(), P["w1u"], P["w2"].double(), P["b2"].double()
    z = (h2 * w3).sum(-1) + b3
    u = torch.sigmoid(z)
    hp = pre + u @ w1u.t()
    h = hp * fac if forced else torch.relu(hp) * fac
    lg = h @ w2.t() + b2
    w = torch.softmax(lg, -1)
    out = w[:, :, None] * s + (1.0 - u)[:, :, None] * c
    with torch.no_grad():
        sz = (h2 * w3).abs().sum(-1) + b3.abs()
        su = u + u * (1.0 - u) * sz
        shp = pre.abs() + (u[:, None, :] * w1u[None]).abs().sum(-1) + su @ w1u.abs().t()
        sh = shp * fac.abs()
        slg = (h.abs() + sh) @ w2.abs().t() + b2.abs()
        sw = _softmax_scale(w, lg, slg)
        sout = (w[:, :, None] * s).abs() + ((1.0 - u)[:, :, None] * c).abs() + sw[:, :, None] * s.abs() + su[:, :, None] * c.abs()
    return dict(z=z, u=u, h=h, lg=lg, w=w, out=out, su=su, sh=sh, sw=sw, sout=sout)


def _attn_leaves(I, B, grad=False):
    d = dict(h2=I["h2"].d.reshape(B, 3, 64), pre=I["pre"].d, s=I["s"].d.reshape(B, 3, 256), c=I["c"].d.reshape(B, 3, 256))
    return {k: v.clone().requires_grad_(grad) for k, v in d.items()}


def _attn_outs(B, f32, ld_av, ld_text):
    av = Mat(B, 512, ld_av, f32)
    text = Mat(B, 256, ld_text, f32, wins=[(512, 768)] if ld_text == 768 else None)   # 768: the right block of a [B][768] row
    return av, text


def _fill(a, **kw):
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _attn_common(a, I, P, B, f32, ld_av, ld_text):
    return _fill(a, h2=I["h2"].ptr(), pre=I["pre"].ptr(), self_out=I["s"].ptr(), cross_out=I["c"].ptr(), est_w3=P["w3"].data_ptr(),
                 est_b3=P["b3"].data_ptr(), wn_w1_unc=P["W1"].ptr(), wn_w2=P["w2"].data_ptr(), wn_b2=P["b2"].data_ptr(),
                 ld_w1_unc=P["ld_w1"], ld_av=ld_av, ld_text=ld_text, B=B, act_f32=f32, stream=_stream())


def _attn_eval(I, P, B, f32, ld_av, ld_text):
    av, text = _attn_outs(B, f32, ld_av, ld_text)
    wts, unc = Mat(B, 3, 3, 1), Mat(B, 3, 3, 1)
    a = _attn_common(_lib.StackBAttnArgs(), I, P, B, f32, ld_av, ld_text)
    _fill(a, out_av=av.ptr(), out_text=text.ptr(), weights=wts.ptr(), uncertainties=unc.ptr())
    rc = _lib.load().mmdeer_stackb_attn_mix(C.byref(a))
    torch.cuda.synchronize()
    return rc, dict(av=av, text=text, wts=wts, unc=unc), a


def _attn_train(I, P, B, f32, ld_av, ld_text, training=0, p=0.0, site=0, seed=0, offset=0, ctr=None):
    av, text = _attn_outs(B, f32, ld_av, ld_text)
    r, w4, u4 = Mat(B, 256, 256, f32), Mat(B, 4, 4, 1), Mat(B, 4, 4, 1)
    a = _attn_common(_lib.StackBAttnTrainArgs(), I, P, B, f32, ld_av, ld_text)
    _fill(a, out_av=av.ptr(), out_text=text.ptr(), r=r.ptr(), weights4=w4.ptr(), unc4=u4.ptr(), training=training, drop_site=site,
          dropout_p=p, seed=seed, offset=offset, offset_dev=ctr.data_ptr() if ctr is not None else None)
    rc = _lib.load().mmdeer_stackb_attn_mix_train_fwd(C.byref(a))
    torch.cuda.synchronize()
    return rc, dict(av=av, text=text, r=r, w4=w4, u4=u4), a


def _keep(site, B, p, seed, offset):
    m = torch.empty(B, 256, dtype=torch.uint8, device=DEV)
    _lib.check(_lib.load().mmdeer_dropout_mask(site, B, 256, p, seed, offset, m.data_ptr(), _stream()))
    torch.cuda.synchronize()
    return m


def _attn_check_fwd(name, O, R, f32, r_too):
    B = R["w"].shape[0]
    _check("attn_mix.out", name + " out_av", O["av"].val.reshape(B, 2, 256), R["out"][:, :2], R["sout"][:, :2], not f32)
    _check("attn_mix.out", name + " out_text", O["text"].val, R["out"][:, 2], R["sout"][:, 2], not f32)
    w = O["w4"].val[:, :3] if r_too else O["wts"].val
    u = O["u4"].val[:, :3] if r_too else O["unc"].val
    _check("attn_mix.weights", name + " weights", w, R["w"], R["sw"])
    _check("attn_mix.unc", name + " uncertainties", u, R["u"], R["su"])
    if r_too:
        _check("attn_mix.r", name + " r", O["r"].val, R["h"], R["sh"], not f32)
        _zero_bits(name + " weights4[:, 3]", O["w4"].val[:, 3])
        _zero_bits(name + " unc4[:, 3]", O["u4"].val[:, 3])


# (B, ld_w1_unc, ld_av, ld_text, variant, p)
ATTN_CASES = [(1, 771, 512, 768, "plain", 0.1), (3, 3, 520, 256, "spread", 0.5), (4, 771, 520, 768, "equal", 0.1),
              (5, 3, 512, 768, "spread", 0.1), (7, 771, 520, 256, "plain", 0.5), (130, 771, 512, 768, "spread", 0.5)]


@pytest.mark.parametrize("case", ATTN_CASES, ids=lambda c: f"B{c[0]}-w{c[1]}-av{c[2]}-t{c[3]}-{c[4]}")
@pytest.mark.parametrize("f32", [1, 0])
def test_attn_mix_forward(f32, case):
    """The eval operator and the training forward (training 0: bit for bit the eval operator; training 1: the keep mask of
    mmdeer_dropout_mask, with and without a device counter) against float64; rows with three equal logits (weights exactly
    equal) and rows whose logit spread exceeds 100 (a weight underflows to exactly 0)."""
    B, ld_w1, ld_av, ld_text, variant, p = case
    P = _attn_params(variant, ld_w1, 11 + B)
    I = _attn_inputs(B, f32, variant, P, 21 + B)
    name = f"attn_mix f32={f32} {case}"
    with torch.no_grad():
        R = _attn_forward64(_attn_leaves(I, B), P, B, torch.ones(B, 256, dtype=torch.float64, device=DEV), False)
    rc, E, _ = _attn_eval(I, P, B, f32, ld_av, ld_text)
    assert rc == 0, f"{name}: {_lib_err()}"
    rc, E2, _ = _attn_eval(I, P, B, f32, ld_av, ld_text)
    assert rc == 0, f"{name}: {_lib_err()}"
    for k in E:
        E[k].check(f"{name} eval {k}")
        _same_bits(f"{name} eval {k}", E[k].snap(), E2[k].snap())
    _attn_check_fwd(name + " eval", E, R, f32, False)
    if variant == "equal":
        assert torch.equal(E["wts"].val[:, 0], E["wts"].val[:, 1]) and torch.equal(E["wts"].val[:, 0], E["wts"].val[:, 2]), f"{name}: equal logits, unequal weights"
    if variant == "spread":
        lg = R["lg"][0::2]
        assert float((lg.max(-1).values - lg.min(-1).values).min()) > 100.0, f"{name}: the constructed rows' logit spread is below 100"
        assert bool((E["wts"].val[0::2].min(-1).values == 0).all()), f"{name}: no weight underflowed to 0"
    # training = 0: the eval operator bit for bit
    rc, T0, _ = _attn_train(I, P, B, f32, ld_av, ld_text, training=0, p=p, site=3, seed=99, offset=5)
    assert rc == 0, f"{name}: {_lib_err()}"
    for k in T0:
        T0[k].check(f"{name} train0 {k}")
    _same_bits(name + " train0 out_av", T0["av"].snap(), E["av"].snap())
    _same_bits(name + " train0 out_text", T0["text"].snap(), E["text"].snap())
    _same_bits(name + " train0 weights", _bits(T0["w4"].val[:, :3].contiguous()), _bits(E["wts"].val.contiguous()))
    _same_bits(name + " train0 uncertainties", _bits(T0["u4"].val[:, :3].contiguous()), _bits(E["unc"].val.contiguous()))
    _attn_check_fwd(name + " train0", T0, R, f32, True)
    # training = 1: r = relu(h) / (1 - p) where the keep mask is 1, exact zero elsewhere; a device counter adds to the offset
    site, seed, offset = 2 + B % 3, 1234 + B, 77
    for ctr in (None, torch.tensor([3], dtype=torch.int64, device=DEV)):
        keep = _keep(site, B, p, seed, offset + (3 if ctr is not None else 0))
        assert 0 < int(keep.sum()) < keep.numel()
        with torch.no_grad():
            Rt = _attn_forward64(_attn_leaves(I, B), P, B, keep.double() / (1.0 - p), False)
        runs = [_attn_train(I, P, B, f32, ld_av, ld_text, training=1, p=p, site=site, seed=seed, offset=offset, ctr=ctr) for _ in range(2)]
        for k in runs[0][1]:
            assert runs[0][0] == 0 and runs[1][0] == 0, f"{name}: {_lib_err()}"
            runs[0][1][k].check(f"{name} train1 {k}")
            _same_bits(f"{name} train1 {k}", runs[0][1][k].snap(), runs[1][1][k].snap())
        T1 = runs[0][1]
        _attn_check_fwd(f"{name} train1 ctr={ctr is not None}", T1, Rt, f32, True)
        _zero_bits(name + " r where the keep mask is 0", T1["r"].val[keep == 0])
    for k in I:
        I[k].check(f"{name} input {k}")
    P["W1"].check(name + " weight_network.0")


def _attn_bwd_case(f32, B, ld_w1, ld_av, ld_text_fwd, ld_text, ld_dcross, with_unc8, training, p, variant="plain"):
    """Forward (training forward), then the backward from the forward's own stored r, weights4, unc4."""
    P = _attn_params(variant, ld_w1, 31 + B)
    I = _attn_inputs(B, f32, variant, P, 41 + B)
    name = f"attn_mix_bwd f32={f32} B={B} w1={ld_w1} av={ld_av} text={ld_text} dcross={ld_dcross} unc8={with_unc8} training={training} p={p}"
    rc, F, a = _attn_train(I, P, B, f32, ld_av, ld_text_fwd, training=training, p=p, site=4, seed=555, offset=9)
    assert rc == 0, f"{name}: {_lib_err()}"
    g = _gen(51 + B)
    gv = _randn(g, B, 3, 256) * (1.0 + torch.arange(3, device=DEV).float())[None, :, None]
    d_av = Mat(B, 512, ld_av, f32, gv[:, :2].reshape(B, 512))
    d_text = Mat(B, 256, ld_text, f32, gv[:, 2], wins=[(512, 768)] if ld_text == 768 else None)
    ms = 1.0 / (1.0 - p) if training and p > 0 else 1.0
    fac = (F["r"].d > 0).double() * ms                     # the mask from the stored bits
    L = _attn_leaves(I, B, grad=True)
    h2mask = I["h2"].d.reshape(B, 3, 64) > 0
    L2 = dict(L, h2=torch.where(h2mask, L["h2"], L["h2"].detach()))
    R = _attn_forward64(L2, P, B, fac, True)
    R["lg"].retain_grad()
    R["z"].retain_grad()
    G = torch.cat([d_av.d.reshape(B, 2, 256), d_text.d.reshape(B, 1, 256)], 1)
    (R["out"] * G).sum().backward()
    with torch.no_grad():
        s, c, w, u, sw, su = L["s"], L["c"], R["w"], R["u"], R["sw"], R["su"]
        w1u, w2, w3 = P["w1u"], P["w2"].double(), P["w3"].double()
        dw, sdw = (G * s).sum(-1), (G * s).abs().sum(-1)
        sduc = (G * c).abs().sum(-1)
        s_dself = G.abs() * (w + sw)[:, :, None]
        s_dcross = G.abs() * ((1.0 - u).abs() + su)[:, :, None]
        dl = R["lg"].grad
        sdl = _softmax_bwd_scale(w, sw, dw, sdw)
        sdp = ((dl.abs() + sdl) @ w2.abs()) * fac.abs()
        dp = L["pre"].grad
        du = R["z"].grad / (u * (1.0 - u))
        sdu = sduc + (dp.abs() + sdp) @ w1u.abs()
        dz = R["z"].grad
        sdz = sdu * u * (1.0 - u) + du.abs() * (su + u * (1.0 - u))
        sdh2 = sdz[:, :, None] * w3.abs() * h2mask
    dense = ld_dcross == 0
    snaps = []
    for _ in range(2):
        d_self, d_pre, d_h2 = Mat(B, 768, 768, f32), Mat(B, 256, 256, f32), Mat(3 * B, 64, 64, f32)
        d_cross = Mat(3 * B, 256, 256, f32) if dense else Mat(3 * B, 256, ld_dcross, f32, wins=[(ld_dcross - 256, ld_dcross)])
        d_lg8, d_z8 = Mat(B, 8, 8, f32), Mat(3 * B, 8, 8, f32)
        unc8 = Mat(B, 8, 8, f32) if with_unc8 else None
        _fill(a, d_av=d_av.ptr(), d_text=d_text.ptr(), d_self=d_self.ptr(), d_cross=d_cross.ptr(), d_pre=d_pre.ptr(), d_logits8=d_lg8.ptr(),
              d_z8=d_z8.ptr(), d_h2=d_h2.ptr(), unc8=unc8.ptr() if unc8 is not None else None, ld_text=ld_text, ld_dcross=ld_dcross,
              out_av=None, out_text=None, pre=None)
        assert _lib.load().mmdeer_stackb_attn_mix_bwd(C.byref(a)) == 0, f"{name}: {_lib_err()}"
        torch.cuda.synchronize()
        outs = dict(d_self=d_self, d_cross=d_cross, d_pre=d_pre, d_h2=d_h2, d_lg8=d_lg8, d_z8=d_z8)
        if unc8 is not None:
            outs["unc8"] = unc8
        for k, o in outs.items():
            o.check(f"{name} {k}")
        snaps.append({k: o.snap() for k, o in outs.items()})
    for k in snaps[0]:
        _same_bits(f"{name} {k}", snaps[0][k], snaps[1][k])
    for k in ("r", "w4", "u4"):
        F[k].check(f"{name} saved {k}")
    bf = not f32
    _check("attn_mix_bwd.d_self", name + " d_self", d_self.val.reshape(B, 3, 256), L["s"].grad, s_dself, bf)
    _check("attn_mix_bwd.d_cross", name + " d_cross", d_cross.val.reshape(B, 3, 256), L["c"].grad, s_dcross, bf)
    _check("attn_mix_bwd.d_logits8", name + " d_logits8", d_lg8.val[:, :3], dl, sdl, bf)
    _check("attn_mix_bwd.d_pre", name + " d_pre", d_pre.val, dp, sdp, bf)
    _check("attn_mix_bwd.d_z8", name + " d_z8", d_z8.val[:, 0].reshape(B, 3), dz, sdz, bf)
    _check("attn_mix_bwd.d_h2", name + " d_h2", d_h2.val.reshape(B, 3, 64), L["h2"].grad, sdh2, bf)
    _zero_bits(name + " d_logits8[:, 3:8]", d_lg8.val[:, 3:])
    _zero_bits(name + " d_z8[:, 1:8]", d_z8.val[:, 1:])
    _zero_bits(name + " d_pre where r <= 0", d_pre.val[fac == 0])
    _zero_bits(name + " d_h2 where h2 <= 0", d_h2.val.reshape(B, 3, 64)[~h2mask])
    if unc8 is not None:
        _same_bits(name + " unc8[:, :3]", _bits(unc8.val[:, :3].contiguous()), _bits(_store(F["u4"].val[:, :3], f32).contiguous()))
        _zero_bits(name + " unc8[:, 3:8]", unc8.val[:, 3:])


# (B, ld_w1_unc, ld_av, ld_text of the forward, ld_text of the backward, ld_dcross, unc8, training, p, variant)
ATTN_BWD_CASES = [(1, 771, 512, 768, 256, 0, 0, 0, 0.0, "plain"), (3, 3, 520, 256, 768, 512, 1, 1, 0.1, "plain"),
                  (4, 771, 520, 768, 768, 0, 1, 1, 0.5, "spread"), (5, 3, 512, 768, 256, 512, 0, 0, 0.3, "equal"),
                  (7, 771, 520, 256, 256, 512, 1, 1, 0.5, "plain"), (130, 771, 512, 768, 256, 512, 1, 1, 0.1, "spread"),
                  (130, 3, 520, 768, 768, 0, 0, 0, 0.0, "plain")]


@pytest.mark.parametrize("case", ATTN_BWD_CASES, ids=lambda c: "-".join(str(x) for x in c))
@pytest.mark.parametrize("f32", [1, 0])
def test_attn_mix_backward(f32, case):
    """Teacher-forced backward against torch.autograd on the float64 forward: d_cross dense and as the right half of a
    [3B][512] matrix, unc8 NULL and given, ld_text 256 dense and 768, training on (mask_scale 1 / (1 - p)) and off; the 8-column
    zero padding of d_logits8, d_z8 and unc8."""
    _attn_bwd_case(f32, *case)


@pytest.mark.parametrize("f32", [1, 0])
def test_attn_mix_refusals(f32):
    lib = _lib.load()
    z = _lib.StackBAttnArgs()
    assert lib.mmdeer_stackb_attn_mix(C.byref(z)) == 0, _lib_err()
    zt = _lib.StackBAttnTrainArgs()
    assert lib.mmdeer_stackb_attn_mix_train_fwd(C.byref(zt)) == 0 and lib.mmdeer_stackb_attn_mix_bwd(C.byref(zt)) == 0, _lib_err()
    B = 1
    P = _attn_params("plain", 3, 5)
    I = _attn_inputs(B, f32, "plain", P, 6)
    av, text, wts, unc = Mat(B, 512, 520, f32), Mat(B, 256, 256, f32), Mat(B, 3, 3, 1), Mat(B, 3, 3, 1)
    r, w4, u4 = Mat(B, 256, 256, f32), Mat(B, 4, 4, 1), Mat(B, 4, 4, 1)
    gv = Mat(B, 768, 768, f32, _randn(_gen(8), B, 768))
    d_self, d_cross, d_pre, d_h2 = Mat(B, 768, 768, f32), Mat(3 * B, 256, 512, f32), Mat(B, 256, 256, f32), Mat(3 * B, 64, 64, f32)
    d_lg8, d_z8, unc8 = Mat(B, 8, 8, f32), Mat(3 * B, 8, 8, f32), Mat(B, 8, 8, f32)
    outs = [av, text, wts, unc, r, w4, u4, d_self, d_cross, d_pre, d_h2, d_lg8, d_z8, unc8]

    def ev(**kw):
        a = _attn_common(_lib.StackBAttnArgs(), I, P, B, f32, 520, 256)
        _fill(a, **dict(dict(out_av=av.ptr(), out_text=text.ptr(), weights=wts.ptr(), uncertainties=unc.ptr()), **kw))
        rc = lib.mmdeer_stackb_attn_mix(C.byref(a))
        torch.cuda.synchronize()
        return rc

    def tr(bwd, **kw):
        a = _attn_common(_lib.StackBAttnTrainArgs(), I, P, B, f32, 520, 256)
        base = dict(out_av=av.ptr(), out_text=text.ptr(), r=r.ptr(), weights4=w4.ptr(), unc4=u4.ptr(), d_av=gv.ptr(), d_text=gv.ptr(512),
                    d_self=d_self.ptr(), d_cross=d_cross.ptr(256), d_pre=d_pre.ptr(), d_logits8=d_lg8.ptr(), d_z8=d_z8.ptr(), d_h2=d_h2.ptr(),
                    unc8=unc8.ptr(), ld_dcross=512)
        _fill(a, **dict(base, **kw))
        rc = (lib.mmdeer_stackb_attn_mix_bwd if bwd else lib.mmdeer_stackb_attn_mix_train_fwd)(C.byref(a))
        torch.cuda.synchronize()
        return rc

    bad_ld = [dict(ld_av=508), dict(ld_av=514), dict(ld_text=252), dict(ld_text=258), dict(ld_w1_unc=2)]
    for kw in bad_ld:
        _refused(f"attn_mix {kw}", ev(**kw), "leading dimension", outs)
        _refused(f"attn_mix_train_fwd {kw}", tr(False, **kw), "leading dimension", outs)
        _refused(f"attn_mix_bwd {kw}", tr(True, **kw), "leading dimension", outs)
    for kw in (dict(ld_dcross=100), dict(ld_dcross=258)):
        _refused(f"attn_mix_train_fwd {kw}", tr(False, **kw), "ld_dcross", outs)
        _refused(f"attn_mix_bwd {kw}", tr(True, **kw), "ld_dcross", outs)
    _refused("attn_mix B=-1", ev(B=-1), "batch", outs)
    _refused("attn_mix NULL h2", ev(h2=None), "NULL", outs)
    _refused("attn_mix_bwd NULL d_z8", tr(True, d_z8=None), "NULL", outs)
    for f in ("h2", "pre", "self_out", "cross_out", "out_av", "out_text"):
        good = getattr(_attn_common(_lib.StackBAttnArgs(), I, P, B, f32, 520, 256), f) or {"out_av": av.ptr(), "out_text": text.ptr()}[f]
        _refused(f"attn_mix misaligned {f}", ev(**{f: _off(good, f32)}), "misaligned", outs)
        _refused(f"attn_mix_train_fwd misaligned {f}", tr(False, **{f: _off(good, f32)}), "misaligned", outs)
    for f, m in (("r", r), ("d_self", d_self), ("d_cross", d_cross), ("d_pre", d_pre), ("d_logits8", d_lg8), ("d_z8", d_z8), ("d_h2", d_h2),
                 ("unc8", unc8), ("d_av", gv)):
        _refused(f"attn_mix_bwd misaligned {f}", tr(True, **{f: _off(m.ptr(), f32)}), "misaligned", outs)
    for f, m in (("weights4", w4), ("unc4", u4)):
        _refused(f"attn_mix_train_fwd misaligned {f}", tr(False, **{f: m.ptr() + 4}), "misaligned", outs)
        _refused(f"attn_mix_bwd misaligned {f}", tr(True, **{f: m.ptr() + 8}), "misaligned", outs)


# ================================================================================================== gate_mix / gate_mix_bwd
def _gate_inputs(B, N, f32, seed, lds):
    g = _gen(seed)
    gl = 2.0 * _randn(g, B, N)
    gl[:, 0::9] = 100.0                               # sigmoid exactly 1
    gl[:, 1::9] = -100.0                              # sigmoid exactly 0
    tri = _randn(g, B, N)                             # about half <= 0
    tri[:, 2::11] = 0.0
    tri[:, 3::11] = -0.0
    av = 3.0 * _randn(g, B, N)
    return Mat(B, N, lds[0], f32, gl), Mat(B, N, lds[1], f32, tri), Mat(B, N, lds[2], f32, av)


def _gate_call(gl, tri, av, out, out32, B, N, f32, **kw):
    a = dict(g=gl.ptr(), ld_g=gl.ld, t=tri.ptr(), ld_t=tri.ld, v=av.ptr(), ld_v=av.ld, o=out.ptr(), ld_o=out.ld,
             o32=out32.ptr() if out32 is not None else None, B=B, N=N)
    a.update(kw)
    rc = _lib.load().mmdeer_stackb_gate_mix(a["g"], a["ld_g"], a["t"], a["ld_t"], a["v"], a["ld_v"], a["o"], a["ld_o"], a["o32"], a["B"], a["N"], f32, _stream())
    torch.cuda.synchronize()
    return rc


def _gate_ref(gl, t, v):
    s = torch.sigmoid(gl)
    return s * t + (1.0 - s) * v, (s * t).abs() + ((1.0 - s) * v).abs() + s * (t.abs() + v.abs())


# B * N / 4 = 1,050,624 groups of 4 against 4096 * 256 = 1,048,576: only the first blocks take a second trip
GATE_SHAPES = [(B, N) for B in (1, 5) for N in (4, 12, 260, 512)] + [(2052, 2048)]


@pytest.mark.parametrize("f32", [1, 0])
def test_gate_mix(f32):
    """N in {4, 12, 260, 512} x B in {1, 5} and one shape past the 4096-block cap; every leading dimension its own; out32 NULL
    and given (dense, the fp32 value before any bf16 rounding: bit-equal to the fp32 operator on the same inputs); logits at
    +-100."""
    for B, N in GATE_SHAPES:
        gl, tri, av = _gate_inputs(B, N, f32, 3 * B + N, (N + 4, N + 8, N + 12))
        ref, scale = _gate_ref(gl.d, tri.d, av.d)
        for with32 in (0, 1):
            name = f"gate_mix f32={f32} B={B} N={N} out32={with32}"
            snaps = []
            for _ in range(2):
                out, out32 = Mat(B, N, N + 16, f32), Mat(B, N, N, 1) if with32 else None
                assert _gate_call(gl, tri, av, out, out32, B, N, f32) == 0, f"{name}: {_lib_err()}"
                out.check(name)
                snaps.append(out.snap())
                if with32:
                    out32.check(name + " out32")
                    snaps[-1] = torch.cat([snaps[-1].int(), out32.snap()])
            _same_bits(name, *snaps)
            _check("gate_mix.out", name, out.val, ref, scale, not f32)
            if with32:
                _check("gate_mix.out", name + " out32", out32.val, ref, scale)
                if f32:
                    _same_bits(name + " out32 vs out", _bits(out32.val.contiguous()), _bits(out.val.contiguous()))
                else:       # the fp32 operator on the same (upcast) inputs stores what out32 holds; out is its bf16 rounding
                    g3 = [Mat(B, N, N + 4, 1, m.val.float()) for m in (gl, tri, av)]
                    o3 = Mat(B, N, N + 4, 1)
                    assert _gate_call(g3[0], g3[1], g3[2], o3, None, B, N, 1) == 0, _lib_err()
                    _same_bits(name + " out32 vs the fp32 operator", _bits(out32.val.contiguous()), _bits(o3.val.contiguous()))
                    _same_bits(name + " out vs bf16(out32)", _bits(out.val.contiguous()), _bits(out32.val.to(torch.bfloat16).contiguous()))
        ex = (gl.d.abs() == 100.0)
        assert bool(ex.any())
        assert torch.equal(out.val[gl.d == 100.0], tri.val[gl.d == 100.0]) and torch.equal(out.val[gl.d == -100.0], av.val[gl.d == -100.0]), \
            f"{name}: a sigmoid at +-100 is not exactly 1 / 0"
        for m in (gl, tri, av):
            m.check(name + " input")


def _gate_bwd_call(ms, B, N, f32, lds=None, ptrs=None):
    p = ptrs or [m.ptr() for m in ms]
    l = lds or [m.ld for m in ms]
    args = []
    for i in range(7):
        args += [p[i], l[i]]
    rc = _lib.load().mmdeer_stackb_gate_mix_bwd(*args, B, N, f32, _stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("f32", [1, 0])
def test_gate_mix_bwd(f32):
    """Against torch.autograd on the float64 forward with the (tri > 0) mask of the stored tri; dtri exact zero where
    tri <= 0 (0.0 and -0.0 among them); seven different leading dimensions; one shape past the 4096-block cap."""
    for B, N in GATE_SHAPES:
        gl, tri, av = _gate_inputs(B, N, f32, 5 * B + N, (N + 4, N + 8, N + 12))
        dout = Mat(B, N, N + 16, f32, _randn(_gen(B + N), B, N))
        name = f"gate_mix_bwd f32={f32} B={B} N={N}"
        G, T, V = (m.d.clone().requires_grad_(True) for m in (gl, tri, av))
        mask = tri.d > 0
        s = torch.sigmoid(G)
        (dout.d * (s * torch.where(mask, T, T.detach()) + (1.0 - s) * V)).sum().backward()
        with torch.no_grad():
            d = dout.d.abs()
            s_dg = d * (tri.d.abs() + av.d.abs()) * (s * (1.0 - s) + s * s)
            s_dt = d * s * mask
            s_dv = d * ((1.0 - s) + s)
        snaps = []
        for _ in range(2):
            dg, dt, dv = Mat(B, N, N + 20, f32), Mat(B, N, N + 24, f32), Mat(B, N, N + 28, f32)
            assert _gate_bwd_call([dout, gl, tri, av, dg, dt, dv], B, N, f32) == 0, f"{name}: {_lib_err()}"
            for o in (dg, dt, dv):
                o.check(name)
            snaps.append(torch.cat([dg.snap(), dt.snap(), dv.snap()]))
        _same_bits(name, *snaps)
        _check("gate_mix_bwd.dg", name + " dg", dg.val, G.grad, s_dg, not f32)
        _check("gate_mix_bwd.dtri", name + " dtri", dt.val, T.grad, s_dt, not f32)
        _check("gate_mix_bwd.dav", name + " dav", dv.val, V.grad, s_dv, not f32)
        assert int((~mask).sum()) > 0 or B * N < 8
        _zero_bits(name + " dtri where tri <= 0", dt.val[~mask])
        for m in (dout, gl, tri, av):
            m.check(name + " input")


@pytest.mark.parametrize("f32", [1, 0])
def test_gate_mix_refusals(f32):
    lib = _lib.load()
    assert lib.mmdeer_stackb_gate_mix(None, 0, None, 0, None, 0, None, 0, None, 0, 8, f32, _stream()) == 0, _lib_err()
    assert lib.mmdeer_stackb_gate_mix_bwd(*([None, 0] * 7), 0, 8, f32, _stream()) == 0, _lib_err()
    B, N = 1, 8
    gl, tri, av = _gate_inputs(B, N, f32, 1, (16, 16, 16))
    dout = Mat(B, N, 16, f32, _randn(_gen(2), B, N))
    out, out32, dg, dt, dv = Mat(B, N, 16, f32), Mat(B, N, N, 1), Mat(B, N, 16, f32), Mat(B, N, 16, f32), Mat(B, N, 16, f32)
    outs = [out, out32, dg, dt, dv]
    ms = [dout, gl, tri, av, dg, dt, dv]
    _refused("gate_mix N=6", _gate_call(gl, tri, av, out, out32, B, 6, f32), "bad shape", outs)
    _refused("gate_mix_bwd N=6", _gate_bwd_call(ms, B, 6, f32), "bad shape", outs)
    _refused("gate_mix B=-1", _gate_call(gl, tri, av, out, out32, -1, N, f32), "bad shape", outs)
    for k in ("ld_g", "ld_t", "ld_v", "ld_o"):
        for ld in (4, 10):
            _refused(f"gate_mix {k}={ld}", _gate_call(gl, tri, av, out, out32, B, N, f32, **{k: ld}), "leading dimension", outs)
    for k in ("g", "t", "v", "o"):
        good = dict(g=gl, t=tri, v=av, o=out)[k].ptr()
        _refused(f"gate_mix misaligned {k}", _gate_call(gl, tri, av, out, out32, B, N, f32, **{k: _off(good, f32)}), "misaligned", outs)
    _refused("gate_mix misaligned out32", _gate_call(gl, tri, av, out, out32, B, N, f32, o32=out32.ptr() + 4), "misaligned", outs)
    for i in range(7):
        for ld in (4, 10):
            lds = [16] * 7
            lds[i] = ld
            _refused(f"gate_mix_bwd ld[{i}]={ld}", _gate_bwd_call(ms, B, N, f32, lds=lds), "leading dimension", outs)
        ptrs = [m.ptr() for m in ms]
        ptrs[i] = _off(ptrs[i], f32)
        _refused(f"gate_mix_bwd misaligned pointer {i}", _gate_bwd_call(ms, B, N, f32, ptrs=ptrs), "misaligned", outs)


# ============================================================================================================== add_masked
def _add_call(out, x, y, mask, scale, M, N, f32, **kw):
    a = dict(po=out.ptr(), ld_o=out.ld, px=x.ptr(), ld_x=x.ld, py=y.ptr() if y is not None else None, ld_y=y.ld if y is not None else 0,
             pm=mask.ptr() if mask is not None else None, ld_m=mask.ld if mask is not None else 0)
    a.update(kw)
    rc = _lib.load().mmdeer_add_masked(a["po"], a["ld_o"], a["px"], a["ld_x"], a["py"], a["ld_y"], a["pm"], a["ld_m"], scale, M, N, f32, _stream())
    torch.cuda.synchronize()
    return rc


def _add_inputs(M, N, f32, seed):
    g = _gen(seed)
    xv, yv, mv = _randn(g, M, N), 2.0 * _randn(g, M, N), _randn(g, M, N)
    flat = mv.reshape(-1)
    for i, v in enumerate((0.0, -0.0, float("inf"), float("nan"), -float("inf"), -1.5)):
        flat[i::13] = v
    return xv, yv, mv


@pytest.mark.parametrize("f32", [1, 0])
def test_add_masked(f32):
    """y and mask given or NULL, scale 1 and 2, mask values 0.0, -0.0, negatives, +-inf and NaN (NaN is not > 0: exact zero),
    out aliasing x, N in {4, 260}, one shape past the 4096-block cap."""
    for M, N in ((1, 4), (5, 4), (3, 260), (2052, 2048)):
        xv, yv, mv = _add_inputs(M, N, f32, M + N)
        y0, m0 = Mat(M, N, N + 8, f32, yv), Mat(M, N, N + 12, f32, mv)
        keep = m0.val.float() > 0                          # from the stored bits
        assert bool(keep.any()) and (M * N < 13 or bool(torch.isnan(m0.val.float()).any()))
        for with_y in (0, 1):
            for with_m in (0, 1):
                for scale in (1.0, 2.0):
                    for alias in (0, 1):
                        if alias and (M > 5 and not (with_y and with_m)):
                            continue
                        name = f"add_masked f32={f32} M={M} N={N} y={with_y} mask={with_m} scale={scale} alias={alias}"
                        y, mask = (y0 if with_y else None), (m0 if with_m else None)
                        x0 = Mat(M, N, N + 4, f32, xv)
                        ref = x0.d + (y0.d if with_y else 0.0)
                        sc = x0.d.abs() + (y0.d.abs() if with_y else 0.0)
                        if with_m:
                            ref, sc = torch.where(keep, ref * scale, torch.zeros_like(ref)), sc * scale * keep
                        snaps = []
                        for _ in range(2):
                            x = Mat(M, N, N + 4, f32, xv)
                            out = x if alias else Mat(M, N, N + 16, f32)
                            assert _add_call(out, x, y, mask, scale, M, N, f32) == 0, f"{name}: {_lib_err()}"
                            out.check(name)
                            x.check(name + " (x)")
                            snaps.append(out.snap())
                        _same_bits(name, *snaps)
                        _check("add_masked.out", name, out.val, ref, sc, not f32)
                        if with_m:
                            _zero_bits(name + " where the mask is not > 0", out.val[~keep])
        y0.check("add_masked y")
        m0.check("add_masked mask", nan_ok=True)


@pytest.mark.parametrize("f32", [1, 0])
def test_add_masked_refusals(f32):
    lib = _lib.load()
    assert lib.mmdeer_add_masked(None, 0, None, 0, None, 0, None, 0, 1.0, 0, 8, f32, _stream()) == 0, _lib_err()
    M, N = 1, 8
    xv, yv, mv = _add_inputs(M, N, f32, 3)
    x, y, mask, out = Mat(M, N, 16, f32, xv), Mat(M, N, 16, f32, yv), Mat(M, N, 16, f32, mv), Mat(M, N, 16, f32)
    _refused("add_masked N=6", _add_call(out, x, y, mask, 1.0, M, 6, f32), "bad shape", [out])
    _refused("add_masked M=-1", _add_call(out, x, y, mask, 1.0, -1, N, f32), "bad shape", [out])
    for k in ("ld_o", "ld_x", "ld_y", "ld_m"):
        for ld in (4, 10):
            _refused(f"add_masked {k}={ld}", _add_call(out, x, y, mask, 1.0, M, N, f32, **{k: ld}), "leading dimension", [out])
    _refused("add_masked NULL x", _add_call(out, x, y, mask, 1.0, M, N, f32, px=None), "pointer", [out])
    for k, m in (("po", out), ("px", x), ("py", y), ("pm", mask)):
        _refused(f"add_masked misaligned {k}", _add_call(out, x, y, mask, 1.0, M, N, f32, **{k: _off(m.ptr(), f32)}), "misaligned", [out])


# ========================================================================================================= head / head_bwd
HEAD_ROWS = (-100.0, -30.0, -17.0, 19.99, 20.0, 20.01, 25.0, 88.0)     # constructed rows: the value in every column
EPS32 = float(np.float32(1e-6))


def _head_ev(B, ld_ev, seed):
    g = _gen(seed)
    ev = 2.0 * _randn(g, B, 12)
    if B >= len(HEAD_ROWS):
        for i, v in enumerate(HEAD_ROWS):
            ev[B - len(HEAD_ROWS) + i] = v
    return Mat(B, 12, ld_ev, 1, ev)


def _head_params(seed):
    g = _gen(seed)
    return [t.contiguous() for t in (torch.tensor([0.7, 1.3, 2.1], device=DEV), _randn(g, 32), 0.5 * _randn(g, 32), 0.3 * _randn(g, 16, 32),
                                     0.2 * _randn(g, 16), 0.5 * _randn(g, 16), torch.tensor([0.15], device=DEV))]


def _softplus64(x):
    return torch.where(x > 20.0, x, torch.log1p(torch.exp(torch.clamp(x, max=30.0))))     # F.softplus, threshold 20


def _head_call(ev, cps, out, B, ld_ev=None, evp=None):
    rc = _lib.load().mmdeer_stackb_head(evp if evp is not None else ev.ptr(), ld_ev or ev.ld, *[t.data_ptr() for t in cps], out.ptr(), B, _stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("ld_ev", [12, 16])
@pytest.mark.parametrize("B", [1, 85, 86])
def test_head(B, ld_ev):
    """3 B straddles 256; raw evidence N(0, 2) plus rows at the softplus threshold, far below it (alpha - 1 == 0: infinite
    uncertainties, inf must equal inf) and far above.  nu, alpha, beta are rounded to fp32 before alpha - 1 and the uncertainties
    are formed, as the kernel and torch do.  The calibrated plane is checked on every row whose fp32 total is finite; the others
    are exactly the three constructed rows at -100, -30 and -17."""
    ev, cps = _head_ev(B, ld_ev, 60 + B), _head_params(61)
    name = f"head B={B} ld_ev={ld_ev}"
    snaps = []
    for _ in range(2):
        out = Mat(8, 3 * B, 3 * B, 1)
        assert _head_call(ev, cps, out, B) == 0, f"{name}: {_lib_err()}"
        out.check(name, nan_ok=True)
        snaps.append(out.snap())
    _same_bits(name, *snaps)
    ev.check(name + " ev")
    got = out.val.reshape(8, B, 3)
    r = ev.d.reshape(B, 3, 4)
    T, w1, b1, w2, b2, w3, b3 = (t.double() for t in cps)
    mu = r[..., 0]
    nu = (_softplus64(r[..., 1]) + EPS32).float().double()
    alpha = (_softplus64(r[..., 2]) + 1.0).float().double()
    beta = (_softplus64(r[..., 3]) + EPS32).float().double()
    am1 = alpha - 1.0
    alea, epi = beta / am1, beta / (nu * am1)
    tot = alea + epi
    s_alea = alea * (2.0 + alpha / am1)
    s_epi = epi * (3.0 + alpha / am1)
    assert torch.equal(_bits(got[0].contiguous()), _bits(mu.float().contiguous())), f"{name}: mu is not the raw value"
    for i, (ref, nm) in enumerate(((nu, "nu"), (alpha, "alpha"), (beta, "beta"))):
        _check("head.nu_alpha_beta", f"{name} {nm}", got[1 + i], ref, ref.abs())
    _check("head.uncertainties", name + " aleatoric", got[4], alea, s_alea, inf_ok=True)
    _check("head.uncertainties", name + " epistemic", got[5], epi, s_epi, inf_ok=True)
    _check("head.uncertainties", name + " total", got[6], tot, s_alea + s_epi, inf_ok=True)
    fin = torch.isfinite(got[6])
    assert torch.equal(fin, torch.isfinite(tot)), f"{name}: total is finite elsewhere than in the reference"
    n_out = int((~fin).sum())
    assert n_out == (9 if B >= len(HEAD_ROWS) else 0), f"{name}: {n_out} elements with a non-finite total"
    if n_out:
        assert bool((~fin[B - 8:B - 5]).all()), f"{name}: the non-finite rows are not the constructed ones"
    assert not bool(torch.isnan(got[:7]).any()), f"{name}: NaN stored"
    # calibration: sigmoid(MLP(total / temperature[d])) on the rows with a finite total
    sc = tot[fin] / T[None, :].expand(B, 3)[fin]
    s_sc = (s_alea + s_epi)[fin] / T[None, :].expand(B, 3)[fin].abs() + sc.abs()
    h1 = torch.relu(sc[:, None] * w1 + b1)
    s_h1 = (sc[:, None] * w1).abs() + b1.abs() + s_sc[:, None] * w1.abs()
    h2 = torch.relu(h1 @ w2.t() + b2)
    s_h2 = (h1.abs() + s_h1) @ w2.abs().t() + b2.abs()
    z = h2 @ w3 + b3
    s_z = (h2.abs() + s_h2) @ w3.abs() + b3.abs()
    cal = torch.sigmoid(z)
    _check("head.calibrated", name + " calibrated", got[7][fin], cal, cal + cal * (1.0 - cal) * s_z)


@pytest.mark.parametrize("ld_dev", [24, 32])
@pytest.mark.parametrize("ld_ev", [12, 16])
@pytest.mark.parametrize("B", [1, 85, 86])
@pytest.mark.parametrize("f32", [1, 0])
def test_head_bwd(f32, B, ld_ev, ld_dev):
    """d raw evidence against torch.autograd on the float64 constraints: softplus' = sigmoid, exactly 1 above the threshold 20;
    columns 8 d + 4 .. 8 d + 7 exact zeros; g4 a contiguous [4][B][3]."""
    ev = _head_ev(B, ld_ev, 70 + B)
    g4 = Mat(4, 3 * B, 3 * B, 1, _randn(_gen(71 + B), 4, 3 * B) * (1.0 + torch.arange(4, device=DEV).float())[:, None])
    name = f"head_bwd f32={f32} B={B} ld_ev={ld_ev} ld_dev={ld_dev}"
    r = ev.d.reshape(B, 3, 4).clone().requires_grad_(True)
    planes = torch.stack([r[..., 0], _softplus64(r[..., 1]) + EPS32, _softplus64(r[..., 2]) + 1.0, _softplus64(r[..., 3]) + EPS32])
    (planes * g4.d.reshape(4, B, 3)).sum().backward()
    snaps = []
    for _ in range(2):
        dev_ = Mat(B, 24, ld_dev, f32)
        rc = _lib.load().mmdeer_stackb_head_bwd(ev.ptr(), ld_ev, g4.ptr(), dev_.ptr(), ld_dev, B, f32, _stream())
        torch.cuda.synchronize()
        assert rc == 0, f"{name}: {_lib_err()}"
        dev_.check(name)
        snaps.append(dev_.snap())
    _same_bits(name, *snaps)
    got = dev_.val.reshape(B, 3, 8)
    _check("head_bwd.dev", name, got[..., :4], r.grad, r.grad.abs(), not f32)
    _zero_bits(name + " columns 8 d + 4 .. 8 d + 7", got[..., 4:])
    if B >= len(HEAD_ROWS):        # above the threshold the factor is exactly 1: the stored value is g4 itself (rounded for bf16)
        rows = slice(B - 3, B)     # 20.01, 25, 88
        want = _store(g4.val.reshape(4, B, 3)[:, rows].permute(1, 2, 0), f32)
        _same_bits(name + " factor 1 above the threshold", _bits(got[rows, :, :4].contiguous()), _bits(want.contiguous()))
    ev.check(name + " ev")
    g4.check(name + " g4")


@pytest.mark.parametrize("f32", [1, 0])
def test_head_refusals(f32):
    lib = _lib.load()
    assert lib.mmdeer_stackb_head(None, 0, *([None] * 8), 0, _stream()) == 0, _lib_err()
    assert lib.mmdeer_stackb_head_bwd(None, 0, None, None, 0, 0, f32, _stream()) == 0, _lib_err()
    B = 1
    ev, cps, out = _head_ev(B, 16, 1), _head_params(2), Mat(8, 3, 3, 1)
    g4, dev_ = Mat(4, 3, 3, 1, _randn(_gen(3), 4, 3)), Mat(B, 24, 32, f32)
    outs = [out, dev_]

    def bwd(ld_ev=16, ld_dev=32, evp=None, devp=None, B=1):
        rc = lib.mmdeer_stackb_head_bwd(evp or ev.ptr(), ld_ev, g4.ptr(), devp or dev_.ptr(), ld_dev, B, f32, _stream())
        torch.cuda.synchronize()
        return rc

    if f32:
        for ld in (8, 14):
            _refused(f"head ld_ev={ld}", _head_call(ev, cps, out, B, ld_ev=ld), "ld_ev", outs)
        _refused("head misaligned ev", _head_call(ev, cps, out, B, evp=ev.ptr() + 4), "misaligned", outs)
        rc = lib.mmdeer_stackb_head(ev.ptr(), 16, *[t.data_ptr() for t in cps], out.ptr(), -1, _stream())
        _refused("head B=-1", rc, "batch", outs)
    for ld in (8, 14):
        _refused(f"head_bwd ld_ev={ld}", bwd(ld_ev=ld), "ld_ev", outs)
    for ld in (20, 28):
        _refused(f"head_bwd ld_dev={ld}", bwd(ld_dev=ld), "ld_dev", outs)
    _refused("head_bwd B=-1", bwd(B=-1), "batch", outs)
    _refused("head_bwd misaligned ev", bwd(evp=ev.ptr() + 8), "misaligned", outs)
    _refused("head_bwd misaligned dev", bwd(devp=_off(dev_.ptr(), f32)), "misaligned", outs)


# ============================================================================================================= softmax_mix
def _mix_inputs(B, S, D, sp, ldp, f32, mode, ld_logits, seed):
    g = _gen(seed)
    wins = [(s * sp, s * sp + D) for s in range(S)]
    P = Mat(B, D, ldp, f32, wins=wins)
    w_att, b_att = _randn(g, D) / D ** 0.5, torch.tensor([0.4], device=DEV)
    for s in range(S):
        P.m[:, s * sp:s * sp + D] = _store(_randn(g, B, D) * (1.0 + s), f32)          # stacked row s scaled by 1 + s
    if mode == "w_att" and S > 1:        # sample 0: logit 0 about 150 above the others
        P.m[0, 0:D] = _store(w_att * (150.0 / float((w_att * w_att).sum())), f32)
    lg = 1.5 * _randn(g, B, S)
    if S > 1:
        lg[0, 0] += 150.0
    logits = Mat(B, S, ld_logits, 1, lg)
    return P, w_att, b_att, logits


def _mix_args(P, w_att, b_att, logits, mode, B, S, D, sp, ldp, f32, w8):
    a = _lib.SoftmaxMixArgs()
    _fill(a, P=P.ptr(0), ldp=ldp, sp=sp, S=S, D=D, B=B, act_f32=f32, weights8=w8.ptr(), stream=_stream())
    if mode == "w_att":
        _fill(a, w_att=w_att.data_ptr(), b_att=b_att.data_ptr())
    else:
        _fill(a, logits=logits.ptr(), ld_logits=logits.ld)
    return a


def _mix_forward64(Pd, w_att, b_att, lg_in, mode):
    """Pd [B][S][D] float64.  Returns lg, w, out and the scales of w and out."""
    if mode == "w_att":
        lg = (Pd * w_att).sum(-1) + b_att
        slg = (Pd * w_att).abs().sum(-1) + b_att.abs()
    else:
        lg, slg = lg_in, torch.zeros_like(lg_in)
    w = torch.softmax(lg, -1)
    out = (w[:, :, None] * Pd).sum(1)
    with torch.no_grad():
        sw = _softmax_scale(w, lg, slg)
        sout = ((w + sw)[:, :, None] * Pd.abs()).sum(1)
    return lg, w, out, sw, sout


# (B, S, D, sp - D, mode, ld_logits - S)
MIX_CASES = [(1, 1, 4, 0, "w_att", 0), (3, 2, 252, 8, "logits", 0), (4, 3, 256, 0, "logits", 12), (5, 7, 260, 8, "w_att", 0),
             (7, 8, 1028, 0, "w_att", 0), (130, 8, 4, 8, "logits", 12), (130, 3, 260, 0, "w_att", 0), (5, 1, 1028, 8, "logits", 12),
             (3, 8, 256, 8, "w_att", 0), (4, 7, 252, 0, "logits", 0), (7, 2, 4, 0, "w_att", 0)]


@pytest.mark.parametrize("case", MIX_CASES, ids=lambda c: "-".join(str(x) for x in c))
@pytest.mark.parametrize("f32", [1, 0])
def test_softmax_mix(f32, case):
    """Forward and (teacher-forced: from the forward's stored weights8) backward against float64 / torch.autograd; S in
    {1, 2, 3, 7, 8}, D in {4, 252, 256, 260, 1028}, both logit sources, sp in {D, D + 8}, ldp past the last stacked row; a logit
    spread above 100; weights8 and dlogits8 exact zeros beyond S; dP with the ds * w_att term in w_att mode, without it in logits
    mode, and its pad columns between the stacked rows intact."""
    B, S, D, dsp, mode, dll = case
    sp = D + dsp
    ldp = (S - 1) * sp + D + 8
    ld_logits = 12 if dll else S
    P, w_att, b_att, logits = _mix_inputs(B, S, D, sp, ldp, f32, mode, ld_logits, 80 + B + S + D)
    name = f"softmax_mix f32={f32} {case}"
    Pd = torch.stack([P.win(s).double() for s in range(S)], 1).requires_grad_(True)
    lgl = logits.d.clone().requires_grad_(True)
    lg, w, out_ref, sw, sout = _mix_forward64(Pd, w_att.double(), b_att.double(), lgl, mode)
    if S > 1:
        assert float(lg[0].max() - lg[0].min()) > 100.0
    snaps = []
    for _ in range(2):
        w8, out = Mat(B, 8, 8, 1), Mat(B, D, D + 4, f32)
        a = _mix_args(P, w_att, b_att, logits, mode, B, S, D, sp, ldp, f32, w8)
        _fill(a, out=out.ptr(), ld_out=out.ld)
        assert _lib.load().mmdeer_softmax_mix_fwd(C.byref(a)) == 0, f"{name}: {_lib_err()}"
        torch.cuda.synchronize()
        w8.check(name + " weights8")
        out.check(name + " out")
        snaps.append(torch.cat([w8.snap(), out.snap().int()]))
    _same_bits(name, *snaps)
    _check("softmax_mix.weights8", name + " weights8", w8.val[:, :S], w, sw)
    _zero_bits(name + " weights8 beyond S", w8.val[:, S:])
    _check("softmax_mix.out", name + " out", out.val, out_ref, sout, not f32)
    # backward from the stored weights8
    dout = Mat(B, D, D + 12, f32, _randn(_gen(90 + B), B, D))
    lg.retain_grad()
    (out_ref * dout.d).sum().backward()
    with torch.no_grad():
        g = dout.d
        dw, sdw = (g[:, None, :] * Pd).sum(-1), (g[:, None, :] * Pd).abs().sum(-1)
        wd = w.detach()
        sds = _softmax_bwd_scale(wd, sw, dw, sdw)
        sdP = (wd + sw)[:, :, None] * g.abs()[:, None, :]
        if mode == "w_att":
            sdP = sdP + (lg.grad.abs() + sds)[:, :, None] * w_att.double().abs()
    snaps = []
    for _ in range(2):
        dP, dl8 = Mat(B, D, ldp, f32, wins=P.wins), Mat(B, 8, 8, f32)
        _fill(a, dout=dout.ptr(), ld_dout=dout.ld, dP=dP.ptr(0), dlogits8=dl8.ptr(), out=None, ld_out=0)
        assert _lib.load().mmdeer_softmax_mix_bwd(C.byref(a)) == 0, f"{name}: {_lib_err()}"
        torch.cuda.synchronize()
        dP.check(name + " dP")
        dl8.check(name + " dlogits8")
        snaps.append(torch.cat([dP.snap(), dl8.snap()]))
    _same_bits(name + " bwd", *snaps)
    _check("softmax_mix_bwd.dlogits8", name + " dlogits8", dl8.val[:, :S], lg.grad, sds, not f32)
    _zero_bits(name + " dlogits8 beyond S", dl8.val[:, S:])
    got_dP = torch.stack([dP.win(s) for s in range(S)], 1)
    _check("softmax_mix_bwd.dP", name + " dP", got_dP, Pd.grad, sdP, not f32)
    for m, nm in ((P, "P"), (logits, "logits"), (dout, "dout"), (w8, "weights8")):
        m.check(f"{name} {nm}")


@pytest.mark.parametrize("f32", [1, 0])
def test_softmax_mix_refusals(f32):
    lib = _lib.load()
    z = _fill(_lib.SoftmaxMixArgs(), S=3, D=8, B=0, act_f32=f32)
    assert lib.mmdeer_softmax_mix_fwd(C.byref(z)) == 0 and lib.mmdeer_softmax_mix_bwd(C.byref(z)) == 0, _lib_err()
    B, S, D, sp, ldp = 1, 3, 8, 8, 32
    P, w_att, b_att, logits = _mix_inputs(B, S, D, sp, ldp, f32, "logits", 4, 9)
    w8, out, dP, dl8 = Mat(B, 8, 8, 1), Mat(B, D, 16, f32), Mat(B, D, ldp, f32, wins=P.wins), Mat(B, 8, 8, f32)
    dout = Mat(B, D, 16, f32, _randn(_gen(4), B, D))
    outs = [w8, out, dP, dl8]

    def call(bwd, mode="w_att", **kw):
        a = _mix_args(P, w_att, b_att, logits, mode, B, S, D, sp, ldp, f32, w8)
        _fill(a, **dict(dict(out=out.ptr(), ld_out=out.ld, dout=dout.ptr(), ld_dout=dout.ld, dP=dP.ptr(0), dlogits8=dl8.ptr()), **kw))
        rc = (lib.mmdeer_softmax_mix_bwd if bwd else lib.mmdeer_softmax_mix_fwd)(C.byref(a))
        torch.cuda.synchronize()
        return rc

    for bwd in (False, True):
        for kw in (dict(S=0), dict(S=9), dict(D=2), dict(D=6), dict(B=-1)):
            _refused(f"softmax_mix bwd={bwd} {kw}", call(bwd, **kw), "bad shape", outs)
        for kw in (dict(sp=4), dict(ldp=20), dict(ldp=30), dict(sp=10, ldp=40)):
            _refused(f"softmax_mix bwd={bwd} {kw}", call(bwd, **kw), "bad P", outs)
        _refused(f"softmax_mix bwd={bwd} no logit source", call(bwd, w_att=None, b_att=None), "needs w_att", outs)
        _refused(f"softmax_mix bwd={bwd} w_att without b_att", call(bwd, b_att=None), "needs w_att", outs)
        _refused(f"softmax_mix bwd={bwd} ld_logits < S", call(bwd, mode="logits", ld_logits=2), "needs w_att", outs)
        _refused(f"softmax_mix bwd={bwd} misaligned P", call(bwd, P=_off(P.ptr(0), f32)), "misaligned", outs)
        _refused(f"softmax_mix bwd={bwd} misaligned weights8", call(bwd, weights8=w8.ptr() + 8), "misaligned", outs)
    _refused("softmax_mix_fwd ld_out < D", call(False, ld_out=4), "bad out", outs)
    _refused("softmax_mix_fwd ld_out % 4", call(False, ld_out=10), "bad out", outs)
    _refused("softmax_mix_fwd misaligned out", call(False, out=_off(out.ptr(), f32)), "misaligned", outs)
    _refused("softmax_mix_bwd ld_dout < D", call(True, ld_dout=4), "bad dout", outs)
    _refused("softmax_mix_bwd NULL dP", call(True, dP=None), "bad dout", outs)
    for f, m in (("dout", dout), ("dP", dP), ("dlogits8", dl8)):
        _refused(f"softmax_mix_bwd misaligned {f}", call(True, **{f: _off(m.ptr(0) if f == "dP" else m.ptr(), f32)}), "misaligned", outs)


# ====================================================================================================== outer_fwd / outer_bwd
def _outer_inputs(B, I, J, f32, seed):
    g = _gen(seed)
    x1 = Mat(B, I, I + 1 + I % 2, f32, _randn(g, B, I) * (1.0 + torch.arange(B, device=DEV).float())[:, None])      # odd ld1: no alignment rule
    x2 = Mat(B, J, J + 4, f32, _randn(g, B, J))
    return x1, x2


# B * I * J / 4 = 2,100,000 groups of 4 against 8192 * 256 = 2,097,152
OUTER_FWD_SHAPES = [(B, I, J) for B in (1, 3) for I, J in ((1, 4), (3, 252), (4, 256), (5, 260), (259, 1024), (4, 1028), (259, 4), (1, 1024))] + [(3, 700, 4000)]


@pytest.mark.parametrize("f32", [1, 0])
def test_outer_fwd(f32):
    """z = x1 (x) x2, dense [B][I J]: I in {1, 3, 4, 5, 259}, J in {4, 252, 256, 260, 1024, 1028}, an odd ld1, ld2 > J, and one
    shape past the 8192-block cap."""
    for B, I, J in OUTER_FWD_SHAPES:
        x1, x2 = _outer_inputs(B, I, J, f32, B + I + J)
        ref = x1.d[:, :, None] * x2.d[:, None, :]
        name = f"outer_fwd f32={f32} B={B} I={I} J={J}"
        snaps = []
        for _ in range(2):
            z = Mat(B, I * J, I * J, f32)
            rc = _lib.load().mmdeer_outer_fwd(x1.ptr(), x1.ld, x2.ptr(), x2.ld, z.ptr(), B, I, J, f32, _stream())
            torch.cuda.synchronize()
            assert rc == 0, f"{name}: {_lib_err()}"
            z.check(name)
            snaps.append(z.snap())
        _same_bits(name, *snaps)
        _check("outer_fwd.z", name, z.val.reshape(B, I, J), ref, ref.abs(), not f32)
        x1.check(name + " x1")
        x2.check(name + " x2")


@pytest.mark.parametrize("f32", [1, 0])
def test_outer_bwd(f32):
    """dx1, dx2 against torch.autograd on the float64 outer product: I < 4 (waves without a row), I = 259, J not a multiple
    of 256, J = 1024; odd ld1 / ldd1, ld2, ldd2 > J."""
    for B in (1, 3):
        for I in (1, 3, 4, 5, 259):
            for J in (4, 252, 256, 260, 1024):
                x1, x2 = _outer_inputs(B, I, J, f32, 2 * B + I + J)
                dz = Mat(B, I * J, I * J, f32, _randn(_gen(B * I + J), B, I * J))
                name = f"outer_bwd f32={f32} B={B} I={I} J={J}"
                a, b = x1.d.clone().requires_grad_(True), x2.d.clone().requires_grad_(True)
                D3 = dz.d.reshape(B, I, J)
                ((a[:, :, None] * b[:, None, :]) * D3).sum().backward()
                s1 = (D3 * x2.d[:, None, :]).abs().sum(2)
                s2 = (D3 * x1.d[:, :, None]).abs().sum(1)
                snaps = []
                for _ in range(2):
                    dx1, dx2 = Mat(B, I, I + 3 - I % 2, f32), Mat(B, J, J + 8, f32)      # ldd1 odd
                    rc = _lib.load().mmdeer_outer_bwd(dz.ptr(), x1.ptr(), x1.ld, x2.ptr(), x2.ld, dx1.ptr(), dx1.ld, dx2.ptr(), dx2.ld, B, I, J, f32, _stream())
                    torch.cuda.synchronize()
                    assert rc == 0, f"{name}: {_lib_err()}"
                    dx1.check(name + " dx1")
                    dx2.check(name + " dx2")
                    snaps.append(torch.cat([dx1.snap(), dx2.snap()]))
                _same_bits(name, *snaps)
                _check("outer_bwd.dx1", name + " dx1", dx1.val, a.grad, s1, not f32)
                _check("outer_bwd.dx2", name + " dx2", dx2.val, b.grad, s2, not f32)
                for m in (x1, x2, dz):
                    m.check(name + " input")


@pytest.mark.parametrize("f32", [1, 0])
def test_outer_refusals(f32):
    lib = _lib.load()
    assert lib.mmdeer_outer_fwd(None, 0, None, 0, None, 0, 3, 8, f32, _stream()) == 0, _lib_err()
    assert lib.mmdeer_outer_bwd(None, None, 0, None, 0, None, 0, None, 0, 0, 3, 8, f32, _stream()) == 0, _lib_err()
    B, I, J = 1, 3, 8
    x1, x2 = _outer_inputs(B, I, J, f32, 5)
    z, dx1, dx2 = Mat(B, I * J, I * J, f32), Mat(B, I, 5, f32), Mat(B, J, 16, f32)
    dz = Mat(B, I * J, I * J, f32, _randn(_gen(6), B, I * J))
    outs = [z, dx1, dx2]

    def fwd(**kw):
        a = dict(x1=x1.ptr(), ld1=x1.ld, x2=x2.ptr(), ld2=x2.ld, z=z.ptr(), B=B, I=I, J=J)
        a.update(kw)
        rc = lib.mmdeer_outer_fwd(a["x1"], a["ld1"], a["x2"], a["ld2"], a["z"], a["B"], a["I"], a["J"], f32, _stream())
        torch.cuda.synchronize()
        return rc

    def bwd(**kw):
        a = dict(dz=dz.ptr(), x1=x1.ptr(), ld1=x1.ld, x2=x2.ptr(), ld2=x2.ld, dx1=dx1.ptr(), ldd1=dx1.ld, dx2=dx2.ptr(), ldd2=dx2.ld, B=B, I=I, J=J)
        a.update(kw)
        rc = lib.mmdeer_outer_bwd(a["dz"], a["x1"], a["ld1"], a["x2"], a["ld2"], a["dx1"], a["ldd1"], a["dx2"], a["ldd2"], a["B"], a["I"], a["J"], f32, _stream())
        torch.cuda.synchronize()
        return rc

    for kw in (dict(J=6), dict(J=0), dict(I=0), dict(B=-1)):
        _refused(f"outer_fwd {kw}", fwd(**kw), "bad shape", outs)
        _refused(f"outer_bwd {kw}", bwd(**kw), "bad shape", outs)
    _refused("outer_bwd J=1028", bwd(J=1028, ld2=1032, ldd2=1032), "J <= 1024", outs)
    for kw in (dict(ld1=2), dict(ld2=4), dict(ld2=10), dict(x1=None)):
        _refused(f"outer_fwd {kw}", fwd(**kw), "leading dimension", outs)
        _refused(f"outer_bwd {kw}", bwd(**kw), "leading dimension", outs)
    for kw in (dict(ldd1=2), dict(ldd2=4), dict(ldd2=10)):
        _refused(f"outer_bwd {kw}", bwd(**kw), "leading dimension", outs)
    _refused("outer_fwd misaligned x2", fwd(x2=_off(x2.ptr(), f32)), "misaligned", outs)
    _refused("outer_fwd misaligned z", fwd(z=_off(z.ptr(), f32)), "misaligned", outs)
    for k, m in (("dz", dz), ("x2", x2), ("dx2", dx2)):
        _refused(f"outer_bwd misaligned {k}", bwd(**{k: _off(m.ptr(), f32)}), "misaligned", outs)
