"""mmdeer_gemm on every kernel route behind it, called through the C ABI (include/mmdeer.h).

One call selects one of about a dozen kernels (csrc/gemm.hip: gemm_route, pick_tile).  ROUTES (tests/gemm_route_table.py) names
each route with the arguments and launch-plan options that select it, the route line the library's dry run (mmdeer_gemm_route)
must answer, and shapes that land on it with ragged M and N, a ragged last K-tile and padded leading dimensions.  Before every
checked call the dry run on the same struct is asserted to name the expected kernel, tile and source modes: a route that moved
onto another kernel fails instead of passing on the fallback.  Every result is compared element-wise with a float64 product of
the operands as the kernel sees them, under an error bound derived from the accumulation (C_BOUND).

Every buffer is filled with a NaN canary bit pattern before the call: C sits inside a buffer with a row above it, a row below
it and ldc - N pad columns; bias_grad and the split-K slab sit inside larger buffers; operands carry canaries in their pad
columns (beyond K, or beyond M / N when transposed) and in two rows past their end.  After each call every canary of an output
buffer must be intact and no stored value may be a NaN (an operand canary that reached a stored output).  A refused call
returns -1, names the field in mmdeer_last_error() and writes nothing."""
import ctypes as C

import pytest
import torch

from mmdeer import _lib

from .gemm_route_table import (PLAN_ROUTES, PLANS, REFUSALS, REPEAT, ROUTES, UNSPLITTABLE, Layout, dry_run, plan_cases,
                               plan_route_line, refusal_spec, route_cases, route_line, without_tiles)
from .gemm_route_table import spec as _spec

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CANARY32 = 0x7FA5A5A5          # a NaN no kernel produces (payload), as int32 / float32 bits
CANARY16 = 0x7FA5              # the same for bf16 storage
U = 2.0 ** -24                 # unit roundoff of the fp32 accumulators
# Bound per compute dtype: |C - ref| <= c * U * sum_k |a_ik w_jk|, plus the rounding of the stored value (fp32: U |ref|; bf16 C:
# half an ulp).  The accumulators add fp32 partial sums over K in a fixed sequence: K / 4 MFMA steps of 4 rounded fp32 products
# (fp32 compute) or K / 32 steps of 32 exact bf16 products, then the fold of the split-K slices.  For the zero-mean data used here
# the rounding errors have random signs and stay within a few units of U * sum |a w| at any K (the worst case, K * U, is never
# approached); fp32 compute also rounds every product, hence its larger constant.  A kernel that drops, repeats or misplaces a
# single product of a K = 4096 sum is off by ~ sum / K, orders of magnitude above these bounds.
C_BOUND = {1: 16.0, 0: 8.0}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _err():
    return _lib.load().mmdeer_last_error().decode()


def _canary(n, f32):
    if f32:
        return torch.full((max(n, 1),), CANARY32, dtype=torch.int32, device=DEV).view(torch.float32)
    return torch.full((max(n, 1),), CANARY16, dtype=torch.int16, device=DEV).view(torch.bfloat16)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16)


def _canaries_broken(buf, written=None):
    c = CANARY32 if buf.dtype == torch.float32 else CANARY16
    bad = _bits(buf) != c
    if written is not None:
        bad &= ~written
    return int(bad.sum())


def _randn(shape, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(*shape, generator=g, device=DEV)


class Opnd:
    """A stored matrix of `rows` x `cols` values at row stride `ld` (fp32 or bf16) starting `shift` elements into a canary
    buffer, followed by two canary rows; the pad columns are canaries.  `val` = the stored values as fp32."""

    def __init__(self, rows, cols, ld, f32, seed, shift=0):
        self.buf = _canary((rows + 2) * ld + shift + 8, f32)
        w = min(cols, ld)
        v = _randn((rows, w), seed)
        if rows:
            self.buf[shift:shift + rows * ld].view(rows, ld)[:, :w] = v if f32 else v.to(torch.bfloat16)
        self.val = v if f32 else v.to(torch.bfloat16).float()


class Call:
    """Operands, canary-wrapped outputs and the argument struct of one mmdeer_gemm call."""

    def __init__(self, s, seed=0):
        M, N = s["M"], s["N"]
        self.s = s
        self.lay = lay = Layout(s)
        self.ldc, self.ldy, self.c_off = lay.ldc, lay.ldy, lay.c_off
        self.A = Opnd(lay.a_rows, lay.a_cols, lay.lda, s["a32"], 100 + seed, lay.a_shift)
        self.W = Opnd(lay.w_rows, lay.w_cols, lay.ldw, s["w32"], 200 + seed, lay.w_shift)
        c32 = s["c32"]
        self.cbuf = _canary(self.c_off + (M + 1) * self.ldc + 8, c32)          # c_off: one canary row above C
        self.C0 = None
        if s["accumulate"]:
            self.C0 = _randn((M, N), 300 + seed)
            self.cwin().copy_(self.C0)
        self.bias = _randn((N,), 400 + seed) if s["bias"] else None
        self.biasbuf = None
        if s["bias"]:
            self.biasbuf = _canary(N + 8, 1)
            self.biasbuf[:N] = self.bias
        self.Yv = None
        if s["Y"]:
            self.Ybuf = _canary((M + 1) * self.ldy + 8, s["y32"])
            w = min(N, self.ldy)
            yv = _randn((M, w), 500 + seed)
            if M:
                self.Ybuf[:M * self.ldy].view(M, self.ldy)[:, :w] = yv if s["y32"] else yv.to(torch.bfloat16)
            self.Yv = yv if s["y32"] else yv.to(torch.bfloat16).float()
        self.bgbuf = _canary(M + 12, 1) if s["bias_grad"] else None
        self.slab = None
        if s["splitk"] > 1:
            # the allocation leaves room for a slice written at row stride ldc > N, so that a wrong stride lands on canaries, not
            # outside the buffer
            self.slab_n = lay.slices * lay.slice
            self.slab = _canary((lay.slices + 1) * max(lay.slice, M * self.ldc + M) + 64, 1)
        self.args = lay.args(s, self.A.buf.data_ptr(), self.W.buf.data_ptr(), self.cbuf.data_ptr(), bias=_lib.ptr(self.biasbuf),
                             bias_grad=_lib.ptr(self.bgbuf), Y=self.Ybuf.data_ptr() if s["Y"] else None, slab=_lib.ptr(self.slab),
                             stream=_stream())

    def cwin(self):
        M, N = self.s["M"], self.s["N"]
        return self.cbuf[self.c_off:self.c_off + M * self.ldc].view(M, self.ldc)[:, :N]

    def written(self):
        M, N = self.s["M"], self.s["N"]
        w = torch.zeros(self.cbuf.numel(), dtype=torch.bool, device=DEV)
        w[self.c_off:self.c_off + M * self.ldc].view(M, self.ldc)[:, :N] = True
        return w

    def run(self):
        rc = _lib.load().mmdeer_gemm(C.byref(self.args))
        torch.cuda.synchronize()
        return rc

    def outputs_untouched(self):
        """Every canary of every output buffer intact (a refused call, M = 0); a preloaded C window still holds C0."""
        if self.C0 is None:
            n = _canaries_broken(self.cbuf)
        else:
            n = _canaries_broken(self.cbuf, self.written()) + int((self.cwin() != self.C0).sum())
        if self.bgbuf is not None:
            n += _canaries_broken(self.bgbuf)
        if self.slab is not None:
            n += _canaries_broken(self.slab)
        return n == 0


def _keep(site, shift, s):
    """The keep mask of a dropout site as the library draws it (mmdeer_dropout_mask), expanded to [M][N]."""
    M, N = s["M"], s["N"]
    cols = (N + (1 << shift) - 1) >> shift
    m = torch.empty(M, cols, dtype=torch.uint8, device=DEV)
    _lib.check(_lib.load().mmdeer_dropout_mask(site, M, cols, s["p"], s["seed"], s["offset"], m.data_ptr(), _stream()))
    torch.cuda.synchronize()
    m = m.double()
    return m if shift == 0 else m.repeat_interleave(1 << shift, dim=1)[:, :N]


def _operands64(c):
    """op(A) [M][K] and op(W) [N][K] in float64, as the kernel sees them (bf16 compute: fp32 sources rounded to bf16, RNE)."""
    s = c.s
    A = c.A.val.t() if s["ta"] else c.A.val
    W = c.W.val.t() if s["tw"] else c.W.val
    if not s["f32"]:
        A, W = A.to(torch.bfloat16), W.to(torch.bfloat16)
    return A.double(), W.double()


def _half_ulp_bf16(x):
    """Half an ulp of bf16 (8 significant bits) at |x|."""
    _, e = torch.frexp(x.float())
    return torch.where(x == 0, torch.zeros_like(x), torch.ldexp(torch.ones_like(x), e - 9))


def _check(c, msg):
    """Values against the float64 reference under the element-wise bound; every canary of the output buffers intact."""
    s = c.s
    M, N = s["M"], s["N"]
    A, W = _operands64(c)
    ref = A @ W.t()
    mag = A.abs() @ W.abs().t()
    if c.bias is not None:
        ref = ref + c.bias.double()
        mag = mag + c.bias.double().abs()
    if s["relu"]:
        ref = ref.clamp_min(0)
    site = s["drop_site"] if s["drop_site"] >= 0 else s["regen_site"]
    if site >= 0:
        k = _keep(site, s["drop_shift"], s) / (1 - s["p"])
        ref, mag = ref * k, mag * k
    if c.Yv is not None:
        k = (c.Yv.double() > 0).double() * s["mask_scale"]
        ref, mag = ref * k, mag * k
    bound = C_BOUND[s["f32"]] * U * mag
    if c.C0 is not None:
        ref = ref + c.C0.double()
        bound = bound + U * c.C0.double().abs()
    bound = bound + U * ref.abs()                        # the fp32 result's own rounding
    if not s["c32"]:
        bound = bound + _half_ulp_bf16(ref.abs() + bound)
    got = c.cwin().double()
    assert bool(torch.isfinite(got).all()), f"{msg}: a stored value is not finite (an operand canary reached C?)"
    excess = (got - ref).abs() - bound
    i = int(excess.argmax())
    assert float(excess.view(-1)[i]) <= 0, (
        f"{msg}: |C - ref| exceeds its bound at ({i // N}, {i % N}): got {float(got.view(-1)[i])!r} ref {float(ref.view(-1)[i])!r} "
        f"bound {float(bound.view(-1)[i]):.3g}; {int((excess > 0).sum())} elements out of bound")
    assert _canaries_broken(c.cbuf, c.written()) == 0, f"{msg}: a canary around C (rows above / below, pad columns) was written"
    if c.bgbuf is not None:
        bg = c.bgbuf[4:4 + M].double()
        bref, bmag = A.sum(1), A.abs().sum(1)
        assert bool(torch.isfinite(bg).all()), f"{msg}: non-finite bias_grad"
        bexc = float(((bg - bref).abs() - C_BOUND[s["f32"]] * U * bmag - U * bref.abs()).max())
        assert bexc <= 0, f"{msg}: bias_grad exceeds its bound by {bexc:.3g}"
        w = torch.zeros(c.bgbuf.numel(), dtype=torch.bool, device=DEV)
        w[4:4 + M] = True
        assert _canaries_broken(c.bgbuf, w) == 0, f"{msg}: a canary around bias_grad was written"
    if c.slab is not None:
        w = torch.zeros(c.slab.numel(), dtype=torch.bool, device=DEV)
        w[:c.slab_n] = True
        assert _canaries_broken(c.slab, w) == 0, f"{msg}: written past the slab's splitk slices"


def _run_checked(s, msg, twice=False, want=None):
    """One checked call.  `want`: the route line (without tiles=) the dry run must answer for the same struct before the call."""
    c = Call(s)
    if want is not None:
        rc, lines = dry_run(c.args)
        assert (rc, [without_tiles(x) for x in lines]) == (1, [want]), f"{msg}: the dry run answers {rc} {lines}, not {want!r}: {_err()}"
    assert c.run() == 0, f"{msg}: {_err()}"
    _check(c, msg)
    if twice:
        c2 = Call(s)
        assert c2.run() == 0, f"{msg}: {_err()}"
        assert torch.equal(_bits(c.cbuf), _bits(c2.cbuf)), f"{msg}: two identical calls differ"
        if c.bgbuf is not None:
            assert torch.equal(_bits(c.bgbuf), _bits(c2.bgbuf)), f"{msg}: two identical calls differ in bias_grad"
    return c


def _name(s):
    return f"M={s['M']} N={s['N']} K={s['K']}"


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_route_edges_and_epilogues(route):
    """Every shape of the route under every epilogue it takes, on the kernel the table names, against float64; some of them twice:
    bitwise identical."""
    with _lib.options(**ROUTES[route].get("opts", {})):
        for s, i, ename in route_cases(route):
            _run_checked(s, f"route={route} {_name(s)} epilogue={ename}", twice=ename in REPEAT, want=route_line(route, i, ename))


@pytest.mark.parametrize("plan", PLANS, ids=lambda d: "-".join(f"{k}{v}" for k, v in d.items()))
def test_launch_plans(plan):
    before = {k: _lib.get_option(k) for k in plan}
    with _lib.options(**plan):
        for route in PLAN_ROUTES:
            for s, i, ename in plan_cases(route):
                _run_checked(s, f"plan={plan} route={route} {_name(s)} {ename}", twice=True, want=plan_route_line(plan, route, i, s))
    assert {k: _lib.get_option(k) for k in plan} == before, "launch-plan options not restored"


@pytest.mark.parametrize("route", ["nt_f32_t0", "glds_128x64_8w", "nt256_256", "nx_bf16_v16v16"])
def test_offset_dev_equals_offset_plus_counter(route):
    """A device counter added to `offset` when the kernel runs: bit-identical to offset + counter passed directly."""
    M, N, K = ROUTES[route]["shapes"][1]
    ctr = torch.tensor([123457], dtype=torch.int64, device=DEV)
    for e in (dict(relu=1, drop_site=3, drop_shift=0, p=0.3), dict(regen_site=2, drop_shift=5, p=0.5)):
        c = Call(_spec(route, M, N, K, offset=11, offset_dev=ctr.data_ptr(), **e))
        assert c.run() == 0, _err()
        d = _run_checked(_spec(route, M, N, K, offset=11 + 123457, **e), f"route={route} offset direct {e}", want=route_line(route, 1))
        assert torch.equal(_bits(c.cbuf), _bits(d.cbuf)), f"route={route} {e}: offset_dev differs from offset + counter"


@pytest.mark.parametrize("case", sorted(UNSPLITTABLE))
def test_split_request_on_unsplittable_outputs_runs_unsplit(case):
    """splitk > 1 on a problem whose C has ldc > N, whose C is not 16-byte aligned, or whose bias_grad has M % 4 != 0: accepted,
    the same bits as splitk = 1, every canary intact (C's pad columns, the slab)."""
    route, kw = UNSPLITTABLE[case]
    kw = dict(kw, bias_grad=1)
    for sk in (3, 8):
        s = _spec(route, splitk=sk, **kw)
        msg = f"route={route} {kw} splitk={sk}"
        c = _run_checked(s, msg, want=route_line(route))
        assert _canaries_broken(c.slab) == 0, f"{msg}: the slab of an unsplit problem was written"
        c1 = Call(dict(s, splitk=1))
        assert c1.run() == 0, _err()
        assert torch.equal(_bits(c.cbuf), _bits(c1.cbuf)), f"{msg}: differs from splitk = 1"
        assert torch.equal(_bits(c.bgbuf), _bits(c1.bgbuf)), f"{msg}: bias_grad differs from splitk = 1"


@pytest.mark.parametrize("f32", [0, 1])
def test_split_k_every_count(f32):
    """Dense C: splitk 2, 3, 8 and more slices than K-tiles all meet the bound; the slab holds only the clamped slices."""
    route = "tt_f32_t2" if f32 else "tt_dma_128k2"
    for (M, N, K) in ((124, 132, 515), (260, 132, 1024)) if f32 else ((260, 132, 1024), (8, 84, 64)):
        for sk in (2, 3, 8, 64):
            _run_checked(_spec(route, M, N, K, splitk=sk, bias_grad=1, dense_c=1), f"f32={f32} M={M} N={N} K={K} splitk={sk}",
                         twice=True, want=route_line(route))


# ---------------------------------------------------------------------------------------------- production shapes, auto tile
# (N, K) of the model's Linear layers (spec.py dims: audio 84, video 256, text 768, fusion 512, in_proj 3 x 512, head 256/128/64)
LAYERS = [(512, 768), (512, 256), (512, 84), (1536, 512), (512, 512), (256, 512), (128, 256), (64, 128), (512, 1536)]


@pytest.mark.parametrize("B", [32, 1024, 4096])
def test_auto_tile_production_shapes(B):
    """tile = -1 on the forward, dX and dW products of the Linear layers at dense strides, as the operator sequences issue them:
    bf16 compute (the fp32 audio input, K = 84, converted by the loader), and fp32 compute on a subset."""
    for (Nl, Kl) in LAYERS:
        a32 = 1 if Kl == 84 else 0
        base = dict(f32=0, w32=0, tile=-1, dense_c=1)
        _run_checked(_spec("nt_f32_t0", B, Nl, Kl, ta=0, tw=0, a32=a32, lda=Kl, ldw=Kl, bias=1, relu=1, **base),
                     f"B={B} forward N={Nl} K={Kl}")
        if Kl != 84:   # dX = dY W: against the packed W^T [K_l][N_l] (NT) with a (Y > 0) mask, and against W [N_l][K_l] (NX)
            _run_checked(_spec("nt_f32_t0", B, Kl, Nl, ta=0, tw=0, a32=0, lda=Nl, ldw=Nl, Y=1, y32=0, mask_scale=1 / 0.9, **base),
                         f"B={B} dX (W^T) N={Kl} K={Nl}")
            _run_checked(_spec("nt_f32_t0", B, Kl, Nl, ta=0, tw=1, a32=0, lda=Nl, ldw=Kl, **base), f"B={B} dX (W) N={Kl} K={Nl}")
        _run_checked(_spec("nt_f32_t0", Nl, Kl, B, ta=1, tw=1, a32=0, lda=Nl, ldw=Kl, bias_grad=1, **dict(base, w32=a32)),
                     f"B={B} dW M={Nl} N={Kl}")
    for (Nl, Kl) in LAYERS[:3]:
        _run_checked(_spec("nt_f32_t0", B, Nl, Kl, tile=-1, lda=Kl, ldw=Kl, bias=1, dense_c=1), f"B={B} fp32 forward N={Nl} K={Kl}")
        _run_checked(_spec("tt_f32_t0", Nl, Kl, B, tile=-1, lda=Nl, ldw=Kl, bias_grad=1, dense_c=1), f"B={B} fp32 dW M={Nl} N={Kl}")


@pytest.mark.parametrize("route", ["nt_f32_t0", "glds_64x64", "nt256_256", "nx_bf16_v16v16", "fb_nt_mask"])
def test_m_zero_writes_nothing(route):
    c = Call(_spec(route, 0, 68, 64, bias=1, Y=int(route == "fb_nt_mask")))
    assert c.run() == 0, f"route={route}: {_err()}"
    assert c.outputs_untouched(), f"route={route}: M = 0 wrote an output"


# ------------------------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusal_writes_nothing(name):
    """Every pointer stays a real allocation: a missing check must not launch on a made-up address."""
    s, post, words = refusal_spec(name)
    c = Call(s)
    if post:
        post(c.args)
    assert dry_run(c.args)[0] == -1, f"{name}: the dry run accepts"
    dry_msg = _err()
    assert c.run() == -1, f"{name}: accepted"
    assert words in _err(), f"{name}: message {_err()!r} does not name {words!r}"
    assert dry_msg == _err(), f"{name}: the dry run refuses with {dry_msg!r}, the call with {_err()!r}"
    assert c.outputs_untouched(), f"{name}: the refused call wrote an output"
