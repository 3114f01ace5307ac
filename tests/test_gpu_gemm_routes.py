"""mmdeer_gemm on every kernel route behind it, called through the C ABI (include/mmdeer.h).

One call selects one of about a dozen kernels (csrc/gemm.hip: launch_gemm_group, pick_tile in gemm.hip, the gemm_dispatch_*
functions).  ROUTES below names each route with the arguments and launch-plan options that select it, and shapes that land
on it with ragged M and N, a ragged last K-tile and padded leading dimensions.  Every result is compared element-wise with a
float64 product of the operands as the kernel sees them, under an error bound derived from the accumulation (C_BOUND).

Every buffer is filled with a NaN canary bit pattern before the call: C sits inside a buffer with a row above it, a row below
it and ldc - N pad columns; bias_grad and the split-K slab sit inside larger buffers; operands carry canaries in their pad
columns (beyond K, or beyond M / N when transposed) and in two rows past their end.  After each call every canary of an output
buffer must be intact and no stored value may be a NaN (an operand canary that reached a stored output).  A refused call
returns -1, names the field in mmdeer_last_error() and writes nothing."""
import ctypes as C

import pytest
import torch

from mmdeer import _lib

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


def _rup(x, m):
    return (x + m - 1) // m * m


def _ld(extent, f32):
    """Default leading dimension: larger than the extent, a multiple of 8 for bf16 storage (16-byte chunks)."""
    return extent + 4 if f32 else _rup(extent, 8) + 8


class Opnd:
    """A stored matrix of `rows` x `cols` values at row stride `ld` (fp32 or bf16) starting `shift` elements into a canary
    buffer, followed by two canary rows; the pad columns are canaries.  `val` = the stored values as fp32."""

    def __init__(self, rows, cols, ld, f32, seed, shift=0):
        self.buf = _canary((rows + 2) * ld + shift + 8, f32)
        self.ptr = self.buf[shift:].data_ptr()
        w = min(cols, ld)
        v = _randn((rows, w), seed)
        if rows:
            self.buf[shift:shift + rows * ld].view(rows, ld)[:, :w] = v if f32 else v.to(torch.bfloat16)
        self.val = v if f32 else v.to(torch.bfloat16).float()


# ---------------------------------------------------------------------------------------------------------- the route table
# route name -> the arguments that select it (launch_gemm_group / pick_tile / gemm_dispatch_*, restated in the comments), launch
# options, and shapes (M, N, K).  Leading dimensions default to _ld(extent) (ld > extent everywhere), ldc to N + 4 (the 256-row
# forward kernel needs ldc % 8 == 0: N rounded up to 8, + 8).  Under bf16 compute the storage of an operand picks its loader
# source mode: fp32 = F32; bf16 with ld % 8 == 0 and extent % 8 == 0 = V16 (extent = K, or M / N when transposed); else V8.
NT, NX, TT = (0, 0), (0, 1), (1, 1)
ROUTES = {
    # register-staged NT kernel (gemm_group_kernel<.., false, false, ..>): fp32 compute; bf16 off the LDS-DMA kernels (a non-V16
    # operand, K % 64 != 0, or 128x128 tiles outside the glds128 condition).  Mode pairs (V16,V16), (F32,V16), (F32,V8), (V8,V8)
    "nt_f32_t0": dict(tr=NT, f32=1, a32=1, w32=1, tile=0, shapes=[(1, 4, 36), (63, 68, 100), (131, 132, 96)]),
    "nt_f32_t1": dict(tr=NT, f32=1, a32=1, w32=1, tile=1, shapes=[(127, 68, 100), (129, 4, 36), (577, 196, 64)]),
    "nt_f32_t2": dict(tr=NT, f32=1, a32=1, w32=1, tile=2, shapes=[(1, 132, 96), (129, 260, 100)]),
    "nt_bf16_v16v16_t0": dict(tr=NT, f32=0, a32=0, w32=0, tile=0, shapes=[(1, 4, 96), (65, 68, 224), (131, 196, 40)]),
    "nt_bf16_v16v16_t1": dict(tr=NT, f32=0, a32=0, w32=0, tile=1, shapes=[(127, 68, 96), (257, 132, 160)]),
    "nt_bf16_v16v16_t2": dict(tr=NT, f32=0, a32=0, w32=0, tile=2, shapes=[(129, 132, 128), (1, 4, 96)]),
    "nt_bf16_f32v16": dict(tr=NT, f32=0, a32=1, w32=0, tile=0, shapes=[(63, 68, 96), (131, 4, 128)]),
    "nt_bf16_f32v16_t2": dict(tr=NT, f32=0, a32=1, w32=0, tile=2, shapes=[(129, 132, 96)]),
    "nt_bf16_f32v8": dict(tr=NT, f32=0, a32=1, w32=0, tile=1, shapes=[(127, 68, 36), (131, 4, 100)]),
    "nt_bf16_v8v8": dict(tr=NT, f32=0, a32=0, w32=0, tile=0, shapes=[(65, 68, 36), (1, 132, 100)]),
    "nt_bf16_v8v8_t2": dict(tr=NT, f32=0, a32=0, w32=0, tile=2, shapes=[(131, 260, 84)]),
    # register-staged NX kernel (dX = dY W with W stored [K][N]): fp32, or bf16 (V16,V16), (V16,V8 = N % 8 == 4)
    "nx_f32": dict(tr=NX, f32=1, a32=1, w32=1, tile=0, shapes=[(1, 4, 36), (65, 68, 100), (131, 196, 64)]),
    "nx_f32_t2": dict(tr=NX, f32=1, a32=1, w32=1, tile=2, shapes=[(129, 132, 96)]),
    "nx_bf16_v16v16": dict(tr=NX, f32=0, a32=0, w32=0, tile=1, shapes=[(127, 136, 96), (1, 8, 64), (131, 264, 40)]),
    "nx_bf16_v16v8": dict(tr=NX, f32=0, a32=0, w32=0, tile=0, shapes=[(65, 68, 96), (63, 4, 128), (131, 132, 40)]),
    # register-staged TT kernel (dW = dY^T X, A stored [K][M], W stored [K][N]; M % 4 == 0): tiles 0 / 1 always, tile 2 with fp32
    # compute or off the DMA kernel.  bf16 (V16,V16), (V16,F32), (V16,V8 = N % 8 == 4)
    "tt_f32_t0": dict(tr=TT, f32=1, a32=1, w32=1, tile=0, shapes=[(4, 4, 1), (60, 68, 100), (132, 196, 37)]),
    "tt_f32_t2": dict(tr=TT, f32=1, a32=1, w32=1, tile=2, shapes=[(124, 132, 515), (260, 68, 64)]),
    "tt_bf16_v16v16": dict(tr=TT, f32=0, a32=0, w32=0, tile=0, shapes=[(8, 8, 3), (56, 72, 100), (136, 200, 37)]),
    "tt_bf16_v16v16_t1": dict(tr=TT, f32=0, a32=0, w32=0, tile=1, shapes=[(120, 136, 260)]),
    "tt_bf16_v16f32": dict(tr=TT, f32=0, a32=0, w32=1, tile=1, shapes=[(136, 68, 100), (8, 4, 37)]),
    "tt_bf16_v16v8": dict(tr=TT, f32=0, a32=0, w32=0, tile=0, shapes=[(72, 68, 100), (136, 4, 64)]),
    # LDS-DMA NT kernel (gemm_nt_glds_kernel<BM, BN, NST, NW>): bf16 V16 x V16, K % 64 == 0, no split-K, no bias_grad.
    # tile 0: 64x64.  tile 1: 8-wave 128x64 up to 320 tiles (option nt8), 4-wave above; 128x128 (glds128, option nt128) when
    # N % 128 == 0, more than 320 tiles of 128x64 and 160..320 tiles of 128x128
    "glds_64x64": dict(tr=NT, f32=0, a32=0, w32=0, tile=0, shapes=[(1, 4, 64), (63, 68, 128), (65, 196, 192), (131, 132, 64),
                                                                               (65, 68, 320)]),   # 5 K-tiles: the ring's steady state
    "glds_128x64_8w": dict(tr=NT, f32=0, a32=0, w32=0, tile=1, shapes=[(127, 68, 64), (129, 4, 128), (1031, 196, 64)]),
    "glds_128x64_4w": dict(tr=NT, f32=0, a32=0, w32=0, tile=1, shapes=[(4093, 708, 64), (2689, 1028, 128)]),
    "glds_128x128": dict(tr=NT, f32=0, a32=0, w32=0, tile=1, shapes=[(2561, 1280, 64), (2049, 2304, 128)]),
    # 256-row forward LDS-DMA kernel (gemm_nt256_kernel<BN>): tile 3, bf16 V16 x V16, K % 32 == 0, no Y / bias_grad / split-K,
    # C 16-byte aligned, ldc % 8 == 0.  BN = 192 (option nt192) when N % 192 == 0, t192 <= 256 and t192 > t256
    "nt256_256": dict(tr=NT, f32=0, a32=0, w32=0, tile=3, shapes=[(1, 4, 32), (257, 260, 96), (255, 1028, 64),
                                                                              (257, 260, 160)]),   # 5 K stages: the ring's steady state
    "nt256_192": dict(tr=NT, f32=0, a32=0, w32=0, tile=3, shapes=[(777, 768, 96), (1, 768, 32)]),
    # weight-gradient LDS-DMA kernel (gemm_tt_dma_kernel<BM, BN, KG>): TT, bf16 A and W in 16-byte chunks (pad256: a half-valid
    # last chunk when ld >= extent rounded up to 8), K % 32 == 0, fp32 C 16-byte aligned, no epilogue but bias_grad / accumulate.
    # tile 3: 256x256; tile 2 with option dw_tile = 2: 128x128, K-split form (dw_kg = 2) when K % 64 == 0; tile 4: 256x128
    "tt_dma_256": dict(tr=TT, f32=0, a32=0, w32=0, tile=3, shapes=[(8, 84, 32), (260, 84, 96), (520, 268, 1024)]),
    "tt_dma_128k2": dict(tr=TT, f32=0, a32=0, w32=0, tile=2, shapes=[(8, 84, 64), (260, 132, 128), (136, 268, 1024)]),
    "tt_dma_128": dict(tr=TT, f32=0, a32=0, w32=0, tile=2, shapes=[(260, 132, 96), (8, 4, 32)]),
    "tt_dma_128_kg1": dict(tr=TT, f32=0, a32=0, w32=0, tile=2, opts=dict(dw_kg=1), shapes=[(260, 132, 128)]),
    "tt_dma_256x128": dict(tr=TT, f32=0, a32=0, w32=0, tile=4, shapes=[(260, 84, 96), (516, 268, 256)]),
    "tt_auto": dict(tr=TT, f32=0, a32=0, w32=0, tile=-1, shapes=[(260, 132, 1024), (512, 84, 96)]),   # pick_tile: dw_tile
    # fallbacks of tiles 3 / 4 where the DMA kernel does not apply
    "fb_tt_k_ragged": dict(tr=TT, f32=0, a32=0, w32=0, tile=3, shapes=[(136, 132, 100)]),         # K % 32 -> TT 128x128
    "fb_tt4_k_ragged": dict(tr=TT, f32=0, a32=0, w32=0, tile=4, shapes=[(136, 132, 37)]),
    "fb_tt_c_unaligned": dict(tr=TT, f32=0, a32=0, w32=0, tile=3, c_shift=2, shapes=[(136, 132, 96)]),   # C % 16 -> TT 128x128
    "fb_nt_k_ragged": dict(tr=NT, f32=0, a32=0, w32=0, tile=3, shapes=[(257, 132, 104)]),         # K % 32 -> NT 128x64
    "fb_nt_c_unaligned": dict(tr=NT, f32=0, a32=0, w32=0, tile=3, c_shift=2, shapes=[(257, 132, 128)]),   # -> LDS-DMA 128x64
    "fb_nt_mask": dict(tr=NT, f32=0, a32=0, w32=0, tile=3, epi_only=("Y32", "Y16"), shapes=[(257, 132, 64)]),   # Y -> DMA 128x64
    "fb_nt4": dict(tr=NT, f32=0, a32=0, w32=0, tile=4, shapes=[(257, 132, 96)]),                  # 256x128 is dW only -> 128x64
}

# epilogues: name -> argument overrides.  NT / NX routes take the forward / dX ones, TT routes the weight-gradient ones.
EPI_FWD = {
    "plain": {},
    "bias_relu": dict(bias=1, relu=1),
    "drop0": dict(bias=1, relu=1, drop_site=4, drop_shift=0, p=0.3),
    "drop5": dict(drop_site=1, drop_shift=5, p=0.25),
    "regen": dict(regen_site=7, p=0.4),
    "Y32": dict(Y=1, y32=1, mask_scale=1.0 / 0.7),
    "Y16": dict(Y=1, y32=0, mask_scale=1.5),
    "acc": dict(accumulate=1, bias=1),
    "c16": dict(c32=0, bias=1, relu=1),
    "c16_drop0": dict(c32=0, bias=1, relu=1, drop_site=4, drop_shift=0, p=0.3),   # dropout on a bf16 C: per column ...
    "c16_drop5": dict(c32=0, drop_site=1, drop_shift=5, p=0.25),                  # ... and per 32 columns
    "bgrad": dict(bias_grad=1),
}
EPI_DW = {
    "plain": {},
    "bgrad": dict(bias_grad=1),
    "sk3": dict(bias_grad=1, splitk=3, dense_c=1),
    "sk8": dict(splitk=8, dense_c=1),
    "sk_big": dict(bias_grad=1, splitk=1000, dense_c=1),
    "acc": dict(accumulate=1, bias_grad=1),
}
REPEAT = ("plain", "bgrad", "sk3", "drop0", "Y16")     # epilogues also run twice: bitwise identical


def _epilogues(name, r):
    if r.get("epi_only"):
        return {k: EPI_FWD[k] for k in r["epi_only"]}
    if r["tr"] == TT:
        e = dict(EPI_DW)
        if not name.startswith(("tt_dma", "fb_tt", "tt_auto")):
            e["c16_relu"] = dict(c32=0, relu=1)       # an epilogue on a register-staged dW
        return e
    e = dict(EPI_FWD)
    if name.startswith(("glds", "nt256")):
        for k in ("Y32", "Y16", "bgrad"):              # each of these moves the call off that kernel (see fb_nt_mask)
            e.pop(k)
    if r.get("c_shift"):
        for k in ("c16", "c16_drop0", "c16_drop5"):    # a bf16 C two elements off is not 8-byte aligned (a refusal)
            e.pop(k)
    return e


def _spec(route, M, N, K, **kw):
    r = ROUTES[route]
    s = dict(M=M, N=N, K=K, ta=r["tr"][0], tw=r["tr"][1], f32=r["f32"], a32=r["a32"], w32=r["w32"], tile=r["tile"],
             c32=1, c_shift=r.get("c_shift", 0), bias=0, relu=0, drop_site=-1, drop_shift=0, regen_site=-1, p=0.0, Y=0,
             y32=1, mask_scale=1.0, accumulate=0, bias_grad=0, splitk=1, seed=1234, offset=5, offset_dev=None)
    s.update(kw)
    return s


class Call:
    """Operands, canary-wrapped outputs and the argument struct of one mmdeer_gemm call."""

    def __init__(self, s, seed=0):
        M, N, K = s["M"], s["N"], s["K"]
        self.s = s
        a_rows, a_cols = (K, M) if s["ta"] else (M, K)
        w_rows, w_cols = (K, N) if s["tw"] else (N, K)
        self.lda = s.get("lda") or _ld(a_cols, s["a32"])
        self.ldw = s.get("ldw") or _ld(w_cols, s["w32"])
        if s.get("ldc"):
            self.ldc = s["ldc"]
        elif s.get("dense_c"):
            self.ldc = N
        else:
            self.ldc = _rup(N, 8) + 8 if s["tile"] == 3 and not s["ta"] else N + 4
        self.ldy = s.get("ldy") or N + 4
        self.A = Opnd(a_rows, a_cols, self.lda, s["a32"], 100 + seed, s.get("a_shift", 0))
        self.W = Opnd(w_rows, w_cols, self.ldw, s["w32"], 200 + seed, s.get("w_shift", 0))
        c32 = s["c32"]
        self.c_off = self.ldc + s["c_shift"]                 # one canary row above C
        self.cbuf = _canary(self.c_off + (M + 1) * self.ldc + 8, c32)
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
            # the library may use min(splitk, K-tiles) slices of M*N + M floats (rounded up to 4); the allocation leaves room for
            # a slice written at row stride ldc > N, so that a wrong stride lands on canaries, not outside the buffer
            self.slice = _rup(M * N + M, 4)
            nk = -(-K // (32 if s["f32"] else 64))
            self.slab_n = min(s["splitk"], nk) * self.slice
            self.slab = _canary((min(s["splitk"], nk) + 1) * max(self.slice, M * self.ldc + M) + 64, 1)
        self.args = _lib.gemm_args(
            A=self.A.ptr, W=self.W.ptr, C=self.cbuf[self.c_off:].data_ptr(),
            bias=self.biasbuf.data_ptr() if self.biasbuf is not None else None,
            bias_grad=self.bgbuf[4:].data_ptr() if self.bgbuf is not None else None, Y=self.Ybuf.data_ptr() if s["Y"] else None,
            M=M, N=N, K=K, lda=self.lda, ldw=self.ldw, ldc=self.ldc, ldy=self.ldy if s["Y"] else 0,
            a_f32=s["a32"], w_f32=s["w32"], c_f32=c32, y_f32=s["y32"], trans_a=s["ta"], trans_w=s["tw"], relu=s["relu"],
            accumulate=s["accumulate"], compute_f32=s["f32"], tile=s["tile"], drop_site=s["drop_site"], drop_shift=s["drop_shift"],
            regen_site=s["regen_site"], dropout_p=s["p"], mask_scale=s["mask_scale"], seed=s["seed"], offset=s["offset"],
            offset_dev=s["offset_dev"], splitk=s["splitk"], slab=self.slab.data_ptr() if self.slab is not None else None, stream=_stream())

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


def _run_checked(s, msg, twice=False):
    c = Call(s)
    assert c.run() == 0, f"{msg}: {_err()}"
    _check(c, msg)
    if twice:
        c2 = Call(s)
        assert c2.run() == 0, f"{msg}: {_err()}"
        assert torch.equal(_bits(c.cbuf), _bits(c2.cbuf)), f"{msg}: two identical calls differ"
        if c.bgbuf is not None:
            assert torch.equal(_bits(c.bgbuf), _bits(c2.bgbuf)), f"{msg}: two identical calls differ in bias_grad"
    return c


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_route_edges_and_epilogues(route):
    """Every shape of the route under every epilogue it takes, against float64; some of them twice: bitwise identical."""
    r = ROUTES[route]
    with _lib.options(**r.get("opts", {})):
        for (M, N, K) in r["shapes"]:
            for ename, e in _epilogues(route, r).items():
                _run_checked(_spec(route, M, N, K, **e), f"route={route} M={M} N={N} K={K} epilogue={ename}",
                             twice=ename in REPEAT)


# a representative subset of the routes, re-run under every non-default launch-plan value
PLAN_ROUTES = ["nt_bf16_v16v16_t1", "glds_64x64", "glds_128x64_8w", "glds_128x64_4w", "glds_128x128", "nt256_256", "nt256_192",
               "tt_dma_256", "tt_dma_128k2", "tt_dma_256x128", "tt_auto", "tt_bf16_v16v16", "nx_bf16_v16v16", "nt_f32_t1"]
PLANS = [dict(glds=0), dict(nt8=0), dict(nt128=0), dict(nt192=0), dict(xcd=0), dict(dw_tile=3), dict(dw_tile=4), dict(dw_kg=1)]


@pytest.mark.parametrize("plan", PLANS, ids=lambda d: "-".join(f"{k}{v}" for k, v in d.items()))
def test_launch_plans(plan):
    before = {k: _lib.get_option(k) for k in plan}
    with _lib.options(**plan):
        for route in PLAN_ROUTES:
            r = ROUTES[route]
            for (M, N, K) in r["shapes"][:2]:
                if r["tr"] == TT and not r["f32"]:
                    # a transposed bf16 A with M % 8 == 4 is read in half-valid chunks by the weight-gradient DMA kernel only;
                    # the plans that move the call off that kernel refuse it (test_refusal_writes_nothing[tt_v8_v16])
                    M = _rup(M, 8)
                for ename in (("bgrad", "sk3") if r["tr"] == TT else ("plain", "drop0")):
                    e = (EPI_DW if r["tr"] == TT else EPI_FWD)[ename]
                    _run_checked(_spec(route, M, N, K, **e), f"plan={plan} route={route} M={M} N={N} K={K} {ename}", twice=True)
    assert {k: _lib.get_option(k) for k in plan} == before, "launch-plan options not restored"


@pytest.mark.parametrize("route", ["nt_f32_t0", "glds_128x64_8w", "nt256_256", "nx_bf16_v16v16"])
def test_offset_dev_equals_offset_plus_counter(route):
    """A device counter added to `offset` when the kernel runs: bit-identical to offset + counter passed directly."""
    M, N, K = ROUTES[route]["shapes"][1]
    ctr = torch.tensor([123457], dtype=torch.int64, device=DEV)
    for e in (dict(relu=1, drop_site=3, drop_shift=0, p=0.3), dict(regen_site=2, drop_shift=5, p=0.5)):
        c = Call(_spec(route, M, N, K, offset=11, offset_dev=ctr.data_ptr(), **e))
        assert c.run() == 0, _err()
        d = _run_checked(_spec(route, M, N, K, offset=11 + 123457, **e), f"route={route} offset direct {e}")
        assert torch.equal(_bits(c.cbuf), _bits(d.cbuf)), f"route={route} {e}: offset_dev differs from offset + counter"


UNSPLITTABLE = {   # name: (route, arguments) of a problem whose outputs the split-K fold cannot take
    "ldc_wide_f32": ("tt_f32_t0", dict(M=60, N=68, K=515, ldc=76)),
    "ldc_wide_bf16": ("tt_bf16_v16v16_t1", dict(M=120, N=136, K=1024, ldc=144)),
    "ldc_wide_dma128": ("tt_dma_128k2", dict(M=260, N=132, K=1024, ldc=140)),
    "ldc_wide_dma256": ("tt_dma_256", dict(M=520, N=268, K=1024, ldc=276)),
    "c_unaligned": ("tt_f32_t2", dict(M=124, N=132, K=515, c_shift=2, dense_c=1)),
    "bias_grad_M130": ("nt_f32_t0", dict(M=130, N=68, K=1000, dense_c=1)),
    "bias_grad_M131": ("nt_f32_t1", dict(M=131, N=132, K=640, dense_c=1)),
}


@pytest.mark.parametrize("case", sorted(UNSPLITTABLE))
def test_split_request_on_unsplittable_outputs_runs_unsplit(case):
    """splitk > 1 on a problem whose C has ldc > N, whose C is not 16-byte aligned, or whose bias_grad has M % 4 != 0: accepted,
    the same bits as splitk = 1, every canary intact (C's pad columns, the slab)."""
    route, kw = UNSPLITTABLE[case]
    kw = dict(kw, bias_grad=1)
    for sk in (3, 8):
        s = _spec(route, splitk=sk, **kw)
        msg = f"route={route} {kw} splitk={sk}"
        c = _run_checked(s, msg)
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
                         twice=True)


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
def _set(**kw):
    return lambda s: s.update(kw)


def _args(**kw):
    return lambda a: [setattr(a, k, v) for k, v in kw.items()]


# name: (route, (M, N, K), change of the spec before the buffers are built, change of the struct after, word(s) of the message).
# Every pointer stays a real allocation: a missing check must not launch on a made-up address.
REFUSALS = {
    "N_mod4": ("nt_f32_t0", (64, 68, 64), None, _args(N=66), "N=66"),
    "K_mod4_A": ("nt_f32_t0", (64, 68, 66), None, None, "K=66"),
    "M_mod4_transA": ("tt_f32_t0", (62, 68, 64), None, None, "M=62"),
    "lda_mod4": ("nt_f32_t0", (64, 68, 64), None, _args(lda=70), "leading dims"),
    "ldw_mod4": ("nt_f32_t0", (64, 68, 64), None, _args(ldw=70), "leading dims"),
    "ldc_mod4": ("nt_f32_t0", (64, 68, 64), None, _args(ldc=70), "leading dims"),
    "ldy_mod4": ("nt_f32_t0", (64, 68, 64), _set(Y=1), _args(ldy=70), "ldy"),
    "A_unaligned": ("nt_f32_t0", (64, 68, 64), _set(a_shift=2), None, "aligned"),
    "W_unaligned": ("nt_bf16_v16v16_t0", (64, 68, 64), _set(w_shift=4), None, "aligned"),
    "accumulate_bf16_C": ("nt_bf16_v16v16_t0", (64, 68, 96), _set(c32=0), _args(accumulate=1), "accumulate"),
    "splitk_bias": ("tt_f32_t0", (64, 68, 512), _set(splitk=3, bias_grad=1, dense_c=1), lambda a: setattr(a, "bias", a.bias_grad),
                    "split-K"),
    "splitk_relu": ("tt_f32_t0", (64, 68, 512), _set(splitk=3, bias_grad=1, dense_c=1), _args(relu=1), "split-K"),
    "splitk_accumulate": ("tt_f32_t0", (64, 68, 512), _set(splitk=3, dense_c=1), _args(accumulate=1), "split-K"),
    "splitk_drop": ("tt_f32_t0", (64, 68, 512), _set(splitk=3, dense_c=1), _args(drop_site=2, dropout_p=0.5), "split-K"),
    "splitk_bf16_C": ("tt_f32_t0", (64, 68, 512), _set(splitk=3, dense_c=1), _args(c_f32=0), "split-K"),
    "splitk_no_slab": ("tt_f32_t0", (64, 68, 512), _set(splitk=3, dense_c=1), _args(slab=None), "slab"),
    "splitk_no_slab_wide_ldc": ("tt_f32_t0", (64, 68, 512), _set(splitk=3), _args(slab=None), "slab"),
    "f32_compute_bf16_A": ("nt_f32_t0", (64, 68, 64), _set(a32=0), None, "fp32 operands"),
    "f32_compute_bf16_W": ("nx_f32", (64, 68, 64), _set(w32=0), None, "fp32 operands"),
    "nt_v16_f32": ("nt_bf16_v16v16_t0", (64, 68, 96), _set(w32=1), None, "not instantiated"),
    "nt_v8_v16": ("nt_bf16_v16v16_t0", (64, 68, 96), _set(lda=100), None, "not instantiated"),
    "nt_v16_v8": ("nt_bf16_v16v16_t0", (64, 68, 96), _set(ldw=100), None, "not instantiated"),
    "nt_v8_f32": ("nt_bf16_v16v16_t0", (64, 68, 36), _set(w32=1), None, "not instantiated"),
    "nx_f32_v16": ("nx_bf16_v16v16", (64, 72, 96), _set(a32=1), None, "not instantiated"),
    "nx_v8_v16": ("nx_bf16_v16v16", (64, 72, 36), None, None, "not instantiated"),
    "nx_v16_f32": ("nx_bf16_v16v16", (64, 72, 96), _set(w32=1), None, "not instantiated"),
    "tt_v8_v16": ("tt_bf16_v16v16", (68, 72, 96), None, None, "not instantiated"),     # M % 8 == 4 off the DMA kernels
    "tt_f32_v16": ("tt_bf16_v16v16", (64, 72, 96), _set(a32=1), None, "not instantiated"),
    "tt_half_valid_A_unaligned_C": ("tt_dma_256", (260, 84, 96), _set(c_shift=2), None, "not instantiated"),
    "transA_only": ("tt_f32_t0", (64, 68, 64), None, _args(trans_w=0), "trans_a=1, trans_b=0"),
    "lda_short": ("nt_f32_t0", (64, 68, 64), _set(lda=60), None, "lda=60"),
    "lda_short_transA": ("tt_f32_t0", (64, 68, 64), _set(lda=60), None, "lda=60"),
    "ldw_short": ("nt_f32_t0", (64, 68, 64), _set(ldw=60), None, "ldw=60"),
    "ldw_short_transW": ("nx_f32", (64, 68, 64), _set(ldw=64), None, "ldw=64"),
    "ldc_short": ("nt_f32_t0", (64, 68, 64), _set(ldc=64), None, "ldc=64"),
    "ldc_short_glds": ("glds_64x64", (64, 68, 64), _set(ldc=64), None, "ldc=64"),
    "ldy_short": ("nt_f32_t0", (64, 68, 64), _set(Y=1, ldy=64), None, "ldy=64"),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusal_writes_nothing(name):
    route, (M, N, K), pre, post, words = REFUSALS[name]
    s = _spec(route, M, N, K, bias_grad=int(ROUTES[route]["tr"] == TT))
    if pre:
        pre(s)
    c = Call(s)
    if post:
        post(c.args)
    assert c.run() == -1, f"{name}: accepted"
    assert words in _err(), f"{name}: message {_err()!r} does not name {words!r}"
    assert c.outputs_untouched(), f"{name}: the refused call wrote an output"
