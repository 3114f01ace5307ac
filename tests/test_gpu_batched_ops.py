"""The batched operators of Stack B's fused training step on their own, called through the C ABI (include/mmdeer.h):
mmdeer_gemm_batch (+ _slab_elems), mmdeer_reduce_batch, mmdeer_pack_transposed_batch and mmdeer_adamw_flat / optim.FlatAdamW.

Tables are drawn at random from fixed seeds, large enough to cross every launch boundary (16 GEMM problems, 48 fold segments,
32 transposed matrices), and compared with float64 PyTorch (torch.optim.AdamW for the optimiser).  Every output lives in a
larger buffer filled with a NaN canary bit pattern before, after and between the windows that may be written; after each call
every canary must be intact.  A refused call returns -1, names the bad entry and writes nothing."""
import copy
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

from mmdeer import _lib

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CANARY32 = 0x7FA5A5A5          # a NaN no kernel produces (payload), as int32 / float32 bits
CANARY16 = 0x7FA5              # the same for bf16 storage
VP = C.c_void_p


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _lib_err():
    return _lib.load().mmdeer_last_error().decode()


def _canary32(n):
    return torch.full((n,), CANARY32, dtype=torch.int32, device=DEV).view(torch.float32)


def _canary16(n):
    return torch.full((n,), CANARY16, dtype=torch.int16, device=DEV).view(torch.bfloat16)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16)


def _untouched(buf, written):
    """Positions outside `written` (bool mask) still hold the canary."""
    c = CANARY32 if buf.dtype == torch.float32 else CANARY16
    bad = (_bits(buf) != c) & ~written
    return int(bad.sum())


def _all_canary(buf):
    return _untouched(buf, torch.zeros(buf.numel(), dtype=torch.bool, device=DEV)) == 0


def _randn(n, seed, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(n, generator=g, device=DEV) * scale


# ============================================================================================== A. mmdeer_gemm_batch
GM = (4, 12, 64, 132, 256, 520)                 # M (rows of dW = columns of dY): the transposed-A loader needs M % 4 == 0
GM_BF16 = (8, 64, 136, 256, 520)                # bf16 compute: dY in whole 16-byte chunks (M % 8 == 0, lda % 8 == 0)
GN = (4, 12, 84, 128, 256, 768)                 # N (columns of dW = columns of X): N % 4 == 0
GK = (1, 7, 64, 100, 515, 1024, 4096, 8192)     # K (batch rows): split and unsplit problems mix in one group
POOL = 8192 * 1040 + 4096                       # one operand pool: every A / W is a window of it (pad columns = other values)


@pytest.fixture(scope="module")
def pools():
    p32 = _randn(POOL, 1234)
    return p32, p32.to(torch.bfloat16)


def _draw_gemm(rng, n, f32):
    """n problems: (M, N, K, lda, ldw, ldc, a_off, w_off, a_f32, w_f32, bias)."""
    out = []
    for _ in range(n):
        M, N, K = int(rng.choice(GM if f32 else GM_BF16)), int(rng.choice(GN)), int(rng.choice(GK))
        lda = M + (4 if f32 else 8) * int(rng.integers(0, 3))
        ldw = N + 4 * int(rng.integers(0, 3))
        lda, ldw = (max(lda, 8) if lda * K < 8 else lda), (max(ldw, 8) if ldw * K < 8 else ldw)  # the 8-element operand minimum
        ldc = N if rng.random() < 0.75 else N + 4 * int(rng.integers(1, 4))
        a_off = 8 * int(rng.integers(0, (POOL - K * lda) // 8))
        w_off = 8 * int(rng.integers(0, (POOL - K * ldw) // 8))
        a32 = f32
        w32 = 1 if f32 else int(rng.random() < 0.3)
        out.append((M, N, K, lda, ldw, ldc, a_off, w_off, a32, w32, bool(rng.random() < 0.5)))
    return out


def _gemm_layout(rng, table):
    """Window offsets of every C (M rows of ldc) and bias_grad (M) in one output buffer, canary gaps between them."""
    cur, offs = 4 * int(rng.integers(1, 8)), []
    for (M, N, K, lda, ldw, ldc, *_r, bias) in table:
        c_off = cur
        cur += M * ldc + 4 * int(rng.integers(1, 8))
        b_off = None
        if bias:
            b_off = cur
            cur += M + 4 * int(rng.integers(1, 8))
        offs.append((c_off, b_off))
    return offs, cur + 64


def _gemm_args(table, offs, out, pools, f32):
    p32, pbf = pools
    args = []
    for (M, N, K, lda, ldw, ldc, a_off, w_off, a32, w32, bias), (c_off, b_off) in zip(table, offs):
        args.append(_lib.gemm_args(
            A=(p32 if a32 else pbf)[a_off:].data_ptr(), W=(p32 if w32 else pbf)[w_off:].data_ptr(), C=out[c_off:].data_ptr(),
            bias_grad=out[b_off:].data_ptr() if b_off is not None else None, M=M, N=N, K=K, lda=lda, ldw=ldw, ldc=ldc,
            a_f32=a32, w_f32=w32, c_f32=1, trans_a=1, trans_w=1, compute_f32=f32))
    return args


def _gemm_call(args, slab, slab_elems):
    n = len(args)
    arr = (_lib.GemmArgs * max(n, 1))(*args)
    rc = _lib.load().mmdeer_gemm_batch(arr, n, None if slab is None else slab.data_ptr(), slab_elems, _stream())
    torch.cuda.synchronize()
    return rc


def _slab_elems(args):
    n = len(args)
    return int(_lib.load().mmdeer_gemm_batch_slab_elems((_lib.GemmArgs * max(n, 1))(*args), n))


def _gemm_written(table, offs, size):
    w = torch.zeros(size, dtype=torch.bool, device=DEV)
    for (M, N, K, lda, ldw, ldc, *_r), (c_off, b_off) in zip(table, offs):
        w[c_off:c_off + M * ldc].view(M, ldc)[:, :N] = True
        if b_off is not None:
            w[b_off:b_off + M] = True
    return w


def _gemm_check(table, offs, out, pools, f32, msg):
    p32, pbf = pools
    tol = 1e-4 if f32 else 2e-2
    for i, ((M, N, K, lda, ldw, ldc, a_off, w_off, a32, w32, bias), (c_off, b_off)) in enumerate(zip(table, offs)):
        A = p32[a_off:a_off + K * lda].view(K, lda)[:, :M]
        W = p32[w_off:w_off + K * ldw].view(K, ldw)[:, :N]
        if not f32:         # bf16 compute: the operands as the kernel sees them (fp32 ones are converted by the loader)
            A = A.to(torch.bfloat16) if a32 else pbf[a_off:a_off + K * lda].view(K, lda)[:, :M]
            W = W.to(torch.bfloat16) if w32 else pbf[w_off:w_off + K * ldw].view(K, ldw)[:, :N]
        A, W = A.double(), W.double()
        bound = tol * max(1.0, math.sqrt(K) / 4)
        got = out[c_off:c_off + M * ldc].view(M, ldc)[:, :N]
        assert bool(torch.isfinite(got).all()), f"{msg} problem {i} {table[i]}: non-finite dW"
        err = float((got.double() - A.t() @ W).abs().max())
        assert err < bound, f"{msg} problem {i} {table[i]}: |dW - ref| = {err:.3g} >= {bound:.3g}"
        if b_off is not None:
            gb = out[b_off:b_off + M]
            err = float((gb.double() - A.sum(0)).abs().max())
            assert bool(torch.isfinite(gb).all()) and err < bound, f"{msg} problem {i} {table[i]}: |db - ref| = {err:.3g}"


@pytest.mark.parametrize("plan", ["default", "dw_tile3_ksteps4"])
@pytest.mark.parametrize("f32", [1, 0])
def test_gemm_batch_random_tables(pools, f32, plan):
    """1-40 weight-gradient problems per call (groups of 16), split and unsplit, ragged K, padded lda / ldw with other data in the
    pad columns, ldc > N, with and without bias_grad, fp32 X (W) under bf16 compute: against float64 dY^T X and the column sums
    of dY; a slab of exactly mmdeer_gemm_batch_slab_elems (NaN-filled, with a canary after it); bitwise equal on a second run; a
    slab one float short is refused with nothing written.  plan dw_tile3_ksteps4: the fixed-slice branch of the split policy."""
    opts = dict(dw_tile=3, ksteps=4) if plan != "default" else {}
    with _lib.options(**opts):
        for seed in range(4):
            rng = np.random.default_rng(1000 * f32 + 10 * seed + (plan != "default"))
            n = int(rng.integers(1, 41)) if seed else 40
            table = _draw_gemm(rng, n, f32)
            offs, size = _gemm_layout(rng, table)
            msg = f"seed={seed} f32={f32} plan={plan} n={n} table(M,N,K,lda,ldw,ldc,a_off,w_off,a32,w32,bias)={table}"
            written = _gemm_written(table, offs, size)
            out = _canary32(size)
            args = _gemm_args(table, offs, out, pools, f32)
            need = _slab_elems(args)
            slab = _canary32(need + 64)
            slab[:need] = float("nan")
            rc = _gemm_call(args, slab, need)
            assert rc == 0, f"{msg}: {_lib_err()}"
            assert _untouched(out, written) == 0, f"{msg}: a canary of the output buffer was overwritten"
            assert _all_canary(slab[need:]), f"{msg}: written past the end of the slab ({need} floats)"
            _gemm_check(table, offs, out, pools, f32, msg)
            out2 = _canary32(size)
            assert _gemm_call(_gemm_args(table, offs, out2, pools, f32), slab, need) == 0, f"{msg}: {_lib_err()}"
            assert torch.equal(_bits(out), _bits(out2)), f"{msg}: two runs differ"
            if need > 0:
                out3 = _canary32(size)
                rc = _gemm_call(_gemm_args(table, offs, out3, pools, f32), slab, need - 1)
                assert rc == -1, f"{msg}: a slab one float short was accepted"
                assert "slab too small" in _lib_err(), f"{msg}: {_lib_err()}"
                assert _all_canary(out3), f"{msg}: the refused call (slab short) wrote outputs"


@pytest.mark.parametrize("f32", [1, 0])
def test_gemm_batch_ldc_wider_than_n_at_every_k(pools, f32):
    """A C with ldc > N is accepted at every K -- whether the library splits the reduction must not decide whether the call is
    refused -- and the pad columns between the rows keep their canaries."""
    for K in (64, 1024, 8192):
        table = [(256, 128, K, 256, 128, 132, 0, 8 * 4096, f32, f32, True), (64, 84, K, 64, 88, 96, 8 * 9000, 8 * 20000, f32, f32, True)]
        offs, size = _gemm_layout(np.random.default_rng(K), table)
        out = _canary32(size)
        args = _gemm_args(table, offs, out, pools, f32)
        need = _slab_elems(args)
        slab = torch.full((need + 4,), float("nan"), device=DEV)
        msg = f"K={K} f32={f32} table={table}"
        assert _gemm_call(args, slab, need) == 0, f"{msg}: {_lib_err()}"
        assert _untouched(out, _gemm_written(table, offs, size)) == 0, f"{msg}: a canary was overwritten"
        _gemm_check(table, offs, out, pools, f32, msg)


def test_gemm_batch_empty_call(pools):
    out = _canary32(64)
    assert _slab_elems([]) == 0
    assert _gemm_call([], None, 0) == 0, _lib_err()
    assert _all_canary(out)


def _refusal_table(pools, f32=0):
    rng = np.random.default_rng(77)
    table = [(int(rng.choice((64, 256))), int(rng.choice((84, 128, 256))), int(rng.choice((1024, 4096, 8192))), 0, 0, 0, 0, 0, 0, 0, True)
             for _ in range(24)]
    table = [(M, N, K, M, N, N, 8 * int(rng.integers(0, (POOL - K * M) // 8)), 8 * int(rng.integers(0, (POOL - K * N) // 8)), f32, f32, b)
             for (M, N, K, *_r, b) in table]
    offs, size = _gemm_layout(rng, table)
    return table, offs, size


BAD_GEMM = {
    "relu": lambda a, keep: setattr(a, "relu", 1),
    "bias": lambda a, keep: setattr(a, "bias", keep.data_ptr()),
    "accumulate": lambda a, keep: setattr(a, "accumulate", 1),
    "compute_dtype": lambda a, keep: setattr(a, "compute_f32", 1 - a.compute_f32),
    "A_null": lambda a, keep: setattr(a, "A", None),
    "W_null": lambda a, keep: setattr(a, "W", None),
    "C_null": lambda a, keep: setattr(a, "C", None),
    "M3": lambda a, keep: (setattr(a, "M", 3), setattr(a, "lda", 4)),
    "M130": lambda a, keep: setattr(a, "M", 130),
    "N3": lambda a, keep: setattr(a, "N", 3),
    "A_fp32_under_bf16": lambda a, keep: setattr(a, "a_f32", 1),
    "M12_under_bf16": lambda a, keep: (setattr(a, "M", 12), setattr(a, "K", 100)),   # K % 32: its group is not on the DMA kernels
}


@pytest.mark.parametrize("bad", sorted(BAD_GEMM))
def test_gemm_batch_refuses_problem_20_and_writes_nothing(pools, bad):
    """Problem 20 of 24 (in the second group) carries an epilogue flag, the other compute dtype, a NULL operand or a shape the
    weight-gradient loader does not take (M or N not a multiple of 4; under bf16 compute an fp32 dY, or M % 8 off the DMA kernels):
    -1, the message names gemm_batch[20], and no output of any problem -- those of the first group included -- was written."""
    table, offs, size = _refusal_table(pools)
    out = _canary32(size)
    keep = torch.zeros(1024, device=DEV)
    args = _gemm_args(table, offs, out, pools, 0)
    need = _slab_elems(args) + (1 << 16)         # plenty: the refusal must come from problem 20
    BAD_GEMM[bad](args[20], keep)
    slab = torch.full((need,), float("nan"), device=DEV)
    rc = _gemm_call(args, slab, need)
    assert rc == -1, f"{bad}: accepted"
    assert "gemm_batch[20]" in _lib_err(), f"{bad}: {_lib_err()}"
    assert _all_canary(out), f"{bad}: the refused call wrote outputs ({size - int((_bits(out) == CANARY32).sum())} floats)"


# ============================================================================================== B. mmdeer_reduce_batch
RCOUNT = (0, 4, 252, 256, 260, 4100)
RPOOL = 1 << 21


def _reduce_call(src, dst, nparts, count, stride):
    n = len(src)
    rc = _lib.load().mmdeer_reduce_batch(n, (VP * n)(*src), (VP * n)(*dst), (C.c_int32 * n)(*nparts), (C.c_int32 * n)(*count),
                                         (C.c_longlong * n)(*stride), _stream())
    torch.cuda.synchronize()
    return rc


def _draw_reduce(rng, n, counts=RCOUNT):
    segs, cur = [], 4 * int(rng.integers(1, 8))
    for _ in range(n):
        cnt, np_ = int(rng.choice(counts)), int(rng.integers(1, 41))
        st = cnt + 4 * int(rng.integers(0, 5))
        s_off = 4 * int(rng.integers(0, (RPOOL - (np_ - 1) * st - cnt) // 4 + 1))
        segs.append((s_off, cur, np_, cnt, st))
        cur += cnt + 4 * int(rng.integers(1, 8))
    return segs, cur + 64


def _reduce_run(pool, segs, size):
    out = _canary32(size)
    rc = _reduce_call([pool[s:].data_ptr() for s, *_r in segs], [out[d:].data_ptr() for _, d, *_r in segs],
                      [p for *_r, p, _c, _s in segs], [c for *_r, c, _s in segs], [s for *_r, s in segs])
    return rc, out


def test_reduce_batch_random_tables():
    """1-120 segments per call (launches of 48), 1-40 parts (the 16-wide loop and its remainder), counts 0 / 4 / 252 / 256 / 260 / 4100,
    stride >= count: the float64 sum within nparts * 2^-23 * sum |x|, an exact copy for one part, bitwise equal on a second run,
    nothing written outside [dst, dst + count)."""
    pool = _randn(RPOOL, 55)
    ar = torch.arange(4100, device=DEV)
    for seed in range(6):
        rng = np.random.default_rng(200 + seed)
        n = int(rng.integers(1, 121)) if seed else 120
        segs, size = _draw_reduce(rng, n)
        msg = f"seed={seed} n={n} segments(src_off,dst_off,nparts,count,stride)={segs}"
        rc, out = _reduce_run(pool, segs, size)
        assert rc == 0, f"{msg}: {_lib_err()}"
        written = torch.zeros(size, dtype=torch.bool, device=DEV)
        for i, (s, d, np_, cnt, st) in enumerate(segs):
            written[d:d + cnt] = True
            if cnt == 0:
                continue
            x = pool[s + (torch.arange(np_, device=DEV)[:, None] * st + ar[None, :cnt])].double()
            got = out[d:d + cnt]
            if np_ == 1:
                assert torch.equal(_bits(got), _bits(pool[s:s + cnt])), f"{msg} segment {i}: nparts = 1 is not a copy"
                continue
            err = (got.double() - x.sum(0)).abs()
            bound = np_ * 2.0 ** -23 * x.abs().sum(0)
            assert bool((err <= bound).all()), f"{msg} segment {i}: error {float((err - bound).max()):.3g} over the bound"
        assert _untouched(out, written) == 0, f"{msg}: a canary was overwritten"
        rc, out2 = _reduce_run(pool, segs, size)
        assert rc == 0 and torch.equal(_bits(out), _bits(out2)), f"{msg}: two runs differ"


BAD_REDUCE = {
    "src_misaligned": lambda t: t.__setitem__(0, t[0] + 1),
    "dst_misaligned": lambda t: t.__setitem__(1, t[1] + 1),
    "count_not_4": lambda t: (t.__setitem__(3, 6), t.__setitem__(4, 8)),
    "stride_not_4": lambda t: (t.__setitem__(3, 4), t.__setitem__(4, 6)),
    "nparts_0": lambda t: t.__setitem__(2, 0),
}


@pytest.mark.parametrize("bad", sorted(BAD_REDUCE))
def test_reduce_batch_refuses_segment_50_and_writes_nothing(bad):
    """Segment 50 of 60 (second launch) misaligned, count or stride not a multiple of 4, or no parts: -1, reduce_batch[50] named,
    every dst untouched."""
    pool = _randn(RPOOL, 56)
    rng = np.random.default_rng(300)
    segs, size = _draw_reduce(rng, 60, counts=(4, 252, 256, 260))
    out = _canary32(size + 64)
    rows = [[s, d, np_, c, st] for s, d, np_, c, st in segs]
    BAD_REDUCE[bad](rows[50])
    rc = _reduce_call([pool[r[0]:].data_ptr() for r in rows], [out[r[1]:].data_ptr() for r in rows], [r[2] for r in rows],
                      [r[3] for r in rows], [r[4] for r in rows])
    assert rc == -1, f"{bad}: accepted"
    assert "reduce_batch[50]" in _lib_err(), f"{bad}: {_lib_err()}"
    assert _all_canary(out), f"{bad}: the refused call wrote outputs"


# ============================================================================================== C. mmdeer_pack_transposed_batch
PDIM = (1, 3, 31, 32, 33, 84, 256, 300)
SPECIAL = (0.0, -0.0, 1e-40, -3e-39, 1.17e-38, float("inf"), float("-inf"), float("nan"), 3.3895e38, -1.0000001)


def _draw_packt(rng, n):
    mats, cur = [], 4 * int(rng.integers(0, 8)) + int(rng.integers(0, 4))
    src_cur = 0
    for _ in range(n):
        r, c = int(rng.choice(PDIM)), int(rng.choice(PDIM))
        if rng.random() < 0.5:
            ld, col = 0, (int(rng.integers(0, 9)) if rng.random() < 0.3 else 0)
            ldd = r
        else:
            col = int(rng.integers(0, 40))
            ld = r + col + int(rng.integers(0, 12))
            ldd = ld
        src_off = src_cur + int(rng.integers(0, 5))
        src_cur = src_off + r * c
        mats.append((src_off, r, c, cur, ld, col))
        cur += col + (c - 1) * ldd + r + int(rng.integers(1, 40))
    return mats, src_cur + 8, cur + 64


def _packt_src(n, seed):
    x = _randn(n, seed)
    rng = np.random.default_rng(seed)
    idx = torch.from_numpy(rng.integers(0, n, size=max(1, n // 50))).to(DEV)
    x[idx] = torch.tensor(SPECIAL, device=DEV)[torch.from_numpy(rng.integers(0, len(SPECIAL), size=idx.numel())).to(DEV)]
    return x


def _packt_call(src, mats, dst, f32):
    n = len(mats)
    rc = _lib.load().mmdeer_pack_transposed_batch(
        n, (VP * n)(*[src[m[0]:].data_ptr() if m[0] is not None else None for m in mats]), (C.c_int32 * n)(*[m[1] for m in mats]),
        (C.c_int32 * n)(*[m[2] for m in mats]), dst.data_ptr(), (C.c_longlong * n)(*[m[3] for m in mats]),
        (C.c_int32 * n)(*[m[4] for m in mats]), (C.c_int32 * n)(*[m[5] for m in mats]), f32, _stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("f32", [1, 0])
def test_pack_transposed_batch_random_tables(f32):
    """1-80 matrices per call (launches of 32), rows / cols in {1, 3, 31, 32, 33, 84, 256, 300}, ld_dst 0 or wider than rows, column
    offsets; inputs with +-0, denormals, +-Inf, NaN: fp32 equals src^T bit for bit, bf16 equals src^T.to(bfloat16) bit for bit (NaN
    stays NaN); everything outside each matrix's window keeps its canary."""
    for seed in range(5):
        rng = np.random.default_rng(400 + 10 * seed + f32)
        n = int(rng.integers(1, 81)) if seed else 80
        mats, nsrc, size = _draw_packt(rng, n)
        src = _packt_src(nsrc, 500 + seed)
        dst = _canary32(size) if f32 else _canary16(size)
        msg = f"seed={seed} f32={f32} n={n} mats(src_off,rows,cols,dst_off,ld_dst,dst_col)={mats}"
        assert _packt_call(src, mats, dst, f32) == 0, f"{msg}: {_lib_err()}"
        written = torch.zeros(size, dtype=torch.bool, device=DEV)
        for i, (so, r, c, off, ld, col) in enumerate(mats):
            ldd = ld or r
            idx = off + col + torch.arange(c, device=DEV)[:, None] * ldd + torch.arange(r, device=DEV)[None, :]
            written[idx] = True
            ref = src[so:so + r * c].view(r, c).t()
            got = dst[idx]
            if not f32:
                ref = ref.to(torch.bfloat16)
            nan = torch.isnan(ref.float())
            assert torch.equal(torch.isnan(got.float()), nan), f"{msg} matrix {i}: NaN positions differ"
            same = (_bits(got.contiguous()) == _bits(ref.contiguous())) | nan
            assert bool(same.all()), f"{msg} matrix {i}: {int((~same).sum())} elements differ from src^T"
        assert _untouched(dst, written) == 0, f"{msg}: a canary was overwritten"


BAD_PACKT = {
    "src_null": lambda m: m.__setitem__(0, None),
    "rows_0": lambda m: m.__setitem__(1, 0),
    "cols_0": lambda m: m.__setitem__(2, 0),
    "dst_off_negative": lambda m: m.__setitem__(3, -1),
    "ld_dst_short": lambda m: (m.__setitem__(4, m[1] + 4), m.__setitem__(5, 8)),
    "dst_col_negative": lambda m: m.__setitem__(5, -1),
}


@pytest.mark.parametrize("bad", sorted(BAD_PACKT))
def test_pack_transposed_batch_refuses_matrix_40_and_writes_nothing(bad):
    """Matrix 40 of 50 (second launch) with no source, an empty shape, a negative offset or column, or rows that do not fit in
    ld_dst: -1, pack_transposed_batch[40] named, nothing written."""
    rng = np.random.default_rng(600)
    mats, nsrc, size = _draw_packt(rng, 50)
    mats = [list(m) for m in mats]
    mats[40] = [0, 32, 32, mats[40][3] + 64, 0, 0]       # room before it for the negative column
    src = _packt_src(max(nsrc, 4096), 601)
    BAD_PACKT[bad](mats[40])
    dst = _canary16(size + 4096)
    rc = _packt_call(src, mats, dst, 0)
    assert rc == -1, f"{bad}: accepted"
    assert "pack_transposed_batch[40]" in _lib_err(), f"{bad}: {_lib_err()}"
    assert _all_canary(dst), f"{bad}: the refused call wrote outputs"


# ============================================================================================== D. mmdeer_adamw_flat / FlatAdamW
def _adamw_call(p, g, m, v, packed, packed_f32, segs, step, gs, max_norm, wd=1e-2, scratch=None, norm=None, flat=None):
    a = _lib.AdamWFlatArgs()
    a.params, a.grads, a.exp_avg, a.exp_avg_sq = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr()
    a.packed, a.packed_f32 = (None if packed is None else packed.data_ptr()), packed_f32
    a.flat_elems = flat if flat is not None else p.numel()
    n = len(segs)
    keep = ((C.c_longlong * n)(*[s[0] for s in segs]), (C.c_longlong * n)(*[s[1] for s in segs]), (C.c_float * n)(*[s[2] for s in segs]))
    a.nseg = n
    a.seg_begin, a.seg_elems, a.seg_lr = keep
    scratch = torch.empty(256, device=DEV) if scratch is None else scratch
    norm = torch.full((), float("nan"), device=DEV) if norm is None else norm
    a.scratch, a.grad_norm, a.step = scratch.data_ptr(), norm.data_ptr(), step
    a.beta1, a.beta2, a.eps, a.weight_decay, a.max_grad_norm, a.grad_scale = 0.9, 0.999, 1e-8, wd, max_norm, gs
    a.stream = _stream()
    rc = _lib.load().mmdeer_adamw_flat(C.byref(a))
    torch.cuda.synchronize()
    return rc, norm


def _adamw_problem(seed, segs, flat, step):
    """Flat params / grads / moments: gradients non-zero everywhere (outside the segments too, and large there), moments holding
    a canary outside the segments (never read)."""
    p = _randn(flat, seed)
    g = _randn(flat, seed + 1, 0.1)
    inside = torch.zeros(flat, dtype=torch.bool, device=DEV)
    for b, n, _lr in segs:
        inside[b:b + n] = True
    g[~inside] = _randn(flat, seed + 2, 10.0)[~inside]
    m, v = _canary32(flat), _canary32(flat)
    if step == 1:
        m[inside], v[inside] = 0.0, 0.0
    else:
        m[inside] = _randn(flat, seed + 3, 0.01)[inside]
        v[inside] = (_randn(flat, seed + 4, 1e-2) ** 2)[inside]
    return p, g, m, v, inside


def _adamw_reference(p, g, m, v, segs, step, gs, max_norm, wd=1e-2):
    """torch: grads times grad_scale, clip_grad_norm_ over the segments, torch.optim.AdamW (one group per segment)."""
    ps = [torch.nn.Parameter(p[b:b + n].clone()) for b, n, _ in segs]
    for t, (b, n, _) in zip(ps, segs):
        t.grad = g[b:b + n].clone() * gs
    if max_norm > 0:
        norm = torch.nn.utils.clip_grad_norm_(ps, max_norm)
    else:
        norm = torch.linalg.vector_norm(torch.cat([t.grad for t in ps]))
    opt = torch.optim.AdamW([{"params": [t], "lr": lr} for t, (_, _, lr) in zip(ps, segs)], betas=(0.9, 0.999), eps=1e-8,
                            weight_decay=wd, foreach=False)
    for t, (b, n, _) in zip(ps, segs):
        opt.state[t] = {"step": torch.tensor(float(step - 1)), "exp_avg": m[b:b + n].clone(), "exp_avg_sq": v[b:b + n].clone()}
    opt.step()
    return [t.detach() for t in ps], [(opt.state[t]["exp_avg"], opt.state[t]["exp_avg_sq"]) for t in ps], float(norm)


ADAM_SEGS = [(8, 4, 1e-3), (64, 260, 5e-4), (332, 12, 1e-3), (1024, 1024, 2e-3), (2304, 1000, 5e-4), (4096, 2048, 1e-3)]


@pytest.mark.parametrize("packed", ["none", "f32", "bf16"])
@pytest.mark.parametrize("step,gs", [(1, 1.0), (3, 0.75)])
@pytest.mark.parametrize("clip", [0, 1])
def test_adamw_flat_against_torch(packed, step, gs, clip):
    """Six segments with gaps between them, three learning rates, steps 1 and 3 (bias correction), grad_scale, clipping off and
    active, no / fp32 / bf16 packed copy: against clip_grad_norm_ + torch.optim.AdamW on the segments' values (rtol 2e-6, atol
    2e-7); grad_norm within 1e-5 of torch's; the bf16 copy is the updated parameters rounded.  Large gradients outside every
    segment change nothing: not the update, not grad_norm; parameters, moments and the packed copy keep their values there."""
    flat, segs = 6400, ADAM_SEGS
    p, g, m, v, inside = _adamw_problem(10 * step + clip, segs, flat, step)
    ref_p, ref_mv, ref_norm = _adamw_reference(p, g, m, v, segs, step, gs, 0.0)
    max_norm = 0.5 * ref_norm if clip else 0.0
    if clip:
        ref_p, ref_mv, ref_norm2 = _adamw_reference(p, g, m, v, segs, step, gs, max_norm)
        assert ref_norm2 == pytest.approx(ref_norm, rel=1e-6)
    p0 = p.clone()
    pk = None if packed == "none" else (_canary32(flat) if packed == "f32" else _canary16(flat))
    rc, norm = _adamw_call(p, g, m, v, pk, int(packed != "bf16"), segs, step, gs, max_norm)
    msg = f"packed={packed} step={step} grad_scale={gs} max_norm={max_norm:.4g} segments={segs}"
    assert rc == 0, f"{msg}: {_lib_err()}"
    assert float(norm) == pytest.approx(ref_norm, rel=1e-5), f"{msg}: grad_norm {float(norm)} vs torch {ref_norm}"
    for (b, n, _), rp, (rm, rv) in zip(segs, ref_p, ref_mv):
        assert torch.allclose(p[b:b + n], rp, rtol=2e-6, atol=2e-7), f"{msg} segment {b}: {float((p[b:b + n] - rp).abs().max())}"
        # the kernel forms 1 - beta2 in fp32 (1.3e-5 relative from torch's double 1 - 0.999): the moments agree to 5e-5
        assert torch.allclose(m[b:b + n], rm, rtol=5e-5, atol=1e-8), f"{msg} segment {b}: exp_avg"
        assert torch.allclose(v[b:b + n], rv, rtol=5e-5, atol=1e-11), f"{msg} segment {b}: exp_avg_sq"
    assert torch.equal(p[~inside], p0[~inside]), f"{msg}: parameters outside the segments changed"
    assert _untouched(m, inside) == 0 and _untouched(v, inside) == 0, f"{msg}: moments outside the segments written"
    if pk is not None:
        assert _untouched(pk, inside) == 0, f"{msg}: packed copy written outside the segments"
        want = p[inside] if packed == "f32" else p[inside].to(torch.bfloat16)
        assert torch.equal(_bits(pk[inside]), _bits(want)), f"{msg}: packed copy != updated parameters"


def test_adamw_flat_segment_limits():
    """56 segments work, 57 are refused; a segment whose length or offset is not a multiple of 4 is refused with its number, and a
    refused call changes nothing."""
    flat = 64 * 60
    segs = [(64 * i + 4 * (i % 3), 4 * (1 + i % 5), (1e-3, 5e-4)[i % 2]) for i in range(57)]
    p, g, m, v, inside = _adamw_problem(7, segs[:56], flat, 3)
    ref_p, _, ref_norm = _adamw_reference(p, g, m, v, segs[:56], 3, 1.0, 1.0)
    rc, norm = _adamw_call(p, g, m, v, None, 1, segs[:56], 3, 1.0, 1.0)
    assert rc == 0, _lib_err()
    assert float(norm) == pytest.approx(ref_norm, rel=1e-5)
    for (b, n, _), rp in zip(segs[:56], ref_p):
        assert torch.allclose(p[b:b + n], rp, rtol=2e-6, atol=2e-7), f"segment at {b}"
    for bad, want in ((segs, "1..56 segments"), (segs[:2] + [(200, 6, 1e-3)] + segs[3:10], "segment 2"),
                      (segs[:2] + [(202, 8, 1e-3)] + segs[3:10], "segment 2")):
        p1, m1, v1 = p.clone(), m.clone(), v.clone()
        rc, _ = _adamw_call(p, g, m, v, None, 1, bad, 4, 1.0, 1.0)
        assert rc == -1, f"accepted: {bad}"
        assert want in _lib_err(), _lib_err()
        assert torch.equal(p, p1) and torch.equal(_bits(m), _bits(m1)) and torch.equal(_bits(v), _bits(v1)), "a refused call wrote"


def test_flat_adamw_on_a_parameter_subset_matches_torch():
    """FlatAdamW(model, params=<the non-encoder parameters of Stack B>, max_grad_norm=1.0) after one fused training step: equal to
    clip_grad_norm_ + torch.optim.AdamW over that subset alone (the frozen encoders' gradients are in the flat buffer and must not
    enter the norm), and the parameters outside the subset are untouched."""
    from mmdeer import stackb, synth
    from mmdeer.optim import FlatAdamW
    with open(os.path.join(os.path.dirname(__file__), "golden", "stackb_state_dict_names.json")) as fh:
        shapes = json.load(fh)
    m2 = stackb.CompleteDEERModel(stackb.ModelConfig(), compute_dtype="fp32")
    m2.load_state_dict({k: torch.from_numpy(v) for k, v in synth.module_fill("stackb", shapes).items()})
    m2 = m2.to(DEV).train()
    m1 = copy.deepcopy(m2)
    b = synth.make_batch(96, seed=34)
    xs = [torch.from_numpy(b[k]).to(DEV) for k in ("audio", "video", "text")]
    m2._train_step = 17
    m2.train_step_fused(*xs, torch.from_numpy(b["targets"]).to(DEV))
    torch.cuda.synchronize()
    g2 = {n: p.grad for n, p in m2.named_parameters()}
    enc = [n for n, _ in m2.named_parameters() if "encoder" in n]
    assert enc and max(float(g2[n].abs().max()) for n in enc) > 0, "the excluded encoders must carry gradients for this test"
    subset = [n for n, _ in m2.named_parameters() if "encoder" not in n and not n.startswith("calibration_layer.")]
    P1, P2 = dict(m1.named_parameters()), dict(m2.named_parameters())
    for n in subset:
        P1[n].grad = g2[n].clone()
    ref_norm = float(torch.nn.utils.clip_grad_norm_([P1[n] for n in subset], 1.0))
    torch.optim.AdamW([P1[n] for n in subset], lr=1e-3, weight_decay=1e-2, eps=1e-8).step()
    before = {n: p.detach().clone() for n, p in m2.named_parameters()}
    opt = FlatAdamW(m2, params=[P2[n] for n in subset], lr=1e-3, weight_decay=1e-2, max_grad_norm=1.0)
    opt.step()
    torch.cuda.synchronize()
    assert float(opt.last_grad_norm) == pytest.approx(ref_norm, rel=1e-5), (float(opt.last_grad_norm), ref_norm)
    for n, p in m2.named_parameters():
        if n in subset:
            assert torch.allclose(p, P1[n], rtol=2e-6, atol=2e-7), (n, float((p - P1[n]).abs().max()))
        else:
            assert torch.equal(p, before[n]), n
