"""LayerNorm (csrc/rowops.hip, csrc/ln_rows.h), the trimodal attention (csrc/attention.hip), the side rows (csrc/side.hip),
mmdeer_convert and the dropout draw as OPERATORS, at their edges, against the float64 restatements of tests/rowkernel_ref.py.

Every kernel the LayerNorm entry points dispatch to runs: ln_fwd_kernel / ln_bwd_kernel in their EXACT (N = 256, 512) and generic
(any N % 4 == 0 up to 1024) forms in both dtypes, ln_fwd_rows2_kernel / ln_bwd_rows16_kernel (bf16, N = 256, 512) with every count of
clamped rows; out32 NULL and given, the three classes of mask_scale, the partials-only call, M = 0.  The attention and the side rows run at
batch sizes around their four-samples-per-block geometry, padded leading dimensions, saturated / degenerate inputs, and the LSTM cell's
second grid-stride trip.  mmdeer_dropout_mask must equal the uint32 restatement bit for bit: that anchors every other dropout test,
which takes its truth from mmdeer_dropout_mask.

Tolerance (tests/rowkernel_ref.py): fp32 outputs |got - ref| <= K 2^-24 scale; bf16-stored outputs the same bound and one rounding to
bf16.  K = twice the float32 CPU evaluation's worst ratio (rounded up) per output family (tests/test_cpu_rowkernel_ref.py measures and asserts
it; DESIGN.md section 15 has the table and the worst ratios an MI355X showed; every test prints its own: pytest -s).  Every output
buffer has a sentinel-filled tail -- one extra row, and the padding columns where ld > width -- which must keep its bits; inputs carry
a NaN tail row and NaN padding columns, so a read outside the operand shows in the result.  No call here passes arguments that a host
check refuses (those are asserted without a GPU in tests/test_cpu_host.py).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mmdeer import _lib  # noqa: E402

from . import rowkernel_ref as R  # noqa: E402

DEV = "cuda:0"
K = R.K
WORST = {}
_INT = {torch.float32: (torch.int32, 0x7FA5A5A5), torch.bfloat16: (torch.int16, 0x7FA5), torch.uint8: (torch.uint8, 0xA5)}


def _note(family, log):
    for _, r in log:
        WORST[family] = max(WORST.get(family, 0.0), r)


def _report(*families):
    print("   worst ratio so far: " + "  ".join(f"{f} {WORST.get(f, 0.0):.2f} (K {K[f]:g})" for f in families))


def stream():
    return _lib.current_stream()


def dt(bf):
    return torch.bfloat16 if bf else torch.float32


class Out:
    """an output buffer of `rows` x `width` elements with leading dimension ld, one extra row, everything filled with a sentinel."""

    def __init__(self, rows, width, dtype, ld=None):
        self.rows, self.width, self.ld = rows, width, ld or width
        it, self.sent = _INT[dtype]
        self.t = torch.full((rows + 1, self.ld), self.sent, dtype=it, device=DEV).view(dtype)
        self.it = it

    @property
    def ptr(self):
        return self.t.data_ptr()

    def live(self):
        return self.t[:self.rows, :self.width].cpu()

    def assert_tail_intact(self, name, written_rows=None):
        """the extra row and the padding columns (and, with written_rows, every row from there on) keep the sentinel's bits"""
        bits = self.t.view(self.it).cpu()
        r = self.rows if written_rows is None else written_rows
        assert bool((bits[r:] == self.sent).all()), f"{name}: wrote past row {r}"
        assert bool((bits[:r, self.width:] == self.sent).all()), f"{name}: wrote into the padding columns"

    def assert_written(self, name):
        bits = self.t.view(self.it)[:self.rows, :self.width]
        assert not bool((bits == self.sent).any().cpu()), f"{name}: elements left unwritten"


def inp(x, dtype, ld=None):
    """an operand on the device: rows x width in a NaN-filled (rows + 1) x ld buffer"""
    x = x.reshape(x.shape[0], -1) if x.dim() > 1 else x.reshape(-1, 1)
    t = torch.full((x.shape[0] + 1, ld or x.shape[1]), float("nan"), dtype=dtype, device=DEV)
    t[:x.shape[0], :x.shape[1]] = x.to(dtype).to(DEV)           # rounded on the host: the values are the reference's inputs, bit for bit
    return t


# =========================================================================== the dropout draw
DROP_SHAPES = [(1, 1), (37, 8), (300, 32), (1027, 512), (70000, 4)]
DROP_SEEDS = (0, 1234, 2 ** 40 + 7, 2 ** 64 - 1)
DROP_OFFSETS = (0, 5, 2 ** 33 + 1)
DROP_P = (0.0, 0.1, 0.3, 0.5, 0.9)


@pytest.mark.parametrize("rows,cols", DROP_SHAPES)
def test_dropout_mask_equals_the_uint32_restatement_bit_for_bit(rows, cols):
    lib = _lib.load()
    outs = []
    for site in range(1, 10):
        for seed in DROP_SEEDS:
            for offset in DROP_OFFSETS:
                for p in DROP_P:
                    o = Out(rows, cols, torch.uint8)
                    _lib.check(lib.mmdeer_dropout_mask(site, rows, cols, p, seed, offset, o.ptr, stream()))
                    outs.append(((site, seed, offset, p), o))
    torch.cuda.synchronize()
    rand, kept = {}, 0
    for (site, seed, offset, p), o in outs:
        key = (site, seed, offset)
        if key not in rand:
            rand = {key: R.drop_rand(site, rows, cols, seed, offset)}            # one draw per key, five thresholds
        want = rand[key] < np.uint64(R.drop_threshold(p)[0])
        got = o.live().numpy()
        assert np.array_equal(got, want.astype(np.uint8)), (site, seed, offset, p, int((got != want).sum()))
        o.assert_tail_intact(f"dropout_mask{(site, seed, offset, p)}")
        kept += int(want.sum())
    assert 0 < kept < len(outs) * rows * cols


# =========================================================================== LayerNorm
def _ln_fwd(lib, y, gamma, beta, M, N, bf, with_out32):
    out, mean, rstd = Out(M, N, dt(bf)), Out(M, 1, torch.float32), Out(M, 1, torch.float32)
    out32 = Out(M, N, torch.float32) if with_out32 else None
    _lib.check(lib.mmdeer_layernorm_fwd(y.data_ptr(), out.ptr, out32.ptr if out32 else None, mean.ptr, rstd.ptr, gamma.data_ptr(),
                                        beta.data_ptr(), M, N, 0 if bf else 1, stream()))
    return out, out32, mean, rstd


def _ln_bwd(lib, dout, y, mean, rstd, gamma, M, N, bf, mask_scale, fold):
    nparts = lib.mmdeer_layernorm_bwd_nparts(M)
    assert nparts == max(1, (M + 15) // 16)
    dz, part = Out(M, N, dt(bf)), Out(nparts * 2, N, torch.float32)
    dgam, dbet = (Out(1, N, torch.float32), Out(1, N, torch.float32)) if fold else (None, None)
    _lib.check(lib.mmdeer_layernorm_bwd(dout.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), dz.ptr,
                                        dgam.ptr if fold else None, dbet.ptr if fold else None, part.ptr, M, N, 0 if bf else 1,
                                        mask_scale, stream()))
    return dz, part, dgam, dbet


@pytest.mark.parametrize("N", R.LN_N)
@pytest.mark.parametrize("bf", [False, True], ids=["fp32", "bf16"])
def test_layernorm_operators_against_float64(bf, N):
    lib = _lib.load()
    for M in (R.LN_M_ALL if N in (256, 512) else R.LN_M_FEW):
        y, dout, gamma, beta = R.ln_inputs(M, N, bf)
        f = R.ln_fwd(y, gamma, beta)
        yd, dd = inp(y, dt(bf)), inp(dout, dt(bf))
        gd, bd = inp(gamma.reshape(1, N), torch.float32), inp(beta.reshape(1, N), torch.float32)
        tag = f"{'bf16' if bf else 'fp32'} M={M} N={N}"
        log = []
        for with_out32 in (False, True):
            out, out32, mean, rstd = _ln_fwd(lib, yd, gd, bd, M, N, bf, with_out32)
            torch.cuda.synchronize()
            R.assert_close(f"{tag} out", out.live(), f["out"], K["ln_fwd"], bf16=bf, log=log)
            R.assert_close(f"{tag} mean", mean.live(), f["mean"], K["ln_fwd"], log=log)
            R.assert_close(f"{tag} rstd", rstd.live(), f["rstd"], K["ln_fwd"], log=log)
            if with_out32:
                R.assert_close(f"{tag} out32", out32.live(), f["out"], K["ln_fwd"], log=log)
                assert torch.equal(out.live().view(torch.int16 if bf else torch.int32),
                                   out32.live().to(dt(bf)).view(torch.int16 if bf else torch.int32)), f"{tag}: out is not out32 stored"
            for o in (out, mean, rstd) + ((out32,) if with_out32 else ()):
                o.assert_tail_intact(tag)
        _note("ln_fwd", log)
        # backward from the reference's own statistics (float32 inputs of the operator): independent of the forward kernel
        mean32, rstd32 = f["mean"].v.float(), f["rstd"].v.float()
        md, rd = inp(mean32, torch.float32), inp(rstd32, torch.float32)
        b = R.ln_bwd(dout, y, mean32, rstd32, gamma, 0.0)
        nonpos = torch.tensor([R.ln_row_class(i, M, N) == 3 for i in range(M)])
        log = []
        for ms in R.LN_MASK_SCALES:
            want = R.ln_mask(b["_dy"], y, ms)
            for fold in (True, False):
                dz, part, dgam, dbet = _ln_bwd(lib, dd, yd, md, rd, gd, M, N, bf, ms, fold)
                torch.cuda.synchronize()
                name = f"{tag} mask_scale={ms:.3g} fold={fold}"
                R.assert_close(f"{name} dz", dz.live(), want, K["ln_bwd"], bf16=bf, log=log)
                if ms > 0 and bool(nonpos.any()):
                    assert bool((dz.live()[nonpos].float() == 0).all()), f"{name}: dz of an all-nonpositive row is not exactly 0"
                if fold:
                    R.assert_close(f"{name} dgamma", dgam.live(), b["dgamma"], K["ln_bwd"], log=log)
                    R.assert_close(f"{name} dbeta", dbet.live(), b["dbeta"], K["ln_bwd"], log=log)
                    dgam.assert_tail_intact(name)
                    dbet.assert_tail_intact(name)
                else:
                    R.assert_close(f"{name} slab", part.live(), b["slab"], K["ln_bwd"], log=log)
                dz.assert_tail_intact(name)
                part.assert_tail_intact(name)
        _note("ln_bwd", log)
    _report("ln_fwd", "ln_bwd")


@pytest.mark.parametrize("N", [256, 260])
@pytest.mark.parametrize("bf", [False, True], ids=["fp32", "bf16"])
def test_layernorm_of_no_rows(bf, N):
    """M = 0: the forward writes nothing; the backward leaves dgamma = dbeta = 0 (one all-zero slab) and writes no dz."""
    lib = _lib.load()
    y, dout, gamma, beta = R.ln_inputs(1, N, bf)
    yd, dd, gd, bd = inp(y, dt(bf)), inp(dout, dt(bf)), inp(gamma.reshape(1, N), torch.float32), inp(beta.reshape(1, N), torch.float32)
    out, out32, mean, rstd = _ln_fwd(lib, yd, gd, bd, 0, N, bf, True)
    torch.cuda.synchronize()
    for o in (out, out32, mean, rstd):
        o.assert_tail_intact("forward, M = 0", written_rows=0)
    for fold in (True, False):
        dz, part, dgam, dbet = _ln_bwd(lib, dd, yd, mean.t, rstd.t, gd, 0, N, bf, 1.0, fold)
        torch.cuda.synchronize()
        dz.assert_tail_intact("backward, M = 0", written_rows=0)
        part.assert_tail_intact("backward, M = 0")
        assert bool((part.live() == 0).all())
        if fold:
            assert bool((dgam.live() == 0).all()) and bool((dbet.live() == 0).all())
            dgam.assert_tail_intact("backward, M = 0")
            dbet.assert_tail_intact("backward, M = 0")


# =========================================================================== trimodal attention
@pytest.mark.parametrize("B", R.TRI_B)
@pytest.mark.parametrize("bf", [False, True], ids=["fp32", "bf16"])
def test_trimodal_attention_operators_against_float64(bf, B):
    lib = _lib.load()
    f32 = 0 if bf else 1
    for cls in R.TRI_CLASSES:
        qkv, dobar = R.tri_inputs(B, cls, bf)
        qd, dod = inp(qkv, dt(bf)), inp(dobar, dt(bf))
        for p in R.TRI_P:
            training = 1 if p > 0 else 0
            keep, av = R.tri_keep(B, p, R.TRI_SEED, R.TRI_OFFSET) if p > 0 else (None, None)
            f = R.tri_attn(qkv, keep, p, av)
            tag = f"{'bf16' if bf else 'fp32'} B={B} {cls} p={p}"
            log = []
            for weights in (True, False):
                obar, probs = Out(B, 512, dt(bf)), Out(B, 32, torch.float32)
                attn_w, av_w = (Out(B, 4, torch.float32), Out(B, 2, torch.float32)) if weights else (None, None)
                _lib.check(lib.mmdeer_trimodal_attn_fwd(qd.data_ptr(), obar.ptr, probs.ptr, attn_w.ptr if weights else None,
                                                        av_w.ptr if weights else None, B, f32, training, p, R.TRI_SEED, R.TRI_OFFSET, stream()))
                torch.cuda.synchronize()
                R.assert_close(f"{tag} obar", obar.live(), f["obar"], K["tri_fwd"], bf16=bf, log=log)
                R.assert_close(f"{tag} probs", probs.live(), f["probs"], K["tri_fwd"], log=log)
                pl = probs.live()
                if cls == "saturated":
                    assert bool(((pl == 0) | (pl == 1)).all()) and bool((pl.view(B, 8, 2, 2).sum(-1) == 1).all()), f"{tag}: probabilities not exactly 0 / 1"
                elif cls in ("identical_tokens", "zeros"):
                    assert bool((pl == 0.5).all()), f"{tag}: probabilities not exactly 0.5"
                if weights:
                    R.assert_close(f"{tag} attn_w", attn_w.live(), f["attn_w"], K["tri_fwd"], log=log)
                    R.assert_close(f"{tag} av_w", av_w.live(), f["av_w"], K["tri_fwd"], log=log)
                    attn_w.assert_tail_intact(tag)
                    av_w.assert_tail_intact(tag)
                obar.assert_tail_intact(tag)
                probs.assert_tail_intact(tag)
            _note("tri_fwd", log)
            # backward from the reference's probabilities as float32 (an input of the operator)
            p32 = f["probs"].v.float()
            want = R.tri_attn_bwd(qkv, dobar, p32, keep, p)
            dqkv, pd = Out(2 * B, 1536, dt(bf)), inp(p32.reshape(B, 32), torch.float32)
            _lib.check(lib.mmdeer_trimodal_attn_bwd(qd.data_ptr(), dod.data_ptr(), pd.data_ptr(), dqkv.ptr, B,
                                                    f32, training, p, R.TRI_SEED, R.TRI_OFFSET, stream()))
            torch.cuda.synchronize()
            log = []
            R.assert_close(f"{tag} dqkv", dqkv.live(), want, K["tri_bwd"], bf16=bf, log=log)
            dqkv.assert_tail_intact(tag)
            _note("tri_bwd", log)
    _report("tri_fwd", "tri_bwd")


def test_trimodal_attention_backward_restatement_is_autograd():
    """the float64 backward the kernel is compared with IS autograd of the float64 forward with the keep mask fixed (asserted here
    beside the kernel comparison; tests/test_cpu_rowkernel_ref.py asserts the same without a GPU)"""
    B, p = 5, 0.3
    qkv, dobar = (t.double() for t in R.tri_inputs(B, "normal", False))
    keep, av = R.tri_keep(B, p, R.TRI_SEED, R.TRI_OFFSET)
    x = qkv.clone().requires_grad_(True)
    f = R.tri_attn(x, keep, p, av)
    (f["obar"].v * dobar).sum().backward()
    mine = R.tri_attn_bwd(qkv, dobar, f["probs"].v.detach(), keep, p).v
    assert float((mine - x.grad).abs().max()) < 1e-12 * float(x.grad.abs().max())


# =========================================================================== CrossModalAttention core
@pytest.mark.parametrize("ld", R.CROSS_LD)
@pytest.mark.parametrize("bf", [False, True], ids=["fp32", "bf16"])
def test_cross_modal_attention_operators_against_float64(bf, ld):
    lib = _lib.load()
    f32 = 0 if bf else 1
    for B in R.CROSS_B:
        for cls in R.CROSS_CLASSES:
            a = R.cross_inputs(B, cls, bf)
            q, ka, va, kv, vv = (inp(t, dt(bf), ld) for t in a[:5])
            gl, g_a, g_v = (inp(t, torch.float32) for t in a[5:])
            f, b = R.cross_modal_attn(*a[:6]), R.cross_modal_attn_bwd(*a)
            tag = f"{'bf16' if bf else 'fp32'} ld={ld} B={B} {cls}"
            out_a, out_v = Out(B, 32, torch.float32), Out(B, 32, torch.float32)
            _lib.check(lib.mmdeer_cross_modal_attn_fwd(q.data_ptr(), ka.data_ptr(), va.data_ptr(), kv.data_ptr(), vv.data_ptr(), ld, gl.data_ptr(),
                                                       out_a.ptr, out_v.ptr, B, f32, stream()))
            d = {k: Out(B, 256, dt(bf), ld) for k in ("dq", "dka", "dva", "dkv", "dvv")}
            d["dgl"] = Out(B, 2, torch.float32)
            _lib.check(lib.mmdeer_cross_modal_attn_bwd(q.data_ptr(), ka.data_ptr(), va.data_ptr(), kv.data_ptr(), vv.data_ptr(), ld, gl.data_ptr(),
                                                       g_a.data_ptr(), g_v.data_ptr(), d["dq"].ptr, d["dka"].ptr, d["dva"].ptr, d["dkv"].ptr,
                                                       d["dvv"].ptr, d["dgl"].ptr, B, f32, stream()))
            torch.cuda.synchronize()
            log = []
            for k, o in (("out_a", out_a), ("out_v", out_v)):
                R.assert_close(f"{tag} {k}", o.live(), f[k], K["cross_fwd"], log=log)
                o.assert_tail_intact(tag)
                if cls == "equal_scores":          # p = 1/8 and gate = 1/2 exactly, v_h = unit vector h: 1/16 in the first 8 dims
                    assert bool((o.live()[:, :8] == 0.0625).all()) and bool((o.live()[:, 8:] == 0).all()), f"{tag}: p is not exactly 1/8"
            _note("cross_fwd", log)
            log = []
            for k, o in d.items():
                R.assert_close(f"{tag} {k}", o.live(), b[k], K["cross_bwd"], bf16=bf and k != "dgl", log=log)
                o.assert_tail_intact(tag)
            _note("cross_bwd", log)
    _report("cross_fwd", "cross_bwd")


# =========================================================================== LSTM cell
@pytest.mark.parametrize("B,H,nd,cls", R.lstm_cases())
@pytest.mark.parametrize("bf", [False, True], ids=["fp32", "bf16"])
def test_lstm_cell_operators_against_float64(bf, B, H, nd, cls):
    lib = _lib.load()
    f32 = 0 if bf else 1
    gates, dout = R.lstm_inputs(B, H, nd, cls, bf)
    ref_h, ref_d = R.lstm_cell_t1(gates, H, nd), R.lstm_cell_t1_bwd(gates, dout, H, nd)
    log = []
    for pad_g, pad_o in ((0, 0), (5, 3)):
        ld_g, ld_o = nd * 4 * H + pad_g, nd * H + pad_o
        gd, dd = inp(gates, dt(bf), ld_g), inp(dout, dt(bf), ld_o)
        h, dg = Out(B, nd * H, dt(bf), ld_o), Out(B, nd * 4 * H, dt(bf), ld_g)
        _lib.check(lib.mmdeer_lstm_cell_t1(gd.data_ptr(), ld_g, h.ptr, ld_o, B, H, nd, f32, stream()))
        _lib.check(lib.mmdeer_lstm_cell_t1_bwd(gd.data_ptr(), ld_g, dd.data_ptr(), ld_o, dg.ptr, B, H, nd, f32, stream()))
        torch.cuda.synchronize()
        tag = f"{'bf16' if bf else 'fp32'} B={B} H={H} ndir={nd} {cls} ld_gates={ld_g} ld_out={ld_o}"
        R.assert_close(f"{tag} h", h.live(), ref_h, K["lstm"], bf16=bf, log=log)
        R.assert_close(f"{tag} dgates", dg.live(), ref_d, K["lstm"], bf16=bf, log=log)
        fblock = dg.live().float().view(B, nd, 4, H)[:, :, 1]
        assert bool((fblock == 0).all()), f"{tag}: the forget block of dgates is not exactly 0"
        for o in (h, dg):
            o.assert_written(tag)
            o.assert_tail_intact(tag)
    _note("lstm", log)
    _report("lstm")


# =========================================================================== convert
@pytest.mark.parametrize("n", [0, 4, 1028, 2 ** 21 + 4])
@pytest.mark.parametrize("src_f32,dst_f32", [(1, 1), (1, 0), (0, 1), (0, 0)], ids=["f32-f32", "f32-bf16", "bf16-f32", "bf16-bf16"])
def test_convert_bit_for_bit(src_f32, dst_f32, n):
    lib = _lib.load()
    edge = R.convert_values()
    rng = np.random.default_rng(n + 2 * src_f32 + dst_f32)
    bits32 = np.concatenate([edge, rng.integers(0, 2 ** 32, max(n, 4), dtype=np.uint64).astype(np.uint32)])[:max(n, 4)]
    if src_f32:
        src = torch.from_numpy(bits32.view(np.int32).copy()).to(DEV)
        src_bits32 = bits32
    else:
        b16 = (bits32 >> 16).astype(np.uint16)                                   # every edge value's upper half: bf16 zeros, inf, NaN, denormals
        src = torch.from_numpy(b16.view(np.int16).copy()).to(DEV)
        src_bits32 = b16.astype(np.uint32) << 16
    dst = Out(1, n, torch.float32 if dst_f32 else torch.bfloat16, ld=n + 64)
    _lib.check(lib.mmdeer_convert(src.data_ptr(), src_f32, dst.ptr, dst_f32, n, stream()))
    torch.cuda.synchronize()
    dst.assert_tail_intact(f"convert n={n}")
    if n == 0:
        return
    got = dst.live().view(torch.int32 if dst_f32 else torch.int16).numpy().reshape(-1)
    got = got.view(np.uint32) if dst_f32 else got.view(np.uint16)
    sb = src_bits32[:n]
    nan = (sb & 0x7FFFFFFF) > 0x7F800000
    want = sb if dst_f32 else R.convert(sb)
    assert np.array_equal(got[~nan], want[~nan]), int((got[~nan] != want[~nan]).sum())
    if dst_f32:
        assert ((got[nan] & 0x7FFFFFFF) > 0x7F800000).all()                      # a NaN stays a NaN
    else:
        assert (((got[nan] & 0x7F80) == 0x7F80) & ((got[nan] & 0x007F) != 0)).all()
    assert nan.any() or n < 8
