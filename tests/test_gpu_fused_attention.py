"""tri_fused_kernel<0> / <1> (csrc/tri_fused.hip: the packed q|k|v projection, the 2x2 scores on the matrix pipe, softmax, attention
dropout, P V and the token mean in one launch; the backward recomputes the head tile) at its edges, through the C ABI
(mmdeer_pack_qkv_headmajor, mmdeer_trimodal_fused_fwd, mmdeer_trimodal_fused_bwd), against the staged float64 statement of
tests/rowkernel_ref.py.

The kernel rounds q and k to bf16 in front of the scores and nothing else, so every stage takes the kernel's own earlier output as an
exact input: qkv_out against sum_k x w + bias; probs against the clamped two-key softmax of the STORED q and k (a score is 64 exact
products, so the probabilities are pinned to K 2^-24 scale and not to half a bf16 ulp of every q and k); obar / attn_w / av_w against
those reference probabilities, the restated keep masks (tri_keep; never the library's mmdeer_dropout_mask) and v of the float64
projection with its scale; dqkv against the restated backward on the float64 projection with the kernel's saved probs.

Batches: 127 / 128 / 129 either side of one 128-sample row tile, 641 = 6 tiles, 1025 = 9 tiles with ONE sample in the last (72 workgroups,
9 per XCD: 127 of its 128 sample slots are redirected to the out-of-range offset), B = 0.  Classes, dropout settings and K: rowkernel_ref
(FUSED_*), DESIGN.md section 17.  Every output is allocated with a sentinel-filled extra sample behind it, which must keep its bits, and
is pre-filled with the same NaN pattern, so a dropped store shows as a non-finite value; x, dobar and probs carry NaN rows beyond the
batch.  No call here passes arguments that a host check refuses (tests/test_cpu_host.py asserts those without a GPU)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mmdeer import _lib  # noqa: E402

from . import rowkernel_ref as R  # noqa: E402

DEV = "cuda:0"
K = R.K
WORST, GAPS = {}, {}
_INT = {torch.float32: (torch.int32, 0x7FA5A5A5), torch.bfloat16: (torch.int16, 0x7FA5)}          # NaN patterns


def stream():
    return _lib.current_stream()


class Out:
    """an output of `rows` x `width` elements with `extra` more rows behind it (one sample), everything filled with a NaN sentinel."""

    def __init__(self, rows, width, dtype, extra):
        self.rows, self.dtype = rows, dtype
        self.it, self.sent = _INT[dtype]
        self.t = torch.full((rows + extra, width), self.sent, dtype=self.it, device=DEV).view(dtype)

    @property
    def ptr(self):
        return self.t.data_ptr()

    def live(self):
        return self.t[:self.rows].cpu()

    def bits(self):
        return self.t.view(self.it).cpu()

    def assert_tail_intact(self, name, written_rows=None):
        r = self.rows if written_rows is None else written_rows
        assert bool((self.bits()[r:] == self.sent).all()), f"{name}: wrote past row {r}"


def inp(x, dtype, extra):
    """an operand on the device with `extra` NaN rows behind it; the values are the reference's inputs bit for bit"""
    x = x.reshape(x.shape[0], -1)
    t = torch.full((x.shape[0] + extra, x.shape[1]), float("nan"), dtype=dtype, device=DEV)
    t[:x.shape[0]] = x.to(dtype).to(DEV)
    return t


_WHM = {}


def weight_image(lib):
    """the head-major image of the one weight matrix every case uses, packed once (and fenced)"""
    if "img" not in _WHM:
        w = R.fused_weights()[0].to(DEV)
        img = Out(1536, 512, torch.bfloat16, 1)
        _lib.check(lib.mmdeer_pack_qkv_headmajor(w.data_ptr(), img.ptr, stream()))
        torch.cuda.synchronize()
        img.assert_tail_intact("weight image")
        _WHM["img"] = img
    return _WHM["img"]


class Run:
    """the device operands of one (B, class) and the calls on them"""

    def __init__(self, lib, B, cls, dobar=None):
        self.lib, self.B = lib, B
        x, bias, dob = R.fused_inputs(B, cls)
        self.x = inp(x, torch.bfloat16, 2)                                          # NaN rows beyond 2B
        self.bias = bias.to(DEV)
        self.dobar = inp(dob if dobar is None else dobar, torch.bfloat16, 1)        # a NaN sample beyond B
        self.whm = weight_image(lib)

    def fwd(self, p, seed, offset, qkv=True, attn_w=True, av_w=True):
        B = self.B
        o = {"obar": Out(B, 512, torch.bfloat16, 1), "probs": Out(B, 32, torch.float32, 1)}     # probs: the NaN sample beyond B the backward sees
        if qkv:
            o["qkv"] = Out(2 * B, 1536, torch.bfloat16, 2)
        if attn_w:
            o["attn_w"] = Out(B, 4, torch.float32, 1)
        if av_w:
            o["av_w"] = Out(B, 2, torch.float32, 1)
        ptr = lambda k: o[k].ptr if k in o else None
        # eval: training = 0 with a dropout rate given -- the flag alone must switch the draw off
        _lib.check(self.lib.mmdeer_trimodal_fused_fwd(self.x.data_ptr(), self.whm.ptr, self.bias.data_ptr(), o["obar"].ptr, o["probs"].ptr,
                                                      ptr("qkv"), ptr("attn_w"), ptr("av_w"), B, 1 if p > 0 else 0, p if p > 0 else 0.3,
                                                      seed, offset, stream()))
        return o

    def bwd(self, probs, p, seed, offset):
        dqkv = Out(2 * self.B, 1536, torch.bfloat16, 2)
        _lib.check(self.lib.mmdeer_trimodal_fused_bwd(self.x.data_ptr(), self.whm.ptr, self.bias.data_ptr(), self.dobar.data_ptr(), probs.ptr,
                                                      dqkv.ptr, self.B, 1 if p > 0 else 0, p if p > 0 else 0.3, seed, offset, stream()))
        return dqkv


def _close(family, name, got, ref, bf=False):
    log = []
    R.assert_close(name, got, ref, K[family], bf16=bf, log=log)
    WORST[family] = max(WORST.get(family, 0.0), log[0][1])


def _same_bits(a, b):
    return torch.equal(a.bits()[:a.rows], b.bits()[:b.rows])


def check_case(lib, run, cls, p, seed, offset):
    """one case: three forward calls (every output; qkv_out NULL with attn_w or av_w alone), the backward, every stage compared"""
    B = run.B
    tag = f"B={B} {cls} p={p} seed={seed} offset={offset}"
    keep, av = R.tri_keep(B, p, seed, offset) if p > 0 else (None, None)
    full = run.fwd(p, seed, offset)
    bare = run.fwd(p, seed, offset, qkv=False, attn_w=False, av_w=True)
    other = run.fwd(p, seed, offset, qkv=False, attn_w=True, av_w=False)
    dqkv = run.bwd(full["probs"], p, seed, offset)
    torch.cuda.synchronize()
    for o in (full, bare, other):
        for k, buf in o.items():
            buf.assert_tail_intact(f"{tag} {k}")
    # without qkv_out, and with either of attn_w / av_w alone, the same bits
    for o in (bare, other):
        assert _same_bits(full["obar"], o["obar"]) and _same_bits(full["probs"], o["probs"]), f"{tag}: outputs depend on the optional ones"
    assert _same_bits(full["av_w"], bare["av_w"]) and _same_bits(full["attn_w"], other["attn_w"]), f"{tag}: attn_w / av_w depend on each other"
    # stage 1: the projection
    proj = R.fused_proj_of(B, cls)
    tile = full["qkv"].live()
    _close("fused_tile", f"{tag} qkv_out", tile, proj, bf=True)
    # stage 2: probabilities from the stored q and k
    ref_p, gap = R.fused_probs(tile.float(), keep, p)
    GAPS[cls] = max(GAPS.get(cls, 0.0), gap)
    pl = full["probs"].live()
    _close("fused_probs", f"{tag} probs", pl, ref_p)
    if cls in ("identical_tokens", "x_zero"):
        assert bool((pl == 0.5).all()), f"{tag}: probabilities of identical tokens are not exactly 0.5"
    # stage 3: context and returned weights from the reference probabilities and the float64 v
    f = R.tri_attn(proj, keep, p, av, probs=ref_p)
    _close("fused_ctx", f"{tag} obar", full["obar"].live(), f["obar"], bf=True)
    _close("fused_ctx", f"{tag} attn_w", full["attn_w"].live(), f["attn_w"])
    _close("fused_ctx", f"{tag} av_w", full["av_w"].live(), f["av_w"])
    if p == 0:
        assert bool((full["av_w"].live() == 1).all())
    # backward: the float64 projection, the kernel's own saved probabilities
    _, _, dobar = R.fused_inputs(B, cls)
    dqkv.assert_tail_intact(f"{tag} dqkv")
    _close("fused_bwd", f"{tag} dqkv", dqkv.live(), R.tri_attn_bwd(proj, dobar, pl, keep, p), bf=True)
    if cls == "normal":
        # the unfused backward kernel on the STORED tile, under its own bound
        dq2 = Out(2 * B, 1536, torch.bfloat16, 2)
        _lib.check(lib.mmdeer_trimodal_attn_bwd(full["qkv"].ptr, run.dobar.data_ptr(), full["probs"].ptr, dq2.ptr, B, 0,
                                                1 if p > 0 else 0, p if p > 0 else 0.3, seed, offset, stream()))
        torch.cuda.synchronize()
        dq2.assert_tail_intact(f"{tag} unfused dqkv")
        _close("tri_bwd", f"{tag} unfused dqkv of the stored tile", dq2.live(), R.tri_attn_bwd(tile.float(), dobar, pl, keep, p), bf=True)


@pytest.mark.parametrize("B", R.FUSED_B)
def test_fused_attention_against_float64(B):
    lib = _lib.load()
    runs = {}
    for cls, p, seed, offset in R.fused_cases(B):
        if cls not in runs:
            runs[cls] = Run(lib, B, cls)
        check_case(lib, runs[cls], cls, p, seed, offset)
    print("\n   worst ratio so far: " + "  ".join(f"{f} {w:.2f} (K {K[f]:g})" for f, w in WORST.items()))
    print("   largest score gap after the 1/8: " + "  ".join(f"{c} {g:.1f}" for c, g in GAPS.items()))


@pytest.mark.parametrize("B", [2, 129])
def test_zero_dobar_gives_exact_zeros(B):
    """d obar = 0: every product of the backward has a zero factor -- dq, dk and dv are exactly 0 (of either sign)"""
    lib = _lib.load()
    cls, p, seed, offset = next(c for c in R.fused_cases(B) if c[0] == "normal" and c[1] == 0.3)
    run = Run(lib, B, cls, dobar=torch.zeros(B, 512))
    o = run.fwd(p, seed, offset, qkv=False, attn_w=False, av_w=False)
    dqkv = run.bwd(o["probs"], p, seed, offset)
    torch.cuda.synchronize()
    dqkv.assert_tail_intact("dqkv")
    assert bool((dqkv.live().float() == 0).all())


@pytest.mark.parametrize("B", [129, 1025])
def test_two_launches_give_the_same_bits(B):
    """the LDS flag handshake, the ring and the ping-pong halves have no other check than correctness and this: one case, launched
    twice, forward and backward, bit for bit."""
    lib = _lib.load()
    cls, p, seed, offset = next(c for c in R.fused_cases(B) if c[0] == "normal" and c[1] == 0.3)
    run = Run(lib, B, cls)
    a = run.fwd(p, seed, offset)
    b = run.fwd(p, seed, offset)
    da, db = run.bwd(a["probs"], p, seed, offset), run.bwd(b["probs"], p, seed, offset)
    torch.cuda.synchronize()
    for k in a:
        assert torch.equal(a[k].bits(), b[k].bits()), f"{k} differs between two launches"
    assert torch.equal(da.bits(), db.bits()), "dqkv differs between two launches"
    assert bool(torch.isfinite(da.live().float()).all())


def test_batch_of_zero_touches_nothing():
    lib = _lib.load()
    run = Run(lib, 1, "normal")
    run.B = 0
    o = run.fwd(0.3, 91, 5)
    dqkv = run.bwd(o["probs"], 0.3, 91, 5)
    torch.cuda.synchronize()
    for k, buf in list(o.items()) + [("dqkv", dqkv)]:
        buf.assert_tail_intact(f"B = 0: {k}", written_rows=0)


def test_weight_image_bit_for_bit():
    """mmdeer_pack_qkv_headmajor against the restated layout and convert()'s rounding: ties both ways, +-0, inf, fp32 and bf16
    denormals, the largest finite values, NaN (stays NaN)."""
    lib = _lib.load()
    rng = np.random.default_rng(18)
    edge = R.convert_values()
    bits = rng.integers(0, 2 ** 32, 1536 * 512, dtype=np.uint64).astype(np.uint32)
    where = rng.permutation(bits.size)[:40 * edge.size]
    bits[where] = np.tile(edge, 40)
    w = torch.from_numpy(bits.view(np.int32).copy()).to(DEV)
    img = Out(1536, 512, torch.bfloat16, 1)
    _lib.check(lib.mmdeer_pack_qkv_headmajor(w.data_ptr(), img.ptr, stream()))
    torch.cuda.synchronize()
    img.assert_tail_intact("weight image")
    got = img.bits()[:1536].numpy().view(np.uint16)
    want = R.fused_weight_image(bits)
    nan = (want & 0x7FFF) > 0x7F80
    assert nan.any() and np.array_equal(got[~nan], want[~nan]), int((got[~nan] != want[~nan]).sum())
    assert (((got[nan] & 0x7F80) == 0x7F80) & ((got[nan] & 0x007F) != 0)).all()
