"""The layer-chain kernel's layer ends (csrc/chain.hip): segment records read as scalars from the kernel arguments, the
LayerNorm-backward fold of the gamma / beta partials (csrc/ln_rows.h: ln_bwd_fold16, shared with ln_bwd_rows16_kernel), and the loss
finals of the backward head chain's prologue (csrc/nig_dev.h: compute_finals).

Every comparison is on bits (buffers viewed as integers) against the launch-by-launch plan of the same library:

* one mmdeer_chain call against the same layers run one by one (tests/test_gpu_chain_routes.py: _run_case -- bit for bit against
  mmdeer_gemm / mmdeer_layernorm_fwd / _bwd / mmdeer_add_masked, plus that file's float64, canary and determinism checks);
* one Stack C training step with the chains against the same step with chain = 0.  The FORWARD chains equal the separate launches
  bit for bit in loss, outputs and every gradient (chain_bwd = 0 on both sides).  The backward chain's LayerNorm backward rounds dz
  differently from the launch the chain_bwd = 0 plan uses (tests/test_gpu_model.py asserts that the two gradients differ), so the
  backward chain of a step is held to its bit-for-bit relations instead: the same step with the head's backward as a launch of its
  own (chain_nig = 0) and with the NIG head as the forward chain's tail (chain_nigf = 1);
* 32-sample workgroups fold 32 rows into one LayerNorm-backward slab where the launch-by-launch plan has two of 16 rows: there dz is
  compared bit for bit and the slabs by their folded sums (the bound of tests/test_gpu_chain_routes.py).

A record that is read a segment late, or a scalar kept from the segment before, changes the result: in RECORDS every pair of
consecutive segments differs in K / 64, in the tile kind or count, in bias / ReLU / dropout site and shift / mask, in the residual bits
or in what the layer end does."""
import pytest
import torch

from mmdeer import _lib
from mmdeer.spec import param_offsets, param_table

from . import rowkernel_ref as R
from .test_gpu_chain_routes import KERNELS, L, S, _run_case
from .test_gpu_nig_loss import _plan_step, _same_bits
from .test_gpu_rowkernels import K as RK, _ln_bwd, dt, inp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ------------------------------------------------------------------------------------------------------------------ records
def _records(wide):
    """Twelve segments (CHAIN_MAX_SEGS) in eight layers.  K / 64 per segment: 12 (16-sample kernels; 8 on 32-sample workgroups), 6, 4,
    2, 4, 6, 1, 4, 2, 4, 2, 1; 128-column tiles except segments 3, 4 and 8 (64-column tiles: N = 192, 192, 64); widths 512, 256, 256,
    384, 256, 512, 192, 512; ends: LayerNorm forward (512), LayerNorm backward (256, masked), LayerNorm backward (256, plain), stash
    split in two, LayerNorm forward (256), LayerNorm backward (512), plain stash, stash split.  (Every layer keeps a stash: the
    float64 check is teacher-forced from the stored panels.)"""
    K0 = 768 if wide else 512
    return dict(K0=K0, p=0.5, offset=3, dev=4, layers=[
        L([S(512, K0, relu=1, site=1)], kind="ln", ld_stash=520),
        L([S(256, 384, kin=64, bias=False, mask=(264, 8, 1.25), res_dup=1)], kind="lnb", ms=1.25),
        L([S(256, 256, bias=False, res_add=1)], kind="lnb", ms=0.0, ld_stash=272),
        L([S(192, 128, kin=64, relu=1, site=2, shift=5), S(192, 256, nout_off=192, bias=False)], split=200, ld_stash=208),
        L([S(128, 384, mask=(136, 0, 0.5)), S(128, 64, kin=320, nout_off=128, relu=1, site=3)], kind="ln"),
        L([S(512, 256)], kind="lnb", ms=1.25),
        L([S(64, 128, kin=384, relu=1), S(128, 256, kin=128, nout_off=64, bias=False, mask=(128, 0, 2.0))], ld_stash=200),
        L([S(256, 128, kin=64, site=5, shift=5), S(256, 64, nout_off=256, bias=False, relu=1)], split=448, ld_stash=456)])


@pytest.mark.parametrize("kernel,rows", [(k, r) for k in ("s16", "s16_d2", "s16_d8") for r in (16, 17, 33)] + [("s32", 32), ("s32", 33)])
def test_records_one_chain_call(kernel, rows):
    case = _records(wide=KERNELS[kernel]["ts"] == 16)
    assert sum(len(lay["segs"]) for lay in case["layers"]) == _lib.CHAIN_MAX_SEGS
    _run_case(case, kernel, rows=rows, seed=rows)


def _forward_chain_step(B, **opts):
    return _plan_step(B, chain_bwd=0, **opts)


@pytest.mark.parametrize("B,ts", [(16, 0), (17, 0), (33, 0), (32, 32), (33, 32)])
def test_records_stack_c_forward_chains_equal_the_separate_launches(B, ts):
    """Stack C's own tables: the audio-visual chain (two row groups, both fold codes, the second input panel, 64-column head tiles in
    F9..F17, LayerNorm forward ends) against chain = 0."""
    on, off = _forward_chain_step(B, chain=1, chain_ts=ts), _forward_chain_step(B, chain=0)
    assert _same_bits(on[0], off[0]) and torch.equal(on[1], off[1]) and _same_bits(on[2], off[2])
    assert _same_bits(on[3], off[3]), f"{int((on[3].view(torch.int32) != off[3].view(torch.int32)).sum())} gradient words differ"


# --------------------------------------------------------------------------------------------------------------------- fold
def _fold_case(n):
    """Two LayerNorm backwards back to back: the second fold writes the scratch the first one's slow waves may still be reading."""
    return dict(K0=256, layers=[L([S(n, 256)], kind="lnb", ms=1.25), L([S(n, n, bias=False)], kind="lnb", ms=0.0),
                                L([S(128, 256, kin=n - 256)])])


@pytest.mark.parametrize("kernel", ["s16", "s32"])
@pytest.mark.parametrize("rows", [1, 15, 16, 17])
@pytest.mark.parametrize("n", [256, 512])
def test_fold_in_the_chain(n, rows, kernel):
    _run_case(_fold_case(n), kernel, rows=rows, seed=n + rows)


@pytest.mark.parametrize("M", [1, 15, 16, 17])
@pytest.mark.parametrize("N", [256, 512])
def test_fold_in_the_row_kernel_against_float64(N, M):
    """ln_bwd_rows16_kernel through mmdeer_layernorm_bwd (bf16), slab and folded gradients, under tests/rowkernel_ref.py's bound."""
    lib = _lib.load()
    y, dout, gamma, beta = R.ln_inputs(M, N, True)
    f = R.ln_fwd(y, gamma, beta)
    mean32, rstd32 = f["mean"].v.float(), f["rstd"].v.float()
    yd, dd, gd = inp(y, dt(True)), inp(dout, dt(True)), inp(gamma.reshape(1, N), torch.float32)
    md, rd = inp(mean32, torch.float32), inp(rstd32, torch.float32)
    b = R.ln_bwd(dout, y, mean32, rstd32, gamma, 0.0)
    for fold in (True, False):
        dz, part, dgam, dbet = _ln_bwd(lib, dd, yd, md, rd, gd, M, N, True, 0.0, fold)
        torch.cuda.synchronize()
        name = f"bf16 M={M} N={N} fold={fold}"
        R.assert_close(f"{name} dz", dz.live(), b["_dy"], RK["ln_bwd"], bf16=True)
        if fold:
            R.assert_close(f"{name} dgamma", dgam.live(), b["dgamma"], RK["ln_bwd"])
            R.assert_close(f"{name} dbeta", dbet.live(), b["dbeta"], RK["ln_bwd"])
        else:
            R.assert_close(f"{name} slab", part.live(), b["slab"], RK["ln_bwd"])
        dz.assert_tail_intact(name)
        part.assert_tail_intact(name)


# ------------------------------------------------------------------------------------------------------------------- finals
HEAD_LO = min(o for (name, _s, _i), o in zip(param_table(), param_offsets()[0]) if ".evidence_net.6." in name)


def _assert_head_chain_equals_head_launch(B, nigf):
    """chain_nig = 1 against chain_nig = 0: loss record, ECE bin counts, outputs and every gradient below the heads' last layers
    bit for bit (dW3 / db3 are summed over other partial blocks: tests/test_gpu_model.py)."""
    on, off = _plan_step(B, chain_nig=1, chain_nigf=nigf), _plan_step(B, chain_nig=0, chain_nigf=nigf)
    assert _same_bits(on[0], off[0]) and torch.equal(on[1], off[1]) and _same_bits(on[2], off[2])
    assert int(on[1].sum()) == 3 * B
    assert _same_bits(on[3][:HEAD_LO], off[3][:HEAD_LO])
    rel = (on[3][HEAD_LO:].double() - off[3][HEAD_LO:].double()).norm() / off[3][HEAD_LO:].double().norm()
    assert float(rel) < 1e-5, float(rel)


@pytest.mark.parametrize("B", [64, 128, 1088, 4096])
def test_finals_from_block_partials(B):
    """nblk = 1, 2, 17 and 64 partials of 64 samples."""
    assert (B + 63) // 64 in (1, 2, 17, 64)
    _assert_head_chain_equals_head_launch(B, nigf=0)


@pytest.mark.parametrize("B", [80, 96, 112, 1072])
def test_finals_from_wave_partials(B):
    """chain_nigf = 1: wave partials of 16 samples; the last block has 1, 2, 3 present waves (B = 80, 96, 112; 1072: 17 blocks, 3 waves)."""
    assert ((B + 15) // 16) % 4 in (1, 2, 3)
    _assert_head_chain_equals_head_launch(B, nigf=1)
