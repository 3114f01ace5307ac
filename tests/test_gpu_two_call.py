"""The two-call backward (mmdeer_backward phase = 1, then phase = 2: the data-parallel overlap plan of MultimodalDEER.train_step(comm=...))
at the batches where each call ends in the weight-gradient launch's OWN fold (option dw_fold): a multiple of 32, so the group is one
launch of the DMA kernel, and from chain_min = 512 on with the head's row partials written by the layer chain.

What the overlap rests on, and which section pins it:
  1. the in-launch fold of either call adds what the fold launch adds, in its order (dw_fold 1 against 0, bit for bit, after each call);
  2. phase 1 leaves bucket 2 untouched -- its tile counters, words of bucket 2, are zero again --, phase 2 neither writes nor reads buckets
     0-1 (they are being exchanged meanwhile), and the dropout counter advances in phase 2 only;
  3. the two calls compute the single call's gradient (buckets 0-1 bit for bit, bucket 2 up to a summation order);
  4. ... which is the bf16-emulating oracle's, through train_step(comm=...) itself;
  5. train_step(comm=...) and capture_train_step(comm=...) with an exchange that leaves a visible trace in every word it handles;
  6. dw_fold 1 against 0 in the modes tests/test_gpu_dw_fold.py leaves out: g_fused, global_stats, fp32 feature blocks.

Whole buffers are compared as int32 views: not one bit may differ, NaN patterns and the counter words included."""
import ctypes as C

import pytest
import torch

from mmdeer import _lib
from mmdeer.spec import DEFAULT_DIMS

from .test_gpu_bf16_parity import check_pair, run_pair
from .test_gpu_dw_fold import DEV, FOLD_LABEL, _inputs, _model, _upstream

pytestmark = pytest.mark.gpu

POISON = 0x7FC0DEAD          # a quiet-NaN word: no gradient is ever this value
AV_CHAIN_LABEL = "chain B13-B17 (audio-visual dX)"


def _lo():
    return int(_lib.load().mmdeer_bucket_end(2))      # buckets 0-1 are flat[lo:], bucket 2 is flat[:lo]


def _bits(x):
    return x.view(torch.int32)


def _same_bits(x, y, what=""):
    assert torch.equal(_bits(x), _bits(y)), f"{what}: {int((_bits(x) != _bits(y)).sum())} words differ"


def _traced(call):
    """Run `call` inside a launch trace; the labels of the launches it made."""
    lib = _lib.load()
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(32)]
    for e in evs:
        e.record()
    arr = (C.c_void_p * 32)(*[e.cuda_event for e in evs])      # the library keeps this pointer until trace_end: it must stay alive
    _lib.check(lib.mmdeer_trace_begin(arr, 32))
    try:
        call()
    finally:
        labels = [lib.mmdeer_trace_label(k).decode() for k in range(lib.mmdeer_trace_end())]
        del arr
    return labels


def backward(B, fold, calls=2, mode="loss", in_bf16=True, g_fused=False, gstats=False, between=None, **opts):
    """One forward (dropout step 1 of a fresh model) and the backward on a zeroed gradient buffer under dw_fold = `fold`: as two calls
    (phase 1, `between(flat)`, phase 2) or as the single call.  Returns a dict: `flat`, `loss`, `after1` (the buffer after phase 1),
    `labels` (one launch list per call)."""
    a, v, t, y = _inputs(B, seed=11, bf16=in_bf16)
    m = _model()
    lib = _lib.load()
    with _lib.options(dw_fold=fold, **opts):
        o = m._launch_forward(a, v, t, y if mode == "loss" else None, want_features=False)
        meta = o["_meta"]
        flat = torch.zeros(m._flat_elems, dtype=torch.float32, device=DEV)
        loss = torch.zeros(_lib.LOSS_OUT, dtype=torch.float32, device=DEV)
        kw = dict(flat=flat, want_views=False)
        if mode == "loss":
            args = (meta["targets"],)
            kw["loss_out"] = loss
        else:
            args = (None, *_upstream(B))
        if g_fused:
            g = torch.Generator(device=DEV).manual_seed(78)
            kw["g_fused"] = torch.randn(B, DEFAULT_DIMS.fusion, generator=g, device=DEV) * 0.01
        if gstats:       # exact-global mode on one rank: the batch's own statistics
            gs = torch.empty(106, dtype=torch.float32, device=DEV)
            _lib.check(lib.mmdeer_loss_stats(meta["ws"].data_ptr(), meta["ws"].numel(), B, 0, gs.data_ptr(), _lib.current_stream()))
            kw["global_stats"] = gs
        res = dict(flat=flat, loss=loss, after1=None, labels=[])
        for phase in ((0,) if calls == 1 else (1, 2)):
            res["labels"].append(_traced(lambda: m._launch_backward(meta, *args, phase=phase, **kw)))
            torch.cuda.synchronize()
            if phase == 1:
                res["after1"] = flat.clone()
                if between is not None:
                    between(flat)
    return res


def _assert_fold_equals_fold_launch(B, calls=2, in_launch=True, **kw):
    """dw_fold 1 against 0: the buffer after every call and the loss record bit for bit; the launch lists prove which fold ran."""
    on, off = backward(B, 1, calls, **kw), backward(B, 0, calls, **kw)
    assert bool(torch.isfinite(off["flat"]).all()) and float(off["flat"].abs().sum()) > 0.0
    if calls == 2:
        assert float(off["after1"][_lo():].abs().sum()) > 0.0
        _same_bits(on["after1"], off["after1"], f"B={B} {kw} after phase 1")
    _same_bits(on["flat"], off["flat"], f"B={B} {kw} after the last call")
    assert torch.equal(on["loss"], off["loss"])
    assert len(on["labels"]) == calls
    for l1, l0 in zip(on["labels"], off["labels"]):
        assert FOLD_LABEL in l0
        if in_launch:
            assert FOLD_LABEL not in l1 and l1 == [x for x in l0 if x != FOLD_LABEL]
        else:
            assert l1 == l0


# ------------------------------------------------------------------ 1. in-launch fold against the fold launch, two calls
@pytest.mark.parametrize("mode", ["loss", "chain"])
@pytest.mark.parametrize("ksteps", [0, 1])
@pytest.mark.parametrize("B", [128, 320, 512, 1024])
def test_both_calls_fold_in_launch_as_the_fold_launch_does(B, ksteps, mode):
    """Phase 2 cuts K eight times shorter (slice_div = 8, at least 4 K-tiles per slice): its B-row / 2B-row problems get 1 / 1 slices at
    B = 128, 2 / 3 at 320 (uneven last slice), 2 / 4 at 512, 4 / 8 at 1024 with automatic slicing, while phase 1 slices as the single
    call does (1 / 2); ksteps = 1 gives both calls 2 / 4, 5 / 8, 8 / 8 and 8 / 8.  The row partials of phase 1 come from the ln_bwd /
    nig_bwd launches at B = 128 and 320 and from the head chain from 512 on; those of phase 2 always from ln_bwd.  Loss mode, and chain
    mode (upstream gradients on the NIG outputs, no targets)."""
    _assert_fold_equals_fold_launch(B, mode=mode, ksteps=ksteps)


@pytest.mark.parametrize("mode", ["loss", "chain"])
@pytest.mark.parametrize("ksteps", [0, 1])
@pytest.mark.parametrize("opts", [dict(dw_tile=3), dict(dw_tile=4), dict(dw_kg=1)], ids=["256x256", "256x128", "128x128-kg1"])
def test_both_calls_fold_in_launch_on_the_other_tiles(opts, ksteps, mode):
    """... and on the other tile shapes of the kernel and the 32-row K stages, B = 512.  The 256-row tiles take their automatic slice
    length from ksteps_target, not from B: one slice per problem at this batch, so only the row partials fold in the launch; with
    ksteps = 1 every problem of either call has 8 slices."""
    _assert_fold_equals_fold_launch(512, mode=mode, ksteps=ksteps, **opts)


# ------------------------------------------------------------------ 2. what the overlap rests on
@pytest.mark.parametrize("B", [512, 1024])
def test_phase_1_leaves_bucket_2_untouched_and_phase_2_leaves_buckets_0_1_alone(B):
    """After phase 1 bucket 2 is all zero bits: nothing written there, every tile counter (words of the AV in_proj's q/k thirds) reset.
    Between the calls buckets 0-1 are overwritten with a NaN pattern, as an exchange in flight might leave anything there: phase 2 must
    not write one word of them (the pattern survives bit for bit) and must not read them (bucket 2 comes out as without the overwrite)."""
    lo = _lo()

    def poison(flat):
        _bits(flat)[lo:] = POISON
        torch.cuda.synchronize()

    clean, dirty = backward(B, 1), backward(B, 1, between=poison)
    for r in (clean, dirty):
        assert int((_bits(r["after1"])[:lo] != 0).sum()) == 0
        assert float(r["after1"][lo:].abs().sum()) > 0.0
    assert FOLD_LABEL not in clean["labels"][0] + clean["labels"][1]
    _same_bits(clean["flat"][lo:], clean["after1"][lo:], "buckets 0-1 over phase 2")
    assert int((_bits(dirty["flat"])[lo:] != POISON).sum()) == 0
    _same_bits(dirty["flat"][:lo], clean["flat"][:lo], "bucket 2 with buckets 0-1 overwritten")
    assert bool(torch.isfinite(clean["flat"]).all()) and float(clean["flat"][:lo].abs().sum()) > 0.0


def _three_two_call_steps(B, fold):
    """Three steps with different inputs on one model, one workspace and ONE gradient buffer zeroed once, the dropout step counter on
    the device with the pending increment (bump_offset_dev): the gradient after each step, the counter's advance over either call."""
    m = _model()
    ctr = torch.full((), 5, dtype=torch.int64, device=DEV)
    flat = torch.zeros(m._flat_elems, dtype=torch.float32, device=DEV)
    grads, bumps = [], []
    with _lib.options(dw_fold=fold):
        for i in range(3):
            a, v, t, y = _inputs(B, seed=100 + i)
            meta = m._launch_forward(a, v, t, y, want_features=False, offset_dev=ctr, bump=True)["_meta"]
            loss = torch.zeros(_lib.LOSS_OUT, dtype=torch.float32, device=DEV)
            seen = [int(ctr)]
            for phase in (1, 2):
                m._launch_backward(meta, meta["targets"], loss_out=loss, flat=flat, want_views=False, phase=phase)
                torch.cuda.synchronize()
                seen.append(int(ctr))
            grads.append(flat.clone())
            bumps.append((seen[1] - seen[0], seen[2] - seen[1]))
    return grads, bumps


@pytest.mark.parametrize("B", [512, 1024])
def test_dropout_counter_advances_in_phase_2_only(B):
    """The counter advances by 0 over phase 1 (the forward's and both calls' masks are drawn at the same step) and by 1 over phase 2;
    three consecutive steps equal the same steps under dw_fold = 0 (a counter left set, a slab read stale, a counter bumped twice would
    all show from the second step on)."""
    g1, b1 = _three_two_call_steps(B, 1)
    g0, b0 = _three_two_call_steps(B, 0)
    assert b1 == [(0, 1)] * 3 and b0 == [(0, 1)] * 3
    for i in range(3):
        _same_bits(g1[i], g0[i], f"step {i + 1}")
    assert not torch.equal(g0[0], g0[1]) and not torch.equal(g0[1], g0[2])


# ------------------------------------------------------------------ 3. two calls against the single call, same dropout step
def _rel_cos(x, y):
    x, y = x.double(), y.double()
    return float((x - y).norm() / y.norm()), float((x @ y) / (x.norm() * y.norm()))


@pytest.mark.parametrize("B", [512, 1024])
def test_two_calls_equal_the_single_call(B):
    """Default options: phase 1 slices every problem as the single call does, so buckets 0-1 are bit-equal; the single call walks the
    audio-visual run as a chain, whose LayerNorm backward sums a row in another order than the ln_bwd launch of phase 2: bucket 2 is held
    to the bound test_backward_chain_matches_the_separate_launches has for that difference."""
    lo = _lo()
    two, one = backward(B, 1), backward(B, 1, calls=1)
    assert torch.equal(two["loss"], one["loss"])
    _same_bits(two["flat"][lo:], one["flat"][lo:], "buckets 0-1")
    assert AV_CHAIN_LABEL in one["labels"][0] and AV_CHAIN_LABEL not in two["labels"][0] + two["labels"][1]
    assert not torch.equal(two["flat"][:lo], one["flat"][:lo])               # the other plan really ran
    rel, cos = _rel_cos(two["flat"][:lo], one["flat"][:lo])
    print(f"two calls vs single call B={B}: bucket 2 rel-l2 {rel:.2e}, cosine {cos:.6f}")
    assert rel < 2e-2 and cos > 0.9998, (rel, cos)


@pytest.mark.parametrize("B", [512, 1024])
def test_two_calls_equal_the_single_call_on_separate_launches(B):
    """chain_bwd = 0: both run the same dX and LayerNorm-backward launches; only the K-slices of phase 2's five weight gradients are
    shorter -- the same bf16 products summed in fp32 in another order."""
    lo = _lo()
    two, one = backward(B, 1, chain_bwd=0), backward(B, 1, calls=1, chain_bwd=0)
    assert AV_CHAIN_LABEL not in one["labels"][0]
    assert torch.equal(two["loss"], one["loss"])
    _same_bits(two["flat"][lo:], one["flat"][lo:], "buckets 0-1")
    rel, _ = _rel_cos(two["flat"][:lo], one["flat"][:lo])
    print(f"two calls vs single call, separate launches B={B}: bucket 2 rel-l2 {rel:.2e}")
    assert rel < 1e-5, rel


# ------------------------------------------------------------------ the communicator double of sections 4 and 5
class SideStreamExchange:
    """Stands in for parallel.BucketedAllReduce: forks a side stream from the current one exactly as its launch_range does and there
    scales the range in place -- by 0.5, exact in fp32, the mean over two ranks holding the same gradient; by 1.0, the identity."""
    active = True

    def __init__(self, scale):
        self.scale = scale
        self.ranges = []
        self._side = None

    def launch_range(self, flat, lo, hi):
        if self._side is None:
            self._side = torch.cuda.Stream(device=flat.device)
        self._side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self._side):
            flat[lo:hi].mul_(self.scale)
        self.ranges.append((lo, hi))

    def join(self):
        if self._side is not None:
            torch.cuda.current_stream().wait_stream(self._side)


# ------------------------------------------------------------------ 4. an independent reference
@pytest.mark.parametrize("B", [512, 1024])
def test_overlapped_step_matches_the_bf16_oracle(B):
    """train_step(comm=...) with an identity exchange against the bf16-emulating oracle, bounds of tests/test_gpu_bf16_parity.py."""
    comm = SideStreamExchange(1.0)
    res = run_pair(B, dropout=0.3, seed=50 + B, step=lambda m, *x: m.train_step(*x, comm=comm))
    lo = _lo()
    assert comm.ranges == [(lo, res[0]._flat_elems), (0, lo)]             # the two-call branch ran
    check_pair(*res, B, f"two-call overlap B={B}")


# ------------------------------------------------------------------ 5. the overlapped plan itself
@pytest.mark.parametrize("B", [512, 1024])
def test_overlapped_train_step_equals_the_manual_two_calls(B):
    """Every word of the step's buffer is half the manual two-call result (the exchange of buckets 0-1 runs beside phase 2: a phase-2
    write into that range lands after the scaling, or is scaled twice, and shows as a word that is not the half)."""
    manual = backward(B, 1)
    m = _model()
    comm = SideStreamExchange(0.5)
    d = m.train_step(*_inputs(B, seed=11), comm=comm)
    torch.cuda.synchronize()
    lo = _lo()
    assert comm.ranges == [(lo, m._flat_elems), (0, lo)]
    _same_bits(m.flat_grad(), manual["flat"] * 0.5, "overlapped step")
    assert float(d["total_loss"]) == float(manual["loss"][16])


def test_captured_overlapped_step_replays_the_eager_one():
    """capture_train_step(comm=...): the side-stream fork and join are part of the graph.  Three replays with different inputs copied
    into the static tensors each equal the eager overlapped step of that input at that dropout step, on a buffer that is never zeroed
    again; the device counter advances by 1 per replay (phase 2's launch alone bumps it)."""
    B = 512
    steps = [_inputs(B, seed=100 + i) for i in range(3)]
    m, e = _model(), _model()
    static = [x.clone() for x in steps[0]]
    replay = m.capture_train_step(*static, comm=SideStreamExchange(0.5))
    ctr = m._graph_counter
    ecomm = SideStreamExchange(0.5)
    seen = []
    for inp in steps:
        for dst, src in zip(static, inp):
            dst.copy_(src)
        before = int(ctr)
        d = replay()
        torch.cuda.synchronize()
        assert int(ctr) - before == 1
        e._step = before                     # the replay draws its masks at step `before` + 1, as the eager step after this does
        de = e.train_step(*inp, comm=ecomm)
        torch.cuda.synchronize()
        _same_bits(m.flat_grad(), e.flat_grad(), f"replay at step {before + 1}")
        assert float(d["total_loss"]) == float(de["total_loss"])
        seen.append(m.flat_grad().clone())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])


# ------------------------------------------------------------------ 6. the modes tests/test_gpu_dw_fold.py leaves out
@pytest.mark.parametrize("calls", [1, 2], ids=["single", "two-call"])
def test_fold_in_launch_with_a_gradient_on_fused_features(calls):
    """g_fused given: the head / trimodal run leaves the chain (plan.bchain off), so at a chain-sized batch the row partials come from
    the ln_bwd launches, nparts = ln_bwd_nparts(B)."""
    _assert_fold_equals_fold_launch(512, calls, g_fused=True)
    _assert_fold_equals_fold_launch(512, calls, g_fused=True, mode="chain")


@pytest.mark.parametrize("chain_nig", [1, 0])
@pytest.mark.parametrize("calls", [1, 2], ids=["single", "two-call"])
def test_fold_in_launch_in_exact_global_mode(calls, chain_nig):
    """global_stats given (the batch's own mmdeer_loss_stats): the head's backward in the chain prologue, or as the nig_bwd launch."""
    _assert_fold_equals_fold_launch(512, calls, gstats=True, chain_nig=chain_nig)


@pytest.mark.parametrize("calls", [1, 2], ids=["single", "two-call"])
def test_fp32_feature_blocks_keep_the_fold_launch(calls):
    """fp32 feature blocks under bf16 compute: the input projections' weight gradients read fp32 operands, the group splits by source
    mode and every call keeps the fold launch under dw_fold = 1 -- same launch list, same bits."""
    _assert_fold_equals_fold_launch(512, calls, in_launch=False, in_bf16=False)
