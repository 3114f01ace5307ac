"""Option dw_fold: the weight-gradient launch (gemm_tt_dma_kernel) adds its own split-K slices, folds the row partials in workgroups
behind its tiles and bumps the dropout step counter, instead of the reduce_partials launch behind it.

Every comparison is torch.equal on the WHOLE flat gradient buffer between dw_fold = 1 and dw_fold = 0, bf16: the in-launch fold adds
the same fp32 values in the same order, so not one bit may differ.  The buffer starts zeroed, and the tile counters of the launch are
words of it that no gradient is written to (the q/k thirds of the AV in_proj): equality also proves they are zero again afterwards."""
import ctypes as C

import pytest
import torch

from mmdeer import _lib, synth
from mmdeer.model import ModelConfig, MultimodalDEER

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FOLD_LABEL = "reduce_partials (fold)"


def _inputs(B, seed, bf16=True):
    b = synth.make_batch(B, seed=seed)
    a, v, t, y = (torch.from_numpy(b[k]).to(DEV) for k in ("audio", "video", "text", "targets"))
    return (a.bfloat16(), v.bfloat16(), t.bfloat16(), y) if bf16 else (a, v, t, y)


def _model(dtype="bf16"):
    return MultimodalDEER(ModelConfig(compute_dtype=dtype, dropout=0.3, seed=8)).to(DEV).train()


def _upstream(B):
    g = torch.Generator(device=DEV).manual_seed(77)
    return [torch.randn(B, 3, generator=g, device=DEV) * 0.1 for _ in range(4)]


def _backward(B, fold, mode="loss", dtype="bf16", trace=False, **opts):
    """One forward + backward on a zeroed gradient buffer under dw_fold = `fold`: (flat gradient, loss_out, launch labels)."""
    a, v, t, y = _inputs(B, seed=11, bf16=dtype == "bf16")
    m = _model(dtype)
    lib = _lib.load()
    with _lib.options(dw_fold=fold, **opts):
        o = m._launch_forward(a, v, t, y if mode == "loss" else None, want_features=False)
        meta = o["_meta"]
        flat = torch.zeros(m._flat_elems, dtype=torch.float32, device=DEV)
        loss = torch.zeros(_lib.LOSS_OUT, dtype=torch.float32, device=DEV)
        labels = arr = None
        if trace:
            evs = [torch.cuda.Event(enable_timing=True) for _ in range(32)]
            for e in evs:
                e.record()
            arr = (C.c_void_p * 32)(*[e.cuda_event for e in evs])      # the library keeps this pointer until trace_end: it must stay alive
            _lib.check(lib.mmdeer_trace_begin(arr, 32))
        try:
            if mode == "loss":
                m._launch_backward(meta, meta["targets"], loss_out=loss, flat=flat, want_views=False)
            else:
                gm, gn, ga, gb = _upstream(B)
                m._launch_backward(meta, None, gm, gn, ga, gb, flat=flat, want_views=False)
        finally:
            if trace:
                labels = [lib.mmdeer_trace_label(k).decode() for k in range(lib.mmdeer_trace_end())]
                del arr
        torch.cuda.synchronize()
    return flat, loss, labels


def _assert_same(B, mode="loss", dtype="bf16", **opts):
    g1, l1, _ = _backward(B, 1, mode, dtype, **opts)
    g0, l0, _ = _backward(B, 0, mode, dtype, **opts)
    assert bool(torch.isfinite(g0).all()) and float(g0.abs().sum()) > 0.0
    assert torch.equal(g1.view(torch.int32), g0.view(torch.int32)), f"B={B} {mode} {opts}: {int((g1.view(torch.int32) != g0.view(torch.int32)).sum())} words differ"
    assert torch.equal(l1, l0)


@pytest.mark.parametrize("dw_tile", [2, 3, 4])
@pytest.mark.parametrize("ksteps", [1, 2])
@pytest.mark.parametrize("B", [128, 320, 512])
def test_slice_counts_and_summation_order(B, ksteps, dw_tile):
    """Slices of `ksteps` 64-row K-tiles, capped at splitk_max = 8: the B-row / 2B-row problems get 2 / 4 (B = 128), 5 / 8 (320) and
    8 / 8 (512) slices with ksteps = 1, and 1 / 2, 3 / 5 (uneven last slices) and 4 / 8 with ksteps = 2 -- the one-by-one tail of the
    fold's order on every lane count, two parts per lane from five slices on.  dw_tile: the three tile shapes (2: the K-split 128 x 128
    form).  Ragged tiles are the model's own: the 84-of-128-column audio projection, the 64-row head tiles."""
    _assert_same(B, ksteps=ksteps, dw_tile=dw_tile)


def test_slice_counts_32_row_stages():
    """... and the 128 x 128 tile on 32-row K stages (dw_kg = 1), the other KG of the kernel."""
    _assert_same(320, ksteps=1, dw_kg=1)
    _assert_same(512, ksteps=2, dw_kg=1)


@pytest.mark.parametrize("mode", ["loss", "chain"])
@pytest.mark.parametrize("B", [512, 128])
def test_row_partials_by_both_producers(B, mode):
    """The LayerNorm gamma / beta slabs and the head's part_w3 / part_b3 are written by the layer chains at B = 512 (chain_min) and
    by the ln_bwd / nig_bwd launches at B = 128; loss mode and chain mode (upstream gradients on the NIG outputs)."""
    _assert_same(B, mode)


def _three_steps(fold, graph):
    """Three training steps with DIFFERENT inputs on one model (one workspace, one gradient buffer), dropout on, the step counter on
    the device: eager with bump_offset_dev, or three replays of one captured graph.  Returns the gradient after each step and the
    counter's advance over each."""
    B = 512
    m = _model()
    steps = [_inputs(B, seed=100 + i) for i in range(3)]
    grads, bumps = [], []
    with _lib.options(dw_fold=fold):
        if graph:
            static = [x.clone() for x in steps[0]]
            replay = m.capture_train_step(*static)
            ctr = m._graph_counter
            for inp in steps:
                for dst, src in zip(static, inp):
                    dst.copy_(src)
                before = int(ctr)
                replay()
                torch.cuda.synchronize()
                grads.append(m.flat_grad().clone())
                bumps.append(int(ctr) - before)
        else:
            ctr = torch.full((), 5, dtype=torch.int64, device=DEV)
            for inp in steps:
                before = int(ctr)
                m.train_step(*inp, _offset_dev=ctr, _bump=True)
                torch.cuda.synchronize()
                grads.append(m.flat_grad().clone())
                bumps.append(int(ctr) - before)
    return grads, bumps


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_stale_data_self_reset_and_dropout_counter(graph):
    """Every step must equal the dw_fold = 0 run of that step: a counter that is not reset, a slab line read stale from the step
    before, or a dropout counter bumped twice or not at all (the masks of steps 2 and 3 follow it) would all show.  The counter
    itself advances by exactly 1 per step."""
    g1, b1 = _three_steps(1, graph)
    g0, b0 = _three_steps(0, graph)
    assert b1 == [1, 1, 1] and b0 == [1, 1, 1]
    for i in range(3):
        assert torch.equal(g1[i].view(torch.int32), g0[i].view(torch.int32)), f"step {i + 1}"
    assert not torch.equal(g0[0], g0[1]) and not torch.equal(g0[1], g0[2])


def test_launch_list():
    """With dw_fold = 1 the step's launch trace has one launch fewer and no fold; with dw_fold = 0 it has both."""
    _, _, on = _backward(512, 1, trace=True)
    _, _, off = _backward(512, 0, trace=True)
    assert FOLD_LABEL in off and FOLD_LABEL not in on
    assert len(on) == len(off) - 1 and on == [x for x in off if x != FOLD_LABEL]


@pytest.mark.parametrize("B,dtype", [(64, "fp32"), (100, "bf16")])
def test_fallback_keeps_the_fold_launch(B, dtype):
    """The fp32 parity path, and a batch that is no multiple of 32 (off the DMA kernel), still run the fold launch under dw_fold = 1
    and still match."""
    g1, l1, on = _backward(B, 1, dtype=dtype, trace=True)
    g0, l0, off = _backward(B, 0, dtype=dtype, trace=True)
    assert FOLD_LABEL in on and on == off
    assert torch.equal(g1.view(torch.int32), g0.view(torch.int32)) and torch.equal(l1, l0)
    assert float(g0.abs().sum()) > 0.0
