"""The device step counter of the three by-value dropout entries (include/mmdeer_drop_dev.h: mmdeer_dropout_mask_dev,
mmdeer_trimodal_attn_fwd_dev, mmdeer_trimodal_attn_bwd_dev) on the GPU.

Everything here is bit for bit: the _dev entries run the plain entries' kernels and differ only in where the step comes from, so
  (offset = a, *counter = b)  ==  the plain entry at offset = a + b (modulo 2^64),
                                  for (a, b) in (0, 0), (5, 0), (0, 5), (3, 4), (2^64 - 2, 5) -- the last pair wraps to 3
  a NULL counter              ==  the plain entry
  the counter                 is not written
  p = 0 with a counter        ==  p = 0 without one (the counter is not read)
  a misaligned counter        is refused before any launch: the outputs keep their fill
The mask at (rows, cols) = (3, 40) and (2049, 257): 257 columns cross the 256 threads of a block inside a row, 2049 rows make
526593 elements, past the 2048 x 256 that one trip of the grid covers.  The attention pair at B = 1 and 3 (one block holds four
samples), fp32 and bf16, forward (with both weight outputs, av_w draws at a second site) and backward.  What the masks ARE is held
to the uint32 restatement and to float64 by tests/test_gpu_rowkernels.py through the plain entries."""
import functools

import pytest
import torch

from mmdeer import _lib

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED = 2 ** 40 + 7
PAIRS = [(0, 0), (5, 0), (0, 5), (3, 4), (2 ** 64 - 2, 5)]
MASK_SHAPES = [(3, 40), (2049, 257)]
FILL = 7.0


def stream():
    return torch.cuda.current_stream().cuda_stream


def counter_of(b):
    t = torch.tensor([b], dtype=torch.int64, device=DEV)
    assert t.data_ptr() % 8 == 0
    return t


def mask(rows, cols, p, offset, counter=None, dev=True, site=113):
    lib = _lib.load()
    out = torch.full((rows, cols), 9, dtype=torch.uint8, device=DEV)
    if dev:
        _lib.check(lib.mmdeer_dropout_mask_dev(site, rows, cols, p, SEED, offset, out.data_ptr(), stream(), None if counter is None else counter.data_ptr()))
    else:
        _lib.check(lib.mmdeer_dropout_mask(site, rows, cols, p, SEED, offset, out.data_ptr(), stream()))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("rows,cols", MASK_SHAPES)
def test_mask_counter_plus_offset_is_the_plain_entry_at_the_sum(rows, cols):
    seen = {}
    for a, b in PAIRS:
        c = counter_of(b)
        got = mask(rows, cols, 0.3, a, c)
        assert int(c) == b, "the call wrote the counter"
        step = (a + b) % 2 ** 64
        want = seen.setdefault(step, mask(rows, cols, 0.3, step, dev=False))
        assert torch.equal(got, want), f"offset {a} + counter {b}: {int((got != want).sum())} of {got.numel()} elements differ"
        assert int(got.max()) == 1 and 0 < int(got.sum()) < got.numel()
    assert sorted(seen) == [0, 3, 5, 7] and not torch.equal(seen[0], seen[5]) and not torch.equal(seen[3], seen[7]), "the step does not reach the mask"
    assert torch.equal(mask(rows, cols, 0.3, 5, None), seen[5]), "a NULL counter"


@pytest.mark.parametrize("rows,cols", MASK_SHAPES)
def test_mask_p0_with_a_counter_is_p0_without_one(rows, cols):
    c = counter_of(9)
    assert torch.equal(mask(rows, cols, 0.0, 3, c), mask(rows, cols, 0.0, 3, dev=False))
    assert torch.equal(mask(rows, cols, 0.0, 3, c), mask(rows, cols, 0.0, 3, None)) and int(c) == 9


# ------------------------------------------------------------------------------------------------ the attention pair
@functools.lru_cache(maxsize=None)
def attn_inputs(B, compute):
    """qkv (2B, 1536) and the gradient of the pooled context (B, 512), drawn once per (B, dtype) and never written; the saved
    probabilities come from one plain forward"""
    g = torch.Generator().manual_seed(50 + B)
    dt = torch.float32 if compute == "fp32" else torch.bfloat16
    qkv = (0.5 * torch.randn(2 * B, 1536, generator=g)).to(dt).to(DEV)
    dobar = torch.randn(B, 512, generator=g).to(dt).to(DEV)
    return qkv, dobar


def attn_fwd(B, compute, p, training, offset, counter=None, dev=True):
    lib, (qkv, _) = _lib.load(), attn_inputs(B, compute)
    out = {"obar": torch.full((B, 512), FILL, dtype=qkv.dtype, device=DEV), "probs": torch.full((B, 8, 4), FILL, device=DEV),
           "attn_w": torch.full((B, 2, 2), FILL, device=DEV), "av_w": torch.full((B, 2), FILL, device=DEV)}
    args = (qkv.data_ptr(), out["obar"].data_ptr(), out["probs"].data_ptr(), out["attn_w"].data_ptr(), out["av_w"].data_ptr(), B,
            int(compute == "fp32"), training, p, SEED, offset, stream())
    if dev:
        _lib.check(lib.mmdeer_trimodal_attn_fwd_dev(*args, None if counter is None else counter.data_ptr()))
    else:
        _lib.check(lib.mmdeer_trimodal_attn_fwd(*args))
    torch.cuda.synchronize()
    return out


def attn_bwd(B, compute, p, training, offset, counter=None, dev=True):
    lib, (qkv, dobar) = _lib.load(), attn_inputs(B, compute)
    probs = attn_fwd(B, compute, 0.0, 0, 0, dev=False)["probs"]              # pre-dropout: the same for every step
    out = {"dqkv": torch.full((2 * B, 1536), FILL, dtype=qkv.dtype, device=DEV)}
    args = (qkv.data_ptr(), dobar.data_ptr(), probs.data_ptr(), out["dqkv"].data_ptr(), B, int(compute == "fp32"), training, p, SEED, offset, stream())
    if dev:
        _lib.check(lib.mmdeer_trimodal_attn_bwd_dev(*args, None if counter is None else counter.data_ptr()))
    else:
        _lib.check(lib.mmdeer_trimodal_attn_bwd(*args))
    torch.cuda.synchronize()
    return out


def same(got, want, what):
    assert set(got) == set(want), what
    for k in want:
        assert torch.equal(got[k], want[k]), f"{what}: {k} differs in {int((got[k] != want[k]).sum())} of {got[k].numel()} elements"


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("run", [attn_fwd, attn_bwd], ids=["fwd", "bwd"])
def test_attention_counter_plus_offset_is_the_plain_entry_at_the_sum(run, B, compute):
    seen = {}
    for a, b in PAIRS:
        c = counter_of(b)
        got = run(B, compute, 0.3, 1, a, c)
        assert int(c) == b, "the call wrote the counter"
        step = (a + b) % 2 ** 64
        want = seen.setdefault(step, run(B, compute, 0.3, 1, step, dev=False))
        same(got, want, f"offset {a} + counter {b}")
        for k, v in got.items():
            assert not bool((v.float() == FILL).all()), f"{k} was not written"
    first = "obar" if run is attn_fwd else "dqkv"
    steps = sorted(seen)
    assert steps == [0, 3, 5, 7]
    # B = 1 has 32 decisions per step at p = 0.3: four steps that all agree would be a frozen step, not chance (0.58^32 per pair)
    assert len({seen[s][first].float().cpu().numpy().tobytes() for s in steps}) > 1, "the step does not reach the masks"
    same(run(B, compute, 0.3, 1, 5, None), seen[5], "a NULL counter")


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("run", [attn_fwd, attn_bwd], ids=["fwd", "bwd"])
def test_attention_without_dropout_does_not_depend_on_the_counter(run, B, compute):
    c = counter_of(9)
    same(run(B, compute, 0.0, 1, 3, c), run(B, compute, 0.0, 1, 3, dev=False), "p = 0")
    same(run(B, compute, 0.3, 0, 3, c), run(B, compute, 0.3, 0, 3, dev=False), "training = 0")
    same(run(B, compute, 0.3, 0, 3, c), run(B, compute, 0.0, 1, 8, dev=False), "training = 0 is p = 0")
    assert int(c) == 9


def test_a_misaligned_counter_is_refused_before_any_launch():
    lib = _lib.load()
    c = torch.zeros(2, dtype=torch.int64, device=DEV)
    bad = c.data_ptr() + 4
    m = torch.full((3, 40), 9, dtype=torch.uint8, device=DEV)
    assert lib.mmdeer_dropout_mask_dev(113, 3, 40, 0.3, SEED, 0, m.data_ptr(), stream(), bad) == -1
    assert "offset_dev must be 8-byte aligned" in lib.mmdeer_last_error().decode()
    qkv, dobar = attn_inputs(3, "fp32")
    obar, probs, dqkv = torch.full((3, 512), FILL, device=DEV), torch.full((3, 8, 4), FILL, device=DEV), torch.full((6, 1536), FILL, device=DEV)
    assert lib.mmdeer_trimodal_attn_fwd_dev(qkv.data_ptr(), obar.data_ptr(), probs.data_ptr(), None, None, 3, 1, 1, 0.3, SEED, 0, stream(), bad) == -1
    assert "offset_dev must be 8-byte aligned" in lib.mmdeer_last_error().decode()
    assert lib.mmdeer_trimodal_attn_bwd_dev(qkv.data_ptr(), dobar.data_ptr(), probs.data_ptr(), dqkv.data_ptr(), 3, 1, 1, 0.3, SEED, 0, stream(), bad) == -1
    assert "offset_dev must be 8-byte aligned" in lib.mmdeer_last_error().decode()
    torch.cuda.synchronize()
    assert bool((m == 9).all()) and bool((obar == FILL).all()) and bool((probs == FILL).all()) and bool((dqkv == FILL).all())
