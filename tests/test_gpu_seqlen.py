"""Per-sample lengths of the temporal audio encoder on the GPU (include/mmdeer_seqlen.h; mmdeer.temporal ``lengths=``): the recurrence
and pool operators against the float64 per-sample definition (tests/seqlen_ref.py), full lengths against the plain path bit for bit,
each sample against itself alone, padding invariance, the whole module with live dropout against float64 on the same masks, the
captured training step replayed with other lengths, and EndToEndDEER with ``audio_lengths``.

Shapes sit at the tile edges of the recurrence (csrc/lstm_seq.hip: SeqCfg): B = 1 (one partial tile), 17 (past the fp32 tile of 16
rows), 37 (past the bf16 tile of 32, a partial second workgroup); T = 2, 7, 33.  Length patterns: all T; all 1; random in [1, T];
two empty samples; an int64 device tensor holding T + 5 and -2 (the kernels clamp); and at B = 37 a short first bf16 workgroup (rows
0..31 at most 3 steps, rows 32..36 full -- the fp32 workgroups straddle).

The bounds are those of the unpadded tests, restated here: the operator bounds of tests/test_gpu_temporal_audio.py (fp32 relative l2
1e-4; bf16 at most twice the bf16 emulation's own distance + 1e-6; pool 1e-5 / 1e-4 in fp32 and 1e-2 / 2e-2 in bf16), the module's
golden bounds (fp32 rtol 1e-3, atol 2e-5; bf16 rtol 1e-1, atol 8e-2) and the dropout-step bounds of this encoder (outputs as the
golden ones; gradients rtol 3e-3 with atol 3e-3 of the largest element; bf16 twice the emulation's distance + 1e-6)."""
import functools

import numpy as np
import pytest
import torch
from torch import nn

from mmdeer import _lib, encoders, fusions, head, side, synth, temporal
from mmdeer.model import HierarchicalMultimodalFusion
from mmdeer.optim import ModuleAdamW
from mmdeer.train_graph import capture_train_step

from . import seqlen_ref as S
from . import temporal_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(B, T) for B in (1, 17, 37) for T in (2, 7, 33)]
OUT_RTOL, OUT_ATOL = 1e-3, 2e-5              # the module's fp32 bounds of its golden test
BF16_RTOL, BF16_ATOL = 1e-1, 8e-2            # the a14 bf16 tolerance of the same test
G_RTOL, G_ATOL_FRAC = 3e-3, 3e-3             # gradients of the dropout-step tests
DROP_SEED, STEP, P_DROP = 11, 5, 0.3


def patterns(B, T):
    """{name: (what the caller passes, the effective lengths)}"""
    g = torch.Generator().manual_seed(100 * B + T)
    rnd = torch.randint(1, T + 1, (B,), generator=g).tolist()
    out = {"full": [T] * B, "ones": [1] * B, "random": rnd}
    if B >= 17:
        z = list(rnd)
        z[1], z[B - 1] = 0, 0
        out["two_empty"] = z
    if B == 37:
        out["short_workgroup"] = [min(T, 1 + (b % 3)) for b in range(32)] + [T] * 5
    res = {k: (torch.tensor(v, dtype=torch.int32, device=DEV), v) for k, v in out.items()}
    if B >= 17:
        raw = list(rnd)
        raw[0], raw[2], raw[B - 1] = T + 5, -2, T + 5
        res["clamp_int64"] = (torch.tensor(raw, dtype=torch.int64, device=DEV), [min(max(v, 0), T) for v in raw])
    return res


CASES = [(B, T, name) for B, T in SHAPES for name in ("full", "ones", "random", "two_empty", "short_workgroup", "clamp_int64")
         if (name in ("full", "ones", "random")) or (name in ("two_empty", "clamp_int64") and B >= 17) or (name == "short_workgroup" and B == 37)]


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _bt(v, T, B):
    """time-major rows (T * B, C) -> batch-first (B, T, C)"""
    return v.reshape(T, B, -1).transpose(0, 1)


def _padded(eff, T):
    """(B, T) bool: True at t >= n_b"""
    return torch.arange(T, device=DEV)[None, :] >= torch.tensor(eff, device=DEV)[:, None]


# ------------------------------------------------------------------------------------------------ 1. the recurrence operator
def _layer_params(seed):
    torch.manual_seed(seed)
    lstm = torch.nn.LSTM(84, R.H, num_layers=1, bidirectional=True, batch_first=True)
    with torch.no_grad():
        for n, p in lstm.named_parameters():
            p.uniform_(-0.12, 0.12)
    return lstm


def _layer_inputs(B, T):
    gen = torch.Generator().manual_seed(B * 7 + T)
    return torch.randn(B, T, 84, generator=gen).to(DEV), torch.randn(B, T, 2 * R.H, generator=gen).to(DEV)


@functools.lru_cache(None)
def _layer_ref(B, T, name, emulate):
    """the float64 definition (or its bf16 emulation), once per case for both compute dtypes"""
    lstm = _layer_params(1000 * T + B).to(DEV)
    x, gout = _layer_inputs(B, T)
    eff = patterns(B, T)[name][1]
    P = {n: p.detach().double().clone().requires_grad_(True) for n, p in lstm.named_parameters()}
    x64 = x.double().clone().requires_grad_(True)
    hr = S.lstm_layer_with_lengths(x64, P, 0, eff, emulate_bf16=emulate)
    (hr * gout.double()).sum().backward()
    out = {"h": hr.detach().cpu(), "dx": x64.grad.cpu()}
    out.update({n: p.grad.cpu() for n, p in P.items()})
    return out


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
@pytest.mark.parametrize("B,T,name", CASES)
def test_recurrence_operator_with_lengths_matches_float64(B, T, name, compute):
    lstm = _layer_params(1000 * T + B).to(DEV)
    x, gout = _layer_inputs(B, T)                     # gout is non-zero at the padded steps too: the kernel must not read it there
    given, eff = patterns(B, T)[name]
    xt = x.transpose(0, 1).reshape(T * B, 84).clone().requires_grad_(True)
    h = temporal.lstm_layer(xt, lstm, 0, T, B, compute, given)
    (h.float() * gout.transpose(0, 1).reshape(T * B, -1)).sum().backward()
    hip = {"h": _bt(h.detach().float(), T, B), "dx": _bt(xt.grad, T, B)}
    hip.update({n: p.grad.clone() for n, p in lstm.named_parameters()})
    pad = _padded(eff, T)
    assert int(torch.count_nonzero(hip["h"][pad])) == 0 and int(torch.count_nonzero(hip["dx"][pad])) == 0
    assert all(bool(torch.isfinite(v).all()) for v in hip.values())
    r64 = _layer_ref(B, T, name, False)
    figs = {}
    if compute == "fp32":
        for k, v in r64.items():
            figs[k] = (_rel(hip[k], v), 1e-4)
    else:
        emu = _layer_ref(B, T, name, True)
        for k, v in r64.items():
            figs[k] = (_rel(hip[k], v), 2 * _rel(emu[k], v) + 1e-6)
    print(f"B={B} T={T} {name} {compute}: " + ", ".join(f"{k} {d:.2e} (bound {b:.2e})" for k, (d, b) in figs.items()))
    for k, (d, b) in figs.items():
        assert d <= b, (k, d, b)


# ------------------------------------------------------------------------------------------------ 2. the pool operators
def _pool_case(B, T, given, eff, compute, seed):
    gen = torch.Generator().manual_seed(seed)
    dt = torch.float32 if compute == "fp32" else torch.bfloat16
    h = torch.randn(T * B, 2 * R.H, generator=gen).to(dt).to(DEV)
    # ds_t = a_t (dout . h_t - sum_u a_u dout . h_u) is a weight times a difference: a sample whose scores lie far apart has tiny
    # weights, and fp32 leaves dz and dw2 few digits there.  In a batch such a sample is a small term of the norm; alone (B = 1) it is
    # all of it, so its scores are kept close together (tests/test_gpu_temporal_audio.py does the same for its B = 1 case).
    z = (torch.randn(T * B, R.H, generator=gen) * (0.1 if B == 1 else 0.5)).to(dt).to(DEV)
    # w2 at the scale the module initialises attention[2] with (xavier on a (1, 256) weight: deviation 0.088), so the scores are of
    # order 1.  The kernel evaluates each score twice (for the normaliser and for the weight), in fp32, and the two evaluations may
    # differ by an ulp of the SCORE; a weight's relative error is that absolute difference, so the 1e-6 bound on the row sums stands
    # for scores of order 1, not for any score.  First measured with 0.4 * randn (scores to +-8, ulp 9.5e-7): row sums off by up to
    # 1.12e-6 at T = 33 in fp32 and 1.004e-6 at B = 1029, T = 2 in bf16, at full lengths too, where the kernel stores the plain entry's
    # bits -- the plain kernel's own error at such scores, which no earlier test bounded.
    w2 = (torch.randn(1, R.H, generator=gen) * 0.1).to(DEV)
    b2 = torch.randn(1, generator=gen).to(DEV)
    gout = torch.randn(B, 2 * R.H, generator=gen).to(DEV)
    hr, zr, w2r, b2r = (t.detach().clone().requires_grad_(True) for t in (h, z, w2, b2))
    att, wts = temporal._TemporalPoolFn.apply(hr, zr, w2r, b2r, T, B, compute, temporal.as_lengths(given, B, T, DEV))
    (att * gout).sum().backward()
    # float64: h, z as the kernel read them
    h64, z64 = _bt(h.double(), T, B).clone().requires_grad_(True), _bt(z.double(), T, B).clone().requires_grad_(True)
    w64, b64 = w2.double().clone().requires_grad_(True), b2.double().clone().requires_grad_(True)
    att64, a64 = S.scores_pool_with_lengths(h64, z64, w64, b64, eff)
    (att64 * gout.double()).sum().backward()
    tol, tol_z = (1e-5, 1e-4) if compute == "fp32" else (1e-2, 2e-2)
    pad = _padded(eff, T)
    n = torch.tensor(eff, device=DEV)
    assert bool(torch.isfinite(att).all()) and bool(torch.isfinite(wts).all())
    assert int(torch.count_nonzero(wts[pad])) == 0
    off = float((wts.double().sum(1) - (n > 0).double()).abs().max())                # summed in float64: the kernel's error, not this sum's
    print(f"B={B} T={T} {compute}: weight rows sum to 1 (0 for an empty sample) within {off:.2e}")
    assert off <= 1e-6
    assert int(torch.count_nonzero(att[n == 0])) == 0
    dh, dz = _bt(hr.grad.float(), T, B), _bt(zr.grad.float(), T, B)
    assert int(torch.count_nonzero(dh[pad])) == 0 and int(torch.count_nonzero(dz[pad])) == 0
    figs = {"attended": (_rel(att, att64), tol), "weights": (_rel(wts, a64), tol), "dh": (_rel(dh, h64.grad), tol)}
    if bool(z64.grad.any()):                                                         # all lengths 1: the softmax has one term
        figs.update({"dz": (_rel(dz, z64.grad), tol_z), "dw2": (_rel(w2r.grad, w64.grad), tol_z)})
    else:
        # No sample has two steps, so the exact ds = a_0 (dout . h_0 - a_0 dout . h_0) is 0 and a relative distance has nothing to
        # stand on.  The kernel forms the 512-term fp32 dot product twice (once for the sum over steps, once per step); each evaluation
        # is within 512 * 2^-24 * sum_i |dout_i h_i| of the exact one whatever its order, so |ds_b| <= 2 * 512 * 2^-24 * that sum;
        # |dz| <= |ds| |w2| (|1 - tanh^2| <= 1; + 2^-7 for the bf16 store) and |dw2| <= sum_b |ds_b| (|tanh| <= 1).
        assert max(eff) <= 1
        ds_max = 2 * 512 * 2.0 ** -24 * (gout.to(dt).double() * h64.detach()[:, 0]).abs().sum(1)          # (B,)
        assert bool((dz[:, 0].double().abs() <= (1 + 2.0 ** -7) * ds_max[:, None] * w2.double().abs()).all())
        assert bool((w2r.grad.double().abs() <= ds_max.sum()).all())
    assert float(b2r.grad.abs().max()) == 0.0
    print(f"B={B} T={T} {compute}: " + ", ".join(f"{k} {d:.2e} (bound {b:.0e})" for k, (d, b) in figs.items()))
    for k, (d, b) in figs.items():
        assert d <= b, (k, d, b)


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
@pytest.mark.parametrize("B,T,name", CASES)
def test_pool_operators_with_lengths_match_float64(B, T, name, compute):
    given, eff = patterns(B, T)[name]
    _pool_case(B, T, given, eff, compute, B + 100 * T)


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_pool_backward_with_lengths_past_its_grid_cap(compute):
    """B = 1029 > 4 * 256: the backward's workgroups stride over the batch, the last round ragged; lengths 0, 1 and 2 mixed"""
    B, T = 1029, 2
    eff = [(b * 7 + b // 5) % 3 for b in range(B)]
    assert {0, 1, 2} == set(eff) and B > 4 * (_lib.TEMPORAL_POOL_SCRATCH // R.H)
    _pool_case(B, T, torch.tensor(eff, dtype=torch.int32, device=DEV), eff, compute, 4242)


# ------------------------------------------------------------------------------------------------ the module
def _encoder(compute, tag="seqlen", **cfg):
    m = temporal.TemporalAudioEncoder({"dropout": P_DROP, "dropout_seed": DROP_SEED, **cfg}, compute_dtype=compute)
    sd = synth.module_fill(tag, {k: tuple(v.shape) for k, v in m.state_dict().items()})
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.to(DEV)


def _train_run(m, x, lengths, w, step=STEP):
    m._train_step = step
    m.zero_grad(set_to_none=True)
    xr = x.clone().requires_grad_(True)
    y = m(xr) if lengths is None else m(xr, lengths)
    (y * w).sum().backward()
    return y.detach(), xr.grad, {n: p.grad.clone() for n, p in m.named_parameters()}


# ------------------------------------------------------------------------------------------------ 3. full lengths are the old path
@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_full_lengths_are_the_plain_path_bit_for_bit(compute):
    B, T = 37, 7
    gen = torch.Generator().manual_seed(31)
    x, w = torch.randn(B, T, 84, generator=gen).to(DEV), torch.randn(B, 512, generator=gen).to(DEV)
    full = torch.full((B,), T, dtype=torch.int32, device=DEV)
    m = _encoder(compute).eval()
    with torch.no_grad():
        assert torch.equal(m(x, full), m(x)) and torch.equal(m(x, lengths=[T] * B), m(x))
        assert torch.equal(m(x, full.long() + 3), m(x))                              # clamped to T
    m.train()
    y0, dx0, g0 = _train_run(m, x, None, w)
    y1, dx1, g1 = _train_run(m, x, full, w)
    assert m._train_step == STEP + 1
    assert torch.equal(y1, y0) and torch.equal(dx1, dx0)
    assert set(g1) == set(g0)
    for k in g0:
        assert torch.equal(g1[k], g0[k]), k


# ------------------------------------------------------------------------------------------------ 4. each sample alone
@pytest.mark.parametrize("compute", ["fp32", "bf16"])
@pytest.mark.parametrize("B,T,name", [(17, 7, "random"), (37, 7, "short_workgroup"), (17, 33, "two_empty")])
def test_each_row_is_its_sample_alone_at_its_own_length(B, T, name, compute):
    given, eff = patterns(B, T)[name]
    x = torch.randn(B, T, 84, generator=torch.Generator().manual_seed(B + T)).to(DEV)
    m = _encoder(compute).eval()
    rtol, atol = (OUT_RTOL, OUT_ATOL) if compute == "fp32" else (BF16_RTOL, BF16_ATOL)
    with torch.no_grad():
        y = m(x, given)
        assert bool(torch.isfinite(y).all())
        empty = [b for b, n in enumerate(eff) if n == 0]
        for b, n in enumerate(eff):
            if n > 0:                                # n = 1 runs the parent's one-step path: the same cell from zero state
                np.testing.assert_allclose(y[b].cpu().numpy(), m(x[b:b + 1, :n])[0].cpu().numpy(), rtol=rtol, atol=atol, err_msg=f"row {b}, n = {n}")
        if empty:                                    # an empty utterance: what output_projection makes of zeros, whatever x holds
            op = m.output_projection                 # (B zero rows: the same GEMM shape as the module's own call, so the same bits)
            z = fusions.linear(fusions.linear(torch.zeros(B, 512, device=DEV), op[0], compute, relu=True), op[3], compute)
            want = side._LayerNormFn.apply(z, op[4].weight, op[4].bias, compute)
            for b in empty:
                assert torch.equal(y[b], want[b]), b


# ------------------------------------------------------------------------------------------------ 5. padding invariance
@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_padding_invariance_forward_and_training(compute):
    B, T = 17, 7
    given, eff = patterns(B, T)["two_empty"]
    pad = _padded(eff, T)[..., None]
    gen = torch.Generator().manual_seed(77)
    x = torch.randn(B, T, 84, generator=gen).to(DEV)
    noise = torch.randn(B, T, 84, generator=gen).to(DEV)
    w = torch.randn(B, 512, generator=gen).to(DEV)
    nonfinite = torch.where(torch.arange(T * B * 84, device=DEV).reshape(B, T, 84) % 3 == 0, float("nan"),
                            torch.where(torch.arange(84, device=DEV) % 2 == 0, float("inf"), float("-inf")).expand(B, T, 84))
    assert int(pad.sum()) > 0
    m = _encoder(compute).eval()
    with torch.no_grad():
        y0 = m(torch.where(pad, 0.0, x), given)
        y1 = m(torch.where(pad, 1e4 * noise, x), given)
        y2 = m(torch.where(pad, nonfinite, x), given)
    assert bool(torch.isfinite(y0).all()) and torch.equal(y1, y0) and torch.equal(y2, y0)
    # training: any finite padding, the same dropout step
    m.train()
    ya, dxa, ga = _train_run(m, torch.where(pad, 0.0, x), given, w)
    yb, dxb, gb = _train_run(m, torch.where(pad, 100.0 * noise, x), given, w)
    assert torch.equal(yb, ya) and torch.equal(dxb, dxa)
    assert int(torch.count_nonzero(dxa[pad.expand_as(dxa)])) == 0 and float(dxa.abs().max()) > 0
    for k in ga:
        assert bool(torch.isfinite(ga[k]).all()) and torch.equal(gb[k], ga[k]), k


# ------------------------------------------------------------------------------------------------ 6. the module with live dropout
@functools.lru_cache(None)
def _module_ref(emulate):
    B, T = 17, 7
    eff = _module_lengths(B, T)
    m = _encoder("fp32")
    P = {k: v.detach().double().cpu().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    x, w = _module_inputs(B, T)
    x64 = x.double().cpu().clone().requires_grad_(True)
    masks = R.draw(R.sites(B, T, P_DROP), DROP_SEED, STEP)
    y, _, _ = S.encoder_with_lengths(P, x64, eff, masks=masks, emulate_bf16=emulate)
    (y * w.double().cpu()).sum().backward()
    return y.detach(), x64.grad, {k: v.grad for k, v in P.items()}


def _module_lengths(B, T):
    eff = patterns(B, T)["random"][1]
    eff[3], eff[5], eff[B - 1] = 0, 1, T
    return eff


def _module_inputs(B, T):
    gen = torch.Generator().manual_seed(5000 + B)
    return torch.randn(B, T, 84, generator=gen).to(DEV), torch.randn(B, 512, generator=gen).to(DEV)


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_training_step_with_lengths_matches_float64_on_the_same_masks(compute):
    B, T = 17, 7
    eff = _module_lengths(B, T)
    x, w = _module_inputs(B, T)
    m = _encoder(compute).train()
    y, dx, grads = _train_run(m, x, eff, w)                       # a Python list: checked on the host, uploaded
    assert m._train_step == STEP + 1
    y64, dx64, g64 = _module_ref(False)
    assert set(grads) == set(g64)
    assert float(grads["attention.2.bias"].abs().max()) == 0.0   # written as an exact zero
    assert int(torch.count_nonzero(dx[_padded(eff, T)])) == 0
    if compute == "fp32":
        np.testing.assert_allclose(y.cpu().numpy(), y64.numpy(), rtol=OUT_RTOL, atol=OUT_ATOL)
        for k, r in list(g64.items()) + [("input", dx64)]:
            if k == "attention.2.bias":
                assert float(r.abs().max()) <= 1e-4 * float(g64["attention.2.weight"].abs().max())
                continue
            have = dx if k == "input" else grads[k]
            assert bool(r.any()), k
            np.testing.assert_allclose(have.cpu().numpy(), r.numpy(), rtol=G_RTOL, atol=G_ATOL_FRAC * float(r.abs().max()), err_msg=k)
    else:
        ye, dxe, ge = _module_ref(True)
        rows = [("output", y, y64, ye), ("input", dx, dx64, dxe)]
        rows += [(k, grads[k], g64[k], ge[k]) for k in g64 if k not in ("attention.0.bias", "attention.2.bias")]   # cancelling sums; a zero
        fails = []
        for k, have, r, e in rows:
            d, own = _rel(have, r), _rel(e, r)
            print(f"{k}: {d:.3e} against the emulation's {own:.3e}")
            if not d <= 2 * own + 1e-6:
                fails.append((k, d, own))
        assert not fails, fails


# ------------------------------------------------------------------------------------------------ 7. graph replay
class _AudioModel(nn.Module):
    def __init__(self, compute):
        super().__init__()
        self.enc = temporal.TemporalAudioEncoder({"dropout_seed": 5}, compute)
        self.head = nn.Linear(512, 3)

    def forward(self, x, lengths, target):
        return nn.functional.mse_loss(self.head(self.enc(x, lengths)), target)


def _make_audio_model(compute, state=None):
    torch.manual_seed(3)
    m = _AudioModel(compute).to(DEV).train()
    if state is not None:
        m.load_state_dict(state)
    named = [(n, p) for n, p in m.named_parameters() if p.requires_grad]
    groups = [{"params": [p for n, p in named if p.ndim >= 2], "weight_decay": 0.01},
              {"params": [p for n, p in named if p.ndim < 2], "weight_decay": 0.0}]
    return m, ModuleAdamW.for_module(m, groups, lr=1e-3, capturable=True, max_grad_norm=1.0)


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_captured_step_replays_with_other_lengths(compute):
    B, T = 17, 7
    g = torch.Generator().manual_seed(90)
    data = []
    for i in range(3):
        n = torch.randint(0 if i == 2 else 1, T + 1, (B,), generator=g).to(torch.int32)
        data.append((torch.randn(B, T, 84, generator=g).to(DEV), n.to(DEV), torch.randn(B, 3, generator=g).to(DEV)))
    assert not torch.equal(data[0][1], data[1][1]) and not torch.equal(data[1][1], data[2][1])
    eager, eopt = _make_audio_model(compute)
    model, opt = _make_audio_model(compute, {k: v.detach().clone() for k, v in eager.state_dict().items()})
    replay = capture_train_step(model, opt, [t.clone() for t in data[0]])
    want = []
    for b in data:
        for p in eager.parameters():
            p.grad = None
        loss = eager(*b)
        loss.backward()
        eopt.step()
        want.append(loss.detach().clone())
    got = [replay(*b).clone() for b in data]
    torch.cuda.synchronize()
    for r, (a, b) in enumerate(zip(got, want)):
        assert bool(torch.isfinite(a)) and torch.equal(a, b), f"loss of step {r}: replay {float(a)!r}, eager {float(b)!r}"
    assert len({float(a.detach()) for a in got}) == 3
    es, ms = eager.state_dict(), model.state_dict()
    for k in es:
        assert torch.equal(ms[k], es[k]), k
    assert [int(t) for _, t in replay.counters] == [x._train_step for x in eager.modules() if hasattr(x, "set_step_counter")]


# ------------------------------------------------------------------------------------------------ 8. EndToEndDEER
def test_end_to_end_step_with_audio_lengths():
    B, L, T = 2, 5, 3

    def make():
        torch.manual_seed(3)
        enc = encoders.ModalityEncoder({"dropout_seed": 5}, "bf16")
        return encoders.EndToEndDEER(enc, HierarchicalMultimodalFusion(512, 512, 512, compute_dtype="bf16", seed=1),
                                     head.MultiDimensionalDEER(512, compute_dtype="bf16", seed=2)).to(DEV).train()
    g = torch.Generator().manual_seed(77)
    mask = torch.ones(B, L, dtype=torch.int64)
    mask[1, 3:] = 0
    batch = {"audio": torch.randn(B, T, 84, generator=g).to(DEV), "video": torch.randn(B, 2, 3, 16, 16, generator=g).to(DEV),
             "text_input_ids": torch.randint(1, 50, (B, L), generator=g).to(DEV), "text_attention_mask": mask.to(DEV)}
    targets = (torch.rand(B, 3, generator=g) * 2 - 1).to(DEV)

    def step(extra):
        m = make()
        out = m({**batch, **extra})
        loss = m.compute_loss(out, targets)["total_loss"]
        loss.backward()
        return loss.detach(), out["encoded_features"]["audio"].detach(), {n: p.grad for n, p in m.named_parameters()}
    loss, feat, grads = step({"audio_lengths": torch.tensor([T, 1], device=DEV)})
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(feat).all())
    audio = {n: v for n, v in grads.items() if n.startswith(("encoders.audio_encoder.lstm.", "encoders.audio_encoder.attention.",
                                                             "encoders.audio_encoder.output_projection.")) and not n.endswith("attention.2.bias")}
    assert len(audio) == 25 and all(v is not None and bool(torch.isfinite(v).all()) and float(v.abs().max()) > 0 for v in audio.values())
    assert all(v is None or bool(torch.isfinite(v).all()) for v in grads.values())
    plain_loss, plain_feat, plain_grads = step({})
    assert not torch.equal(feat[1], plain_feat[1]) and torch.equal(feat[0], plain_feat[0])       # row 1 is cut, row 0 is not
    full_loss, full_feat, full_grads = step({"audio_lengths": torch.full((B,), T, dtype=torch.int32, device=DEV)})
    assert torch.equal(full_loss, plain_loss) and torch.equal(full_feat, plain_feat)
    for n, v in plain_grads.items():
        assert (v is None and full_grads[n] is None) or torch.equal(full_grads[n], v), n
