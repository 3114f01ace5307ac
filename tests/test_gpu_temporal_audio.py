"""The temporal audio encoder (mmdeer.temporal) on the GPU: the recurrence and pool operators against the float64 restatement
(tests/temporal_ref.py), the whole encoder against the golden vectors captured from the reference (tests/golden/audio_seq.npz),
edges, training and HIP-graph capture."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from mmdeer import _lib, side, synth, temporal

from . import temporal_ref as R
from .test_oracle_golden import check_side_grads

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "audio_seq.npz")
CASES = [(9, 2), (5, 5), (3, 33)]


def _fill(module, tag):
    """The closed-form parameter fill of tests/golden/make_golden.py, keyed by state_dict name."""
    sd = synth.module_fill(tag, {k: tuple(v.shape) for k, v in module.state_dict().items()})
    module.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return module


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


# ------------------------------------------------------------------------------------------------ golden (reference capture)
@pytest.mark.parametrize("B,T", CASES)
def test_golden_fp32_outputs_and_gradients(B, T):
    g = np.load(GOLDEN)
    tag = f"seq{B}x{T}"
    m = _fill(temporal.TemporalAudioEncoder(compute_dtype="fp32"), tag).to(DEV).eval()
    x = torch.from_numpy(g[f"{tag}.input"]).to(DEV).requires_grad_(True)
    y = m(x)
    np.testing.assert_allclose(y.detach().cpu().numpy(), g[f"{tag}.out"], rtol=1e-3, atol=2e-5)
    (y * torch.from_numpy(g[f"{tag}.loss_w"]).to(DEV)).sum().backward()
    grads = {n: p.grad for n, p in m.named_parameters()}
    check_side_grads(g, tag, grads, {"audio": x.grad}, rtol=3e-3, atol_frac=3e-3)
    # the reference's attention.2.bias gradient is rounding noise: ours must be (near) zero against the weight's gradient
    assert abs(float(g[f"{tag}.gradnoise.attention.2.bias"].reshape(-1)[0])) <= 1e-4 * float(np.abs(g[f"{tag}.grad.attention.2.weight"]).max())
    assert float(grads["attention.2.bias"].abs().max()) <= 1e-4 * float(grads["attention.2.weight"].abs().max())


@pytest.mark.parametrize("B,T", CASES)
def test_golden_bf16_outputs_and_gradients_track_fp32(B, T):
    g = np.load(GOLDEN)
    tag = f"seq{B}x{T}"
    x = torch.from_numpy(g[f"{tag}.input"]).to(DEV)
    w = torch.from_numpy(g[f"{tag}.loss_w"]).to(DEV)
    res = {}
    for compute in ("fp32", "bf16"):
        m = _fill(temporal.TemporalAudioEncoder(compute_dtype=compute), tag).to(DEV).eval()
        y = m(x)
        if compute == "bf16" and T <= 5:
            np.testing.assert_allclose(y.detach().cpu().numpy(), g[f"{tag}.out"], rtol=1e-1, atol=8e-2)   # the a14 bf16 tolerance
        (y * w).sum().backward()
        res[compute] = {n: p.grad.double().flatten() for n, p in m.named_parameters()}
    for n, a in res["fp32"].items():
        # attention.2.bias: analytically zero in both.  attention.0.bias: the sum over steps of dz, whose terms cancel (the
        # softmax gradient sums to zero over the steps of a sample), so the bf16 rounding of h sets it at the tens-of-percent
        # level; test_golden_fp32_outputs_and_gradients pins it against the reference.
        if n in ("attention.2.bias", "attention.0.bias"):
            continue
        b = res["bf16"][n]
        assert float((a @ b) / (a.norm() * b.norm())) > 0.97, n


# ------------------------------------------------------------------------------------------------ the recurrence operator
def _layer_params(seed):
    torch.manual_seed(seed)
    lstm = torch.nn.LSTM(84, R.H, num_layers=1, bidirectional=True, batch_first=True)
    with torch.no_grad():
        for n, p in lstm.named_parameters():
            p.uniform_(-0.12, 0.12)
    return lstm


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
@pytest.mark.parametrize("T", [1, 2, 7, 33])
@pytest.mark.parametrize("B", [1, 37, 1027, 4096])
def test_recurrence_operator_matches_float64(B, T, compute):
    lstm = _layer_params(1000 * T + B).to(DEV)
    gen = torch.Generator().manual_seed(B * 7 + T)
    x = torch.randn(B, T, 84, generator=gen).to(DEV)
    gout = torch.randn(B, T, 2 * R.H, generator=gen).to(DEV)
    # HIP: time-major rows through mmdeer.temporal.lstm_layer (input GEMM + one recurrence launch)
    xt = x.transpose(0, 1).reshape(T * B, 84).clone().requires_grad_(True)
    h = temporal.lstm_layer(xt, lstm, 0, T, B, compute)
    (h.float() * gout.transpose(0, 1).reshape(T * B, -1)).sum().backward()
    hip = {"h": h.detach().float().reshape(T, B, -1).transpose(0, 1), "dx": xt.grad.reshape(T, B, -1).transpose(0, 1)}
    hip.update({n: p.grad.clone() for n, p in lstm.named_parameters()})
    # float64 restatement (and its bf16 emulation) on the same device
    def ref(emulate):
        P = {n: p.detach().double().clone().requires_grad_(True) for n, p in lstm.named_parameters()}
        x64 = x.double().clone().requires_grad_(True)
        hr = R.lstm_layer(x64, P, 0, emulate_bf16=emulate)
        (hr * gout.double()).sum().backward()
        out = {"h": hr.detach(), "dx": x64.grad}
        out.update({n: p.grad for n, p in P.items()})
        return out
    r64 = ref(False)
    if compute == "fp32":
        for k, v in r64.items():
            assert _rel(hip[k], v) <= 1e-4, (k, _rel(hip[k], v))
    else:
        emu = ref(True)
        for k, v in r64.items():
            assert _rel(hip[k], v) <= 2 * _rel(emu[k], v) + 1e-6, (k, _rel(hip[k], v), _rel(emu[k], v))
    if T == 1:                                    # one step from zero state: the T = 1 cell kernel on the same gates
        lib = _lib.load()
        dt = torch.float32 if compute == "fp32" else torch.bfloat16
        with torch.no_grad():
            w = torch.cat([lstm.weight_ih_l0, lstm.weight_ih_l0_reverse]).to(dt)
            b = torch.cat([lstm.bias_ih_l0 + lstm.bias_hh_l0, lstm.bias_ih_l0_reverse + lstm.bias_hh_l0_reverse])
            xg = (x[:, 0].to(dt).float() @ w.float().t() + b).to(dt).contiguous()
            hs = temporal._LstmSeqFn.apply(xg, lstm.weight_hh_l0, lstm.weight_hh_l0_reverse, 1, B, compute)
            h1 = torch.empty(B, 2 * R.H, dtype=dt, device=DEV)
            _lib.check(lib.mmdeer_lstm_cell_t1(xg.data_ptr(), xg.shape[1], h1.data_ptr(), 2 * R.H, B, R.H, 2, int(compute == "fp32"),
                                               _lib.current_stream()))
        assert torch.equal(hs, h1)


# ------------------------------------------------------------------------------------------------ the pool operators
@pytest.mark.parametrize("compute", ["fp32", "bf16"])
@pytest.mark.parametrize("T", [1, 2, 33])
@pytest.mark.parametrize("B", [5, 37])
def test_pool_operators_match_float64(B, T, compute):
    gen = torch.Generator().manual_seed(B + 100 * T)
    dt = torch.float32 if compute == "fp32" else torch.bfloat16
    h = torch.randn(T * B, 2 * R.H, generator=gen).to(dt).to(DEV)
    z = torch.randn(T * B, R.H, generator=gen).to(dt).to(DEV)
    w2 = (torch.randn(1, R.H, generator=gen) * 0.4).to(DEV)
    b2 = torch.randn(1, generator=gen).to(DEV)
    if T > 1:   # sample 0: scores +-sum|w2| (about +-80), alternating between steps (the softmax must subtract the max)
        zz = z.float().reshape(T, B, -1)
        sign = torch.tensor([1.0 if t % 2 else -1.0 for t in range(T)], device=DEV)
        zz[:, 0, :] = 20.0 * sign[:, None] * torch.sign(w2)
        z = zz.reshape(T * B, -1).to(dt).contiguous()
    hr, zr, w2r, b2r = (t.detach().clone().requires_grad_(True) for t in (h, z, w2, b2))
    att, wts = temporal._TemporalPoolFn.apply(hr, zr, w2r, b2r, T, B, compute)
    gout = torch.randn(B, 2 * R.H, generator=gen).to(DEV)
    (att * gout).sum().backward()
    # float64: h, z as the kernel read them
    h64, z64 = h.double().reshape(T, B, -1).transpose(0, 1).clone().requires_grad_(True), z.double().reshape(T, B, -1).transpose(0, 1).clone().requires_grad_(True)
    w64, b64 = w2.double().clone().requires_grad_(True), b2.double().clone().requires_grad_(True)
    s = (torch.tanh(z64) @ w64.t() + b64)[..., 0]
    a = torch.softmax(s, dim=1)
    att64 = (a.unsqueeze(-1) * h64).sum(1)
    (att64 * gout.double()).sum().backward()
    tol = 1e-5 if compute == "fp32" else 1e-2
    assert torch.isfinite(att).all() and torch.isfinite(wts).all()
    assert _rel(att, att64) <= tol and _rel(wts, a) <= tol
    assert _rel(hr.grad.float().reshape(T, B, -1).transpose(0, 1), h64.grad) <= tol
    if T > 1:
        assert _rel(zr.grad.float().reshape(T, B, -1).transpose(0, 1), z64.grad) <= (1e-4 if compute == "fp32" else 2e-2)
        assert _rel(w2r.grad, w64.grad) <= (1e-4 if compute == "fp32" else 2e-2)
    assert float(b2r.grad.abs().max()) == 0.0       # written as an exact zero (the reference's value is rounding noise)


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
@pytest.mark.parametrize("B", [1, 1024, 1029])
def test_pool_backward_past_its_grid_cap_and_the_fold(B, compute):
    """The backward runs at most `cap` workgroups of four samples and strides over the batch beyond them.  B = 1: one workgroup, three
    idle waves; B = 1024: exactly the cap; B = 1029: the stride runs and its last round is ragged (sample 1028 alone).  Same float64
    restatement and bounds as test_pool_operators_match_float64; and dw2 must be the workgroups' partials, read back from the
    caller's scratch buffer, added in index order in fp32 -- bit for bit -- with db2 = +0.0."""
    T, W = 2, R.H
    cap = _lib.TEMPORAL_POOL_SCRATCH // W
    nparts = min((B + 3) // 4, cap)
    gen = torch.Generator().manual_seed(B + 100 * T)
    dt = torch.float32 if compute == "fp32" else torch.bfloat16
    h = torch.randn(T * B, 2 * R.H, generator=gen).to(dt).to(DEV)
    z = torch.randn(T * B, R.H, generator=gen)
    w2 = (torch.randn(1, R.H, generator=gen) * 0.4).to(DEV)
    b2 = torch.randn(1, generator=gen).to(DEV)
    if B > 1:   # sample 0: scores about -+80, as in the test above
        z.reshape(T, B, -1)[:, 0, :] = 20.0 * torch.tensor([-1.0, 1.0])[:, None] * torch.sign(w2.cpu())
    else:
        # Alone in the batch a sample has to carry the relative bounds itself.  ds_t = a_t (dout . h_t - sum_u a_u dout . h_u) is
        # a_0 a_1 times a difference for T = 2: with z ~ N(0, 1) the two scores are some 9 apart (w2 . tanh z has deviation 5), a_0
        # is 1e-4 and fp32 leaves dz and dw2 three digits -- in a batch such a sample is a small term of the norm, here it would be
        # all of it.  A tenth of the spread keeps both weights between 0.1 and 0.9.
        z *= 0.1
    z = z.to(dt).to(DEV)
    gout = torch.randn(B, 2 * R.H, generator=gen).to(DEV)
    with torch.no_grad():
        _, wts = temporal._TemporalPoolFn.apply(h, z, w2, b2, T, B, compute)
    dout = gout.to(dt).contiguous()
    dh, dz = torch.full_like(h, float("nan")), torch.full_like(z, float("nan"))
    dw2, db2 = torch.full((W,), float("nan"), device=DEV), torch.full((1,), -1.0, device=DEV)
    scratch = torch.full((_lib.TEMPORAL_POOL_SCRATCH,), float("nan"), device=DEV)
    w2f = w2.reshape(-1).contiguous()
    a = _lib.TemporalPoolArgs()
    a.h, a.ld_h, a.z, a.ld_z, a.w2, a.weights = h.data_ptr(), 2 * R.H, z.data_ptr(), R.H, w2f.data_ptr(), wts.data_ptr()
    a.dout, a.ld_dout, a.dh, a.ld_dh, a.dz, a.ld_dz = dout.data_ptr(), 2 * R.H, dh.data_ptr(), 2 * R.H, dz.data_ptr(), R.H
    a.dw2, a.db2, a.scratch = dw2.data_ptr(), db2.data_ptr(), scratch.data_ptr()
    a.T, a.B, a.hidden, a.act_f32, a.stream = T, B, R.H, int(compute == "fp32"), _lib.current_stream()
    _lib.check(_lib.load().mmdeer_temporal_pool_bwd(C.byref(a)))
    # float64: h, z as the kernel read them
    bt = lambda t: t.double().reshape(T, B, -1).transpose(0, 1)                      # noqa: E731
    h64, z64 = bt(h).clone().requires_grad_(True), bt(z).clone().requires_grad_(True)
    w64 = w2.double().clone().requires_grad_(True)
    s = (torch.tanh(z64) @ w64.t() + b2.double())[..., 0]
    ((torch.softmax(s, dim=1).unsqueeze(-1) * h64).sum(1) * gout.double()).sum().backward()
    assert all(torch.isfinite(t.grad).all() for t in (h64, z64, w64))
    tol, tol_z = (1e-5, 1e-4) if compute == "fp32" else (1e-2, 2e-2)
    figs = {"dh": (_rel(bt(dh), h64.grad), tol), "dz": (_rel(bt(dz), z64.grad), tol_z), "dw2": (_rel(dw2, w64.grad[0]), tol_z)}
    print(f"B={B} {compute} nparts={nparts}: " + ", ".join(f"{k} {d:.3e} (bound {b:.0e})" for k, (d, b) in figs.items()))
    for k, (d, b) in figs.items():
        assert d <= b, (k, d, b)
    # the fold: the partials in index order from zero, one column per thread
    parts = scratch.cpu().numpy().reshape(cap, W)
    assert np.isfinite(parts[:nparts]).all() and np.isnan(parts[nparts:]).all()
    acc = np.zeros(W, np.float32)
    for p in range(nparts):
        acc = acc + parts[p]
    assert acc.dtype == np.float32 and np.array_equal(acc.view(np.uint32), dw2.cpu().numpy().view(np.uint32))
    assert db2.cpu().numpy().view(np.uint32)[0] == 0                                 # +0.0


def test_pool_operators_empty_batch():
    lib = _lib.load()
    a = _lib.TemporalPoolArgs()
    a.T, a.B, a.hidden, a.act_f32, a.stream = 4, 0, 256, 1, _lib.current_stream()
    assert lib.mmdeer_temporal_pool_fwd(C.byref(a)) == 0 and lib.mmdeer_temporal_pool_bwd(C.byref(a)) == 0
    m = temporal.TemporalAudioEncoder().to(DEV).eval()
    y = m(torch.zeros(0, 6, 84, device=DEV))
    assert tuple(y.shape) == (0, 512)


# ------------------------------------------------------------------------------------------------ edges
@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_one_step_equals_the_parent_and_eval_is_deterministic(compute):
    torch.manual_seed(3)
    m = temporal.TemporalAudioEncoder(compute_dtype=compute).to(DEV).eval()
    p = side.EnhancedAudioEncoder(compute_dtype=compute).to(DEV).eval()
    p.load_state_dict(m.state_dict(), strict=True)
    x = torch.randn(17, 1, 84, device=DEV)
    assert torch.equal(m(x), p(x))
    assert torch.equal(m(x[:, 0]), p(x[:, 0]))
    xs = torch.randn(17, 6, 84, device=DEV)
    with torch.no_grad():
        assert torch.equal(m(xs), m(xs))
    with pytest.raises(RuntimeError):
        m.cpu()(torch.randn(2, 5, 84))


# ------------------------------------------------------------------------------------------------ training
def test_training_dropout_gradients_and_sgd():
    torch.manual_seed(5)
    m = temporal.TemporalAudioEncoder({"dropout_seed": 11}, compute_dtype="fp32").to(DEV).train()
    x = torch.randn(64, 8, 84, device=DEV)
    with torch.no_grad():
        assert not torch.equal(m(x), m(x))          # the step counter moves the masks
    target = torch.randn(64, 512, device=DEV) * 0.5
    losses = []
    opt = torch.optim.SGD(m.parameters(), lr=0.05)
    for it in range(10):
        opt.zero_grad()
        loss = (m(x) - target).square().mean()
        loss.backward()
        losses.append(float(loss))
        for n, p in m.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all(), n
            if it == 0 and n != "attention.2.bias" and ("weight_hh" in n or n.startswith("attention.") or "bias" in n):
                assert float(p.grad.abs().max()) > 0, n
        opt.step()
    assert losses[-1] < losses[0], losses


# ------------------------------------------------------------------------------------------------ HIP graph capture
@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_graph_capture_replays_eager(compute):
    torch.manual_seed(9)
    m = temporal.TemporalAudioEncoder(compute_dtype=compute).to(DEV).eval()
    x = torch.randn(256, 8, 84, device=DEV)
    w = torch.randn(256, 512, device=DEV)

    def step():
        for p in m.parameters():
            p.grad = None
        y = m(x)
        (y * w).sum().backward()
        return y.detach().clone(), [p.grad.detach().clone() for p in m.parameters()]

    y0, g0 = step()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()                                        # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    for p in m.parameters():
        p.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = m(x)
        (y * w).sum().backward()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, y0)
    for p, g in zip(m.parameters(), g0):
        assert torch.equal(p.grad, g)
