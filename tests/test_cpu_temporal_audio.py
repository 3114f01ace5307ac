"""The temporal audio encoder without a GPU: the float64 restatement (tests/temporal_ref.py) against the golden vectors
captured from the reference (tests/golden/audio_seq.npz), the state_dict contract, and every refusal of the new C entry
points and of the module that is decided on the host."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from mmdeer import _lib, side, synth, temporal

from . import temporal_ref as R
from .test_oracle_golden import check_side_grads, side_shapes

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "audio_seq.npz")
CASES = [(9, 2), (5, 5), (3, 33)]


def _state(tag):
    return {k: torch.from_numpy(v).double() for k, v in synth.module_fill(tag, side_shapes("aenc")).items()}


@pytest.mark.parametrize("B,T", CASES)
def test_restatement_reproduces_the_reference_capture(B, T):
    g = np.load(GOLDEN)
    tag = f"seq{B}x{T}"
    P = {k: v.requires_grad_(True) for k, v in _state(tag).items()}
    x = torch.from_numpy(g[f"{tag}.input"]).double().requires_grad_(True)
    y, lstm_out, a = R.encoder(P, x)
    np.testing.assert_allclose(y.detach().numpy(), g[f"{tag}.out"], rtol=1e-4, atol=5e-6)
    np.testing.assert_allclose(lstm_out.detach().numpy(), g[f"{tag}.lstm_out"], rtol=1e-4, atol=5e-6)
    np.testing.assert_allclose(a.detach().numpy(), g[f"{tag}.attn"], rtol=1e-4, atol=5e-6)
    (y * torch.from_numpy(g[f"{tag}.loss_w"]).double()).sum().backward()
    check_side_grads(g, tag, {k: v.grad for k, v in P.items()}, {"audio": x.grad}, rtol=3e-4, atol_frac=3e-5)
    # b2 shifts every score equally: its exact gradient is zero, the reference's value is rounding noise
    assert abs(float(P["attention.2.bias"].grad)) <= 1e-12
    assert abs(float(g[f"{tag}.gradnoise.attention.2.bias"].reshape(-1)[0])) <= 1e-4 * float(np.abs(g[f"{tag}.grad.attention.2.weight"]).max())


def test_restatement_layer_equals_torch_lstm():
    torch.manual_seed(0)
    lstm = torch.nn.LSTM(84, R.H, num_layers=2, bidirectional=True, batch_first=True).double()
    x = torch.randn(3, 6, 84, dtype=torch.float64)
    P = dict(lstm.named_parameters())
    h = R.lstm_layer(R.lstm_layer(x, P, 0), P, 1)
    torch.testing.assert_close(h, lstm(x)[0], rtol=1e-12, atol=1e-12)


def test_state_dict_matches_the_reference_and_the_parent():
    m = temporal.TemporalAudioEncoder()
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == side_shapes("aenc")
    p = side.EnhancedAudioEncoder()
    p.load_state_dict(m.state_dict(), strict=True)
    m.load_state_dict(p.state_dict(), strict=True)


A = 1 << 20     # a plausible, aligned address: never dereferenced by the host checks


def _seq(**kw):
    a = _lib.LstmSeqArgs()
    a.xg, a.ld_xg, a.w_hh, a.w_hh_t, a.h, a.ld_h = A, 2048, A, A, A, 512
    a.tape_gates, a.tape_c, a.dh_out, a.ld_dh, a.dgates, a.ld_dg = A, A, A, 512, A, 2048
    a.T, a.B, a.hidden, a.ndir, a.act_f32 = 4, 8, 256, 2, 0
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _pool(**kw):
    a = _lib.TemporalPoolArgs()
    a.h, a.ld_h, a.z, a.ld_z, a.w2, a.b2, a.attended, a.ld_att, a.weights = A, 512, A, 256, A, A, A, 512, A
    a.dout, a.ld_dout, a.dh, a.ld_dh, a.dz, a.ld_dz, a.dw2, a.db2, a.scratch = A, 512, A, 512, A, 256, A, A, A
    a.T, a.B, a.hidden, a.act_f32 = 4, 8, 256, 0
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("op", ["mmdeer_lstm_seq_fwd", "mmdeer_lstm_seq_bwd"])
def test_recurrence_operators_refuse_on_the_host(op):
    lib = _lib.load()
    f = getattr(lib, op)
    bwd = op.endswith("bwd")
    for kw, msg in [({"hidden": 128}, b"hidden"), ({"ndir": 1}, b"ndir"),
                    ({"dh_out" if bwd else "xg": None}, b"NULL"), ({"w_hh_t" if bwd else "w_hh": None}, b"NULL"),
                    ({"ld_dh" if bwd else "ld_h": 256}, b"leading"), ({"ld_dg" if bwd else "ld_xg": 1024}, b"leading"),
                    ({"dgates" if bwd else "h": A + 2}, b"misaligned"), ({"tape_c": A + 4}, b"misaligned"),
                    ({"ld_dh" if bwd else "ld_h": 516}, b"misaligned")]:
        assert f(C.byref(_seq(**kw))) != 0, kw
        assert msg in lib.mmdeer_last_error(), (kw, lib.mmdeer_last_error())
    for kw in ({"B": 0}, {"T": 0}):
        assert f(C.byref(_seq(xg=None, w_hh=None, w_hh_t=None, h=None, dh_out=None, dgates=None, **kw))) == 0
    assert f(None) != 0
    assert lib.mmdeer_lstm_seq_pack(A, A, 128, A, A, 0, None) != 0 and b"hidden" in lib.mmdeer_last_error()
    assert lib.mmdeer_lstm_seq_pack(None, A, 256, A, A, 0, None) != 0 and b"NULL" in lib.mmdeer_last_error()


@pytest.mark.parametrize("op", ["mmdeer_temporal_pool_fwd", "mmdeer_temporal_pool_bwd"])
def test_pool_operators_refuse_on_the_host(op):
    lib = _lib.load()
    f = getattr(lib, op)
    bwd = op.endswith("bwd")
    for kw, msg in [({"hidden": 128}, b"hidden"), ({"h": None}, b"NULL"), ({"dz" if bwd else "attended": None}, b"NULL"),
                    ({"ld_h": 256}, b"leading"), ({"ld_dz" if bwd else "ld_att": 128}, b"leading"),
                    ({"z": A + 8}, b"misaligned"), ({"dh" if bwd else "attended": A + 2}, b"misaligned")]:
        assert f(C.byref(_pool(**kw))) != 0, kw
        assert msg in lib.mmdeer_last_error(), (kw, lib.mmdeer_last_error())
    for kw in ({"B": 0}, {"T": 0}):
        assert f(C.byref(_pool(h=None, z=None, attended=None, dz=None, **kw))) == 0
    assert f(None) != 0


def test_module_input_errors():
    m = temporal.TemporalAudioEncoder()
    with pytest.raises(ValueError):
        m(torch.zeros(2, 3, 4, 84))
    with pytest.raises(NotImplementedError):
        m(torch.zeros(2, 5, 40))
    with pytest.raises(NotImplementedError):
        temporal.TemporalAudioEncoder({"hidden_dim": 256})(torch.zeros(2, 5, 84))
    with pytest.raises(NotImplementedError):
        temporal.TemporalAudioEncoder({"bidirectional": False})
    with pytest.raises(RuntimeError):
        m(torch.zeros(2, 5, 84))          # no CPU fallback
