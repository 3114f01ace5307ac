"""Per-sample lengths of the temporal audio encoder without a GPU: the per-sample definition (tests/seqlen_ref.py) against torch's own
pack_padded_sequence -> nn.LSTM -> pad_packed_sequence chain with a -inf-masked softmax pool, in float64; include/mmdeer_seqlen.h
through the strict parser, its struct layouts, exported symbols and every host refusal of the four entries; the host checks of
``TemporalAudioEncoder.forward(x, lengths)``; and ``ModalityEncoder``'s ``audio_lengths`` key."""
import ctypes as C
import os

import pytest
import torch
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

from mmdeer import _header, _lib, build, encoders, temporal

from . import seqlen_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, T, LENGTHS = 5, 7, [7, 1, 4, 7, 2]


# ------------------------------------------------------------------------------------------------ the definition against torch
def _torch_chain(m, x, lengths):
    """torch's packed-sequence chain on the module's own nn.LSTM / attention / output_projection (float64, evaluation mode)"""
    n = torch.tensor(lengths)
    packed = pack_padded_sequence(x, n, batch_first=True, enforce_sorted=False)
    h, _ = pad_packed_sequence(m.lstm(packed)[0], batch_first=True, total_length=x.shape[1])
    s = m.attention[2](torch.tanh(m.attention[0](h)))[..., 0]
    s = s.masked_fill(torch.arange(x.shape[1])[None, :] >= n[:, None], float("-inf"))
    a = torch.softmax(s, dim=1)
    return m.output_projection((a.unsqueeze(-1) * h).sum(1)), h, a


def test_per_sample_definition_is_torchs_packed_sequence_chain():
    torch.manual_seed(7)
    m = temporal.TemporalAudioEncoder().double().eval()
    x = torch.randn(B, T, 84, dtype=torch.float64)
    w = torch.randn(B, 512, dtype=torch.float64)
    xt = x.clone().requires_grad_(True)
    yt, ht, at = _torch_chain(m, xt, LENGTHS)
    (yt * w).sum().backward()
    P = {k: v.detach().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    xr = x.clone().requires_grad_(True)
    yr, hr, ar = S.encoder_with_lengths(P, xr, LENGTHS)
    (yr * w).sum().backward()

    def rel(a, b):
        return float((a.detach() - b.detach()).norm() / b.detach().norm())
    assert rel(yr, yt) <= 1e-10 and rel(hr, ht) <= 1e-10 and rel(ar, at) <= 1e-10
    assert rel(xr.grad, xt.grad) <= 1e-10
    for b, n in enumerate(LENGTHS):                  # pad_packed_sequence's zeros, and nothing comes back to the padding
        assert not hr[b, n:].any() and not ht[b, n:].any() and not ar[b, n:].any() and not xr.grad[b, n:].any() and not xt.grad[b, n:].any()
    grads = dict(m.named_parameters())
    assert set(grads) == set(P)
    for k, p in grads.items():
        if k == "attention.2.bias":                  # a shift of every score of a sample: exactly nothing, rounding noise in both
            assert float(p.grad.abs().max()) <= 1e-12 and float(P[k].grad.abs().max()) <= 1e-12
            continue
        assert rel(P[k].grad, p.grad) <= 1e-10, k


def test_definition_layer_and_pool_versions_and_the_empty_sample():
    torch.manual_seed(8)
    lstm = torch.nn.LSTM(84, S.H, num_layers=1, bidirectional=True, batch_first=True).double()
    x = torch.randn(4, 5, 84, dtype=torch.float64)
    lengths = [5, 0, 3, 1]
    P = dict(lstm.named_parameters())
    h = S.lstm_layer_with_lengths(x, P, 0, lengths)
    keep = [0, 2, 3]
    packed = pack_padded_sequence(x[keep], torch.tensor([5, 3, 1]), batch_first=True, enforce_sorted=False)
    ht, _ = pad_packed_sequence(lstm(packed)[0], batch_first=True, total_length=5)
    torch.testing.assert_close(h[keep], ht, rtol=1e-12, atol=1e-12)
    assert not h[1].any()
    z = torch.randn(4, 5, S.H, dtype=torch.float64)
    w2, b2 = torch.randn(1, S.H, dtype=torch.float64), torch.randn(1, dtype=torch.float64)
    att, a = S.scores_pool_with_lengths(h, z, w2, b2, lengths)
    assert not att[1].any() and not a[1].any()
    torch.testing.assert_close(a.sum(1), torch.tensor([1.0, 0.0, 1.0, 1.0], dtype=torch.float64))
    assert float(a[3, 0]) == 1.0 and torch.equal(att[3], h[3, 0])
    # the empty sample of the whole encoder: what output_projection makes of zeros, and no gradient through the LSTM or the pool
    m = temporal.TemporalAudioEncoder().double().eval()
    Pm = {k: v.detach().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    xe = x.clone().requires_grad_(True)
    y, _, _ = S.encoder_with_lengths(Pm, xe, [0, 0, 0, 0])
    torch.testing.assert_close(y, m.output_projection(torch.zeros(4, 512, dtype=torch.float64)), rtol=1e-12, atol=1e-12)
    y.sum().backward()
    assert torch.isfinite(y).all() and (xe.grad is None or not xe.grad.any())
    assert all(Pm[k].grad is None or not Pm[k].grad.any() for k in Pm if k.startswith(("lstm.", "attention.")))


# ------------------------------------------------------------------------------------------------ the header
SYMBOLS = {"mmdeer_lstm_seq_len_fwd": "LstmSeqLenArgs", "mmdeer_lstm_seq_len_bwd": "LstmSeqLenArgs",
           "mmdeer_temporal_pool_len_fwd": "TemporalPoolLenArgs", "mmdeer_temporal_pool_len_bwd": "TemporalPoolLenArgs"}
COUNTERPART = {"lstm_seq_len_args": "lstm_seq_args", "temporal_pool_len_args": "temporal_pool_args"}


def test_header_parses_strictly_and_the_four_symbols_are_exported():
    lib = _lib.load()
    assert _lib.ABI_VERSION == 16 and lib.mmdeer_abi_version() == 16               # additions only
    assert _header.SEQLEN_HEADER_PATH == build.SEQLEN_HEADER_PATH
    assert os.path.samefile(build.SEQLEN_HEADER_PATH, os.path.join(ROOT, "include", "mmdeer_seqlen.h"))
    got = {n: (res, args) for n, res, args in _lib.SEQLEN_SYMBOLS}
    assert set(got) == set(SYMBOLS) and _lib.SEQLEN_CONSTANTS == {} and set(_lib.SEQLEN_STRUCTS) == set(COUNTERPART)
    for name, (res, args) in got.items():
        assert res is C.c_int32 and args == [C.POINTER(getattr(_lib, SYMBOLS[name]))], name
        fn = getattr(lib, name)
        assert fn.restype is res and fn.argtypes == args
    src = _header.read(_header.SEQLEN_HEADER_PATH)
    for bad in (src.replace("const int32_t* lengths;", "const uint16_t* lengths;", 1),
                src.replace("#include <stdint.h>", "#include <stdint.h>\n#if 0\n#endif"),
                src.replace("int mmdeer_lstm_seq_len_fwd(", "static int mmdeer_lstm_seq_len_fwd(")):
        assert bad != src
        with pytest.raises(_header.HeaderError):
            _header.parse(bad, _lib._SEQLEN_NAMES, {})
    # no name of the older headers is taken
    assert not set(_lib.SEQLEN_STRUCTS) & (set(_lib.STRUCTS) | set(_lib.VIDEO_STRUCTS) | set(_lib.FRAME_STRUCTS) | set(_lib.BERT_STRUCTS) |
                                           set(_lib.BERT_DROP_STRUCTS) | set(_lib.OPTIM_STRUCTS) | set(_lib.GRAPH_STRUCTS))
    assert {"lstm_seq_args", "temporal_pool_args"} <= set(_lib.STRUCTS)


@pytest.mark.parametrize("name", sorted(COUNTERPART))
def test_struct_layout_is_the_counterparts_with_lengths_appended(name):
    lib = _lib.load()
    new, old = _lib.SEQLEN_STRUCTS[name], _lib.STRUCTS[COUNTERPART[name]]
    assert lib.mmdeer_sizeof(name.encode()) == C.sizeof(new)                        # the mirror against the compiler's layout
    assert lib.mmdeer_sizeof(COUNTERPART[name].encode()) == C.sizeof(old)
    assert [f for f, _ in new._fields_] == [f for f, _ in old._fields_] + ["lengths"]
    for (f, t_new), (_, t_old) in zip(new._fields_, old._fields_):
        assert t_new is t_old and getattr(new, f).offset == getattr(old, f).offset, f
    assert new.lengths.offset == C.sizeof(old) and C.sizeof(new) == C.sizeof(old) + 8


A = 1 << 20     # a plausible, aligned address: never dereferenced by the host checks


def _seq(**kw):
    a = _lib.LstmSeqLenArgs()
    a.xg, a.ld_xg, a.w_hh, a.w_hh_t, a.h, a.ld_h = A, 2048, A, A, A, 512
    a.tape_gates, a.tape_c, a.dh_out, a.ld_dh, a.dgates, a.ld_dg = A, A, A, 512, A, 2048
    a.T, a.B, a.hidden, a.ndir, a.act_f32, a.lengths = 4, 8, 256, 2, 0, A
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _pool(**kw):
    a = _lib.TemporalPoolLenArgs()
    a.h, a.ld_h, a.z, a.ld_z, a.w2, a.b2, a.attended, a.ld_att, a.weights = A, 512, A, 256, A, A, A, 512, A
    a.dout, a.ld_dout, a.dh, a.ld_dh, a.dz, a.ld_dz, a.dw2, a.db2, a.scratch = A, 512, A, 512, A, 256, A, A, A
    a.T, a.B, a.hidden, a.act_f32, a.lengths = 4, 8, 256, 0, A
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _refused(lib, rc, op, msg, kw):
    assert rc == -1, kw
    err = lib.mmdeer_last_error()
    assert msg in err and err.startswith(op.removeprefix("mmdeer_").encode() + b":"), (kw, err)


@pytest.mark.parametrize("op", ["mmdeer_lstm_seq_len_fwd", "mmdeer_lstm_seq_len_bwd"])
def test_recurrence_entries_refuse_on_the_host(op):
    lib = _lib.load()
    f = getattr(lib, op)
    bwd = op.endswith("bwd")
    cases = [({"T": -1}, b"bad shape"), ({"B": -1}, b"bad shape"), ({"hidden": 128}, b"hidden"), ({"ndir": 1}, b"ndir"),
             ({"ld_dh" if bwd else "ld_h": 256}, b"leading"), ({"ld_dg" if bwd else "ld_xg": 1024}, b"leading"),
             ({"w_hh_t" if bwd else "w_hh": A + 8}, b"misaligned"), ({"tape_gates": A + 4}, b"misaligned"), ({"tape_c": A + 4}, b"misaligned"),
             ({"dgates" if bwd else "h": A + 2}, b"misaligned"), ({"dh_out" if bwd else "xg": A + 2}, b"misaligned"),
             ({"ld_dh" if bwd else "ld_h": 516}, b"misaligned"), ({"ld_dg" if bwd else "ld_xg": 2052}, b"misaligned"),
             ({"lengths": None}, b"lengths is NULL or not 4-byte aligned")]
    cases += [({"lengths": A + off}, b"lengths is NULL or not 4-byte aligned") for off in (1, 2, 3)]
    if bwd:
        cases += [({k: None}, b"NULL") for k in ("w_hh_t", "tape_gates", "tape_c", "dh_out", "dgates")]
    else:
        cases += [({k: None}, b"NULL") for k in ("xg", "w_hh", "h")] + [({"tape_c": None}, b"go together"), ({"tape_gates": None}, b"go together")]
    for kw, msg in cases:
        _refused(lib, f(C.byref(_seq(**kw))), op, msg, kw)
    for kw in ({"B": 0}, {"T": 0}):                            # nothing to do: no launch, no error, lengths not asked for
        assert f(C.byref(_seq(xg=None, w_hh=None, w_hh_t=None, h=None, dh_out=None, dgates=None, lengths=None, **kw))) == 0
    assert f(None) == -1 and b"NULL argument struct" in lib.mmdeer_last_error()
    if not bwd:                                                # inference: no tape at all is accepted by the checks up to lengths
        _refused(lib, f(C.byref(_seq(tape_gates=None, tape_c=None, lengths=None))), op, b"lengths is NULL", {})


@pytest.mark.parametrize("op", ["mmdeer_temporal_pool_len_fwd", "mmdeer_temporal_pool_len_bwd"])
def test_pool_entries_refuse_on_the_host(op):
    lib = _lib.load()
    f = getattr(lib, op)
    bwd = op.endswith("bwd")
    cases = [({"T": -1}, b"bad shape"), ({"B": -1}, b"bad shape"), ({"hidden": 128}, b"hidden"),
             ({"ld_h": 256}, b"leading"), ({"ld_z": 128}, b"leading"), ({"z": A + 8}, b"misaligned"), ({"h": A + 8}, b"misaligned"),
             ({"w2": A + 4}, b"misaligned"), ({"ld_h": 516}, b"misaligned"), ({"ld_z": 260}, b"misaligned"),
             ({"lengths": None}, b"lengths is NULL or not 4-byte aligned")]
    cases += [({"lengths": A + off}, b"lengths is NULL or not 4-byte aligned") for off in (1, 2, 3)]
    cases += [({k: None}, b"NULL") for k in ("h", "z", "w2", "weights")]
    if bwd:
        cases += [({k: None}, b"NULL") for k in ("dout", "dh", "dz", "dw2", "db2", "scratch")]
        cases += [({"ld_dout": 256}, b"leading"), ({"ld_dh": 256}, b"leading"), ({"ld_dz": 128}, b"leading"),
                  ({"dout": A + 2}, b"misaligned"), ({"dh": A + 2}, b"misaligned"), ({"dz": A + 2}, b"misaligned"), ({"scratch": A + 4}, b"misaligned"),
                  ({"ld_dout": 516}, b"misaligned"), ({"ld_dh": 516}, b"misaligned"), ({"ld_dz": 260}, b"misaligned")]
    else:
        cases += [({"b2": None}, b"NULL"), ({"attended": None}, b"NULL"), ({"ld_att": 256}, b"leading"), ({"attended": A + 2}, b"misaligned"),
                  ({"ld_att": 516}, b"misaligned")]
    for kw, msg in cases:
        _refused(lib, f(C.byref(_pool(**kw))), op, msg, kw)
    for kw in ({"B": 0}, {"T": 0}):
        assert f(C.byref(_pool(h=None, z=None, attended=None, dz=None, lengths=None, **kw))) == 0
    assert f(None) == -1 and b"NULL argument struct" in lib.mmdeer_last_error()


# ------------------------------------------------------------------------------------------------ the module's host checks
def test_forward_refuses_bad_lengths_on_the_host():
    m = temporal.TemporalAudioEncoder()
    x = torch.zeros(3, 5, 84)
    for bad in ([5, 5], [[5, 5, 5]], torch.tensor([5, 5, 5, 5]), torch.tensor(5)):               # wrong shape
        with pytest.raises(ValueError, match="shape"):
            m(x, bad)
    for bad in ([5, 6, 1], [-1, 2, 2], torch.tensor([0, 5, 9], dtype=torch.int32)):              # outside [0, T]
        with pytest.raises(ValueError, match=r"\[0, 5\]"):
            m(x, lengths=bad)
    for bad in ([5.0, 1.0, 2.0], torch.tensor([5.0, 1.0, 2.0]), torch.tensor([True, False, True])):
        with pytest.raises(TypeError):
            m(x, lengths=bad)
    with pytest.raises(ValueError, match=r"\[0, 1\]"):                                           # a 2-D input is T = 1
        m(torch.zeros(3, 84), lengths=[1, 2, 0])
    for ok in ([5, 0, 3], torch.tensor([5, 0, 3]), torch.tensor([5, 0, 3], dtype=torch.int32)):
        with pytest.raises(RuntimeError, match="GPU tensors"):                                   # good lengths, a CPU x: no CPU path
            m(x, lengths=ok)
    with pytest.raises(RuntimeError, match="GPU tensors"):
        m(torch.zeros(3, 84), lengths=[1, 1, 0])
    with pytest.raises(RuntimeError, match="GPU tensors"):                                       # as before
        m(x)
    with pytest.raises(RuntimeError, match="GPU tensors"):
        m(x, lengths=None)
    assert torch.equal(temporal.as_lengths([5, 0, 3], 3, 5, "cpu"), torch.tensor([5, 0, 3], dtype=torch.int32))


def test_modality_encoder_passes_audio_lengths_through():
    m = encoders.ModalityEncoder()
    calls = []

    def spy(*args, **kw):
        calls.append((args, kw))
        return torch.zeros(2, 512)
    m.encode_audio = spy
    audio, n = torch.zeros(2, 4, 84), torch.tensor([4, 2])
    out = m({"audio": audio, "audio_lengths": n})
    assert list(out) == ["audio"] and len(calls) == 1
    assert len(calls[0][0]) == 1 and calls[0][0][0] is audio and list(calls[0][1]) == ["lengths"] and calls[0][1]["lengths"] is n
    m({"audio": audio})
    assert len(calls[1][0]) == 1 and calls[1][0][0] is audio and calls[1][1] == {}             # without the key: the old call
    m({"audio": audio, "audio_lengths": None})
    assert len(calls[2][0]) == 1 and calls[2][1] == {}
    assert m({"audio_lengths": n}) == {}                                                         # lengths without audio: no audio
    # the real method hands them to the audio encoder
    m2 = encoders.ModalityEncoder()
    seen = []
    m2.audio_encoder.forward = lambda x, lengths=None: seen.append((x, lengths)) or torch.zeros(2, 512)
    m2({"audio": audio, "audio_lengths": n})
    m2({"audio": audio})
    assert seen[0][0] is audio and seen[0][1] is n and seen[1][0] is audio and seen[1][1] is None
