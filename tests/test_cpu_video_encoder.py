"""The temporal video encoder without a GPU: the float64 restatement (tests/video_ref.py) against the golden vectors captured from
the reference (tests/golden/video_seq.npz), the state_dict contract, the new symbols of the built library, the companion header's
binding, and every refusal of the new C entry points and of the module that is decided on the host."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from mmdeer import _header, _lib, build, video

from . import video_ref as R
from .test_oracle_golden import check_side_grads

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "video_seq.npz")
NAMES = os.path.join(HERE, "golden", "video_state_dict_names.json")
CASES = [(9, 2, False), (3, 17, False), (4, 1, False), (5, 5, True), (2, 17, True)]
NOISE_BIASES = ("temporal_cnn.0.bias", "temporal_cnn.4.bias")
NEW_SYMBOLS = {"mmdeer_conv3_time_pack": 7, "mmdeer_conv3_time": 1, "mmdeer_bn_time_stats": 1, "mmdeer_bn_time_apply": 1,
               "mmdeer_bn_time_bwd": 1}


def shapes():
    return {k: tuple(s) for k, s in json.load(open(NAMES))}


def state64(tag):
    """The case's closed-form state in float64, without the backbone (never run); num_batches_tracked as the integer it loads as."""
    sd = R.filled_state(tag, shapes())
    return {k: torch.from_numpy(v.astype(np.int64) if k.endswith("num_batches_tracked") else v).double()
            for k, v in sd.items() if not k.startswith("spatial_backbone.")}


@pytest.mark.parametrize("B,T,train", CASES)
def test_restatement_reproduces_the_reference_capture(B, T, train):
    g = np.load(GOLDEN)
    tag = f"vid{B}x{T}"
    P = state64(tag)
    for k, v in P.items():
        if v.dim() and "running" not in k:
            v.requires_grad_(True)
    x = torch.from_numpy(g[f"{tag}.input"].astype(np.float32)).double().requires_grad_(True)
    y, buffers = R.encoder(P, x, train)
    np.testing.assert_allclose(y.detach().numpy(), g[f"{tag}.out"], rtol=1e-4, atol=5e-6)
    (y * torch.from_numpy(g[f"{tag}.loss_w"]).double()).sum().backward()
    grads = {k: v.grad for k, v in P.items() if v.requires_grad}
    check_side_grads(g, tag, grads, {"video": x.grad}, rtol=3e-4, atol_frac=3e-5)
    if T == 1:      # the temporal CNN and the pool are skipped: no gradient (None, not zeros), no buffer moves
        for k in grads:
            assert (grads[k] is None) == k.startswith(("temporal_cnn.", "temporal_attention.")), k
            assert (f"{tag}.gradnone.{k}" in g) == (grads[k] is None), k
        assert all(torch.equal(buffers[k], P[k]) for k in buffers)
        return
    # b2 shifts every score of a sample equally: the exact gradient is zero, the reference's value is rounding noise
    assert abs(float(grads["temporal_attention.2.bias"])) <= 1e-12
    assert float(np.abs(g[f"{tag}.gradnoise.temporal_attention.2.bias"]).max()) <= 1e-4 * float(np.abs(g[f"{tag}.grad.temporal_attention.2.weight"]).max())
    if train:
        for n in NOISE_BIASES:      # BatchNorm subtracts the mean that the convolution's bias shifts
            wmax = float(grads[n.replace("bias", "weight")].abs().max())
            assert float(grads[n].abs().max()) <= 1e-10 * wmax, n
            assert float(np.abs(g[f"{tag}.gradnoise.{n}"]).max()) <= 1e-4 * wmax, n
        # atol: the capture is fp32 -- a running mean near zero still carries the rounding of the O(1) convolution outputs it
        # averages, one fp32 ulp at 1.0
        for k, v in buffers.items():
            np.testing.assert_allclose(v.numpy(), g[f"{tag}.buffer.{k}"], rtol=1e-5, atol=1.2e-7, err_msg=k)
        assert int(g[f"{tag}.buffer.temporal_cnn.1.num_batches_tracked"]) == 1
    else:
        assert all(f"{tag}.grad.{n}" in g for n in NOISE_BIASES)          # real gradients under running statistics
        assert all(torch.equal(buffers[k], P[k]) for k in buffers)


def test_restatement_operators_equal_torch():
    torch.manual_seed(0)
    B, T = 3, 6
    conv = torch.nn.Conv1d(16, 24, 3, padding=1).double()
    bn = torch.nn.BatchNorm1d(24).double().train()
    x = torch.randn(B, T, 16, dtype=torch.float64)
    rows = x.transpose(0, 1).reshape(T * B, 16)
    y = R.conv3_time(R.pad_time(rows, B), conv.weight, conv.bias, T, B)
    ref = conv(x.transpose(1, 2))                                          # (B, 24, T)
    torch.testing.assert_close(y.reshape(T, B, 24).permute(1, 2, 0), ref, rtol=1e-12, atol=1e-12)
    out, bm, bv = R.batchnorm_rows(y, bn.weight, bn.bias)
    torch.testing.assert_close(out.reshape(T, B, 24).permute(1, 2, 0), torch.relu(bn(ref)), rtol=1e-10, atol=1e-12)
    rm, rv, nbt = R.running_update(torch.zeros(24, dtype=torch.float64), torch.ones(24, dtype=torch.float64), 0, bm, bv, T * B)
    torch.testing.assert_close(rm, bn.running_mean, rtol=1e-12, atol=1e-14)
    torch.testing.assert_close(rv, bn.running_var, rtol=1e-12, atol=1e-14)
    assert nbt == int(bn.num_batches_tracked) == 1


def test_state_dict_matches_the_reference():
    m = video.TemporalVideoEncoder()
    sd = m.state_dict()
    assert [[k, list(v.shape)] for k, v in sd.items()] == json.load(open(NAMES))
    assert len(sd) == 52 and sum(v.numel() for v in sd.values()) == 3798407
    assert sum(v.numel() for k, v in sd.items() if k.startswith("spatial_backbone.")) == 1562500
    assert [n for n, _ in m.named_children()] == ["spatial_backbone", "spatial_projection", "temporal_cnn", "temporal_attention", "output_projection"]
    for bn in (m.temporal_cnn[1], m.temporal_cnn[5]):
        assert type(bn) is torch.nn.BatchNorm1d and bn.num_batches_tracked.dtype == torch.int64
    # the closed-form state of a golden case loads strictly; the running variances it carries are positive
    filled = R.filled_state("vid9x2", shapes())
    m.load_state_dict({k: torch.from_numpy(v) for k, v in filled.items()}, strict=True)
    assert float(m.temporal_cnn[1].running_var.min()) >= 0.5 and int(m.temporal_cnn[5].num_batches_tracked) == 0


def test_fixture_is_small_and_complete():
    assert os.path.getsize(GOLDEN) <= 701611
    g = np.load(GOLDEN)
    for B, T, train in CASES:
        tag = f"vid{B}x{T}"
        assert g[f"{tag}.input"].shape == (B, T, 512) and g[f"{tag}.out"].shape == g[f"{tag}.loss_w"].shape == (B, 512)
        assert (f"{tag}.buffer.temporal_cnn.5.running_var" in g) == train
        assert not any(k.startswith(f"{tag}.") and "spatial_backbone" in k for k in g)


def test_compat_exports_the_encoder():
    code = ("import sys; sys.path[:0] = [%r, %r]\nimport encoders\nfrom mmdeer.video import TemporalVideoEncoder\n"
            "assert encoders.EnhancedVideoEncoder is TemporalVideoEncoder\nprint('ok')\n") % (ROOT, os.path.join(ROOT, "compat"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-2000:]


# ------------------------------------------------------------------------------------------------ the C ABI additions
def test_new_symbols_are_declared_bound_and_exported():
    lib = _lib.load()
    assert {n: len(args) for n, _, args in _lib.VIDEO_SYMBOLS} == NEW_SYMBOLS
    for name, res, args in _lib.VIDEO_SYMBOLS:
        fn = getattr(lib, name)                                           # exported by the built library
        assert fn.restype is C.c_int32 and fn.argtypes == args, name
    assert set(_lib.VIDEO_STRUCTS) == {"conv3_time_args", "bn_time_args"}
    for name, cls in _lib.VIDEO_STRUCTS.items():                          # the ctypes mirrors against the compiler's layout
        assert lib.mmdeer_sizeof(name.encode()) == C.sizeof(cls), name
    assert _lib.BN_TIME_SCRATCH == 1024 * 1024 and _lib.VIDEO_CONSTANTS == {"BN_TIME_SCRATCH": 1024 * 1024}
    assert not {n for n, _, _ in _lib.VIDEO_SYMBOLS} & {n for n, _, _ in _lib.SYMBOLS}
    assert {"conv_time.hip", "bn_time.hip"} <= set(build.SOURCES)
    assert lib.mmdeer_abi_version() == _lib.ABI_VERSION == 16            # additions only


def test_companion_header_layout_matches_the_compiler(tmp_path):
    """Offsets and sizes of every field of the two new structs, as ctypes lays them out, asserted by the compiler on the header."""
    lines = ["#include <stddef.h>", '#include "mmdeer_video.h"']
    for cname, cls in _lib._VIDEO_CLASSES.items():
        lines.append(f'static_assert(sizeof({cname}) == {C.sizeof(cls)}, "sizeof {cname}");')
        for field, _ in cls._fields_:
            d = getattr(cls, field)
            lines.append(f'static_assert(offsetof({cname}, {field}) == {d.offset}, "offsetof {cname}.{field}");')
            lines.append(f'static_assert(sizeof((({cname}*)0)->{field}) == {d.size}, "sizeof {cname}.{field}");')
    tu = tmp_path / "layout.cpp"
    tu.write_text("\n".join(lines) + "\n")
    r = subprocess.run([build._hipcc(), "-x", "c++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(tu)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    with pytest.raises(_header.HeaderError):                               # the companion header goes through the same strict parser
        _header.parse(_header.read(_header.VIDEO_HEADER_PATH).replace("int mmdeer_conv3_time(", "int mmdeer_conv3_time(uint16_t f, "),
                      _lib._VIDEO_NAMES, {})


A = 1 << 20     # a plausible, aligned address: never dereferenced by the host checks


def _conv(**kw):
    a = _lib.Conv3TimeArgs()
    a.x, a.ld_x, a.w, a.bias, a.y, a.ld_y = A, 512, A, A, A, 512
    a.T, a.B, a.C, a.N, a.act_f32, a.tile = 4, 8, 512, 512, 0, -1
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _bn(**kw):
    a = _lib.BnTimeArgs()
    a.x, a.ld_x, a.mean, a.rstd, a.gamma, a.beta, a.out, a.ld_out = A, 512, A, A, A, A, A, 512
    a.dout, a.ld_dout, a.dx, a.ld_dx, a.dgamma, a.dbeta, a.scratch = A, 512, A, 512, A, A, A
    a.R, a.C, a.act_f32, a.drop_site, a.eps, a.momentum, a.mask_scale = 32, 512, 0, -1, 1e-5, 0.1, 1.0
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_conv_operator_refuses_on_the_host():
    lib = _lib.load()
    f = lib.mmdeer_conv3_time
    for kw, msg in [({"C": 256}, b"must be 512"), ({"N": 1024}, b"must be 512"), ({"C": 256, "x": None, "T": 0}, b"must be 512"),
                    ({"T": -1}, b"bad shape"), ({"tile": 1}, b"tile"), ({"tile": 3}, b"tile"), ({"x": None}, b"NULL"), ({"w": None}, b"NULL"),
                    ({"y": None}, b"NULL"), ({"ld_x": 256}, b"leading"), ({"ld_y": 508}, b"leading"), ({"x": A + 8}, b"misaligned"),
                    ({"bias": A + 4}, b"misaligned"), ({"ld_x": 516}, b"misaligned"), ({"T": 1 << 20, "B": 1 << 10}, b"too many")]:
        assert f(C.byref(_conv(**kw))) == -1, kw
        assert msg in lib.mmdeer_last_error(), (kw, lib.mmdeer_last_error())
    for kw in ({"B": 0}, {"T": 0}):
        assert f(C.byref(_conv(x=None, w=None, y=None, bias=None, **kw))) == 0
    assert f(None) == -1
    p = lib.mmdeer_conv3_time_pack
    assert p(A, 256, 512, A, A, 0, None) == -1 and b"must be 512" in lib.mmdeer_last_error()
    assert p(A, 512, 64, A, A, 0, None) == -1 and b"must be 512" in lib.mmdeer_last_error()
    assert p(None, 512, 512, A, A, 0, None) == -1 and b"NULL" in lib.mmdeer_last_error()
    assert p(A, 512, 512, None, A, 0, None) == -1 and b"NULL" in lib.mmdeer_last_error()


@pytest.mark.parametrize("op", ["mmdeer_bn_time_stats", "mmdeer_bn_time_apply", "mmdeer_bn_time_bwd"])
def test_batchnorm_operators_refuse_on_the_host(op):
    lib = _lib.load()
    f = getattr(lib, op)
    cases = [({"C": 256}, b"must be 512"), ({"R": -1}, b"row count"), ({"x": None}, b"x"), ({"ld_x": 256}, b"ld"), ({"x": A + 8}, b"aligned"),
             ({"ld_x": 516}, b"16 bytes"), ({"mean": None}, b"mean")]
    if op.endswith("stats"):
        cases += [({"scratch": None}, b"scratch"), ({"running_mean": A}, b"go together"), ({"num_batches_tracked": A}, b"running")]
    elif op.endswith("apply"):
        cases += [({"out": None}, b"out"), ({"gamma": None}, b"gamma"), ({"beta": A + 4}, b"aligned"), ({"dropout_p": 1.0}, b"dropout_p"),
                  ({"ld_out": 500}, b"ld")]
    else:
        cases += [({"dout": None}, b"dout"), ({"dx": A + 2}, b"aligned"), ({"dgamma": None}, b"dgamma"), ({"scratch": None}, b"scratch"),
                  ({"out": A + 4}, b"aligned"), ({"ld_dx": 256}, b"ld")]
    for kw, msg in cases:
        assert f(C.byref(_bn(**kw))) == -1, kw
        assert msg in lib.mmdeer_last_error(), (kw, lib.mmdeer_last_error())
    assert f(C.byref(_bn(R=0, x=None, mean=None, out=None, dout=None, dx=None, scratch=None))) == 0
    assert f(None) == -1


def test_module_input_errors():
    m = video.TemporalVideoEncoder()
    for shape in ((2, 3, 224, 224), (2, 5, 3, 224, 224)):
        with pytest.raises(NotImplementedError):
            m(torch.zeros(*shape))                                         # frame tensors: the backbone is outside the hot path
    with pytest.raises(ValueError):
        m(torch.zeros(2, 5, 256))
    with pytest.raises(ValueError):
        m(torch.zeros(2, 0, 512))
    with pytest.raises(NotImplementedError):
        video.TemporalVideoEncoder({"hidden_dim": 256})(torch.zeros(2, 5, 512))
    for x in (torch.zeros(2, 5, 512), torch.zeros(2, 512)):
        with pytest.raises(RuntimeError):
            m(x)                                                           # no CPU fallback
