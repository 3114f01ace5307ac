"""The frame video encoder without a GPU: the float64 restatement (tests/frames_ref.py) against the golden vectors captured from the
reference (tests/golden/frame_seq.npz), the reference's own rounding against a quarter of the GPU tolerance, the state_dict contract,
the third companion header's binding and layout, the new symbols of the built library, and every refusal of the new C entry points
and of the module that is decided on the host."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from mmdeer import _header, _lib, build, frames

from . import frames_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "frame_seq.npz")
NAMES = os.path.join(HERE, "golden", "video_state_dict_names.json")
# (B, T, H, W, train, given as a 4-D tensor): tests/golden/make_golden_frames.py, in its order (the input stream is 940 + index)
CASES = [(2, 3, 19, 23, False, False), (5, 5, 16, 16, True, False), (2, 2, 1, 1, False, False), (6, 1, 5, 7, True, False),
         (2, 1, 224, 224, False, True)]
RTOL, ATOL = 1e-3, 2e-5          # the module tolerance of the GPU tests in fp32 (tests/test_gpu_video_encoder.py)
NEW_SYMBOLS = {"mmdeer_frames_pack": 7, "mmdeer_conv2d_pack": 7, "mmdeer_conv2d_s2": 1, "mmdeer_bn2d_stats": 1, "mmdeer_bn2d_apply": 1}


def shapes():
    return {k: tuple(s) for k, s in json.load(open(NAMES))}


def tag_of(B, T, H, W):
    return f"frm{B}x{T}x{H}x{W}"


def state64(tag):
    sd = R.filled_state(tag, shapes())
    return {k: torch.from_numpy(v.astype(np.int64) if k.endswith("num_batches_tracked") else v).double() for k, v in sd.items()}


@functools.lru_cache(maxsize=None)
def restated(i):
    """(features, output, buffers) of case i in float64: computed once, shared, left unchanged"""
    B, T, H, W, train, _ = CASES[i]
    x = torch.from_numpy(R.frames_input(940 + i, B, T, H, W)).double()
    return R.encoder(state64(tag_of(B, T, H, W)), x, train)


@pytest.mark.parametrize("i", range(len(CASES)))
def test_restatement_reproduces_the_reference_within_a_quarter_of_the_gpu_bound(i):
    """The reference's own fp32 result against float64: it may use up a quarter of the tolerance the GPU path is held to."""
    B, T, H, W, train, _ = CASES[i]
    g, tag = np.load(GOLDEN), tag_of(B, T, H, W)
    feats, y, buffers = restated(i)
    for name, ref in (("feats", feats.numpy()), ("out", y.numpy())):
        got = g[f"{tag}.{name}"].astype(np.float64)
        assert got.shape == ref.shape == ((B, T, 512) if name == "feats" else (B, 512))
        excess = np.abs(got - ref) / (0.25 * (ATOL + RTOL * np.abs(ref)))
        print(f"{tag}.{name}: worst |reference - float64| = {excess.max():.3f} of a quarter of the bound")
        assert excess.max() <= 1.0, (tag, name, float(excess.max()))
    if train:
        for k in R.BUFFERS:
            # a quarter of the GPU tests' buffer bound (rtol 1e-5, atol 1.2e-7), as for the features and outputs
            np.testing.assert_allclose(g[f"{tag}.buffer.{k}"], buffers[k].numpy(), rtol=0.25e-5, atol=0.3e-7, err_msg=k)
            assert not k.endswith("num_batches_tracked") or int(g[f"{tag}.buffer.{k}"]) == 1
    else:
        assert all(torch.equal(buffers[k], state64(tag)[k]) for k in R.BUFFERS)
        assert not any(k.startswith(f"{tag}.buffer.") for k in g)


def test_restatement_operators_equal_torch():
    """The layout-level operators against torch's float64 Conv2d / BatchNorm2d / MaxPool2d / mean, on odd sizes, both kernel sizes."""
    torch.manual_seed(0)
    N, H, W = 3, 9, 7
    x = torch.randn(N, 3, H, W, dtype=torch.float64)
    c1 = torch.nn.Conv2d(3, 16, 7, 2, 3).double()
    c2 = torch.nn.Conv2d(16, 8, 3, 2, 1).double()
    bn = torch.nn.BatchNorm2d(16).double().train()
    for Cp in (4, 8):
        y = R.conv2d_s2(R.pack_frames(x, Cp), R.pack_weight(c1.weight, Cp, 8), c1.bias, N, H, W, 7)
        ref = c1(x)
        OH, OW = ref.shape[2:]
        torch.testing.assert_close(y.reshape(N, OH, OW, 16).permute(0, 3, 1, 2), ref, rtol=1e-12, atol=1e-12)
    v, bm, bv = R.batchnorm_relu(y, bn.weight, bn.bias)
    act = torch.relu(bn(ref))
    torch.testing.assert_close(v.reshape(N, OH, OW, 16).permute(0, 3, 1, 2), act, rtol=1e-10, atol=1e-12)
    rm, rv, nbt = R.running_update(torch.zeros(16, dtype=torch.float64), torch.ones(16, dtype=torch.float64), 0, bm, bv, N * OH * OW)
    torch.testing.assert_close(rm, bn.running_mean, rtol=1e-12, atol=1e-14)
    torch.testing.assert_close(rv, bn.running_var, rtol=1e-12, atol=1e-14)
    assert nbt == int(bn.num_batches_tracked) == 1
    pooled = torch.nn.functional.max_pool2d(act, 3, 2, 1)
    PH, PW = pooled.shape[2:]
    xp = R.maxpool_padded(v, N, OH, OW).detach()
    assert xp.shape == (N, PH + 2, PW + 2, 16)
    torch.testing.assert_close(xp[:, 1:-1, 1:-1].permute(0, 3, 1, 2), pooled, rtol=1e-10, atol=1e-12)
    assert float(xp[:, 0].abs().max()) == float(xp[:, -1].abs().max()) == float(xp[:, :, 0].abs().max()) == float(xp[:, :, -1].abs().max()) == 0
    y2 = R.conv2d_s2(xp.reshape(-1, 16), R.pack_weight(c2.weight, 16, 3), c2.bias, N, PH, PW, 3)
    ref2 = c2(pooled)
    torch.testing.assert_close(y2.reshape(N, *ref2.shape[2:], 8).permute(0, 3, 1, 2), ref2, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(R.frame_means(v, N), act.mean((2, 3)), rtol=1e-12, atol=1e-14)
    torch.testing.assert_close(R.to_padded(v, N, OH, OW)[:, 1:-1, 1:-1].permute(0, 3, 1, 2), act, rtol=1e-10, atol=1e-12)


def test_state_dict_matches_the_reference():
    m = frames.FrameVideoEncoder()
    sd = m.state_dict()
    assert [[k, list(v.shape)] for k, v in sd.items()] == json.load(open(NAMES))
    assert len(sd) == 52 and sum(v.numel() for v in sd.values()) == 3798407
    filled = R.filled_state("frm2x3x19x23", shapes())
    m.load_state_dict({k: torch.from_numpy(v) for k, v in filled.items()}, strict=True)
    assert isinstance(m, frames.TemporalVideoEncoder) and m.frame_chunk == frames.DEFAULT_FRAME_CHUNK == 256
    assert 256 * 112 * 112 * 64 * 4 < 1e9 <= 512 * 112 * 112 * 64 * 4          # the default chunk's conv1 output at 224 x 224 in fp32
    assert frames.FrameVideoEncoder({"frame_chunk": 7}).frame_chunk == 7
    with pytest.raises(ValueError):
        frames.FrameVideoEncoder({"frame_chunk": 0})


def test_fixture_is_small_and_complete():
    assert os.path.getsize(GOLDEN) < 1 << 20
    g = np.load(GOLDEN)
    for B, T, H, W, train, _ in CASES:
        tag = tag_of(B, T, H, W)
        assert g[f"{tag}.feats"].shape == (B, T, 512) and g[f"{tag}.out"].shape == (B, 512)
        assert all((f"{tag}.buffer.{k}" in g) == train for k in R.BUFFERS)
    assert len(R.BUFFERS) == 12


def test_compat_exports_the_encoder():
    code = ("import sys; sys.path[:0] = [%r, %r]\nimport encoders\nfrom mmdeer.frames import FrameVideoEncoder\nfrom mmdeer.video import TemporalVideoEncoder\n"
            "assert encoders.FrameVideoEncoder is FrameVideoEncoder and encoders.EnhancedVideoEncoder is TemporalVideoEncoder\nprint('ok')\n"
            ) % (ROOT, os.path.join(ROOT, "compat"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-2000:]


# ------------------------------------------------------------------------------------------------ the C ABI additions
def test_new_symbols_are_declared_bound_and_exported():
    lib = _lib.load()
    assert {n: len(args) for n, _, args in _lib.FRAME_SYMBOLS} == NEW_SYMBOLS
    for name, res, args in _lib.FRAME_SYMBOLS:
        fn = getattr(lib, name)                                           # exported by the built library
        assert fn.restype is C.c_int32 and fn.argtypes == args, name
    assert set(_lib.FRAME_STRUCTS) == {"conv2d_args", "bn2d_args"}
    for name, cls in _lib.FRAME_STRUCTS.items():                          # the ctypes mirrors against the compiler's layout
        assert lib.mmdeer_sizeof(name.encode()) == C.sizeof(cls), name
    assert _lib.FRAME_CONSTANTS == {"BN2D_SCRATCH": 1024 * 1024, "BN2D_PAD": 0, "BN2D_POOL": 1, "BN2D_AVG": 2}
    assert _lib.BN2D_SCRATCH == 1024 * 1024
    names = {n for n, _, _ in _lib.FRAME_SYMBOLS}
    assert not names & {n for n, _, _ in _lib.SYMBOLS} and not names & {n for n, _, _ in _lib.VIDEO_SYMBOLS}
    assert not set(_lib.FRAME_STRUCTS) & (set(_lib.STRUCTS) | set(_lib.VIDEO_STRUCTS))
    assert {"conv2d.hip", "bn2d.hip"} <= set(build.SOURCES)
    assert _header.FRAMES_HEADER_PATH == build.FRAMES_HEADER_PATH and os.path.samefile(build.FRAMES_HEADER_PATH, os.path.join(ROOT, "include", "mmdeer_frames.h"))
    assert lib.mmdeer_abi_version() == _lib.ABI_VERSION == 16            # additions only


def test_frames_header_layout_matches_the_compiler(tmp_path):
    """Offsets and sizes of every field of the two new structs, as ctypes lays them out, asserted by the compiler on the header."""
    lines = ["#include <stddef.h>", '#include "mmdeer_frames.h"']
    for cname, cls in _lib._FRAME_CLASSES.items():
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
    with pytest.raises(_header.HeaderError):                               # the new header goes through the same strict parser
        _header.parse(_header.read(_header.FRAMES_HEADER_PATH).replace("int mmdeer_conv2d_s2(", "int mmdeer_conv2d_s2(uint16_t f, "),
                      _lib._FRAME_NAMES, {})


A = 1 << 20     # a plausible, aligned address: never dereferenced by the host checks


def _conv(**kw):
    a = _lib.Conv2dArgs()
    a.x, a.w, a.bias, a.y = A, A, A, A
    a.N, a.H, a.W, a.Cin, a.Cout, a.k, a.act_f32, a.tile = 2, 9, 7, 64, 128, 3, 0, -1
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _bn(**kw):
    a = _lib.Bn2dArgs()
    a.x, a.mean, a.rstd, a.gamma, a.beta, a.out, a.scratch = A, A, A, A, A, A, A
    a.N, a.H, a.W, a.C, a.act_f32, a.eps, a.momentum, a.dest = 2, 5, 3, 128, 0, 1e-5, 0.1, 0
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_conv_operator_refuses_on_the_host():
    lib = _lib.load()
    f = lib.mmdeer_conv2d_s2
    for kw, msg in [({"k": 5}, b"unsupported kernel size"), ({"k": 7}, b"unsupported kernel size"), ({"k": 7, "Cin": 4}, b"unsupported kernel size"),
                    ({"Cin": 12}, b"unsupported kernel size"), ({"Cin": 4}, b"unsupported kernel size"), ({"Cin": 0}, b"unsupported kernel size"),
                    ({"Cout": 96}, b"unsupported Cout"), ({"Cout": 0}, b"unsupported Cout"), ({"Cout": 96, "x": None, "N": 0}, b"unsupported Cout"),
                    ({"N": -1}, b"bad shape"), ({"H": 0}, b"bad shape"), ({"W": 0}, b"bad shape"), ({"tile": 1}, b"tile"), ({"tile": 3}, b"tile"),
                    ({"x": None}, b"NULL"), ({"w": None}, b"NULL"), ({"y": None}, b"NULL"), ({"x": A + 8}, b"misaligned"), ({"w": A + 4}, b"misaligned"),
                    ({"y": A + 2}, b"misaligned"), ({"bias": A + 4}, b"misaligned"),
                    ({"N": 1 << 10, "H": 255, "W": 127}, b"2^31"),                   # the padded input: 2^10 * 257 * 129 * 64 >= 2^31
                    ({"N": 1 << 12, "H": 127, "W": 127, "Cin": 8, "Cout": 512}, b"2^31"),   # the output: 2^12 * 64 * 64 * 512 = 2^33
                    ({"k": 7, "Cin": 3, "N": 1 << 13, "H": 250, "W": 250}, b"2^31")]:  # 2^13 * 256 * 256 pixels of 8 bf16
        assert f(C.byref(_conv(**kw))) == -1, kw
        assert msg in lib.mmdeer_last_error(), (kw, lib.mmdeer_last_error())
    assert f(C.byref(_conv(Cin=4, act_f32=1, N=0, x=None, w=None, y=None, bias=None))) == 0      # fp32: a 16-byte chunk is 4 elements
    assert f(C.byref(_conv(N=0, x=None, w=None, y=None, bias=None))) == 0
    assert f(C.byref(_conv(k=7, Cin=3, N=0, x=None, w=None, y=None, bias=None))) == 0
    assert f(None) == -1
    p = lib.mmdeer_conv2d_pack
    for args, msg in [((A, 64, 3, 3, A, 0, None), b"unsupported kernel size"), ((A, 64, 64, 5, A, 0, None), b"unsupported kernel size"),
                      ((A, 64, 4, 3, A, 0, None), b"unsupported kernel size"), ((A, 100, 64, 3, A, 0, None), b"unsupported Cout"),
                      ((None, 64, 64, 3, A, 0, None), b"NULL"), ((A, 64, 64, 3, None, 0, None), b"NULL"), ((A, 64, 64, 3, A + 8, 0, None), b"misaligned"),
                      ((A + 2, 64, 64, 3, A, 0, None), b"misaligned")]:
        assert p(*args) == -1 and msg in lib.mmdeer_last_error(), (args, lib.mmdeer_last_error())
    q = lib.mmdeer_frames_pack
    for args, msg in [((A, -1, 4, 4, A, 0, None), b"bad shape"), ((A, 2, 0, 4, A, 0, None), b"bad shape"), ((None, 2, 4, 4, A, 0, None), b"NULL"),
                      ((A, 2, 4, 4, None, 0, None), b"NULL"), ((A, 2, 4, 4, A + 8, 1, None), b"misaligned"), ((A + 1, 2, 4, 4, A, 1, None), b"misaligned"),
                      ((A, 1 << 13, 250, 250, A, 0, None), b"2^31"), ((A, 1 << 14, 250, 250, A, 1, None), b"2^31")]:
        assert q(*args) == -1 and msg in lib.mmdeer_last_error(), (args, lib.mmdeer_last_error())
    assert q(None, 0, 4, 4, None, 0, None) == 0


@pytest.mark.parametrize("op", ["mmdeer_bn2d_stats", "mmdeer_bn2d_apply"])
def test_batchnorm_operators_refuse_on_the_host(op):
    lib = _lib.load()
    f = getattr(lib, op)
    cases = [({"C": 32}, b"unsupported C"), ({"C": 1024}, b"unsupported C"), ({"C": 96}, b"unsupported C"), ({"C": 96, "N": 0, "x": None}, b"unsupported C"),
             ({"N": -1}, b"bad shape"), ({"H": 0}, b"bad shape"), ({"x": None}, b"x"), ({"x": A + 8}, b"aligned"), ({"mean": None}, b"mean"),
             ({"N": 1 << 12, "H": 64, "W": 64, "C": 128}, b"2^31")]
    if op.endswith("stats"):
        cases += [({"scratch": None}, b"scratch"), ({"scratch": A + 4}, b"scratch"), ({"running_mean": A}, b"go together"),
                  ({"num_batches_tracked": A}, b"running")]
    else:
        cases += [({"out": None}, b"out"), ({"out": A + 8}, b"aligned"), ({"gamma": None}, b"gamma"), ({"beta": A + 4}, b"aligned"),
                  ({"dest": 3}, b"dest"), ({"dest": -1}, b"dest"),
                  ({"N": 1 << 14, "H": 15, "W": 15, "C": 512}, b"out has 2^31")]       # x fits (2^14 * 225 * 512), the padded out (289) does not
    for kw, msg in cases:
        assert f(C.byref(_bn(**kw))) == -1, kw
        assert msg in lib.mmdeer_last_error(), (kw, lib.mmdeer_last_error())
    assert f(C.byref(_bn(N=0, x=None, mean=None, out=None, scratch=None))) == 0
    assert f(None) == -1


def test_module_input_errors():
    m = frames.FrameVideoEncoder().eval()
    z = torch.zeros(1)
    for shape in ((2, 5, 4, 8, 8), (2, 1, 8, 8), (2, 3, 224, 224, 7), (2, 3, 224, 224, 224), (2, 5, 256), (2, 0, 512), (2, 0, 3, 8, 8), (2, 3, 8, 8, 8, 8),
                  (1, 256, 3, 2000, 2000),      # a chunk of 256 padded frames of 2006 x 2006 x 4 elements: 2^31 or more, decided on the host
                  (2, 3, 3, 0, 8)):
        with pytest.raises(ValueError):
            m(z.expand(*shape))
    m.train()
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        m(z.expand(1, 1, 3, 2, 2))                                         # one frame, 1 x 1 from the first layer on
    m.spatial_backbone.eval()
    for x in (torch.zeros(1, 1, 3, 2, 2), torch.zeros(2, 3, 8, 8), torch.zeros(2, 5, 512), torch.zeros(2, 512)):
        with pytest.raises(RuntimeError):
            m(x)                                                           # no CPU fallback
    with pytest.raises(ValueError, match="requires_grad"):
        m(torch.zeros(2, 2, 3, 8, 8, requires_grad=True))
    cum = frames.FrameVideoEncoder().train()
    cum.spatial_backbone[5].momentum = None                                # cumulative averaging: the device update has no form of it
    with pytest.raises(ValueError, match="momentum"):
        cum(torch.zeros(2, 2, 3, 8, 8))
    cum.spatial_backbone.eval()                                            # unused in evaluation mode: the refusal is the CPU tensor's
    with pytest.raises(RuntimeError):
        cum(torch.zeros(2, 2, 3, 8, 8))
    with pytest.raises(ValueError):
        m.extract_spatial_features(torch.zeros(2, 3, 8, 8))               # the method takes 5-D only, as the reference's
    with pytest.raises(NotImplementedError):
        frames.FrameVideoEncoder({"hidden_dim": 256})(torch.zeros(2, 2, 3, 8, 8))
