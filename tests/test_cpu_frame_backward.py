"""The frame video encoder's backward without a GPU: the fourth companion header (include/mmdeer_frames_bwd.h) through the strict
parser, its layout against the compiler, its symbols in the built library, every refusal of the new C entry points that is decided
on the host, the gradient fixture captured from the reference (tests/golden/frame_grad.npz) and the float64 restatement
(tests/frames_bwd_ref.py) against it within a quarter of the GPU bound, and the module's switch."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

from mmdeer import _header, _lib, build, frames, synth

from . import frames_bwd_ref as RB
from . import frames_ref as R
from .test_cpu_frame_encoder import NEW_SYMBOLS as FORWARD_SYMBOLS
from .test_cpu_frame_encoder import state64, tag_of

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GRAD_GOLDEN = os.path.join(HERE, "golden", "frame_grad.npz")
# (index of the case in test_cpu_frame_encoder.CASES: its fill and its frames, B, T, H, W, backbone in train mode) -- the head always
# trains; tests/golden/make_golden_frames_grad.py, in its order
GRAD_CASES = [(1, 5, 5, 16, 16, True), (3, 6, 1, 5, 7, True), (0, 2, 3, 19, 23, False)]
WHOLE = 16384                   # a gradient of more elements is stored as a strided slice of at most this many
RTOL, ATOL_FRAC = 3e-3, 3e-3    # the GPU test's gradient bound (test_gpu_video_encoder: check_side_grads)
BWD_SYMBOLS = {"mmdeer_bn2d_bwd": 1, "mmdeer_conv2d_wgrad_scratch": 1, "mmdeer_conv2d_wgrad": 1, "mmdeer_conv2d_pack_t": 7, "mmdeer_conv2d_dgrad": 1}
CONV_BIASES = [f"{conv}.bias" for conv, _ in R.LAYERS]


def loss_weight(idx, B):
    """w of loss = sum(out * w) of the case with index idx: the counter-based generator, stream 980 + idx"""
    return synth.normal(980 + idx, B * 512).reshape(B, 512).astype(np.float32)


def slice_of(g):
    """the stored slice of a gradient of more than WHOLE elements"""
    flat = np.asarray(g).reshape(-1)
    return flat[::-(-flat.size // WHOLE)][:WHOLE]


@functools.lru_cache(maxsize=None)
def restated(i):
    """(output, gradients by name) of gradient case i in float64: computed once, shared, left unchanged"""
    idx, B, T, H, W, bb_train = GRAD_CASES[i]
    x = torch.from_numpy(R.frames_input(940 + idx, B, T, H, W)).double()
    _, out, grads = RB.module_grads(state64(tag_of(B, T, H, W)), x, torch.from_numpy(loss_weight(idx, B)).double(), bb_train, True)
    return out, grads


def test_fixture_is_small_and_complete():
    assert os.path.getsize(GRAD_GOLDEN) < 1 << 20
    g = np.load(GRAD_GOLDEN)
    shapes = {k: tuple(v.shape) for k, v in frames.FrameVideoEncoder().state_dict().items()}
    want = set()
    for idx, B, T, H, W, bb_train in GRAD_CASES:
        tag = tag_of(B, T, H, W)
        assert g[f"{tag}.out"].shape == (B, 512)
        want.add(f"{tag}.out")
        for name in RB.BACKBONE_PARAMS:
            numel = int(np.prod(shapes[name]))
            if bb_train and name in CONV_BIASES:
                want.add(f"{tag}.gradnoise.{name}")
                assert g[f"{tag}.gradnoise.{name}"].shape == shapes[name]
            elif numel <= WHOLE:
                want.add(f"{tag}.grad.{name}")
                assert g[f"{tag}.grad.{name}"].shape == shapes[name]
            else:
                want |= {f"{tag}.gradslice.{name}", f"{tag}.gradnorm.{name}", f"{tag}.gradmax.{name}"}
                assert g[f"{tag}.gradslice.{name}"].shape == slice_of(np.zeros(numel)).shape and g[f"{tag}.gradslice.{name}"].size <= WHOLE
    assert set(g.keys()) == want and len(RB.BACKBONE_PARAMS) == 16


@pytest.mark.parametrize("i", range(len(GRAD_CASES)))
def test_restatement_reproduces_the_reference_gradients_within_a_quarter_of_the_gpu_bound(i):
    """The reference's own fp32 gradients against float64 autograd through the restatement: they may use up a quarter of
    rtol |ref| + atol_frac max|ref|.  The analytically-zero conv biases: the restatement returns (almost) exact zeros, the reference
    noise below 1e-4 max|dW|."""
    idx, B, T, H, W, bb_train = GRAD_CASES[i]
    g, tag = np.load(GRAD_GOLDEN), tag_of(B, T, H, W)
    out, grads = restated(i)
    assert np.abs(g[f"{tag}.out"] - out.numpy()).max() <= 0.25 * 2e-5 + 0.25 * 1e-3 * np.abs(out.numpy()).max()
    for name in RB.BACKBONE_PARAMS:
        ref = grads[name].numpy()
        top = float(np.abs(ref).max())
        if f"{tag}.gradnoise.{name}" in g:
            wtop = float(np.abs(grads[name[:-4] + "weight"].numpy()).max())
            assert top <= 1e-9 * wtop and float(np.abs(g[f"{tag}.gradnoise.{name}"]).max()) <= 1e-4 * wtop, name
            continue
        if f"{tag}.grad.{name}" in g:
            got, want = g[f"{tag}.grad.{name}"].astype(np.float64), ref
        else:
            got, want = g[f"{tag}.gradslice.{name}"].astype(np.float64), slice_of(ref)
            assert float(g[f"{tag}.gradnorm.{name}"]) == pytest.approx(float(np.linalg.norm(ref)), rel=0.25 * RTOL)
            assert float(g[f"{tag}.gradmax.{name}"]) == pytest.approx(top, rel=0.25 * RTOL)
        excess = np.abs(got - want) / (0.25 * (ATOL_FRAC * top + RTOL * np.abs(want)))
        print(f"{tag} {name}: worst |reference - float64| = {excess.max():.4f} of a quarter of the bound")
        assert excess.max() <= 1.0, (name, float(excess.max()))


def test_restatement_operators_equal_torch():
    """The operator-level restatement against torch's own float64 autograd through Conv2d / BatchNorm2d / ReLU / MaxPool2d / mean."""
    torch.manual_seed(1)
    N, H, W, Cin, Cout = 2, 6, 7, 8, 16
    x = torch.randn(N, Cin, H, W, dtype=torch.float64)
    conv = torch.nn.Conv2d(Cin, Cout, 3, 2, 1).double()
    bn = torch.nn.BatchNorm2d(Cout).double().train()
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(-0.3, 0.3)
    xr = x.clone().requires_grad_(True)
    y = conv(xr)
    OH, OW = y.shape[2:]
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])        # noqa: E731
    for src, head in ((RB.DENSE, lambda v: v), (RB.POOL, lambda v: torch.nn.functional.max_pool2d(v, 3, 2, 1)), (RB.AVG, lambda v: v.mean((2, 3)))):
        out = head(torch.relu(bn(y)))
        dout = torch.randn_like(out)
        dy, dgamma, dbeta, dw, db, dx = torch.autograd.grad((out * dout).sum(), [y, bn.weight, bn.bias, conv.weight, conv.bias, xr], retain_graph=True)
        d_rows = dout if src == RB.AVG else rows(dout)
        got = RB.bn2d_bwd(rows(y).detach(), bn.weight.detach(), bn.bias.detach(), d_rows, N, OH, OW, src)
        for a, b in zip(got, (rows(dy), dgamma, dbeta)):
            torch.testing.assert_close(a, b, rtol=1e-9, atol=1e-11)
        assert not bool(RB.undecided(rows(y).detach(), bn.weight.detach(), bn.bias.detach(), d_rows, N, OH, OW, src)[0].any())
        xp = R.pad_pixels(x.permute(0, 2, 3, 1), 1, Cin)
        gw, gb, gx = RB.conv_grads(xp, conv.weight.detach(), conv.bias.detach(), rows(dy), N, H, W, 3, 3)
        torch.testing.assert_close(gw, dw, rtol=1e-9, atol=1e-11)
        torch.testing.assert_close(gb, db, rtol=1e-9, atol=1e-11)
        torch.testing.assert_close(gx, rows(dx), rtol=1e-9, atol=1e-11)
    assert torch.equal(RB.pack_weight_t(conv.weight.detach())[2, 0, 5, 7], conv.weight.detach()[7, 5, 2, 0])


def test_the_switch_is_off_by_default():
    m = frames.FrameVideoEncoder()
    assert m.train_backbone is False and frames.FrameVideoEncoder({"train_backbone": True}).train_backbone is True
    assert [n for n, _ in m.named_parameters() if n.startswith("spatial_backbone.")] == RB.BACKBONE_PARAMS
    named = dict(m.named_parameters())
    assert all(p is named[n] for p, n in zip(m._backbone_params(), RB.BACKBONE_PARAMS))
    assert (frames.SRC_DENSE, frames.SRC_POOL, frames.SRC_AVG) == (RB.DENSE, RB.POOL, RB.AVG) == (frames.PAD, frames.POOL, frames.AVG)
    with pytest.raises(ValueError, match="requires_grad"):                 # still refused, whatever the switch
        frames.FrameVideoEncoder({"train_backbone": True})(torch.zeros(2, 2, 3, 8, 8, requires_grad=True))
    with pytest.raises(RuntimeError):                                      # no CPU fallback with the switch either
        frames.FrameVideoEncoder({"train_backbone": True})(torch.zeros(2, 2, 3, 8, 8))


# ------------------------------------------------------------------------------------------------ the C ABI additions
def test_new_symbols_are_declared_bound_and_exported():
    lib = _lib.load()
    assert {n: len(args) for n, _, args in _lib.FRAME_BWD_SYMBOLS} == BWD_SYMBOLS
    for name, res, args in _lib.FRAME_BWD_SYMBOLS:
        fn = getattr(lib, name)                                           # exported by the built library
        assert fn.restype is (C.c_longlong if name.endswith("_scratch") else C.c_int32) and fn.argtypes == args, name
    assert set(_lib.FRAME_BWD_STRUCTS) == {"bn2d_bwd_args", "conv2d_wgrad_args", "conv2d_dgrad_args"}
    for name, cls in _lib.FRAME_BWD_STRUCTS.items():                      # the ctypes mirrors against the compiler's layout
        assert lib.mmdeer_sizeof(name.encode()) == C.sizeof(cls), name
    assert _lib.FRAME_BWD_CONSTANTS == {"BN2D_BWD_SCRATCH": 1024 * 1024, "BN2D_SRC_DENSE": 0, "BN2D_SRC_POOL": 1, "BN2D_SRC_AVG": 2,
                                        "CONV2D_WGRAD_MAX_SLICES": 256}
    # the three older companion tables and mmdeer.h's are as they were: additions only, in a table of their own
    assert {n: len(args) for n, _, args in _lib.FRAME_SYMBOLS} == FORWARD_SYMBOLS and set(_lib.FRAME_STRUCTS) == {"conv2d_args", "bn2d_args"}
    names = {n for n, _, _ in _lib.FRAME_BWD_SYMBOLS}
    for older in (_lib.SYMBOLS, _lib.VIDEO_SYMBOLS, _lib.FRAME_SYMBOLS, _lib.ROUTE_SYMBOLS):
        assert not names & {n for n, _, _ in older}
    assert not set(_lib.FRAME_BWD_STRUCTS) & (set(_lib.STRUCTS) | set(_lib.VIDEO_STRUCTS) | set(_lib.FRAME_STRUCTS))
    assert {"conv2d_bwd.hip", "bn2d_bwd.hip"} <= set(build.SOURCES)
    assert _header.FRAMES_BWD_HEADER_PATH == build.FRAMES_BWD_HEADER_PATH
    assert os.path.samefile(build.FRAMES_BWD_HEADER_PATH, os.path.join(ROOT, "include", "mmdeer_frames_bwd.h"))
    assert lib.mmdeer_abi_version() == _lib.ABI_VERSION == 16            # additions only


def test_header_layout_matches_the_compiler(tmp_path):
    """Offsets and sizes of every field of the three new structs, as ctypes lays them out, asserted by the compiler on the header."""
    lines = ["#include <stddef.h>", '#include "mmdeer_frames_bwd.h"']
    for cname, cls in _lib._FRAME_BWD_CLASSES.items():
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
    text = _header.read(_header.FRAMES_BWD_HEADER_PATH)
    for bad in (text.replace("int mmdeer_bn2d_bwd(", "int mmdeer_bn2d_bwd(uint16_t f, "),                  # the same strict parser
                text.replace("#define MMDEER_BN2D_SRC_AVG 2", "#define MMDEER_BN2D_SRC_AVG 2\n#if 0\n#endif"),
                text.replace("void* pool_idx;", "void* pool_idx; short s;")):
        assert bad != text
        with pytest.raises(_header.HeaderError):
            _header.parse(bad, _lib._FRAME_BWD_NAMES, {})


A = 1 << 20     # a plausible, aligned address: never dereferenced by the host checks


def _set(a, kw):
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _bnb(**kw):
    a = _lib.Bn2dBwdArgs()
    a.y, a.mean, a.rstd, a.gamma, a.beta, a.dout, a.dy, a.dgamma, a.dbeta, a.scratch, a.pool_idx = (A,) * 11
    a.N, a.H, a.W, a.C, a.act_f32, a.eps, a.src = 2, 5, 3, 128, 0, 1e-5, 0
    return _set(a, kw)


def _wg(**kw):
    a = _lib.Conv2dWgradArgs()
    a.x, a.dy, a.dw, a.dbias, a.scratch, a.scratch_elems = A, A, A, A, A, 1 << 30
    a.N, a.H, a.W, a.Cin, a.Cout, a.k, a.act_f32, a.slices = 2, 9, 7, 64, 128, 3, 0, -1
    return _set(a, kw)


def _dg(**kw):
    a = _lib.Conv2dDgradArgs()
    a.dy, a.wt, a.dx = A, A, A
    a.N, a.H, a.W, a.Cin, a.Cout, a.k, a.act_f32 = 2, 9, 7, 64, 128, 3, 0
    return _set(a, kw)


def _refused(f, arg, msg):
    lib = _lib.load()
    assert f(arg) == -1, msg
    assert msg in lib.mmdeer_last_error(), (msg, lib.mmdeer_last_error())


def test_bn2d_bwd_refuses_on_the_host():
    f = _lib.load().mmdeer_bn2d_bwd
    for kw, msg in [({"C": 32}, b"unsupported C"), ({"C": 1024}, b"unsupported C"), ({"C": 96}, b"unsupported C"), ({"C": 96, "N": 0, "y": None}, b"unsupported C"),
                    ({"N": -1}, b"bad shape"), ({"H": 0}, b"bad shape"), ({"W": 0}, b"bad shape"), ({"src": 3}, b"src"), ({"src": -1}, b"src"),
                    ({"y": None}, b"NULL"), ({"dout": None}, b"NULL"), ({"dy": None}, b"NULL"), ({"mean": None}, b"NULL"), ({"rstd": None}, b"NULL"),
                    ({"gamma": None}, b"NULL"), ({"beta": None}, b"NULL"), ({"dgamma": None}, b"NULL"), ({"dbeta": None}, b"NULL"), ({"scratch": None}, b"NULL"),
                    ({"src": 1, "pool_idx": None}, b"pool_idx"),
                    ({"y": A + 8}, b"misaligned"), ({"dout": A + 4}, b"misaligned"), ({"dy": A + 2}, b"misaligned"), ({"mean": A + 4}, b"misaligned"),
                    ({"dbeta": A + 8}, b"misaligned"), ({"scratch": A + 4}, b"misaligned"), ({"pool_idx": A + 1}, b"misaligned"),
                    ({"N": 1 << 12, "H": 64, "W": 64, "C": 128}, b"2^31")]:
        _refused(f, C.byref(_bnb(**kw)), msg)
    assert f(C.byref(_bnb(N=0, y=None, dout=None, dy=None, mean=None, scratch=None))) == 0
    assert f(C.byref(_bnb(src=0, pool_idx=None, N=0))) == 0                # only the POOL source needs the index bytes
    assert f(None) == -1


def test_wgrad_refuses_on_the_host():
    lib = _lib.load()
    f, q = lib.mmdeer_conv2d_wgrad, lib.mmdeer_conv2d_wgrad_scratch
    shape_cases = [({"k": 5}, b"unsupported kernel size"), ({"k": 7}, b"unsupported kernel size"), ({"k": 7, "Cin": 4}, b"unsupported kernel size"),
                   ({"Cin": 12}, b"unsupported kernel size"), ({"Cin": 4}, b"unsupported kernel size"), ({"Cin": 0}, b"unsupported kernel size"),
                   ({"Cout": 96}, b"unsupported Cout"), ({"Cout": 0}, b"unsupported Cout"), ({"N": -1}, b"bad shape"), ({"H": 0}, b"bad shape"),
                   ({"W": 0}, b"bad shape"), ({"slices": 0}, b"slices"), ({"slices": -2}, b"slices"), ({"slices": 257}, b"slices"),
                   ({"N": 1 << 10, "H": 255, "W": 127}, b"2^31"),                   # the padded input: 2^10 * 257 * 129 * 64 >= 2^31
                   ({"N": 1 << 12, "H": 127, "W": 127, "Cin": 8, "Cout": 512}, b"2^31"),   # dy: 2^12 * 64 * 64 * 512 = 2^33
                   ({"Cin": 512, "Cout": 2048, "slices": 256}, b"scratch has 2^31")]   # 256 slices of 2048 * 9 * 512 partials
    for kw, msg in shape_cases:
        _refused(f, C.byref(_wg(**kw)), msg)
        assert q(C.byref(_wg(**kw))) == -1 and msg in lib.mmdeer_last_error(), kw      # the query refuses the same shapes
    for kw, msg in [({"x": None}, b"NULL"), ({"dy": None}, b"NULL"), ({"dw": None}, b"NULL"), ({"scratch": None}, b"NULL"),
                    ({"x": A + 8}, b"misaligned"), ({"dy": A + 4}, b"misaligned"), ({"dw": A + 4}, b"misaligned"), ({"dbias": A + 8}, b"misaligned"),
                    ({"scratch": A + 4}, b"misaligned")]:
        _refused(f, C.byref(_wg(**kw)), msg)
    assert f(None) == -1 and q(None) == -1
    # the query: slices x (Cout x k x KWe Cp partials + Cout bias partials); it looks at no pointer
    assert q(C.byref(_wg(slices=5, x=None, dy=None, dw=None, scratch=None))) == 5 * (128 * 3 * 192 + 128)
    assert q(C.byref(_wg(slices=1, k=7, Cin=3, Cout=64))) == 64 * 7 * 64 + 64 and q(C.byref(_wg(slices=1, k=7, Cin=3, Cout=64, act_f32=1))) == 64 * 7 * 32 + 64
    auto = q(C.byref(_wg()))                                               # M = 2 * 5 * 4 = 40 rows: one K-tile, so one slice
    assert auto == 128 * 3 * 192 + 128
    _refused(f, C.byref(_wg(scratch_elems=auto - 1)), b"scratch too short")
    _refused(f, C.byref(_wg(slices=2, scratch_elems=auto)), b"scratch too short")
    assert f(C.byref(_wg(N=0, x=None, dy=None, dw=None, dbias=None, scratch=None, scratch_elems=0))) == 0


def test_dgrad_and_pack_t_refuse_on_the_host():
    lib = _lib.load()
    f = lib.mmdeer_conv2d_dgrad
    for kw, msg in [({"k": 7, "Cin": 3}, b"unsupported kernel size"), ({"k": 7}, b"no input gradient"), ({"k": 5}, b"unsupported kernel size"),
                    ({"Cin": 12}, b"unsupported kernel size"), ({"Cin": 4}, b"unsupported kernel size"), ({"Cin": 0}, b"unsupported kernel size"),
                    ({"Cout": 96}, b"unsupported Cout"), ({"Cout": 0}, b"unsupported Cout"), ({"N": -1}, b"bad shape"), ({"H": 0}, b"bad shape"), ({"W": 0}, b"bad shape"),
                    ({"dy": None}, b"NULL"), ({"wt": None}, b"NULL"), ({"dx": None}, b"NULL"), ({"dy": A + 8}, b"misaligned"), ({"wt": A + 4}, b"misaligned"),
                    ({"dx": A + 2}, b"misaligned"),
                    ({"N": 1 << 10, "H": 255, "W": 129}, b"2^31"),                   # dx: 2^10 * 255 * 129 * 64 >= 2^31
                    ({"N": 1 << 12, "H": 127, "W": 127, "Cin": 8, "Cout": 512}, b"2^31")]:   # dy: (2^12 * 64 * 64 + 1) * 512
        _refused(f, C.byref(_dg(**kw)), msg)
    assert f(C.byref(_dg(Cin=4, act_f32=1, N=0, dy=None, wt=None, dx=None))) == 0      # fp32: a 16-byte chunk is 4 elements
    assert f(C.byref(_dg(N=0, dy=None, wt=None, dx=None))) == 0
    assert f(None) == -1
    p = lib.mmdeer_conv2d_pack_t
    for args, msg in [((A, 64, 3, 7, A, 0, None), b"unsupported kernel size"), ((A, 64, 64, 5, A, 0, None), b"unsupported kernel size"),
                      ((A, 64, 4, 3, A, 0, None), b"unsupported kernel size"), ((A, 100, 64, 3, A, 0, None), b"unsupported Cout"),
                      ((None, 64, 64, 3, A, 0, None), b"NULL"), ((A, 64, 64, 3, None, 0, None), b"NULL"), ((A, 64, 64, 3, A + 8, 0, None), b"misaligned"),
                      ((A + 4, 64, 64, 3, A, 0, None), b"misaligned")]:
        assert p(*args) == -1 and msg in lib.mmdeer_last_error(), (args, lib.mmdeer_last_error())
