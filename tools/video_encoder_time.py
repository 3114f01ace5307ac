#!/usr/bin/env python3
"""Time mmdeer.video.TemporalVideoEncoder (training-mode forward under no_grad, and forward + backward; dropout off) for
(B, T) in {1024, 4096} x {8, 32}, fp32 and bf16, and beside each figure the same model restated in torch.nn (nn.Conv1d,
nn.BatchNorm1d, an eager attention pool) in the same dtype on the same GPU, as a yardstick.

It also times the convolution launch alone (mmdeer_conv3_time) and reports its achieved FLOP/s from 2 * T * B * 1536 * 512,
next to two yardsticks measured alternately with it, repetition by repetition:
  gemm_k1536  one mmdeer_gemm at M = T * B, N = 512, K = 1536 (the same FLOPs as one dense product, automatic tile)
  gemm_x3     the same convolution as three mmdeer_gemm calls on the row-shifted views, the second and third accumulating
              (accumulate needs an fp32 C, so under bf16 this lowering ends with one mmdeer_convert to bf16)
Prints one JSON object (and writes it to --out): per cell the median / min / max of `--reps` timed repetitions (each the mean
over `--iters` back-to-back calls between two events), after `--warmup` calls.

    python tools/video_encoder_time.py [--reps 7] [--iters 5] [--warmup 3] [--B 1024,4096] [--T 8,32] [--out profiles/video_encoder_time.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from mmdeer import _lib, video  # noqa: E402

W = 512


class TorchEncoder(torch.nn.Module):
    """the yardstick: the module's own submodules run by torch (nn.Conv1d / nn.BatchNorm1d through MIOpen, eager pool)"""

    def __init__(self, m):
        super().__init__()
        self.m = m

    def forward(self, x):
        m = self.m
        h = m.spatial_projection(x)
        h = m.temporal_cnn(h.transpose(1, 2)).transpose(1, 2)
        a = m.temporal_attention(h)
        return m.output_projection((h * a).sum(1))


def summary(out):
    return {"median_ms": round(statistics.median(out), 4), "min_ms": round(min(out), 4), "max_ms": round(max(out), 4)}


def one(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def timed(fn, reps, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    return summary([one(fn, iters) for _ in range(reps)])


def timed_alternating(fns, reps, iters, warmup):
    """{name: fn} measured in turn within every repetition, so that a drift of the box hits all of them alike"""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            out[k].append(one(fn, iters))
    return {k: summary(v) for k, v in out.items()}


def conv_cell(B, T, compute, a):
    lib, dev = _lib.load(), "cuda:0"
    dt = torch.float32 if compute == "fp32" else torch.bfloat16
    f32, R, s = int(compute == "fp32"), T * B, _lib.current_stream()
    xp = video.padded(T, B, dt, dev)
    video.interior(xp, B).copy_(torch.randn(R, W, device=dev))
    w = torch.randn(W, W, 3, device=dev) * 0.03
    bias = torch.randn(W, device=dev)
    img, _ = video.conv3_pack(w, dt, False)
    y = torch.empty(R, W, dtype=dt, device=dev)
    # yardstick 1: one dense product of the same FLOPs
    A1, W1 = torch.randn(R, 3 * W, device=dev).to(dt), torch.randn(W, 3 * W, device=dev).to(dt)
    g1 = _lib.gemm_args(A=A1.data_ptr(), W=W1.data_ptr(), C=y.data_ptr(), bias=bias.data_ptr(), M=R, N=W, K=3 * W, lda=3 * W, ldw=3 * W,
                        ldc=W, a_f32=f32, w_f32=f32, c_f32=f32, compute_f32=f32, stream=s)
    # yardstick 2: three products on the row-shifted views into an fp32 C
    c32 = y if f32 else torch.empty(R, W, device=dev)
    g3 = [_lib.gemm_args(A=xp[j * B:].data_ptr(), W=img[j].data_ptr(), C=c32.data_ptr(), bias=bias.data_ptr() if j == 0 else None, M=R, N=W,
                         K=W, lda=W, ldw=W, ldc=W, a_f32=f32, w_f32=f32, c_f32=1, accumulate=int(j > 0), compute_f32=f32, stream=s) for j in range(3)]

    def gemm_x3():
        for g in g3:
            _lib.check(lib.mmdeer_gemm(C.byref(g)))
        if not f32:
            _lib.check(lib.mmdeer_convert(c32.data_ptr(), 1, y.data_ptr(), 0, R * W, s))

    ca = _lib.Conv3TimeArgs()        # built once, like the yardsticks' argument structs: the loop times launches, not host set-up
    ca.x, ca.ld_x, ca.w, ca.bias, ca.y, ca.ld_y = xp.data_ptr(), W, img.data_ptr(), bias.data_ptr(), y.data_ptr(), W
    ca.T, ca.B, ca.C, ca.N, ca.act_f32, ca.tile, ca.stream = T, B, W, W, f32, -1, s
    fns = {"conv3_time": lambda: _lib.check(lib.mmdeer_conv3_time(C.byref(ca))),
           "gemm_k1536": lambda: _lib.check(lib.mmdeer_gemm(C.byref(g1))),
           "gemm_x3": gemm_x3}
    fns["conv3_time"]()
    want = y.clone()
    gemm_x3()
    torch.cuda.synchronize()
    err = float((y.float() - want.float()).norm() / want.float().norm())          # the two lowerings agree
    row = {"compute": compute, "B": B, "T": T, "lowerings_rel_diff": err, **timed_alternating(fns, a.reps, 4 * a.iters, a.warmup)}
    flop = 2.0 * R * 3 * W * W
    for k in fns:
        row[k]["tflops"] = round(flop / (row[k]["median_ms"] * 1e-3) / 1e12, 1)
    route = C.create_string_buffer(256)
    lib.mmdeer_gemm_route(C.byref(g1), route, len(route))
    row["gemm_k1536_route"] = route.value.decode()
    lib.mmdeer_gemm_route(C.byref(g3[1]), route, len(route))
    row["gemm_x3_route"] = route.value.decode()
    return row


def module_cell(B, T, compute, a):
    dev = "cuda:0"
    torch.manual_seed(0)
    m = video.TemporalVideoEncoder({"dropout": 0.0}, compute_dtype=compute).to(dev).train()
    params = [p for n, p in m.named_parameters() if not n.startswith("spatial_backbone.")]
    x, w = torch.randn(B, T, W, device=dev), torch.randn(B, W, device=dev)
    row = {"compute": compute, "B": B, "T": T}

    def fwd():
        with torch.no_grad():
            m(x)

    def step():
        for p in params:
            p.grad = None
        (m(x) * w).sum().backward()

    row["mmdeer_fwd"] = timed(fwd, a.reps, a.iters, a.warmup)
    row["mmdeer_fwd_bwd"] = timed(step, a.reps, a.iters, a.warmup)
    dt = torch.float32 if compute == "fp32" else torch.bfloat16
    y = TorchEncoder(video.TemporalVideoEncoder({"dropout": 0.0}).to(dev).to(dt).train())
    yparams = [p for n, p in y.named_parameters() if "spatial_backbone." not in n]
    xd, wd = x.to(dt), w.to(dt)

    def tfwd():
        with torch.no_grad():
            y(xd)

    def tstep():
        for p in yparams:
            p.grad = None
        (y(xd) * wd).sum().backward()

    try:
        row["torch_fwd"] = timed(tfwd, a.reps, a.iters, a.warmup)
        row["torch_fwd_bwd"] = timed(tstep, a.reps, a.iters, a.warmup)
    except RuntimeError as e:                # e.g. a dtype a backend does not take
        row["torch_error"] = str(e).splitlines()[0][:200]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--B", default="1024,4096")
    ap.add_argument("--T", default="8,32")
    ap.add_argument("--only", default="", help="'conv' or 'module': one of the two tables")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "iters": a.iters, "warmup": a.warmup, "conv": [], "module": []}
    cells = [(c, B, T) for c in ("fp32", "bf16") for B in map(int, a.B.split(",")) for T in map(int, a.T.split(","))]
    for name, cell in (("conv", conv_cell), ("module", module_cell)):
        if a.only and a.only != name:
            continue
        for compute, B, T in cells:
            row = cell(B, T, compute, a)
            res[name].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
            torch.cuda.empty_cache()
    text = json.dumps(res, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
