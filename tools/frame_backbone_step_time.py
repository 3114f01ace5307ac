#!/usr/bin/env python3
"""Time one training step of the frame video encoder's Conv2d backbone -- forward + backward through
mmdeer.frames.FrameVideoEncoder(train_backbone=True).extract_spatial_features, batch statistics -- at B x T = 32 x 8 frames of
224 x 224, fp32 and bf16, and beside each figure the same nn.Sequential through torch autograd in the same dtype on the same GPU
(MIOpen), as a yardstick: the two measured alternately, repetition by repetition.  The loss is sum(features * w) on both sides.

It also times each launch of the backward alone, per layer (mmdeer_bn2d_bwd, mmdeer_conv2d_wgrad, mmdeer_conv2d_pack_t +
mmdeer_conv2d_dgrad), and for the two GEMM-shaped ones reports the useful FLOP/s -- 2 * N * OH * OW * Cout * Cin * k * k each -- and its
share of the calibrated bf16 MFMA rate (profiles/r04_calibration.txt), so that a slow total names its launch.  Prints one JSON object
(and writes it to --out): per cell the median / min / max of `--reps` timed repetitions (each the mean over `--iters` back-to-back
calls between two events; `--layer-iters` for the per-launch cells), after `--warmup` calls.

    python tools/frame_backbone_step_time.py [--reps 7] [--iters 3] [--layer-iters 20] [--warmup 2] [--B 32] [--T 8] [--size 224] [--out profiles/frame_backbone_step_time.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402
from frame_encoder_time import _kw, timed_alternating  # noqa: E402

from mmdeer import frames  # noqa: E402

MFMA_BF16_TFLOPS = 1970.5       # profiles/r04_calibration.txt


def launch_cells(m, n, size, dt, a):
    """each backward launch alone, per layer, on the shapes of n frames"""
    dev, out = "cuda:0", {}
    sb = m.spatial_backbone
    for li, ((ci, bi, dest), (k, cin, cout, h, w, oh, ow, elems)) in enumerate(zip(frames.LAYERS, frames.plan(n, size, size, dt))):
        cp = frames.pixel_channels(cin, k, dt)
        xp = (torch.randn(elems // cp, cp, device=dev) * 0.5).to(dt)
        bn = sb[bi]
        gamma, beta = bn.weight.detach().float(), bn.bias.detach().float()
        y = frames.conv2d_s2(xp, frames.conv2d_pack(sb[ci].weight, dt), sb[ci].bias.detach().float(), n, h, w, cin)
        mean, rstd = frames.bn2d_stats(y, n, oh, ow, None, bn.eps)
        src = (frames.SRC_POOL, frames.SRC_DENSE, frames.SRC_DENSE, frames.SRC_AVG)[li]
        rows = {frames.SRC_POOL: n * frames.conv_out(oh, 3) * frames.conv_out(ow, 3), frames.SRC_DENSE: n * oh * ow, frames.SRC_AVG: n}[src]
        dout = torch.randn(rows, cout, device=dev)
        dout = dout if src == frames.SRC_AVG else dout.to(dt)
        scratch = torch.empty(frames._lib.BN2D_BWD_SCRATCH, device=dev)
        dy = frames.bn2d_bwd(y, n, oh, ow, mean, rstd, gamma, beta, dout, src, bn.eps, scratch=scratch, zero_row=True)[0]
        fns = {"bn2d_bwd": lambda: frames.bn2d_bwd(y, n, oh, ow, mean, rstd, gamma, beta, dout, src, bn.eps, scratch=scratch, zero_row=True),
               "wgrad": lambda: frames.conv2d_wgrad(xp, dy, n, h, w, cin, k)}
        if li:
            wt = frames.conv2d_pack_t(sb[ci].weight, dt)
            fns["pack_t"] = lambda: frames.conv2d_pack_t(sb[ci].weight, dt)
            fns["dgrad"] = lambda: frames.conv2d_dgrad(dy, wt, n, h, w)
        cell = timed_alternating(fns, a.reps, a.layer_iters, a.warmup)
        flop = 2.0 * n * oh * ow * cout * cin * k * k
        for name in ("wgrad", "dgrad"):
            if name in cell:
                cell[name]["useful_gflop"] = round(flop / 1e9, 3)
                cell[name]["tflops"] = round(flop / (cell[name]["median_ms"] * 1e-3) / 1e12, 2)
                cell[name]["share_of_bf16_mfma_rate"] = round(cell[name]["tflops"] / MFMA_BF16_TFLOPS, 4)
        cell["shape"] = {"k": k, "Cin": cin, "Cout": cout, "H": h, "W": w, "M": n * oh * ow, "source": ("pool", "dense", "dense", "avg")[li]}
        out[f"layer{li + 1}"] = cell
        del xp, y, dy, dout
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--layer-iters", type=int, default=20, help="back-to-back calls per repetition of a per-launch cell")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--T", type=int, default=8)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_backbone_step_time.json"))
    a = ap.parse_args()
    dev = "cuda:0"
    torch.manual_seed(0)
    x = torch.randn(a.B, a.T, 3, a.size, a.size, device=dev)
    n = a.B * a.T
    w = torch.randn(a.B, a.T, 512, device=dev)
    res = {"device": torch.cuda.get_device_name(0), "frames": n, "size": a.size, "reps": a.reps, "iters": a.iters, "layer_iters": a.layer_iters,
           "warmup": a.warmup, "cells": {}}
    for compute in ("fp32", "bf16"):
        dt = torch.float32 if compute == "fp32" else torch.bfloat16
        m = frames.FrameVideoEncoder({"dropout": 0.0, "train_backbone": True}, compute_dtype=compute).to(dev).train()
        yard = torch.nn.Sequential(*[type(l)(**_kw(l)) for l in m.spatial_backbone]).to(dev)
        yard.load_state_dict(m.spatial_backbone.state_dict())
        yard = yard.to(dt).train()
        xt = x.reshape(n, 3, a.size, a.size).to(dt)

        def hip_step():
            for p in m.spatial_backbone.parameters():
                p.grad = None
            (m.extract_spatial_features(x) * w).sum().backward()

        def torch_step():
            for p in yard.parameters():
                p.grad = None
            (yard(xt).reshape(a.B, a.T, 512).float() * w).sum().backward()

        def hip_forward():
            with torch.no_grad():
                m.extract_spatial_features(x)

        def torch_forward():
            with torch.no_grad():
                yard(xt)

        cell = {"step": timed_alternating({"hip": hip_step, "torch": torch_step}, a.reps, a.iters, a.warmup),
                "forward": timed_alternating({"hip": hip_forward, "torch": torch_forward}, a.reps, a.iters, a.warmup)}
        cell["step"]["hip_over_torch"] = round(cell["step"]["hip"]["median_ms"] / cell["step"]["torch"]["median_ms"], 3)
        for p in list(m.parameters()) + list(yard.parameters()):
            p.grad = None
        cell["launches"] = launch_cells(m, n, a.size, dt, a)
        res["cells"][compute] = cell
        del m, yard, xt
        torch.cuda.empty_cache()
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
