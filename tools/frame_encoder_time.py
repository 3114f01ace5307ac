#!/usr/bin/env python3
"""Time mmdeer.frames.FrameVideoEncoder.extract_spatial_features (the Conv2d backbone, evaluation mode and training mode under
no_grad) at B x T = 32 x 8 frames of 224 x 224, fp32 and bf16, and beside each figure the same nn.Sequential run by torch in the same
dtype on the same GPU (its convolutions through MIOpen), as a yardstick -- the two measured alternately, repetition by repetition.

It also times each layer's convolution launch alone (mmdeer_conv2d_s2) and reports its achieved FLOP/s from the useful work
2 * N * OH * OW * Cout * Cin * k * k, and the BatchNorm launches of each layer together, so that a slow total names its layer.
Prints one JSON object (and writes it to --out): per cell the median / min / max of `--reps` timed repetitions (each the mean over
`--iters` back-to-back calls between two events -- `--layer-iters` for the per-layer cells, whose calls are 0.01 to 1 ms, so that a timed
window stays in the milliseconds), after `--warmup` calls.

    python tools/frame_encoder_time.py [--reps 7] [--iters 10] [--layer-iters 50] [--warmup 3] [--B 32] [--T 8] [--size 224] [--out profiles/frame_encoder_time.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from mmdeer import frames  # noqa: E402


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


def layer_cells(m, n, size, dt, a):
    """each layer's convolution launch alone, and its BatchNorm launches (statistics + apply) together, on the shapes of n frames"""
    dev, out = "cuda:0", {}
    sb = m.spatial_backbone
    for (ci, bi, dest), (k, cin, cout, h, w, oh, ow, elems) in zip(frames.LAYERS, frames.plan(n, size, size, dt)):
        cp = frames.pixel_channels(cin, k, dt)
        xp = (torch.randn(elems // cp, cp, device=dev) * 0.5).to(dt)
        img, bias, bn = frames.conv2d_pack(sb[ci].weight, dt), sb[ci].bias.detach().float(), sb[bi]
        gamma, beta = bn.weight.detach().float(), bn.bias.detach().float()
        y = frames.conv2d_s2(xp, img, bias, n, h, w, cin)

        def bn_train():
            mean, rstd = frames.bn2d_stats(y, n, oh, ow, None, bn.eps)
            frames.bn2d_apply(y, n, oh, ow, mean, rstd, gamma, beta, dest, bn.eps)

        cell = timed_alternating({"conv": lambda: frames.conv2d_s2(xp, img, bias, n, h, w, cin),
                                  "bn_eval": lambda: frames.bn2d_apply(y, n, oh, ow, bn.running_mean, bn.running_var, gamma, beta, dest, bn.eps, running=True),
                                  "bn_train": bn_train}, a.reps, a.layer_iters, a.warmup)
        flop = 2.0 * n * oh * ow * cout * cin * k * k
        cell["conv"]["useful_gflop"] = round(flop / 1e9, 3)
        cell["conv"]["tflops"] = round(flop / (cell["conv"]["median_ms"] * 1e-3) / 1e12, 2)
        cell["shape"] = {"k": k, "Cin": cin, "Cout": cout, "H": h, "W": w, "M": n * oh * ow, "K_per_tap": frames.taps(k) * cp}
        out[f"conv{len(out) + 1}"] = cell
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--layer-iters", type=int, default=50, help="back-to-back calls per repetition of a per-layer cell")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--T", type=int, default=8)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_encoder_time.json"))
    a = ap.parse_args()
    dev = "cuda:0"
    torch.manual_seed(0)
    x = torch.randn(a.B, a.T, 3, a.size, a.size, device=dev)
    n = a.B * a.T
    res = {"device": torch.cuda.get_device_name(0), "frames": n, "size": a.size, "reps": a.reps, "iters": a.iters, "layer_iters": a.layer_iters, "warmup": a.warmup,
           "useful_gflop": round(sum(2.0 * n * oh * ow * cout * cin * k * k for k, cin, cout, _, _, oh, ow, _ in
                                     frames.plan(n, a.size, a.size, torch.float32)) / 1e9, 2), "cells": {}}
    for compute in ("fp32", "bf16"):
        dt = torch.float32 if compute == "fp32" else torch.bfloat16
        m = frames.FrameVideoEncoder({"dropout": 0.0}, compute_dtype=compute).to(dev)
        yard = m.spatial_backbone if compute == "fp32" else torch.nn.Sequential(*[type(l)(**_kw(l)) for l in m.spatial_backbone]).to(dev).to(dt)
        if compute != "fp32":
            yard.load_state_dict(m.spatial_backbone.state_dict())
        xt = x.reshape(n, 3, a.size, a.size).to(dt)
        cell = {}
        with torch.no_grad():
            for mode in ("eval", "train"):
                m.spatial_backbone.train(mode == "train")
                yard.train(mode == "train")
                t = timed_alternating({"hip": lambda: m.extract_spatial_features(x), "torch": lambda: yard(xt)}, a.reps, a.iters, a.warmup)
                t["hip"]["tflops"] = round(res["useful_gflop"] / t["hip"]["median_ms"], 2)
                t["torch"]["tflops"] = round(res["useful_gflop"] / t["torch"]["median_ms"], 2)
                cell[mode] = t
            m.spatial_backbone.eval()
            cell["layers"] = layer_cells(m, n, a.size, dt, a)
        res["cells"][compute] = cell
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


def _kw(l):
    """constructor arguments of a backbone layer, for the yardstick's copy in another dtype"""
    if isinstance(l, torch.nn.Conv2d):
        return {"in_channels": l.in_channels, "out_channels": l.out_channels, "kernel_size": l.kernel_size, "stride": l.stride, "padding": l.padding}
    if isinstance(l, torch.nn.BatchNorm2d):
        return {"num_features": l.num_features}
    if isinstance(l, torch.nn.MaxPool2d):
        return {"kernel_size": l.kernel_size, "stride": l.stride, "padding": l.padding}
    if isinstance(l, torch.nn.AdaptiveAvgPool2d):
        return {"output_size": l.output_size}
    return {"inplace": True}


if __name__ == "__main__":
    main()
