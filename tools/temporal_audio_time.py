#!/usr/bin/env python3
"""Time mmdeer.temporal.TemporalAudioEncoder (eval forward, and forward + backward) for B in {1024, 4096}, T in {8, 32},
fp32 and bf16, and beside each figure the same model as torch.nn.LSTM (MIOpen) + an eager attention pool and output
projection on the same GPU, as a yardstick.  Prints one JSON object: per configuration the median / min / max of `--reps`
timed repetitions (each the mean over `--iters` back-to-back calls between two events), after `--warmup` calls.

    python tools/temporal_audio_time.py [--reps 7] [--iters 5] [--warmup 3] [--B 1024,4096] [--T 8,32]
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

from mmdeer import temporal  # noqa: E402


class TorchEncoder(torch.nn.Module):
    """the yardstick: nn.LSTM (MIOpen) + the eager pool / projection, parameters shared with `m`"""

    def __init__(self, m):
        super().__init__()
        self.m = m

    def forward(self, x):
        h, _ = self.m.lstm(x)
        a = torch.softmax(self.m.attention[2](torch.tanh(self.m.attention[0](h))), dim=1)
        return self.m.output_projection((h * a).sum(1))


def timed(fn, reps, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / iters)
    return {"median_ms": round(statistics.median(out), 4), "min_ms": round(min(out), 4), "max_ms": round(max(out), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--B", default="1024,4096")
    ap.add_argument("--T", default="8,32")
    a = ap.parse_args()
    dev = "cuda:0"
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "iters": a.iters, "warmup": a.warmup, "rows": []}
    for compute in ("fp32", "bf16"):
        for B in [int(v) for v in a.B.split(",")]:
            for T in [int(v) for v in a.T.split(",")]:
                torch.manual_seed(0)
                m = temporal.TemporalAudioEncoder(compute_dtype=compute).to(dev).eval()
                x = torch.randn(B, T, 84, device=dev)
                w = torch.randn(B, 512, device=dev)
                row = {"compute": compute, "B": B, "T": T}

                def fwd():
                    with torch.no_grad():
                        m(x)

                def step():
                    for p in m.parameters():
                        p.grad = None
                    (m(x) * w).sum().backward()

                row["mmdeer_fwd"] = timed(fwd, a.reps, a.iters, a.warmup)
                row["mmdeer_fwd_bwd"] = timed(step, a.reps, a.iters, a.warmup)
                # yardstick: torch.nn.LSTM (MIOpen) in the same dtype
                dt = torch.float32 if compute == "fp32" else torch.bfloat16
                # train mode (MIOpen's RNN backward refuses eval mode) with every dropout off
                y = TorchEncoder(temporal.TemporalAudioEncoder({"dropout": 0.0}).to(dev).to(dt).train())
                xd, wd = x.to(dt), w.to(dt)

                def tfwd():
                    with torch.no_grad():
                        y(xd)

                def tstep():
                    for p in y.parameters():
                        p.grad = None
                    (y(xd) * wd).sum().backward()

                try:
                    row["torch_fwd"] = timed(tfwd, a.reps, a.iters, a.warmup)
                    row["torch_fwd_bwd"] = timed(tstep, a.reps, a.iters, a.warmup)
                except RuntimeError as e:                # e.g. a dtype the RNN backend does not take
                    row["torch_error"] = str(e).splitlines()[0][:200]
                res["rows"].append(row)
                print(json.dumps(row), file=sys.stderr, flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
