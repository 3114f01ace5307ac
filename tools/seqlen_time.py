#!/usr/bin/env python3
"""What per-sample lengths cost and what the early stop buys: the training step (forward + backward) of
mmdeer.temporal.TemporalAudioEncoder on a padded batch, B in {32, 256}, T = 33, bf16 and fp32, under four variants

    none     lengths=None (the plain entries)
    full     every length T (the length entries, no step skipped)
    random   uniform random lengths in [T / 4, T], unsorted (most workgroups hold a long row)
    sorted   the same lengths sorted, longest first (whole workgroups are short and stop early)

All variants of a configuration run in ONE process, interleaved: each repetition times every variant once (`--iters` back-to-back
steps between two device events), after `--warmup` steps of every variant; the figure is the median over `--reps` repetitions, with
min and max.  Prints one JSON object and, with --out, writes it to a file.

    python tools/seqlen_time.py [--reps 15] [--iters 10] [--warmup 5] [--out profiles/seqlen_step_time.json]

Against an earlier build of the library, which has no length entries, only `none` can run:

    python tools/bench_with_lib.py <that build's .so> tools/seqlen_time.py --plain-only
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

from mmdeer import _lib, temporal  # noqa: E402

T = 33


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--B", default="32,256")
    ap.add_argument("--plain-only", action="store_true", help="the library has no length entries (an earlier build): time lengths=None alone")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.plain_only:                       # bind and check only what that build exports
        _lib.SEQLEN_SYMBOLS, _lib.SEQLEN_STRUCTS = [], {}
    dev = "cuda:0"
    res = {"device": torch.cuda.get_device_name(0), "library": os.path.basename(_lib.lib_path()), "T": T, "reps": a.reps, "iters": a.iters,
           "warmup": a.warmup, "what": "TemporalAudioEncoder training step (forward + backward), ms", "rows": []}
    for compute in ("bf16", "fp32"):
        for B in [int(v) for v in a.B.split(",")]:
            torch.manual_seed(0)
            m = temporal.TemporalAudioEncoder(compute_dtype=compute).to(dev).train()
            x = torch.randn(B, T, 84, device=dev)
            w = torch.randn(B, 512, device=dev)
            rnd = torch.randint(T // 4, T + 1, (B,), generator=torch.Generator().manual_seed(B)).to(torch.int32)
            variants = {"none": None}
            if not a.plain_only:
                variants.update({"full": torch.full((B,), T, dtype=torch.int32, device=dev), "random": rnd.to(dev),
                                 "sorted": rnd.sort(descending=True).values.to(dev)})

            def step(n):
                for p in m.parameters():
                    p.grad = None
                y = m(x) if n is None else m(x, n)
                (y * w).sum().backward()

            for n in variants.values():
                for _ in range(a.warmup):
                    step(n)
            torch.cuda.synchronize()
            times = {k: [] for k in variants}
            for _ in range(a.reps):
                for k, n in variants.items():                     # interleaved: every variant once per repetition
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.iters):
                        step(n)
                    e1.record()
                    torch.cuda.synchronize()
                    times[k].append(e0.elapsed_time(e1) / a.iters)
            row = {"compute": compute, "B": B, "mean_length": round(float(rnd.float().mean()), 2)}
            for k, v in times.items():
                row[k] = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
            res["rows"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
