#!/usr/bin/env python3
"""Time the BERT fine-tuning step eagerly and as one HIP graph (mmdeer.train_graph.capture_train_step), in one process:

  eager             host dropout counters, ModuleAdamW.for_module (non-capturable): the step as it was
  eager_capturable  the same with ModuleAdamW(capturable=True): the device step count and lr records, still launched by the host
  replay            capture_train_step's graph: one launch of the whole step from the host

on TemporalTextEncoder(bert=BertEncoder(BERT-base, finetune_layers=6, dropout=True)) + nn.Linear(512, 3) + MSE, L = 128, clip 1.0,
decay 0 on LayerNorm and biases.  Cells: bf16 at B = 8 (bound by the host's launch rate) and B = 32, fp32 at B = 8.  Every variant has a
model copy of its own from one state dict; a figure is a window of ``--iters`` steps between two device events divided by the steps,
the variants alternating window by window, ``--reps`` windows each after ``--warmup`` steps; min, median and max are kept.

``--root DIR --only eager`` runs the eager variant against another tree (the parent commit's, with its own library), as one process
after the other on the same box: that tree needs none of what this change adds.  Prints one JSON object; ``--out`` also writes it.

    python tools/bert_train_graph_time.py [--reps 30] [--iters 5] [--warmup 5] [--cells bf16:8,bf16:32,fp32:8] [--only eager,eager_capturable,replay]
                                          [--root DIR --label NAME] [--out profiles/bert_train_graph_time.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--cells", default="bf16:8,bf16:32,fp32:8")
ap.add_argument("--only", default="eager,eager_capturable,replay")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--label", default="this build")
ap.add_argument("--out", default=None)
ARGS = ap.parse_args()
sys.path.insert(0, os.path.abspath(ARGS.root))

import torch  # noqa: E402
from torch import nn  # noqa: E402

from mmdeer import bert, text  # noqa: E402
from mmdeer.optim import ModuleAdamW  # noqa: E402

L, TAIL, LR, CLIP, DEV = 128, 6, 2e-5, 1.0, "cuda:0"


class Model(nn.Module):
    def __init__(self, compute):
        super().__init__()
        self.enc = text.TemporalTextEncoder({"hidden_dim": 512}, compute, bert=bert.BertEncoder(None, compute, finetune_layers=TAIL, dropout=True))
        self.head = nn.Linear(512, 3)

    def forward(self, ids, mask, target):
        return nn.functional.mse_loss(self.head(self.enc(ids, mask)), target)


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def cell(compute, B, only, sd):
    gen = torch.Generator().manual_seed(B)
    ids = torch.randint(1, 30000, (B, L), generator=gen).to(DEV)
    mask = torch.ones(B, L, dtype=torch.int64)
    mask[B // 2:, L // 2:] = 0
    mask, target = mask.to(DEV), torch.randn(B, 3, generator=gen).to(DEV)
    fns = {}
    for v in only:
        m = Model(compute)
        m.load_state_dict(sd)
        m = m.to(DEV).train()
        named = [(n, p) for n, p in m.named_parameters() if p.requires_grad]
        groups = [{"params": [p for _, p in named if p.ndim >= 2], "weight_decay": 0.01}, {"params": [p for _, p in named if p.ndim < 2], "weight_decay": 0.0}]
        kw = {} if v == "eager" else {"capturable": True}
        opt = ModuleAdamW.for_module(m, groups, lr=LR, max_grad_norm=CLIP, **kw)
        if v == "replay":
            from mmdeer.train_graph import capture_train_step
            replay = capture_train_step(m, opt, [ids.clone(), mask.clone(), target.clone()])
            fns[v] = lambda replay=replay: replay(ids, mask, target)
        else:
            def step(m=m, opt=opt):
                for p in m.parameters():
                    p.grad = None
                m(ids, mask, target).backward()
                opt.step()
            fns[v] = step
    for fn in fns.values():
        for _ in range(ARGS.warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(ARGS.reps):
        for k, fn in fns.items():
            ms[k].append(window(fn, ARGS.iters))
    out = {"compute": compute, "B": B, "L": L, **{k: stats(v) for k, v in ms.items()}}
    if "replay" in ms and "eager" in ms:
        out["replay_over_eager_median"] = round(out["replay"]["median_ms"] / out["eager"]["median_ms"], 4)
        out["replay_over_eager_min"] = round(out["replay"]["min_ms"] / out["eager"]["min_ms"], 4)
    return out


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bert_train_graph_time.py measures on the GPU: none found")
    only = ARGS.only.split(",")
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "tree": ARGS.label, "reps": ARGS.reps, "iters": ARGS.iters,
           "warmup": ARGS.warmup, "model": f"TemporalTextEncoder(bert=BertEncoder(bert-base, finetune_layers={TAIL}, dropout=True)) + Linear(512, 3) + MSE, L = {L}",
           "cells": []}
    torch.manual_seed(0)
    sd = Model("fp32").state_dict()
    for spec in ARGS.cells.split(","):
        compute, B = spec.split(":")
        c = cell(compute, int(B), only, sd)
        res["cells"].append(c)
        print(json.dumps(c), file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
    txt = json.dumps(res, indent=1)
    print(txt)
    if ARGS.out:
        with open(ARGS.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
