#!/usr/bin/env python3
"""Time the optimiser half of a training step for modules that train through autograd: mmdeer.optim.ModuleAdamW beside the yardstick
on the same GPU, ``clip_grad_norm_`` + ``torch.optim.AdamW`` as the reference trainer builds it (three groups by parameter name, eps
1e-8, clip 1.0).  Two parameter sets:

  bert      BertEncoder (BERT-base, 12 layers) with finetune_layers=6: 96 tensors, 42.5 M parameters; bf16 and fp32 operands.  Each
            variant's step ends with the ``_operands()`` call the next forward would make (the rebuild of the tail's packed operands
            where the step moved the version counters; nothing where the step wrote them itself).
  composed  ComposedDEER(HierarchicalMultimodalFusion(84, 256, 768), MultiDimensionalDEER(512)): small and launch-bound.  The step
            alone (its modules' pack caches rebuild inside the next forward for every variant alike).

Variants: (a) clip_grad_norm_ + torch.optim.AdamW, (b) the same with fused=True where this torch offers it, (c) ModuleAdamW without
mirrors, (d) ModuleAdamW.for_module.  Every variant has a model copy of its own; gradients are drawn once and held fixed.  A figure is
the median over ``--reps`` repetitions of ``--iters`` steps between two device events, the variants alternating repetition by
repetition; min and max are kept.  The byte counts of the two launches over the 6.29 TB/s copy rate are printed beside them; the two
kernels' own times come from a kernel trace of ``--only d`` (a run of its own).  Prints one JSON object; ``--out`` also writes it.

    python tools/module_adamw_time.py [--reps 7] [--iters 20] [--warmup 3] [--sets bert,composed] [--compute bf16,fp32] [--only a,b,c,d]
                                      [--out profiles/module_adamw_time.json]
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

from mmdeer import bert, head  # noqa: E402
from mmdeer.model import HierarchicalMultimodalFusion  # noqa: E402
from mmdeer.optim import ModuleAdamW  # noqa: E402

LR, WD, EPS, CLIP, TAIL = 1e-4, 1e-5, 1e-8, 1.0, 6
COPY_RATE = 6.29e12          # bytes / s, the chip's measured copy rate


def trainer_groups(model):
    """the reference trainer's three groups (training.py:121-150): 'encoder'-named parameters at half the rate"""
    enc, att, rest = [], [], []
    for name, p in model.named_parameters():
        if p.requires_grad:
            (enc if "encoder" in name else att if "attention" in name else rest).append(p)
    return [g for g in ({"params": enc, "lr": LR * 0.5}, {"params": att, "lr": LR}, {"params": rest, "lr": LR}) if g["params"]]


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


def interleaved(fns, reps, iters, warmup):
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ms[k].append(window(fn, iters))
    return {k: stats(v) for k, v in ms.items()}


def variants(make, only, after=None):
    """{variant: step callable}, each on a model of its own with the same fixed gradients"""
    fns, note = {}, {}
    gen = torch.Generator().manual_seed(1)
    grads = None
    for v in only:
        model = make()
        params = [p for p in model.parameters() if p.requires_grad]
        if grads is None:
            grads = [(torch.randn(p.shape, generator=gen) * 1e-3).to(p.device) for p in params]
        for p, g in zip(params, grads):
            p.grad = g.clone()
        tail = (lambda m=model: after(m)) if after is not None else (lambda: None)
        if v in ("a", "b"):
            try:
                opt = torch.optim.AdamW(trainer_groups(model), weight_decay=WD, eps=EPS, **({"fused": True} if v == "b" else {}))
            except (TypeError, RuntimeError, ValueError) as e:
                note[v] = f"not offered by torch {torch.__version__}: {e}"
                continue

            def step(opt=opt, params=params, tail=tail):
                torch.nn.utils.clip_grad_norm_(params, CLIP)
                opt.step()
                tail()
        else:
            kw = dict(lr=LR, weight_decay=WD, eps=EPS, max_grad_norm=CLIP)
            opt = ModuleAdamW(trainer_groups(model), **kw) if v == "c" else ModuleAdamW.for_module(model, trainer_groups(model), **kw)
            note[v] = f"{sum(t is not None for t in opt._mirrors)} mirrors"

            def step(opt=opt, tail=tail):
                opt.step()
                tail()
        fns[v] = step
    return fns, note


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sets", default="bert,composed")
    ap.add_argument("--compute", default="bf16,fp32")
    ap.add_argument("--only", default="a,b,c,d")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("module_adamw_time.py measures on the GPU: none found")
    dev, only = "cuda:0", a.only.split(",")
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "reps": a.reps, "iters": a.iters, "warmup": a.warmup,
           "yardstick": "a: clip_grad_norm_ + torch.optim.AdamW, the reference trainer's groups", "hyper": {"lr": LR, "weight_decay": WD, "eps": EPS, "clip": CLIP},
           "cells": []}
    for which in a.sets.split(","):
        for compute in (a.compute.split(",") if which == "bert" else ["fp32"]):
            if which == "bert":
                torch.manual_seed(0)
                sd = bert.BertEncoder(None, "fp32").state_dict()

                def make(compute=compute, sd=sd):
                    enc = bert.BertEncoder(None, compute, finetune_layers=TAIL)
                    enc.load_state_dict(sd, strict=True)
                    enc = enc.to(dev)
                    enc._operands()
                    return enc
                fns, note = variants(make, only, after=lambda m: m._operands())
                name = f"BertEncoder(bert-base, finetune_layers={TAIL}), {compute} operands; step + _operands()"
            else:
                def make():
                    return head.ComposedDEER(HierarchicalMultimodalFusion(84, 256, 768), head.MultiDimensionalDEER(512)).to(dev)
                fns, note = variants(make, only)
                name = "ComposedDEER(HierarchicalMultimodalFusion(84, 256, 768), MultiDimensionalDEER(512)); step alone"
            model = make()
            sizes = [p.numel() for p in model.parameters() if p.requires_grad]
            del model
            n = sum(sizes)
            mirror_bytes = (2 if compute == "bf16" else 4) if which == "bert" else 0
            # matrices are mirrored in the compute dtype, vectors in fp32: the vectors are 0.1 % of BERT's tail, counted as matrices here
            cell = {"set": name, "tensors": len(sizes), "elements": n, "notes": note,
                    "bytes": {"sumsq_launch": 4 * n, "update_launch_no_mirrors": 28 * n, "update_launch_with_mirrors": (28 + mirror_bytes) * n},
                    "bytes_over_copy_rate_ms": {"sumsq_launch": round(4 * n / COPY_RATE * 1e3, 4), "update_launch_no_mirrors": round(28 * n / COPY_RATE * 1e3, 4),
                                                "update_launch_with_mirrors": round((28 + mirror_bytes) * n / COPY_RATE * 1e3, 4)}}
            with torch.no_grad():
                cell.update(interleaved(fns, a.reps, a.iters, a.warmup))
            for v in ("b", "c", "d"):
                if v in fns and "a" in fns:
                    cell[f"{v}_over_a"] = round(cell[v]["median_ms"] / cell["a"]["median_ms"], 4)
            res["cells"].append(cell)
            print(json.dumps(cell), file=sys.stderr, flush=True)
            del fns
            torch.cuda.empty_cache()
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
