#!/usr/bin/env python3
"""Time the END-TO-END training step eagerly and as one HIP graph (mmdeer.train_graph.capture_train_step), in one process:

  eager             host dropout counters, ModuleAdamW.for_module (non-capturable)
  eager_capturable  the same with ModuleAdamW(capturable=True): the device step count and lr records, still launched by the host
  replay            capture_train_step's graph: one launch of the whole step from the host

on EndToEndDEER(ModalityEncoder({'train_backbone': True}, bert=BertEncoder(BERT-base, finetune_layers=6, dropout=True)),
HierarchicalMultimodalFusion(512, 512, 512), MultiDimensionalDEER(512)) + MultiTaskDEERLoss, random weights, at the reference's data
shapes: audio (B, 84), video (B, 3, 224, 224), ids and mask (B, 128), targets (B, 3); clip 1.0, decay 0 on the one-dimensional
parameters.  Cells: bf16 at B = 8 and B = 32.  Every variant has a model copy of its own from one state dict; a figure is a window of
``--iters`` steps between two device events divided by the steps, the variants alternating window by window, ``--reps`` windows each
after ``--warmup`` steps of every variant; min, median and max are kept.

``launches``: the nodes of the step's graph by kind, counted by the runtime (hipGraphGetNodes) on a second capture of the same region
that is kept as a graph and never replayed (``capture_train_step``'s own graph is instantiated and its graph object released).
``--trace-steps N`` instead runs N eager steps of the first cell's capturable variant and exits: the program of a kernel trace
(``rocprofv3 --kernel-trace --stats -- python tools/e2e_train_graph_time.py --trace-steps N``; the dispatches of N = 6 minus those of
N = 2, over 4, are one step's).  Prints one JSON object; ``--out`` also writes it.

    python tools/e2e_train_graph_time.py [--reps 20] [--iters 10] [--warmup 5] [--cells bf16:8,bf16:32] [--only eager,eager_capturable,replay]
                                         [--out profiles/e2e_train_graph_time.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--cells", default="bf16:8,bf16:32")
ap.add_argument("--only", default="eager,eager_capturable,replay")
ap.add_argument("--bert-layers", type=int, default=12, help="trunk depth (12: BERT-base; smaller for a rehearsal)")
ap.add_argument("--trace-steps", type=int, default=0)
ap.add_argument("--out", default=None)
ARGS = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from mmdeer import bert, encoders, head  # noqa: E402
from mmdeer.model import HierarchicalMultimodalFusion  # noqa: E402
from mmdeer.optim import ModuleAdamW  # noqa: E402

L, TAIL, LR, CLIP, DEV = 128, 6, 2e-5, 1.0, "cuda:0"


def model_of(compute):
    cfg = None if ARGS.bert_layers == 12 else {"num_hidden_layers": ARGS.bert_layers}
    trunk = bert.BertEncoder(cfg, compute, finetune_layers=min(TAIL, ARGS.bert_layers), dropout=True)
    enc = encoders.ModalityEncoder({"train_backbone": True}, compute, bert=trunk)
    return encoders.EndToEndDEER(enc, HierarchicalMultimodalFusion(512, 512, 512, compute_dtype=compute), head.MultiDimensionalDEER(512, compute_dtype=compute))


def step_fn_of(m):
    def step_fn(audio, video, ids, mask, targets):
        out = m({"audio": audio, "video": video, "text_input_ids": ids, "text_attention_mask": mask})
        return m.compute_loss(out, targets)["total_loss"]
    return step_fn


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


NODE_KINDS = {0: "kernel", 1: "memcpy", 2: "memset", 3: "host", 4: "graph", 5: "empty", 6: "wait_event", 7: "event_record"}     # hipGraphNodeType


def _hip_runtime():
    """the HIP runtime this process already runs on (torch's own copy), by the path it is mapped from"""
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64" in line}
    if len(paths) != 1:
        raise RuntimeError(f"expected one mapped libamdhip64, found {sorted(paths)}")
    return C.CDLL(paths.pop())


def count_nodes(step_fn, opt, static, counters):
    """The nodes of the step's graph by kind (hipGraphGetNodes / hipGraphNodeGetType), from a second capture of the same region that
    is kept as a graph and never instantiated or replayed (a capture runs nothing).  None with the reason where that fails."""
    try:
        for group in opt.param_groups:        # as capture_train_step does: with gradients in place the backward would record one
            for p in group["params"]:         # accumulating add per parameter that the replayed graph does not have
                p.grad = None
        g = torch.cuda.CUDAGraph(keep_graph=True)
        with torch.cuda.graph(g):
            step_fn(*static).backward()
            opt.step()
            for mod, t in counters:           # the region's closing adds, one per module that drew
                k = mod.take_step_count()
                if k:
                    t.add_(k)
        hip, raw, n = _hip_runtime(), C.c_void_p(g.raw_cuda_graph()), C.c_size_t(0)
        if hip.hipGraphGetNodes(raw, None, C.byref(n)) != 0:
            raise RuntimeError("hipGraphGetNodes failed")
        nodes = (C.c_void_p * n.value)()
        if hip.hipGraphGetNodes(raw, nodes, C.byref(n)) != 0:
            raise RuntimeError("hipGraphGetNodes failed")
        kinds = {}
        for node in nodes:
            t = C.c_int(-1)
            if hip.hipGraphNodeGetType(C.c_void_p(node), C.byref(t)) != 0:
                raise RuntimeError("hipGraphNodeGetType failed")
            name = NODE_KINDS.get(t.value, f"type {t.value}")
            kinds[name] = kinds.get(name, 0) + 1
        return {"nodes": n.value, "by_kind": kinds}
    except Exception as e:      # noqa: BLE001  (a count that cannot be taken is reported as such; the timings stand)
        return {"nodes": None, "reason": f"{type(e).__name__}: {e}"[:300]}


def cell(compute, B, only, sd):
    gen = torch.Generator().manual_seed(B)
    audio = torch.randn(B, 84, generator=gen).to(DEV)
    video = torch.randn(B, 3, 224, 224, generator=gen).to(DEV)
    ids = torch.randint(1, 30000, (B, L), generator=gen).to(DEV)
    mask = torch.ones(B, L, dtype=torch.int64)
    mask[B // 2:, L // 2:] = 0
    mask, targets = mask.to(DEV), (torch.rand(B, 3, generator=gen) * 2 - 1).to(DEV)
    batch = (audio, video, ids, mask, targets)
    fns, counting = {}, None
    for v in only:
        m = model_of(compute)
        m.load_state_dict(sd)
        m = m.to(DEV).train()
        named = [(n, p) for n, p in m.named_parameters() if p.requires_grad]
        groups = [{"params": [p for _, p in named if p.ndim >= 2], "weight_decay": 0.01}, {"params": [p for _, p in named if p.ndim < 2], "weight_decay": 0.0}]
        kw = {} if v == "eager" else {"capturable": True}
        opt = ModuleAdamW.for_module(m, groups, lr=LR, max_grad_norm=CLIP, **kw)
        if v == "replay":
            from mmdeer.train_graph import capture_train_step
            static = [t.clone() for t in batch]
            replay = capture_train_step(step_fn_of(m), opt, static)
            counting = (step_fn_of(m), opt, static, replay.counters)
            fns[v] = lambda replay=replay: replay(*batch)
        else:
            def step(m=m, opt=opt, fn=step_fn_of(m)):
                for p in m.parameters():
                    p.grad = None
                fn(*batch).backward()
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
    if counting is not None:          # after the timings: the counting capture is never replayed, and what it leaves behind is not timed
        out["launches"] = count_nodes(*counting)
    if "replay" in ms and "eager" in ms:
        out["replay_over_eager_median"] = round(out["replay"]["median_ms"] / out["eager"]["median_ms"], 4)
        out["replay_over_eager_min"] = round(out["replay"]["min_ms"] / out["eager"]["min_ms"], 4)
    return out


def main():
    if not torch.cuda.is_available():
        raise SystemExit("e2e_train_graph_time.py measures on the GPU: none found")
    only = ARGS.only.split(",")
    if ARGS.trace_steps:
        compute, B = ARGS.cells.split(",")[0].split(":")
        ARGS.warmup, ARGS.reps, ARGS.iters = 0, 1, ARGS.trace_steps
        torch.manual_seed(0)
        print(json.dumps(cell(compute, int(B), ["eager_capturable"], model_of("fp32").state_dict())))
        return
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "reps": ARGS.reps, "iters": ARGS.iters, "warmup": ARGS.warmup,
           "model": f"EndToEndDEER(ModalityEncoder(train_backbone, bert=BertEncoder({ARGS.bert_layers} layers of BERT-base, finetune_layers="
                    f"{min(TAIL, ARGS.bert_layers)}, dropout=True)), HierarchicalMultimodalFusion(512, 512, 512), MultiDimensionalDEER(512)); "
                    f"audio (B, 84), video (B, 3, 224, 224), L = {L}",
           "cells": []}
    torch.manual_seed(0)
    sd = model_of("fp32").state_dict()
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
