#!/usr/bin/env python3
"""Time one fine-tuning step of mmdeer.bert.BertEncoder(finetune_layers=6) -- forward + backward with every tail gradient
materialised -- at BERT-base geometry (12 layers, random weights), L = 128, half of the samples padded to 64 tokens, B in {32, 8},
in bf16 and fp32.  Beside each figure the yardstick on the same GPU in the same dtype: ``transformers.BertModel`` (built from a
config, never from a pretrained name) with both dropout probabilities 0 and the same parameters frozen (embeddings and layers
0-5), same weights, its default attention implementation.  The two alternate repetition by repetition; a figure is the median
over ``--reps`` repetitions of ``--iters`` steps.  Then every launch of ONE tail layer's backward on buffers of its own.  Prints
one JSON object; ``--out`` also writes it to a file.

    python tools/bert_backward_time.py [--reps 7] [--iters 3] [--launch-iters 20] [--warmup 3] [--B 32,8] [--out profiles/bert_finetune_step_time.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("HF_HUB_OFFLINE", "1")
os.environ.setdefault("TRANSFORMERS_OFFLINE", "1")

import torch  # noqa: E402

from bert_time import MFMA_BF16_TFLOPS, interleaved  # noqa: E402
from mmdeer import _lib, bert, ops, opseq  # noqa: E402

L = 128
LAYERS = 12
TAIL = 6


def yardstick(cfg, sd, dt, dev):
    import transformers
    hf = transformers.BertConfig(**{k: v for k, v in cfg.items() if k not in ("add_pooling_layer", "position_embedding_type", "hidden_dropout_prob",
                                                                             "attention_probs_dropout_prob")},
                                 hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    model = transformers.BertModel(hf, add_pooling_layer=False)
    model.load_state_dict({k: v for k, v in sd.items() if not k.startswith("pooler.")}, strict=True)
    model = model.to(dev).to(dt).train()
    for n, p in model.named_parameters():
        p.requires_grad_(n.startswith("encoder.layer.") and int(n.split(".")[2]) >= LAYERS - TAIL)
    return f"transformers.BertModel {transformers.__version__}, dropout 0, layers {LAYERS - TAIL}-{LAYERS - 1} trainable", model


def step_of(params, forward, up):
    def step():
        for p in params:
            p.grad = None
        forward().backward(up)
    return step


def launch_cells(enc, B, mask, a):
    """every launch of one tail layer's backward on buffers of its own, alternating within a repetition"""
    H, inter, M, c = enc.hidden_size, enc.config["intermediate_size"], B * L, enc.compute_dtype
    dt, f32, dev, lib = ops._act_dtype(c), int(c == "fp32"), mask.device, _lib.load()
    p = enc._operands()["layers"][-1]
    ex = opseq.Exec(c)
    rnd = lambda *s: torch.randn(*s, device=dev).to(dt)           # noqa: E731
    g, g2, y, x, ds, dx1 = (rnd(M, H) for _ in range(6))
    qkv, dqkv, h, dh = rnd(M, 3 * H), rnd(M, 3 * H), rnd(M, inter), rnd(M, inter)
    m = (mask != 0).float().reshape(-1).contiguous()
    gw_o2, gw_i, gw_o, gw_qkv = (torch.empty(s, device=dev) for s in ((H, inter), (inter, H), (H, H), (3 * H, H)))
    gb_h, gb_i, gb_qkv = torch.empty(H, device=dev), torch.empty(inter, device=dev), torch.empty(3 * H, device=dev)
    ln = _lib.BertAddLnBwdArgs()
    dgamma, dbeta = torch.empty(H, device=dev), torch.empty(H, device=dev)
    ln.scratch_elems = lib.mmdeer_bert_add_ln_bwd_scratch(M, H)
    scratch = torch.empty(ln.scratch_elems, device=dev)
    ln.y, ln.x, ln.g, ln.g2, ln.gamma, ln.ds = y.data_ptr(), x.data_ptr(), g.data_ptr(), g2.data_ptr(), p["g2"].data_ptr(), ds.data_ptr()
    ln.dgamma, ln.dbeta, ln.scratch, ln.eps = dgamma.data_ptr(), dbeta.data_ptr(), scratch.data_ptr(), enc.eps
    ln.M, ln.N, ln.ld_y, ln.ld_x, ln.ld_g, ln.ld_g2, ln.ld_ds, ln.act_f32, ln.stream = M, H, H, H, H, H, H, f32, ex.s
    ge = _lib.BertGeluBwdArgs()
    ge.x, ge.g, ge.dx, ge.M, ge.N, ge.ld_x, ge.ld_g, ge.ld_dx, ge.act_f32, ge.stream = h.data_ptr(), dh.data_ptr(), dh.data_ptr(), M, inter, inter, inter, inter, f32, ex.s
    ab = _lib.BertAttnBwdArgs()
    ab.workspace_bytes = lib.mmdeer_bert_attn_bwd_workspace(B, L, H)
    ws = torch.empty(ab.workspace_bytes // 4, device=dev)
    ab.qkv, ab.mask, ab.dctx, ab.dqkv, ab.workspace = qkv.data_ptr(), m.data_ptr(), dx1.data_ptr(), dqkv.data_ptr(), ws.data_ptr()
    ab.B, ab.L, ab.H, ab.ld_qkv, ab.ld_dctx, ab.ld_dqkv, ab.act_f32, ab.stream = B, L, H, 3 * H, H, 3 * H, f32, ex.s
    fns = {"add_ln_bwd": lambda: _lib.check(lib.mmdeer_bert_add_ln_bwd(C.byref(ln))),
           "dW_ffn_out": lambda: ex.dw(ds, H, h, inter, gw_o2, gb_h, M, H, inter),
           "dX_ffn_out": lambda: ex.dx(ds, H, p["wo2"], dh, inter, M),
           "gelu_bwd": lambda: _lib.check(lib.mmdeer_bert_gelu_bwd(C.byref(ge))),
           "dW_ffn_in": lambda: ex.dw(dh, inter, x, H, gw_i, gb_i, M, inter, H),
           "dX_ffn_in": lambda: ex.dx(dh, inter, p["wi"], dx1, H, M),
           "dW_out_proj": lambda: ex.dw(ds, H, x, H, gw_o, gb_h, M, H, H),
           "dX_out_proj": lambda: ex.dx(ds, H, p["wo"], dx1, H, M),
           "attention_bwd": lambda: _lib.check(lib.mmdeer_bert_attn_bwd(C.byref(ab))),
           "dW_qkv": lambda: ex.dw(dqkv, 3 * H, x, H, gw_qkv, gb_qkv, M, 3 * H, H),
           "dX_qkv": lambda: ex.dx(dqkv, 3 * H, p["wqkv"], dx1, H, M)}
    cells = interleaved(fns, a.reps, a.launch_iters, a.warmup)
    valid = (mask != 0).sum(1).double()
    flop = {"dW_ffn_out": 2.0 * M * H * inter, "dX_ffn_out": 2.0 * M * H * inter, "dW_ffn_in": 2.0 * M * H * inter, "dX_ffn_in": 2.0 * M * H * inter,
            "dW_out_proj": 2.0 * M * H * H, "dX_out_proj": 2.0 * M * H * H, "dW_qkv": 2.0 * M * 3 * H * H, "dX_qkv": 2.0 * M * 3 * H * H,
            "attention_bwd": 10.0 * 64 * (H // 64) * float((valid * L).sum())}       # five products over (queries x VALID keys x 64), S computed twice more
    for k, f in flop.items():
        cells[k]["useful_gflop"] = round(f / 1e9, 3)
        cells[k]["tflops"] = round(f / (cells[k]["median_ms"] * 1e-3) / 1e12, 2)
        cells[k]["share_of_bf16_mfma_rate"] = round(cells[k]["tflops"] / MFMA_BF16_TFLOPS, 4)
    cells["sum_of_medians_one_layer_ms"] = round(sum(v["median_ms"] for k, v in cells.items()) + cells["add_ln_bwd"]["median_ms"], 4)
    return cells


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--launch-iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--B", default="32,8")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bert_backward_time.py measures on the GPU: none found")
    dev = "cuda:0"
    cfg = {**bert.DEFAULTS, "num_hidden_layers": LAYERS}
    res = {"device": torch.cuda.get_device_name(0), "geometry": "bert-base: 768 / 12 heads / 3072, 12 layers", "finetune_layers": TAIL, "L": L,
           "what": "forward + backward, every tail gradient materialised", "reps": a.reps, "iters": a.iters, "launch_iters": a.launch_iters,
           "warmup": a.warmup, "cells": []}
    torch.manual_seed(0)
    base = bert.BertEncoder(cfg, "fp32")
    with torch.no_grad():                                             # wider than the std-0.02 initialisation: attention away from uniform
        for n, p in base.named_parameters():
            if ".query." in n or ".key." in n:
                p.mul_(4.0)
            elif "LayerNorm.weight" in n:
                p.uniform_(0.5, 1.5)
    sd = base.state_dict()
    for compute in ("bf16", "fp32"):
        dt = ops._act_dtype(compute)
        enc = bert.BertEncoder(cfg, compute, finetune_layers=TAIL)
        enc.load_state_dict(sd, strict=True)
        enc = enc.to(dev)
        res["yardstick"], model = yardstick(cfg, sd, dt, dev)
        for B in [int(v) for v in a.B.split(",")]:
            ids = torch.randint(1, cfg["vocab_size"], (B, L), device=dev)
            mask = torch.ones(B, L, dtype=torch.int64, device=dev)
            mask[1::2, L // 2:] = 0                                   # half of the samples padded to L / 2
            up = (torch.randn(B, L, 768, device=dev) * mask.unsqueeze(-1)).to(dt)
            hip_params = [p for p in enc.parameters() if p.requires_grad]
            ref_params = [p for p in model.parameters() if p.requires_grad]
            hip = step_of(hip_params, lambda: enc(ids, mask).last_hidden_state, up)
            ref = step_of(ref_params, lambda: model(input_ids=ids, attention_mask=mask).last_hidden_state, up)
            hip(), ref()
            torch.cuda.synchronize()
            names = [n for n, p in enc.named_parameters() if p.requires_grad]
            got, want = dict(zip(names, (p.grad.float() for p in hip_params))), {n: p.grad.float() for n, p in model.named_parameters() if p.requires_grad}
            rel = {n: float((got[n] - want[n]).norm() / want[n].norm().clamp_min(1e-30)) for n in names if not n.endswith(".key.bias")}
            worst = max(rel, key=rel.get)
            cell = {"compute": compute, "B": B, "trainable_tensors": len(names),
                    "largest_relative_l2_difference_of_a_gradient_from_the_yardsticks": {"name": worst, "value": round(rel[worst], 5)}}
            cell.update(interleaved({"mmdeer_step": hip, "torch_step": ref}, a.reps, a.iters, a.warmup))
            cell["mmdeer_over_torch"] = round(cell["mmdeer_step"]["median_ms"] / cell["torch_step"]["median_ms"], 4)
            with torch.no_grad():
                fwd = {"mmdeer_forward_no_grad": lambda: enc(ids, mask).last_hidden_state,
                       "torch_forward_no_grad": lambda: model(input_ids=ids, attention_mask=mask).last_hidden_state}
                cell.update(interleaved(fwd, a.reps, a.iters, a.warmup))
                cell["one_tail_layer_backward_launches"] = launch_cells(enc, B, mask, a)
            for p in hip_params + ref_params:
                p.grad = None
            res["cells"].append(cell)
            print(json.dumps({k: v for k, v in cell.items() if k != "one_tail_layer_backward_launches"}), file=sys.stderr, flush=True)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
