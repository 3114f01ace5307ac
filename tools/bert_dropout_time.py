#!/usr/bin/env python3
"""Time one fine-tuning step of mmdeer.bert.BertEncoder(finetune_layers=6, dropout=True) -- the reference's training configuration,
hidden and attention dropout 0.1 -- beside the same step without dropout (the same build, the same weights) and beside the
yardstick on the same GPU in the same dtype: ``transformers.BertModel`` in train() with both probabilities 0.1 and the same
parameters frozen.  Geometry, batches, masks and the timing scheme are tools/bert_backward_time.py's (BERT-base, 12 layers, L = 128,
half of the samples padded to 64 tokens, B in {32, 8}, bf16 and fp32; the three steps alternate repetition by repetition, a figure
is the median over ``--reps`` repetitions of ``--iters`` steps).  Then each dropout entry beside its plain counterpart on buffers of
its own, to say where the difference goes.  Prints one JSON object; ``--out`` also writes it to a file.

    python tools/bert_dropout_time.py [--reps 7] [--iters 3] [--launch-iters 20] [--warmup 3] [--B 32,8] [--out profiles/bert_dropout_step_time.json]
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

from bert_backward_time import L, LAYERS, TAIL, step_of  # noqa: E402
from bert_time import interleaved  # noqa: E402
from mmdeer import _lib, bert, ops  # noqa: E402

P = 0.1


def yardstick(cfg, sd, dt, dev):
    import transformers
    hf = transformers.BertConfig(**{k: v for k, v in cfg.items() if k not in ("add_pooling_layer", "position_embedding_type", "hidden_dropout_prob",
                                                                             "attention_probs_dropout_prob")},
                                 hidden_dropout_prob=P, attention_probs_dropout_prob=P)
    model = transformers.BertModel(hf, add_pooling_layer=False)
    model.load_state_dict({k: v for k, v in sd.items() if not k.startswith("pooler.")}, strict=True)
    model = model.to(dev).to(dt).train()
    for n, p in model.named_parameters():
        p.requires_grad_(n.startswith("encoder.layer.") and int(n.split(".")[2]) >= LAYERS - TAIL)
    return f"transformers.BertModel {transformers.__version__}, train(), both dropout probabilities {P}, layers {LAYERS - TAIL}-{LAYERS - 1} trainable", model


def launch_cells(enc, B, mask, a):
    """each dropout entry and its plain counterpart on the same buffers, alternating within a repetition"""
    H, M, c = enc.hidden_size, B * L, enc.compute_dtype
    dt, f32, dev, lib, stream = ops._act_dtype(c), int(c == "fp32"), mask.device, _lib.load(), _lib.current_stream()
    p = enc._operands()["layers"][-1]
    rnd = lambda *s: torch.randn(*s, device=dev).to(dt)           # noqa: E731
    y, x, out, g, g2, ds, dy, ctx, dctx = (rnd(M, H) for _ in range(9))
    qkv, dqkv = rnd(M, 3 * H), rnd(M, 3 * H)
    m = (mask != 0).float().reshape(-1).contiguous()
    dgamma, dbeta = torch.empty(H, device=dev), torch.empty(H, device=dev)
    nscr = lib.mmdeer_bert_add_ln_bwd_scratch(M, H)
    scratch = torch.empty(nscr, device=dev)
    nws = lib.mmdeer_bert_attn_bwd_workspace(B, L, H)
    ws = torch.empty(nws // 4, device=dev)

    def with_drop(a_, site):
        a_.site, a_.dropout_p, a_.seed, a_.offset = site, P, 1, 2
        return a_

    def attn(a_):
        a_.qkv, a_.mask, a_.ctx = qkv.data_ptr(), m.data_ptr(), ctx.data_ptr()
        a_.B, a_.L, a_.H, a_.ld_qkv, a_.ld_ctx, a_.act_f32, a_.stream = B, L, H, 3 * H, H, f32, stream
        return a_

    def attn_bwd(a_):
        a_.qkv, a_.mask, a_.dctx, a_.dqkv, a_.workspace, a_.workspace_bytes = qkv.data_ptr(), m.data_ptr(), dctx.data_ptr(), dqkv.data_ptr(), ws.data_ptr(), nws
        a_.B, a_.L, a_.H, a_.ld_qkv, a_.ld_dctx, a_.ld_dqkv, a_.act_f32, a_.stream = B, L, H, 3 * H, H, 3 * H, f32, stream
        return a_

    def ln(a_):
        a_.y, a_.x, a_.gamma, a_.beta, a_.out, a_.eps = y.data_ptr(), x.data_ptr(), p["g2"].data_ptr(), p["b2"].data_ptr(), out.data_ptr(), enc.eps
        a_.M, a_.N, a_.ld_y, a_.ld_x, a_.ld_out, a_.act_f32, a_.stream = M, H, H, H, H, f32, stream
        return a_

    def ln_bwd(a_):
        a_.y, a_.x, a_.g, a_.g2, a_.gamma, a_.ds = y.data_ptr(), x.data_ptr(), g.data_ptr(), g2.data_ptr(), p["g2"].data_ptr(), ds.data_ptr()
        a_.dgamma, a_.dbeta, a_.scratch, a_.scratch_elems, a_.eps = dgamma.data_ptr(), dbeta.data_ptr(), scratch.data_ptr(), nscr, enc.eps
        a_.M, a_.N, a_.ld_y, a_.ld_x, a_.ld_g, a_.ld_g2, a_.ld_ds, a_.act_f32, a_.stream = M, H, H, H, H, H, H, f32, stream
        return a_

    at, atd = attn(_lib.BertAttnArgs()), with_drop(attn(_lib.BertAttnDropArgs()), bert.site(11, 0))
    ab, abd = attn_bwd(_lib.BertAttnBwdArgs()), with_drop(attn_bwd(_lib.BertAttnDropBwdArgs()), bert.site(11, 0))
    lf, lfd = ln(_lib.BertAddLnArgs()), with_drop(ln(_lib.BertDropAddLnArgs()), bert.site(11, 2))
    lb, lbd = ln_bwd(_lib.BertAddLnBwdArgs()), with_drop(ln_bwd(_lib.BertDropAddLnBwdArgs()), bert.site(11, 2))
    lbd.dy, lbd.ld_dy = dy.data_ptr(), H
    call = lambda f, a_: (lambda: _lib.check(f(C.byref(a_))))       # noqa: E731
    fns = {"attn_fwd": call(lib.mmdeer_bert_attn_fwd, at), "attn_drop_fwd": call(lib.mmdeer_bert_attn_drop_fwd, atd),
           "attn_bwd": call(lib.mmdeer_bert_attn_bwd, ab), "attn_drop_bwd": call(lib.mmdeer_bert_attn_drop_bwd, abd),
           "add_ln_fwd": call(lib.mmdeer_bert_add_ln_fwd, lf), "drop_add_ln_fwd": call(lib.mmdeer_bert_drop_add_ln_fwd, lfd),
           "add_ln_bwd": call(lib.mmdeer_bert_add_ln_bwd, lb), "drop_add_ln_bwd": call(lib.mmdeer_bert_drop_add_ln_bwd, lbd)}
    cells = interleaved(fns, a.reps, a.launch_iters, a.warmup)
    for plain, dropped in (("attn_fwd", "attn_drop_fwd"), ("attn_bwd", "attn_drop_bwd"), ("add_ln_fwd", "drop_add_ln_fwd"), ("add_ln_bwd", "drop_add_ln_bwd")):
        cells[dropped]["over_plain"] = round(cells[dropped]["median_ms"] / cells[plain]["median_ms"], 4)
    # what a step adds by these launches alone: 12 attention forwards and 24 add-LN forwards, 6 attention backwards and 12 add-LN backwards
    d = lambda k, q: cells[k]["median_ms"] - cells[q]["median_ms"]      # noqa: E731
    cells["step_difference_from_these_launches_ms"] = round(LAYERS * d("attn_drop_fwd", "attn_fwd") + 2 * LAYERS * d("drop_add_ln_fwd", "add_ln_fwd") +
                                                            TAIL * d("attn_drop_bwd", "attn_bwd") + 2 * TAIL * d("drop_add_ln_bwd", "add_ln_bwd"), 4)
    return cells


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--launch-iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--B", default="32,8")
    ap.add_argument("--compute", default="bf16,fp32")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bert_dropout_time.py measures on the GPU: none found")
    dev = "cuda:0"
    cfg = {**bert.DEFAULTS, "num_hidden_layers": LAYERS, "hidden_dropout_prob": P, "attention_probs_dropout_prob": P}
    res = {"device": torch.cuda.get_device_name(0), "geometry": "bert-base: 768 / 12 heads / 3072, 12 layers", "finetune_layers": TAIL, "L": L,
           "dropout": {"hidden_dropout_prob": P, "attention_probs_dropout_prob": P},
           "what": "forward + backward, every tail gradient materialised; mmdeer_step: dropout=False, mmdeer_dropout_step: dropout=True in train()",
           "reps": a.reps, "iters": a.iters, "launch_iters": a.launch_iters, "warmup": a.warmup, "cells": []}
    torch.manual_seed(0)
    base = bert.BertEncoder(cfg, "fp32")
    with torch.no_grad():                                             # bert_backward_time.py's weights
        for n, p in base.named_parameters():
            if ".query." in n or ".key." in n:
                p.mul_(4.0)
            elif "LayerNorm.weight" in n:
                p.uniform_(0.5, 1.5)
    sd = base.state_dict()
    for compute in a.compute.split(","):
        dt = ops._act_dtype(compute)
        encs = {}
        for name, on in (("plain", False), ("drop", True)):
            enc = bert.BertEncoder(cfg, compute, finetune_layers=TAIL, dropout=on, dropout_seed=1)
            enc.load_state_dict(sd, strict=True)
            encs[name] = enc.to(dev).train()
        res["yardstick"], model = yardstick(cfg, sd, dt, dev)
        for B in [int(v) for v in a.B.split(",")]:
            ids = torch.randint(1, cfg["vocab_size"], (B, L), device=dev)
            mask = torch.ones(B, L, dtype=torch.int64, device=dev)
            mask[1::2, L // 2:] = 0                                   # half of the samples padded to L / 2
            up = (torch.randn(B, L, 768, device=dev) * mask.unsqueeze(-1)).to(dt)
            params = {k: [p for p in e.parameters() if p.requires_grad] for k, e in encs.items()}
            ref_params = [p for p in model.parameters() if p.requires_grad]
            steps = {"mmdeer_step": step_of(params["plain"], lambda: encs["plain"](ids, mask).last_hidden_state, up),
                     "mmdeer_dropout_step": step_of(params["drop"], lambda: encs["drop"](ids, mask).last_hidden_state, up),
                     "torch_dropout_step": step_of(ref_params, lambda: model(input_ids=ids, attention_mask=mask).last_hidden_state, up)}
            cell = {"compute": compute, "B": B}
            cell.update(interleaved(steps, a.reps, a.iters, a.warmup))
            cell["dropout_over_no_dropout"] = round(cell["mmdeer_dropout_step"]["median_ms"] / cell["mmdeer_step"]["median_ms"], 4)
            cell["mmdeer_dropout_over_torch_dropout"] = round(cell["mmdeer_dropout_step"]["median_ms"] / cell["torch_dropout_step"]["median_ms"], 4)
            with torch.no_grad():
                cell["dropout_entries_beside_plain"] = launch_cells(encs["drop"], B, mask, a)
            for p in params["plain"] + params["drop"] + ref_params:
                p.grad = None
            res["cells"].append(cell)
            print(json.dumps({k: v for k, v in cell.items() if k != "dropout_entries_beside_plain"}), file=sys.stderr, flush=True)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
