#!/usr/bin/env python3
"""Time mmdeer.bert.BertEncoder (the BERT trunk's forward on HIP) at BERT-base geometry (12 layers, random weights), L = 128,
B in {32, 8}, half of the samples padded to L / 2, in bf16 and fp32, eager and replayed from a captured HIP graph -- and beside each
figure the same trunk in torch on the same GPU in the same dtype as a yardstick: ``transformers.BertModel`` (built from a config,
never from a pretrained name) if it imports, else torch.nn layers with ``scaled_dot_product_attention``, either with the same
weights.  The HIP trunk and the yardstick alternate within every repetition.  Then every launch of one layer on its own: its
median, and for the GEMMs and the attention kernel the useful GFLOP (attention: 4 * 64 * queries * VALID keys per head and
sample), TFLOP/s and the share of the bf16 MFMA rate.  Prints one JSON object; ``--out`` also writes it to a file.

    python tools/bert_time.py [--reps 7] [--iters 3] [--launch-iters 20] [--warmup 3] [--B 32,8] [--out profiles/bert_forward_time.json]
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
os.environ.setdefault("HF_HUB_OFFLINE", "1")
os.environ.setdefault("TRANSFORMERS_OFFLINE", "1")

import torch  # noqa: E402
from torch import nn  # noqa: E402
from torch.nn import functional as F  # noqa: E402

from mmdeer import _lib, bert, ops  # noqa: E402

MFMA_BF16_TFLOPS = 1970.5       # profiles/r04_calibration.txt
L = 128
LAYERS = 12


class TorchBert(nn.Module):
    """the fallback yardstick: BertModel's forward on torch.nn layers, attention through scaled_dot_product_attention"""

    def __init__(self, cfg):
        super().__init__()
        H, inter = cfg["hidden_size"], cfg["intermediate_size"]
        self.heads, self.eps = cfg["num_attention_heads"], cfg["layer_norm_eps"]
        self.word, self.pos, self.typ = nn.Embedding(cfg["vocab_size"], H), nn.Embedding(cfg["max_position_embeddings"], H), nn.Embedding(cfg["type_vocab_size"], H)
        self.ln0 = nn.LayerNorm(H, eps=self.eps)
        self.layers = nn.ModuleList(nn.ModuleDict({"qkv": nn.Linear(H, 3 * H), "o": nn.Linear(H, H), "ln1": nn.LayerNorm(H, eps=self.eps),
                                                   "i": nn.Linear(H, inter), "o2": nn.Linear(inter, H), "ln2": nn.LayerNorm(H, eps=self.eps)})
                                    for _ in range(cfg["num_hidden_layers"]))

    def load_bert(self, sd):
        get = lambda k: sd[k].detach().float()                        # noqa: E731
        with torch.no_grad():
            for dst, k in ((self.word, "word_embeddings"), (self.pos, "position_embeddings"), (self.typ, "token_type_embeddings")):
                dst.weight.copy_(get(f"embeddings.{k}.weight"))
            self.ln0.weight.copy_(get("embeddings.LayerNorm.weight")), self.ln0.bias.copy_(get("embeddings.LayerNorm.bias"))
            for n, lyr in enumerate(self.layers):
                p = f"encoder.layer.{n}."
                lyr["qkv"].weight.copy_(torch.cat([get(p + f"attention.self.{r}.weight") for r in ("query", "key", "value")]))
                lyr["qkv"].bias.copy_(torch.cat([get(p + f"attention.self.{r}.bias") for r in ("query", "key", "value")]))
                for dst, k in (("o", "attention.output.dense"), ("ln1", "attention.output.LayerNorm"), ("i", "intermediate.dense"),
                               ("o2", "output.dense"), ("ln2", "output.LayerNorm")):
                    lyr[dst].weight.copy_(get(p + k + ".weight")), lyr[dst].bias.copy_(get(p + k + ".bias"))
        return self

    def forward(self, input_ids, attention_mask):
        B, T = input_ids.shape
        x = self.ln0(self.word(input_ids) + self.typ.weight[0] + self.pos.weight[:T])
        keep = (attention_mask != 0)[:, None, None, :]
        for lyr in self.layers:
            q, k, v = (t.reshape(B, T, self.heads, -1).transpose(1, 2) for t in lyr["qkv"](x).chunk(3, dim=-1))
            ctx = F.scaled_dot_product_attention(q, k, v, attn_mask=keep).transpose(1, 2).reshape(B, T, -1)
            x = lyr["ln1"](lyr["o"](ctx) + x)
            x = lyr["ln2"](lyr["o2"](F.gelu(lyr["i"](x))) + x)
        return x


def yardstick(cfg, sd, dt, dev):
    """(name, callable(ids, mask) -> last hidden state)"""
    try:
        import transformers
        model = transformers.BertModel(transformers.BertConfig(**{k: v for k, v in cfg.items() if k not in ("add_pooling_layer", "position_embedding_type")}),
                                       add_pooling_layer=False)
        model.load_state_dict({k: v for k, v in sd.items() if not k.startswith("pooler.")}, strict=True)
        model = model.to(dev).to(dt).eval()
        return f"transformers.BertModel {transformers.__version__}", lambda ids, mask: model(input_ids=ids, attention_mask=mask).last_hidden_state
    except ImportError:
        model = TorchBert(cfg).load_bert(sd).to(dev).to(dt).eval()
        return "torch.nn + scaled_dot_product_attention", model


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
    """{name: stats}: every repetition times each of ``fns`` once, in turn"""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ms[k].append(window(fn, iters))
    return {k: stats(v) for k, v in ms.items()}


def captured(fn, warmup):
    """a callable that replays ``fn`` from a HIP graph"""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(warmup):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g.replay


def launch_cells(enc, B, mask, a):
    """every launch of one layer on buffers of its own, alternating within a repetition"""
    H, inter, M, c = enc.hidden_size, enc.config["intermediate_size"], B * L, enc.compute_dtype
    dt, f32, dev, lib, stream = ops._act_dtype(c), int(c == "fp32"), mask.device, _lib.load(), _lib.current_stream()
    p = enc._operands()["layers"][0]
    x, y, ctx, z = (torch.randn(M, H, device=dev).to(dt) for _ in range(4))
    qkv, h, h2 = torch.randn(M, 3 * H, device=dev).to(dt), torch.randn(M, inter, device=dev).to(dt), torch.empty(M, inter, dtype=dt, device=dev)
    m = (mask != 0).float().reshape(-1).contiguous()
    ids = torch.randint(0, enc.config["vocab_size"], (M,), device=dev)
    word, pos, typ, g0, b0 = enc._operands()["emb"]
    em = _lib.BertEmbedArgs()
    em.ids, em.word, em.pos, em.type, em.gamma, em.beta, em.x, em.eps = [t.data_ptr() for t in (ids, word, pos, typ, g0, b0, x)] + [enc.eps]
    em.B, em.L, em.H, em.ld_x, em.act_f32, em.stream = B, L, H, H, f32, stream
    em.V, em.P, em.T = enc.config["vocab_size"], enc.config["max_position_embeddings"], enc.config["type_vocab_size"]
    at = _lib.BertAttnArgs()
    at.qkv, at.mask, at.ctx, at.B, at.L, at.H, at.ld_qkv, at.ld_ctx, at.act_f32, at.stream = qkv.data_ptr(), m.data_ptr(), ctx.data_ptr(), B, L, H, 3 * H, H, f32, stream
    ln = _lib.BertAddLnArgs()
    ln.y, ln.x, ln.gamma, ln.beta, ln.out, ln.eps = y.data_ptr(), x.data_ptr(), p["g1"].data_ptr(), p["b1"].data_ptr(), z.data_ptr(), enc.eps
    ln.M, ln.N, ln.ld_y, ln.ld_x, ln.ld_out, ln.act_f32, ln.stream = M, H, H, H, H, f32, stream
    ge = _lib.BertGeluArgs()
    ge.x, ge.out, ge.M, ge.N, ge.ld_x, ge.ld_out, ge.act_f32, ge.stream = h.data_ptr(), h2.data_ptr(), M, inter, inter, inter, f32, stream
    fns = {"embed_ln": lambda: _lib.check(lib.mmdeer_bert_embed_fwd(C.byref(em))),
           "qkv_gemm": lambda: ops.linear_into(x, p["wqkv"], p["bqkv"], qkv, compute=c),
           "attention": lambda: _lib.check(lib.mmdeer_bert_attn_fwd(C.byref(at))),
           "out_proj_gemm": lambda: ops.linear_into(ctx, p["wo"], p["bo"], y, compute=c),
           "add_ln": lambda: _lib.check(lib.mmdeer_bert_add_ln_fwd(C.byref(ln))),
           "ffn_in_gemm": lambda: ops.linear_into(y, p["wi"], p["bi"], h, compute=c),
           "gelu": lambda: _lib.check(lib.mmdeer_bert_gelu_fwd(C.byref(ge))),
           "ffn_out_gemm": lambda: ops.linear_into(h, p["wo2"], p["bo2"], x, compute=c)}
    cells = interleaved(fns, a.reps, a.launch_iters, a.warmup)
    valid = (mask != 0).sum(1).double()
    flop = {"qkv_gemm": 2.0 * M * 3 * H * H, "out_proj_gemm": 2.0 * M * H * H, "ffn_in_gemm": 2.0 * M * inter * H, "ffn_out_gemm": 2.0 * M * H * inter,
            "attention": 4.0 * 64 * (H // 64) * float((valid * L).sum())}
    for k, f in flop.items():
        cells[k]["useful_gflop"] = round(f / 1e9, 3)
        cells[k]["tflops"] = round(f / (cells[k]["median_ms"] * 1e-3) / 1e12, 2)
        cells[k]["share_of_bf16_mfma_rate"] = round(cells[k]["tflops"] / MFMA_BF16_TFLOPS, 4)
    per_layer = sum(cells[k]["median_ms"] for k in fns if k not in ("embed_ln", "add_ln")) + 2 * cells["add_ln"]["median_ms"]
    cells["sum_of_medians_ms"] = round(cells["embed_ln"]["median_ms"] + LAYERS * per_layer, 4)
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
        raise SystemExit("bert_time.py measures on the GPU: none found")
    dev = "cuda:0"
    cfg = {**bert.DEFAULTS, "num_hidden_layers": LAYERS}
    res = {"device": torch.cuda.get_device_name(0), "geometry": "bert-base: 768 / 12 heads / 3072, 12 layers", "L": L, "reps": a.reps,
           "iters": a.iters, "launch_iters": a.launch_iters, "warmup": a.warmup, "cells": []}
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
        enc = bert.BertEncoder(cfg, compute)
        enc.load_state_dict(sd, strict=True)
        enc = enc.to(dev)
        name, torch_fwd = yardstick(cfg, sd, dt, dev)
        res["yardstick"] = name
        for B in [int(v) for v in a.B.split(",")]:
            ids = torch.randint(1, cfg["vocab_size"], (B, L), device=dev)
            mask = torch.ones(B, L, dtype=torch.int64, device=dev)
            mask[1::2, L // 2:] = 0                                   # half of the samples padded to L / 2
            with torch.no_grad():
                hip = lambda: enc(ids, mask).last_hidden_state       # noqa: E731
                ref = lambda: torch_fwd(ids, mask)                    # noqa: E731
                valid = mask.bool().unsqueeze(-1)
                d = ((hip().float() - ref().float()) * valid).abs()
                cell = {"compute": compute, "B": B, "max_abs_difference_on_valid_rows": round(float(d.max()), 5),
                        "rms_difference_on_valid_rows": round(float((d.pow(2).sum() / (valid.sum() * 768)).sqrt()), 6)}
                cell.update(interleaved({"mmdeer_eager": hip, "torch_eager": ref}, a.reps, a.iters, a.warmup))
                graphs = {"mmdeer_graph": captured(hip, a.warmup)}
                try:
                    graphs["torch_graph"] = captured(ref, a.warmup)
                except Exception as e:  # noqa: BLE001  (the yardstick may not be capturable: say so, time the rest)
                    cell["torch_graph"] = f"not captured: {type(e).__name__}"
                    torch.cuda.synchronize()
                cell.update(interleaved(graphs, a.reps, a.iters, a.warmup))
                cell["launches"] = launch_cells(enc, B, mask, a)
            res["cells"].append(cell)
            print(json.dumps({k: v for k, v in cell.items() if k != "launches"}), file=sys.stderr, flush=True)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
