#!/usr/bin/env python3
"""Time mmdeer.text.TemporalTextEncoder (eval forward, and training forward + backward) at (B, L) = (1024, 128) and (4096, 64),
fp32 and bf16, both entry points, and beside each figure the same encoder written with torch.nn (rocBLAS GEMMs + eager
element-wise kernels) in the same dtype on the same GPU, as a yardstick; the two alternate within one process.  The yardstick
comes in two forms: `torch_loop` computes the ten token statistics as the reference does, in a Python loop over the batch with
its host syncs (timed with one repetition, it takes seconds), and `torch_vec` computes them with a vectorised torch
restatement (sort + run lengths), which is the form the module is required not to be slower than.

Also times the pool kernel alone (mmdeer_token_pool_fwd) and states its bytes moved / time; with --calibrate PATH (the binary
built from tools/probes/calibrate.hip) the streaming read bandwidth that probe reports on the same box is put beside it.

Prints one JSON object: per configuration the median / min / max of `--reps` timed repetitions (each the mean over `--iters`
back-to-back calls between two events), after `--warmup` calls.

    python tools/text_encoder_time.py [--reps 7] [--iters 5] [--warmup 3] [--shapes 1024x128,4096x64] [--calibrate tools/probes/calibrate]
"""
from __future__ import annotations

import argparse
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
from torch import nn  # noqa: E402

from mmdeer import text  # noqa: E402

E, A = 768, 384


def stats_loop(ids, mask, max_length):
    """the reference's extract_linguistic_features: a Python loop over the batch, several host syncs per sample"""
    feats = []
    for i in range(ids.shape[0]):
        v = ids[i][mask[i].bool()]
        n = len(v)
        u = len(torch.unique(v))
        counts = torch.bincount(v)
        avg = torch.mean(counts.float()) if len(counts) > 0 else 0
        mx = torch.max(counts.float()) if len(counts) > 0 else 0
        punct = torch.sum((v >= 999) & (v <= 1030))
        special = torch.sum((v >= 100) & (v <= 999))
        feats.append(torch.tensor([n / max_length, u / max(n, 1), avg, mx, punct / max(n, 1), special / max(n, 1), 0.0, 0.0, 0.0, 0.0],
                                  dtype=torch.float32))
    return torch.stack(feats).to(ids.device)


def stats_vec(ids, mask, max_length):
    """the same ten features without a host loop: sort each row (masked positions behind every id) and read run lengths"""
    B, L = ids.shape
    valid = mask != 0
    n = valid.sum(1)
    big = torch.iinfo(torch.int64).max
    s, _ = torch.sort(torch.where(valid, ids, torch.full_like(ids, big)), dim=1)
    sv = s != big
    head = torch.ones_like(sv)
    head[:, 1:] = s[:, 1:] != s[:, :-1]
    head &= sv
    u = head.sum(1)
    pos = torch.arange(L, device=ids.device).expand(B, L)
    start = torch.cummax(torch.where(head, pos, torch.zeros_like(pos)), dim=1)[0]
    cmax = torch.where(sv, pos - start + 1, torch.zeros_like(pos)).max(1)[0]
    idmax = torch.where(valid, ids, torch.full_like(ids, -1)).max(1)[0]
    punct = (valid & (ids >= 999) & (ids <= 1030)).sum(1)
    special = (valid & (ids >= 100) & (ids <= 999)).sum(1)
    nf, den = n.float(), n.clamp(min=1).float()
    z = torch.zeros_like(nf)
    f = torch.stack([nf / max_length, u / den, nf / (idmax + 1).clamp(min=1).float(), cmax.float(), punct / den, special / den, z, z, z, z], dim=1)
    return torch.where((n > 0)[:, None], f, torch.zeros_like(f))


class TorchText(nn.Module):
    """the yardstick: encoders.EnhancedTextEncoder's no-BERT configuration, layer for layer, with torch.nn"""

    def __init__(self, stats, dropout=0.3):
        super().__init__()
        self.stats, self.max_length = stats, 128
        self.embedding = nn.Embedding(30000, E, padding_idx=0)
        self.positional_encoding = nn.Embedding(128, E)
        self.token_attention = nn.Sequential(nn.Linear(E, A), nn.Tanh(), nn.Linear(A, 1), nn.Softmax(dim=1))
        self.bert_projection = nn.Sequential(nn.Linear(E, 512), nn.ReLU(), nn.Dropout(dropout))
        self.linguistic_projection = nn.Sequential(nn.Linear(10, 128), nn.ReLU(), nn.Dropout(dropout))
        self.output_projection = nn.Sequential(nn.Linear(640, 512), nn.ReLU(), nn.Dropout(dropout), nn.LayerNorm(512))

    def tail(self, tok, ids, mask):
        dt = tok.dtype
        x = tok * mask.unsqueeze(-1).to(dt)
        w = self.token_attention(x) * mask.unsqueeze(-1).to(dt)
        w = w / (w.sum(1, keepdim=True) + 1e-10)
        pb = self.bert_projection((x * w).sum(1))
        pl = self.linguistic_projection(self.stats(ids, mask, self.max_length).to(dt))
        return self.output_projection(torch.cat([pb, pl], dim=1)).float()

    def forward(self, ids, mask):
        ids = ids.clamp(0, 29999)
        t = torch.arange(ids.shape[1], device=ids.device).clamp(max=127)
        return self.tail(self.embedding(ids) + self.positional_encoding(t)[None], ids, mask)

    def forward_embeddings(self, tok, ids, mask):
        return self.tail(tok, ids, mask)


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


def pool_row(B, L, compute, a):
    """mmdeer_token_pool_fwd alone: x and z read once, attended + weights + probs written"""
    dt = torch.float32 if compute == "fp32" else torch.bfloat16
    dev = "cuda:0"
    mask = (torch.rand(B, L, device=dev) < 0.8).float()
    x = (torch.randn(B * L, E, device=dev) * mask.reshape(-1, 1)).to(dt)
    z = torch.randn(B * L, A, device=dev).to(dt)
    w2, b2 = torch.randn(1, A, device=dev) * 0.1, torch.zeros(1, device=dev)
    m = mask.reshape(-1).contiguous()
    el = x.element_size()
    valid = int(mask.sum())
    nbytes = valid * E * el + B * L * A * el + B * E * el + B * L * 4 * 4      # masked rows of x are not read; mask, scores in / out, probs
    with torch.no_grad():
        t = timed(lambda: text._TokenPoolFn.apply(x, z, m, w2, b2, B, L, compute), a.reps, a.iters, a.warmup)
    return {"compute": compute, "B": B, "L": L, "op": "token_pool_fwd (+ the fp32 copy of attended)", "bytes": nbytes, **t,
            "tbps": round(nbytes / (t["median_ms"] * 1e-3) / 1e12, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="1024x128,4096x64")
    ap.add_argument("--calibrate", default=None, help="binary of tools/probes/calibrate.hip: its streaming read bandwidth is recorded")
    ap.add_argument("--no-loop", action="store_true", help="skip the per-sample Python loop yardstick (seconds per call)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("text_encoder_time.py needs a GPU")
    dev = "cuda:0"
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "iters": a.iters, "warmup": a.warmup, "rows": [], "pool": []}
    if a.calibrate:
        out = subprocess.run([a.calibrate], capture_output=True, text=True, timeout=120).stdout
        mt = re.search(r"streaming read of .*: ([0-9.]+) TB/s", out)
        res["stream_read_tbps"] = float(mt.group(1)) if mt else None
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    for compute in ("fp32", "bf16"):
        dt = torch.float32 if compute == "fp32" else torch.bfloat16
        for B, L in shapes:
            torch.manual_seed(0)
            m = text.TemporalTextEncoder(compute_dtype=compute).to(dev)
            yv, yl = TorchText(stats_vec).to(dev).to(dt), TorchText(stats_loop).to(dev).to(dt)
            ids = torch.randint(0, 30000, (B, L), device=dev)
            lens = torch.randint(L // 4, L + 1, (B,), device=dev)
            mask = (torch.arange(L, device=dev)[None] < lens[:, None]).long()
            Em = torch.randn(B, L, E, device=dev)
            Ed = Em.to(dt)
            tgt = torch.randn(B, 512, device=dev)
            assert torch.allclose(stats_vec(ids[:32], mask[:32], 128), stats_loop(ids[:32], mask[:32], 128), rtol=1e-6, atol=0)
            assert torch.allclose(m.extract_linguistic_features(ids[:32], mask[:32]), stats_loop(ids[:32], mask[:32], 128), rtol=1e-6, atol=0)
            for path in ("ids", "embeddings"):
                row = {"compute": compute, "B": B, "L": L, "path": path}

                def call(mod, e):
                    return mod(ids, mask) if path == "ids" else mod.forward_embeddings(e, ids, mask)

                def fwd(mod, e):
                    with torch.no_grad():
                        call(mod, e)

                def step(mod, e):
                    for p in mod.parameters():
                        p.grad = None
                    (call(mod, e) - tgt).square().mean().backward()

                for mod in (m, yv, yl):
                    mod.eval()
                row["mmdeer_fwd"] = timed(lambda: fwd(m, Em), a.reps, a.iters, a.warmup)
                row["torch_vec_fwd"] = timed(lambda: fwd(yv, Ed), a.reps, a.iters, a.warmup)
                if not a.no_loop and path == "ids":
                    row["torch_loop_fwd"] = timed(lambda: fwd(yl, Ed), 1, 1, 0)
                for mod in (m, yv, yl):
                    mod.train()                            # dropout 0.3 live on both sides
                row["mmdeer_fwd_bwd"] = timed(lambda: step(m, Em), a.reps, a.iters, a.warmup)
                row["torch_vec_fwd_bwd"] = timed(lambda: step(yv, Ed), a.reps, a.iters, a.warmup)
                res["rows"].append(row)
                print(json.dumps(row), file=sys.stderr, flush=True)
            res["pool"].append(pool_row(B, L, compute, a))
            print(json.dumps(res["pool"][-1]), file=sys.stderr, flush=True)
            del m, yv, yl
    print(json.dumps(res))


if __name__ == "__main__":
    main()
