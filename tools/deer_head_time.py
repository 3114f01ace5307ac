#!/usr/bin/env python3
"""Time mmdeer.head.MultiDimensionalDEER (eval forward, and training forward + MultiTaskDEERLoss + backward) at
(input_dim, emotion_dims, hidden_dim) = (512, 3, 256) and (192, 3, 128), B in {1024, 4096}, fp32 and bf16, and beside each
figure the same layers written with torch.nn (rocBLAS GEMMs + eager element-wise kernels) in the same dtype on the same GPU, as
a yardstick; the two alternate within one process.  Prints one JSON object: per configuration the median / min / max of
`--reps` timed repetitions (each the mean over `--iters` back-to-back calls between two events), after `--warmup` calls.

    python tools/deer_head_time.py [--reps 7] [--iters 5] [--warmup 3] [--B 1024,4096]
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
from torch import nn  # noqa: E402
from torch.nn import functional as F  # noqa: E402

from mmdeer import head, losses  # noqa: E402

DIMS = ("valence", "arousal", "dominance")


class TorchHead(nn.Module):
    """the yardstick: shared Linear-ReLU x 2, per dimension Linear-ReLU x 2 + Linear(., 4), NIG activations, uncertainties"""

    def __init__(self, input_dim, hidden):
        super().__init__()
        self.shared = nn.Sequential(nn.Linear(input_dim, hidden), nn.ReLU(), nn.Linear(hidden, hidden), nn.ReLU())
        self.heads = nn.ModuleList([nn.Sequential(nn.Linear(hidden, hidden // 2), nn.ReLU(), nn.Linear(hidden // 2, hidden // 4), nn.ReLU(),
                                                  nn.Linear(hidden // 4, 4)) for _ in DIMS])

    def forward(self, x):
        f = self.shared(x)
        out = {}
        for name, net in zip(DIMS, self.heads):
            e = net(f).float()
            nu, alpha, beta = F.softplus(e[:, 1:2]) + 1e-6, F.softplus(e[:, 2:3]) + 1.0, F.softplus(e[:, 3:4]) + 1e-6
            alea = beta / (alpha - 1)
            epi = beta / (nu * (alpha - 1))
            out.update({f"{name}_mu": e[:, 0:1], f"{name}_nu": nu, f"{name}_alpha": alpha, f"{name}_beta": beta,
                        f"{name}_uncertainty": alea + epi})
        return out


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
    a = ap.parse_args()
    dev = "cuda:0"
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "iters": a.iters, "warmup": a.warmup, "rows": []}
    loss = losses.MultiTaskDEERLoss()
    for compute in ("fp32", "bf16"):
        dt = torch.float32 if compute == "fp32" else torch.bfloat16
        for input_dim, hidden in ((512, 256), (192, 128)):
            for B in [int(v) for v in a.B.split(",")]:
                torch.manual_seed(0)
                m = head.MultiDimensionalDEER(input_dim, 3, hidden, compute_dtype=compute).to(dev)
                y = TorchHead(input_dim, hidden).to(dev).to(dt)
                x = torch.randn(B, input_dim, device=dev)
                xd = x.to(dt)
                t = torch.tanh(torch.randn(B, 3, device=dev))
                row = {"compute": compute, "input_dim": input_dim, "hidden_dim": hidden, "B": B}

                def fwd(mod, inp):
                    with torch.no_grad():
                        mod(inp)

                def step(mod, inp):
                    for p in mod.parameters():
                        p.grad = None
                    loss(mod(inp), t)["total_loss"].backward()

                m.eval(), y.eval()
                row["mmdeer_fwd"] = timed(lambda: fwd(m, x), a.reps, a.iters, a.warmup)
                row["torch_fwd"] = timed(lambda: fwd(y, xd), a.reps, a.iters, a.warmup)
                m.train(), y.train()                       # dropout 0.3 live in the module; the yardstick has none
                row["mmdeer_fwd_bwd"] = timed(lambda: step(m, x), a.reps, a.iters, a.warmup)
                row["torch_fwd_bwd"] = timed(lambda: step(y, xd), a.reps, a.iters, a.warmup)
                res["rows"].append(row)
                print(json.dumps(row), file=sys.stderr, flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
