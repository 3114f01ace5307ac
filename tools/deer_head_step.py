#!/usr/bin/env python3
"""One training step (forward + MultiTaskDEERLoss + backward + SGD update) of mmdeer.head.MultiDimensionalDEER, for a kernel
trace:

    rocprofv3 --kernel-trace --stats -d OUT -- python tools/deer_head_step.py [--B 4096] [--dtype bf16]

The step runs once, after the inputs are made, so the trace holds the step's launches and the few of the setup."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from mmdeer import head, losses  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--input-dim", type=int, default=512)
    ap.add_argument("--hidden-dim", type=int, default=256)
    ap.add_argument("--dtype", default="bf16")
    a = ap.parse_args()
    m = head.MultiDimensionalDEER(a.input_dim, 3, a.hidden_dim, compute_dtype=a.dtype).to("cuda:0").train()
    loss_fn = losses.MultiTaskDEERLoss()
    x = torch.randn(a.B, a.input_dim, device="cuda:0")
    target = torch.tanh(torch.randn(a.B, 3, device="cuda:0"))
    torch.cuda.synchronize()
    loss = loss_fn(m(x), target)["total_loss"]
    loss.backward()
    with torch.no_grad():
        for p in m.parameters():
            p.add_(p.grad, alpha=-1e-3)
    torch.cuda.synchronize()
    print(f"step ok: B={a.B} {a.input_dim}/{a.hidden_dim} {a.dtype} loss={float(loss):.6f}")


if __name__ == "__main__":
    main()
