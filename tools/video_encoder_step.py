#!/usr/bin/env python3
"""One training step (forward + backward + SGD update) of mmdeer.video.TemporalVideoEncoder, for a kernel trace:

    rocprofv3 --kernel-trace --stats -d OUT -- python tools/video_encoder_step.py [--B 4096] [--T 8] [--dtype bf16]

The step runs once, after the inputs are made, so the trace holds the step's launches and the few of the setup."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from mmdeer import video  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--T", type=int, default=8)
    ap.add_argument("--dtype", default="bf16")
    a = ap.parse_args()
    m = video.TemporalVideoEncoder(compute_dtype=a.dtype).to("cuda:0").train()
    params = [p for n, p in m.named_parameters() if not n.startswith("spatial_backbone.")]
    x = torch.randn(a.B, a.T, 512, device="cuda:0")
    target = torch.randn(a.B, 512, device="cuda:0")
    torch.cuda.synchronize()
    loss = (m(x) - target).square().mean()
    loss.backward()
    with torch.no_grad():
        for p in params:
            p.add_(p.grad, alpha=-1e-3)
    torch.cuda.synchronize()
    print(f"step ok: B={a.B} T={a.T} {a.dtype} loss={float(loss.detach()):.6f}")


if __name__ == "__main__":
    main()
