#!/usr/bin/env python3
"""Capture tests/golden/frame_grad.npz from the IMPORTED reference (build container only).

Run from the repo root:  python tests/golden/make_golden_frames_grad.py
encoders.EnhancedVideoEncoder (reference src/models/encoders.py:392-550) trained END TO END from frames, on the CPU in fp32,
dropout = 0, loss = sum(out * w).  Cases (B, T, H, W): train() at (5, 5, 16, 16) and (6, 1, 5, 7), and (2, 3, 19, 23) with the
backbone in eval() under a training head (frozen statistics) -- the fills (tests/video_ref.filled_state, tag frm<B>x<T>x<H>x<W>) and
the frames (tests/frames_ref.frames_input, stream 940 + index in make_golden_frames.CASES) of frame_seq.npz's cases; w comes from
the counter-based generator, stream 980 + that index.  None of the three is stored.

Per case: the (B, 512) output and the gradient of every ``spatial_backbone.*`` parameter -- a tensor of up to 16,384 elements whole
(``grad.``), a larger one as the strided slice flat[::stride][:16384], stride = ceil(numel / 16384) (``gradslice.``), with its L2 norm
(``gradnorm.``) and its largest magnitude (``gradmax.``).  Under batch statistics a convolution's bias shifts every position of a
channel equally and BatchNorm removes the shift: its gradient is analytically zero, the reference returns rounding noise, stored as
``gradnoise.``.

Prints, per tensor, the distance of this fp32 capture to the float64 restatement (tests/frames_bwd_ref.module_grads) as a fraction
of the tensor's largest element: it must stay below a quarter of the GPU test's bound (atol_frac 3e-3)."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as G  # noqa: E402  (sets up the import paths of the reference and of mmdeer)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from make_golden_video import reference_encoder  # noqa: E402

from mmdeer import synth  # noqa: E402
from tests import frames_bwd_ref as RB  # noqa: E402
from tests import frames_ref as R  # noqa: E402

# (index of the case in make_golden_frames.CASES, B, T, H, W, backbone in train mode)
CASES = [(1, 5, 5, 16, 16, True), (3, 6, 1, 5, 7, True), (0, 2, 3, 19, 23, False)]
WHOLE = 16384
CONV_BIASES = [f"{conv}.bias" for conv, _ in R.LAYERS]


def tag_of(B, T, H, W):
    return f"frm{B}x{T}x{H}x{W}"


def loss_weight(i, B):
    return synth.normal(980 + i, B * 512).reshape(B, 512).astype(np.float32)


def stride_of(numel):
    return -(-numel // WHOLE)


def capture():
    out = {}
    for i, B, T, H, W, train in CASES:
        tag = tag_of(B, T, H, W)
        enc = reference_encoder()
        shapes = {k: tuple(v.shape) for k, v in enc.state_dict().items()}
        sd = R.filled_state(tag, shapes)
        enc.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        enc.train()
        enc.spatial_backbone.train(train)
        x, w = R.frames_input(940 + i, B, T, H, W), loss_weight(i, B)
        y = enc(torch.from_numpy(x))
        (y * torch.from_numpy(w)).sum().backward()
        out[f"{tag}.out"] = G.tnp(y)
        P = {k: torch.from_numpy(v.astype(np.int64) if k.endswith("num_batches_tracked") else v).double() for k, v in sd.items()}
        _, y64, g64 = RB.module_grads(P, torch.from_numpy(x).double(), torch.from_numpy(w).double(), train, True)
        print(f"{tag} (backbone {'train' if train else 'eval'}): out max abs {np.abs(out[f'{tag}.out'] - y64.numpy()).max():.2e}")
        wmax = {conv: float(dict(enc.named_parameters())[f"{conv}.weight"].grad.abs().max()) for conv, _ in R.LAYERS}
        for name, p in enc.named_parameters():
            if not name.startswith("spatial_backbone."):
                continue
            g = p.grad.detach().numpy()
            if train and name in CONV_BIASES:
                out[f"{tag}.gradnoise.{name}"] = g
                print(f"    gradnoise {name}: max {np.abs(g).max():.2e}  (1e-4 max|dW| = {1e-4 * wmax[name[:-5]]:.2e}; float64 {float(g64[name].abs().max()):.1e})")
                continue
            if g.size <= WHOLE:
                out[f"{tag}.grad.{name}"] = g
            else:
                out[f"{tag}.gradslice.{name}"] = g.reshape(-1)[::stride_of(g.size)][:WHOLE].copy()
                out[f"{tag}.gradnorm.{name}"] = np.float64(np.linalg.norm(g.astype(np.float64)))
                out[f"{tag}.gradmax.{name}"] = np.float64(np.abs(g).max())
            d = np.abs(g - g64[name].numpy()).max() / np.abs(g64[name].numpy()).max()
            print(f"    {name}: |reference - float64| = {d:.2e} of the largest element ({d / (0.25 * 3e-3):.3f} of a quarter of the bound)")
    return out


def main():
    out = capture()
    path = os.path.join(HERE, "frame_grad.npz")
    np.savez_compressed(path, **out)
    print("frame_grad.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
