#!/usr/bin/env python3
"""Capture tests/golden/frame_seq.npz from the IMPORTED reference (build container only).

Run from the repo root:  python tests/golden/make_golden_frames.py
encoders.EnhancedVideoEncoder (reference src/models/encoders.py:392-550) on frames, on the CPU, dropout = 0.  Cases (B, T, H, W):
eval() at (2, 3, 19, 23), (2, 2, 1, 1) and (2, 1, 224, 224) -- the last given as the 4-D tensor (2, 3, 224, 224), the reference's
single-frame path -- and train() at (5, 5, 16, 16) and (6, 1, 5, 7).  Each case has its own closed-form parameter fill
(tests/video_ref.filled_state, tag frm<B>x<T>x<H>x<W>) and its frames from the counter-based generator
(tests/frames_ref.frames_input, stream 940 + case index): neither is stored.  Per case: the (B, T, 512) features of
``extract_spatial_features``, the (B, 512) output and, for train cases, the twelve BatchNorm2d buffers after the step.

The train cases are larger than the smallest that would run: at (3, 2, 16, 16) and (2, 1, 5, 7) the last BatchNorm2d layers see six
and two values per channel, 1 / sqrt(var + eps) amplifies the rounding of a near-constant channel up to 1 / (2 sqrt(eps)) = 158
times, and the reference's own fp32 result is then 1.1 and 24 times a quarter of the module tolerance (rtol 1e-3, atol 2e-5) away
from float64 -- at every input scale tried (0.25 .. 16): BatchNorm removes the scale.  At these sizes it is 0.6 and 0.3 times;
(6, 1, 5, 7) still has one value per frame at the last three layers, and (5, 5, 16, 16) gives the temporal BatchNorm1d layers downstream
the 25 positions of the smallest training case of video_seq.npz, the one the bf16 module tolerance was set on.

Prints, per stored tensor, the distance of this fp32 capture to the float64 restatement tests/frames_ref.py on the same inputs:
the part of a test bound that the reference's own rounding uses up.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as G  # noqa: E402  (sets up the import paths of the reference and of mmdeer)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from make_golden_video import reference_encoder, rel  # noqa: E402

from tests import frames_ref as R  # noqa: E402

# (B, T, H, W, train, given as a 4-D tensor)
CASES = [(2, 3, 19, 23, False, False), (5, 5, 16, 16, True, False), (2, 2, 1, 1, False, False), (6, 1, 5, 7, True, False),
         (2, 1, 224, 224, False, True)]


def tag_of(B, T, H, W):
    return f"frm{B}x{T}x{H}x{W}"


def capture():
    out = {}
    for i, (B, T, H, W, train, four_d) in enumerate(CASES):
        tag = tag_of(B, T, H, W)
        enc = reference_encoder()
        shapes = {k: tuple(v.shape) for k, v in enc.state_dict().items()}
        sd = R.filled_state(tag, shapes)
        enc.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        enc.train(train)
        x = R.frames_input(940 + i, B, T, H, W)
        seen = {}
        inner = enc.extract_spatial_features
        enc.extract_spatial_features = lambda v: seen.setdefault("feats", inner(v))
        with torch.no_grad():
            y = enc(torch.from_numpy(x[:, 0] if four_d else x))
        out[f"{tag}.feats"], out[f"{tag}.out"] = G.tnp(seen["feats"]), G.tnp(y)
        if train:
            after = enc.state_dict()
            for k in R.BUFFERS:
                out[f"{tag}.buffer.{k}"] = G.tnp(after[k])
        # ---- distance of this capture to the float64 restatement
        P = {k: torch.from_numpy(v.astype(np.int64) if k.endswith("num_batches_tracked") else v).double() for k, v in sd.items()}
        f64, y64, buf64 = R.encoder(P, torch.from_numpy(x).double(), train)
        print(f"{tag} ({'train' if train else 'eval'}): feats rel {rel(out[f'{tag}.feats'], f64):.2e}  max |feats| {np.abs(out[f'{tag}.feats']).max():.2e}"
              f"  out rel {rel(out[f'{tag}.out'], y64):.2e}  max abs {np.abs(out[f'{tag}.out'] - y64.numpy()).max():.2e}")
        for k in R.BUFFERS if train else ():
            print(f"    buffer {k}: rel {rel(out[f'{tag}.buffer.{k}'], buf64[k].numpy()):.2e}")
    return out


def main():
    out = capture()
    path = os.path.join(HERE, "frame_seq.npz")
    np.savez_compressed(path, **out)
    print("frame_seq.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
