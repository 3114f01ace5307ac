#!/usr/bin/env python3
"""Capture tests/golden/audio_seq.npz from the IMPORTED reference (build container only).

Run from the repo root:  python tests/golden/make_golden_temporal.py
encoders.EnhancedAudioEncoder (reference src/models/encoders.py:356-389) on (B, T, 84) pre-extracted features, eval mode,
for (B, T) in CASES; each case has its own closed-form parameter fill (synth.module_fill, tag seq<B>x<T>) and synth inputs.
Per case: the input, the output, lstm_out and the attention weights (for debugging), and the input / parameter gradients of
sum(y * w), w = synth.normal (stored as loss_w), in make_golden.store_grads' format.  The attention.2.bias gradient is
rounding noise in the reference (b2 shifts every score of a sample equally): it is stored as `gradnoise.`, a kind that
check_side_grads skips, and tested against an absolute bound instead.
"""
import contextlib
import io
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as G  # noqa: E402  (sets up the import paths of the reference and of mmdeer)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from mmdeer import synth  # noqa: E402

CASES = [(9, 2), (5, 5), (3, 33)]


def reference_encoder():
    # encoders.py imports librosa / cv2 at module level; the feature branch touches neither (as make_golden.capture_side)
    for missing in ("librosa", "cv2"):
        if missing not in sys.modules:
            m = types.ModuleType(missing)
            m.__spec__ = __import__("importlib.machinery").machinery.ModuleSpec(missing, None)
            sys.modules[missing] = m
    with contextlib.redirect_stdout(io.StringIO()):
        import encoders as ref_enc  # (reference)
        return ref_enc.EnhancedAudioEncoder().eval()


def capture():
    out = {}
    for i, (B, T) in enumerate(CASES):
        tag = f"seq{B}x{T}"
        enc = reference_encoder()
        G.fill_module(enc, tag)
        x = synth.normal(700 + i, B * T * 84).reshape(B, T, 84).astype(np.float32)
        xa = torch.from_numpy(x).requires_grad_(True)
        y = enc(xa)
        with torch.no_grad():
            lstm_out, _ = enc.lstm(xa)
            a = enc.attention(lstm_out)[..., 0]
        w = synth.normal(720 + i, y.numel()).reshape(y.shape).astype(np.float32)
        out[f"{tag}.input"], out[f"{tag}.out"], out[f"{tag}.loss_w"] = x, G.tnp(y), w
        out[f"{tag}.lstm_out"], out[f"{tag}.attn"] = G.tnp(lstm_out), G.tnp(a)
        (y * torch.from_numpy(w)).sum().backward()
        G.store_grads(out, tag, enc, {"audio": xa})
        out[f"{tag}.gradnoise.attention.2.bias"] = out.pop(f"{tag}.grad.attention.2.bias")
    return out


def main():
    path = os.path.join(HERE, "audio_seq.npz")
    np.savez_compressed(path, **capture())
    print("audio_seq.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
