#!/usr/bin/env python3
"""Capture tests/golden/video_seq.npz and video_state_dict_names.json from the IMPORTED reference (build container only).

Run from the repo root:  python tests/golden/make_golden_video.py
encoders.EnhancedVideoEncoder (reference src/models/encoders.py:392-550) downstream of its spatial CNN: the reference's own
forward runs on per-frame features (B, T, 512) by replacing ``extract_spatial_features`` with a function that returns them (the
frame tensor it is then called with is a (B, T, 1, 1, 1) placeholder).  dropout = 0.  Cases: eval() at (B, T) = (9, 2), (3, 17),
(4, 1); train() at (5, 5), (2, 17).  Each case has its own closed-form parameter fill (tests/video_ref.filled_state, tag
vid<B>x<T>: synth.module_fill with the running variances made positive) and synth inputs.  Per case: the input, the output,
loss_w, the input / parameter gradients of sum(y * loss_w) in make_golden.store_grads' format and, for train cases, the three
buffers of both BatchNorm1d layers after the step.  spatial_backbone.* is never run: its (absent) gradients are not stored.

Under batch statistics the gradients of the two Conv1d biases are analytically zero (BatchNorm subtracts the mean they shift);
the reference returns rounding noise.  They are stored as `gradnoise.`, a kind that check_side_grads skips, and tested against an
absolute bound.  In eval() they are real gradients and stay `grad.`.  The gradient of temporal_attention.2.bias is noise of the
same kind in every case with T > 1 (as attention.2.bias in audio_seq.npz).

Prints, per stored tensor, the distance of this fp32 capture to the float64 restatement tests/video_ref.py on the same inputs:
the part of a test bound that the reference's own rounding uses up.
"""
import contextlib
import io
import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as G  # noqa: E402  (sets up the import paths of the reference and of mmdeer)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from mmdeer import synth  # noqa: E402
from tests import video_ref as R  # noqa: E402

EVAL_CASES = [(9, 2), (3, 17), (4, 1)]
TRAIN_CASES = [(5, 5), (2, 17)]
NOISE_BIASES = ("temporal_cnn.0.bias", "temporal_cnn.4.bias")
BUFFERS = [f"{l}.{k}" for l in R.BN_LAYERS for k in ("running_mean", "running_var", "num_batches_tracked")]


def reference_encoder():
    for missing in ("librosa", "cv2"):      # encoders.py imports them at module level; this path touches neither
        if missing not in sys.modules:
            m = types.ModuleType(missing)
            m.__spec__ = __import__("importlib.machinery").machinery.ModuleSpec(missing, None)
            sys.modules[missing] = m
    with contextlib.redirect_stdout(io.StringIO()):
        import encoders as ref_enc  # (reference)
        return ref_enc.EnhancedVideoEncoder({"dropout": 0.0})


def rel(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def restated(sd, x, w, train):
    """tests/video_ref.encoder in float64 on the same state: output, gradients by state_dict name, buffers after the step."""
    P = {k: torch.from_numpy(v.astype(np.int64) if k.endswith("num_batches_tracked") else v).double()
         for k, v in sd.items() if not k.startswith("spatial_backbone.")}
    for k, v in P.items():
        if v.dim() and "running" not in k:
            v.requires_grad_(True)
    x64 = torch.from_numpy(x).double().requires_grad_(True)
    y, buffers = R.encoder(P, x64, train)
    (y * torch.from_numpy(w).double()).sum().backward()
    return y.detach().numpy(), {k: v.grad for k, v in P.items() if v.requires_grad}, x64.grad.numpy(), buffers


def capture():
    out, names = {}, None
    for i, (B, T, train) in enumerate([(*c, False) for c in EVAL_CASES] + [(*c, True) for c in TRAIN_CASES]):
        tag = f"vid{B}x{T}"
        enc = reference_encoder()
        shapes = {k: tuple(v.shape) for k, v in enc.state_dict().items()}
        sd = R.filled_state(tag, shapes)
        enc.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        enc.train(train)
        if names is None:
            names = [[k, list(s)] for k, s in shapes.items()]
        # inputs are rounded to fp16-representable values and stored as fp16 (exactly): half the bytes of the fixture's largest part
        x = synth.normal(900 + i, B * T * 512).reshape(B, T, 512).astype(np.float16).astype(np.float32)
        xa = torch.from_numpy(x).requires_grad_(True)
        enc.extract_spatial_features = lambda v, feats=xa: feats
        y = enc(torch.empty(B, T, 1, 1, 1))
        w = synth.normal(920 + i, y.numel()).reshape(y.shape).astype(np.float32)
        out[f"{tag}.input"], out[f"{tag}.out"], out[f"{tag}.loss_w"] = x.astype(np.float16), G.tnp(y), w
        (y * torch.from_numpy(w)).sum().backward()
        G.store_grads(out, tag, enc, {"video": xa})
        for k in [k for k in out if k.startswith(f"{tag}.gradnone.spatial_backbone.")]:
            del out[k]
        if T > 1:      # b2 shifts every score of a sample equally: the reference's gradient is rounding noise, ours an exact zero
            out[f"{tag}.gradnoise.temporal_attention.2.bias"] = out.pop(f"{tag}.grad.temporal_attention.2.bias")
        if train:
            for n in NOISE_BIASES:
                out[f"{tag}.gradnoise.{n}"] = out.pop(f"{tag}.grad.{n}")
            after = enc.state_dict()
            for k in BUFFERS:
                out[f"{tag}.buffer.{k}"] = G.tnp(after[k])
        # ---- distance of this capture to the float64 restatement
        y64, g64, dx64, buf64 = restated(sd, x, w, train)
        print(f"{tag} ({'train' if train else 'eval'}): out rel {rel(out[f'{tag}.out'], y64):.2e}  max abs {np.abs(out[f'{tag}.out'] - y64).max():.2e}"
              f"  dx rel {rel(out[f'{tag}.dx.video'], dx64):.2e}")
        for k in sorted(out):
            if not k.startswith(tag + "."):
                continue
            kind, _, name = k[len(tag) + 1:].partition(".")
            if kind == "grad" and np.abs(out[k]).max() > 0:
                d = np.abs(out[k] - g64[name].numpy()).max() / np.abs(out[k]).max()
                print(f"    grad {name}: max abs err / max abs {d:.2e}")
            elif kind == "gradnorm":
                v = g64[name].reshape(-1)
                idx = torch.linspace(0, v.numel() - 1, 1024).round().long()
                d = np.abs(out[f"{tag}.gradsample.{name}"] - v[idx].numpy()).max() / np.abs(out[f"{tag}.gradsample.{name}"]).max()
                print(f"    grad {name}: norm rel {abs(float(out[k]) - float(v.norm())) / float(v.norm()):.2e}  sample max abs err / max abs {d:.2e}")
            elif kind == "gradnoise":
                wmax = float(np.abs(g64[name.replace("bias", "weight")].numpy()).max())
                print(f"    gradnoise {name}: max |.| {np.abs(out[k]).max():.2e} = {np.abs(out[k]).max() / wmax:.2e} of max |dW|")
            elif kind == "buffer":
                print(f"    buffer {name}: rel {rel(out[k], buf64[name].numpy()):.2e}")
    return out, names


def main():
    out, names = capture()
    path = os.path.join(HERE, "video_seq.npz")
    np.savez_compressed(path, **out)
    with open(os.path.join(HERE, "video_state_dict_names.json"), "w") as f:
        json.dump(names, f, indent=0)
        f.write("\n")
    print("video_seq.npz", os.path.getsize(path), "bytes;", len(names), "state_dict entries,", sum(int(np.prod(s)) for _, s in names), "elements")


if __name__ == "__main__":
    main()
