#!/usr/bin/env python3
"""Capture tests/golden/text_seq.npz + text_state_dict_names.json from the IMPORTED reference (build container only).

Run from the repo root:  python tests/golden/make_golden_text.py
encoders.EnhancedTextEncoder (reference src/models/encoders.py:553-761) in its no-BERT configuration, eval mode, for (B, L) in
CASES; each case has its own closed-form parameter fill (synth.module_fill, tag txt<B>x<L>).

The reference builds a BertModel whenever `transformers` imports, and that constructor fetches weights.  This script therefore
puts None in sys.modules["transformers"] BEFORE the reference's encoders module is imported, so that the reference takes its own
ImportError branch, and asserts that it did (TRANSFORMERS_AVAILABLE is False, enc.bert is None) before going on.

Per case two captures:
  tag  = txt<B>x<L>    forward(ids, mask), the fallback branch: ids (with ids < 0 and >= 30000), mask, output, attention weights,
                       linguistic features (of the clamped ids), loss_w and the gradients of sum(y * loss_w) in
                       make_golden.store_grads' format; embedding.weight (23 M elements, past what store_grads' float32
                       index arithmetic holds) as its l2 norm and the touched ids with their gradient rows (whole for the
                       two small cases, per-row l2 norms for the large one); every other row is an exact zero.
  tag + "e"            the BERT branch downstream of last_hidden_state: enc.bert replaced by a function that returns the
                       closed-form matrix E = synth.normal(760 + i) (not stored: the tests regenerate it), ids clamped below at 0
                       (the reference's bincount raises on negative ids) and NOT above; output, attention weights, features,
                       parameter gradients and dE (whole where small, else l2 norm + 1024 evenly spaced elements).
The token_attention.2.bias gradient is rounding noise in the reference (b2 shifts every score of a sample equally): it is
stored as `gradnoise.`, a kind that check_side_grads skips.
"""
import contextlib
import io
import json
import os
import sys
import types

sys.modules["transformers"] = None      # `import transformers` raises ImportError: the reference takes its no-BERT branch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as G  # noqa: E402  (sets up the import paths of the reference and of mmdeer)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from mmdeer import synth  # noqa: E402

CASES = [(9, 2), (5, 7), (3, 130)]
SMALL = 20000          # dE / embedding rows are stored whole up to this many elements


def reference_encoder():
    for missing in ("librosa", "cv2"):
        if missing not in sys.modules:
            m = types.ModuleType(missing)
            m.__spec__ = __import__("importlib.machinery").machinery.ModuleSpec(missing, None)
            sys.modules[missing] = m
    with contextlib.redirect_stdout(io.StringIO()):
        import encoders as ref_enc  # (reference)
        assert ref_enc.TRANSFORMERS_AVAILABLE is False
        enc = ref_enc.EnhancedTextEncoder().eval()
    assert enc.bert is None
    return enc


def inputs(i, B, L):
    """ids (int64, some < 0 and >= 30000) and mask (int64) of case i, closed form."""
    ids = (synth.uniform01(740 + i, B * L) * 30000).astype(np.int64).reshape(B, L)
    mask = (synth.uniform01(750 + i, B * L) < 0.7).astype(np.int64).reshape(B, L)
    if (B, L) == (9, 2):
        ids[0] = [7, 7]; mask[0] = [1, 1]               # full, one id twice          # noqa: E702
        mask[1] = [0, 0]                                # fully masked                  # noqa: E702
        ids[2] = [0, 101]; mask[2] = [1, 0]             # id 0 valid, single token      # noqa: E702
        ids[3] = [5, 40000]; mask[3] = [0, 1]           # id >= 30000                   # noqa: E702
        ids[4] = [-5, 7]; mask[4] = [1, 1]              # id < 0, id 7 again            # noqa: E702
        ids[5] = [999, 1030]; mask[5] = [1, 1]          # both range ends               # noqa: E702
        ids[6] = [100, 1005]; mask[6] = [1, 1]          # noqa: E702
    elif (B, L) == (5, 7):
        ids[0] = [101, 2023, 2003, 2023, 1012, 102, 0]; mask[0] = [1, 1, 1, 1, 1, 1, 0]        # noqa: E702
        ids[1, :] = 1005; mask[1] = [1, 0, 1, 1, 0, 0, 1]        # one id everywhere, holes in the middle     # noqa: E702
        mask[2] = 0                                                                              # fully masked
        ids[3] = [31000, -1, 29999, 0, 7, 7, 7]; mask[3] = 1                                     # noqa: E702
        mask[4] = [0, 0, 0, 0, 0, 0, 1]                                                          # only the last token
    else:
        mask[0] = 1                                                                              # full, positions past 127
        ids[0, :6] = [101, 7, 7, 40000, -3, 0]
        ids[0, 120:] = 2023
        ids[1] = 995 + (ids[1] % 40); mask[1, 50:90] = 0                                         # 995 .. 1034: many repeats  # noqa: E702
        mask[2] = 0; mask[2, L - 1] = 1; ids[2, L - 1] = 2023                                    # single token at t = 129    # noqa: E702
    return ids, mask


def embeddings(i, B, L):
    return synth.normal(760 + i, B * L * 768).reshape(B, L, 768).astype(np.float32)


def capture():
    out, names = {}, {}
    for i, (B, L) in enumerate(CASES):
        tag = f"txt{B}x{L}"
        ids, mask = inputs(i, B, L)
        idt, mt = torch.from_numpy(ids), torch.from_numpy(mask)
        w = synth.normal(770 + i, B * 512).reshape(B, 512).astype(np.float32)
        out[f"{tag}.ids"], out[f"{tag}.mask"], out[f"{tag}.loss_w"] = ids, mask, w

        def run(enc, t, ids_t):
            feats = {}
            hook = enc.token_attention.register_forward_hook(lambda mod, inp, o: feats.__setitem__("p", o))
            y = enc(ids_t, mt)
            hook.remove()
            p = feats["p"][..., 0].detach() * mt
            out[f"{t}.out"], out[f"{t}.attn"] = G.tnp(y), G.tnp(p / (p.sum(1, keepdim=True) + 1e-10))
            assert torch.isfinite(y).all()
            (y * torch.from_numpy(w)).sum().backward()
            return y

        # the fallback branch
        enc = reference_encoder()
        G.fill_module(enc, tag)
        names[tag] = {k: list(v.shape) for k, v in enc.state_dict().items()}
        run(enc, tag, idt)
        out[f"{tag}.ling"] = G.tnp(enc.extract_linguistic_features(torch.clamp(idt, 0, enc.vocab_size - 1), mt))
        ge = enc.embedding.weight.grad
        enc.embedding.weight.grad = None        # 23 M elements: store_grads' float32 linspace runs past the last index there
        G.store_grads(out, tag, enc, {})
        del out[f"{tag}.gradnone.embedding.weight"]
        out[f"{tag}.embnorm"] = np.float64(ge.double().norm().item())
        out[f"{tag}.gradnoise.token_attention.2.bias"] = out.pop(f"{tag}.grad.token_attention.2.bias")
        touched = torch.nonzero(ge.abs().sum(1) > 0)[:, 0]
        out[f"{tag}.emb_ids"] = touched.numpy()
        if touched.numel() * 768 <= 2 * SMALL:
            out[f"{tag}.emb_rows"] = G.tnp(ge[touched])
        else:
            out[f"{tag}.emb_rownorm"] = ge[touched].double().norm(dim=1).numpy()
        assert float(ge[0].abs().max()) == 0.0

        # the BERT branch downstream of last_hidden_state
        te = tag + "e"
        enc = reference_encoder()
        G.fill_module(enc, tag)
        Et = torch.from_numpy(embeddings(i, B, L)).requires_grad_(True)
        enc.bert = lambda input_ids, attention_mask: types.SimpleNamespace(last_hidden_state=Et)     # noqa: E731
        ide = idt.clamp(min=0)
        out[f"{te}.ids"] = ide.numpy()
        run(enc, te, ide)
        out[f"{te}.ling"] = G.tnp(enc.extract_linguistic_features(ide, mt))
        G.store_grads(out, te, enc, {})
        out[f"{te}.gradnoise.token_attention.2.bias"] = out.pop(f"{te}.grad.token_attention.2.bias")
        dE = Et.grad
        if dE.numel() <= 2 * SMALL:
            out[f"{te}.dE"] = G.tnp(dE)
        else:
            v = dE.double().reshape(-1)
            idx = torch.linspace(0, v.numel() - 1, 1024).round().long()
            out[f"{te}.dEnorm"], out[f"{te}.dEsample"] = np.float64(v.norm().item()), v[idx].numpy().astype(np.float32)
    return out, names


def main():
    out, names = capture()
    path = os.path.join(HERE, "text_seq.npz")
    np.savez_compressed(path, **out)
    with open(os.path.join(HERE, "text_state_dict_names.json"), "w") as f:
        json.dump(names[f"txt{CASES[0][0]}x{CASES[0][1]}"], f, indent=1)
        f.write("\n")
    print("text_seq.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
