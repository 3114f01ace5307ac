#!/usr/bin/env python3
"""Capture tests/golden/deer_head.npz + deer_head_state_dict_names.json from the IMPORTED reference (build container only).

Run from the repo root:  python tests/golden/make_golden_head.py
deer.MultiDimensionalDEER (reference src/models/deer.py:198-266) and deer.DEERLayer (:30-108) with dropout = 0, each case with
its own closed-form parameter fill (synth.module_fill, tag = case name) and synth.normal inputs.  Per case: the input, every
output, and the input / parameter gradients of sum_k sum(out_k * w_k) over ALL output keys (w_k = synth.normal, stored as
`<tag>.w.<key>`), in make_golden.store_grads' format.  One extra DEERLayer(8, 4, 16) case (`dlx`, eval outputs only) has its
last layer's weight zeroed and its biases set by tests/head_ref.extreme_state, so that its four outputs sit at evidence
-104, -25, -3 and 25: alpha - 1 underflows to 0 in the first two and the uncertainties are inf there, as recorded.

The generator asserts what the tolerances of the tests rest on: min(alpha - 1) >= 0.1 and min(nu) >= 0.1 in every ordinary case,
at least one inf and one finite entry in each uncertainty output of the extreme case.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as G  # noqa: E402  (sets up the import paths of the reference and of mmdeer)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from mmdeer import synth  # noqa: E402
from tests import head_ref  # noqa: E402

KEYS = head_ref.NIG_KEYS


def _weights(stream, out):
    return {k: synth.normal(stream + j, v.numel()).reshape(tuple(v.shape)).astype(np.float32) for j, (k, v) in enumerate(out.items())}


def _capture_case(out, names, tag, mod, B, input_dim, stream):
    names[tag] = {k: list(v.shape) for k, v in mod.state_dict().items()}
    G.fill_module(mod, tag)
    mod.train()                                        # dropout = 0: train == eval, and the graph is recorded
    x = synth.normal(stream, B * input_dim).reshape(B, input_dim).astype(np.float32)
    xa = torch.from_numpy(x).requires_grad_(True)
    o = mod(xa)
    w = _weights(stream + 1, o)
    out[f"{tag}.input"] = x
    for k, v in o.items():
        out[f"{tag}.out.{k}"], out[f"{tag}.w.{k}"] = G.tnp(v), w[k]
    sum((v * torch.from_numpy(w[k])).sum() for k, v in o.items()).backward()
    G.store_grads(out, tag, mod, {"x": xa})
    return {k: v.detach() for k, v in o.items()}


def capture():
    out, names = {}, {}
    for i, (tag, (I, D, H, B)) in enumerate(head_ref.MD_CASES.items()):
        mod = G.ref_deer.MultiDimensionalDEER(I, emotion_dims=D, hidden_dim=H, dropout=0.0)
        o = _capture_case(out, names, tag, mod, B, I, 800 + 40 * i)
        am1 = min(float((o[f"{n}_alpha"] - 1).min()) for n in mod.dimension_names)
        nu = min(float(o[f"{n}_nu"].min()) for n in mod.dimension_names)
        assert am1 >= 0.1 and nu >= 0.1, (tag, am1, nu)
        print(tag, "min(alpha - 1) = %.3f  min(nu) = %.3f" % (am1, nu))
    for i, (tag, (I, O, H, B)) in enumerate(head_ref.DL_CASES.items()):
        mod = G.ref_deer.DEERLayer(I, output_dim=O, hidden_dim=H, dropout=0.0)
        o = _capture_case(out, names, tag, mod, B, I, 1000 + 40 * i)
        am1, nu = float((o["alpha"] - 1).min()), float(o["nu"].min())
        assert am1 >= 0.1 and nu >= 0.1, (tag, am1, nu)
        print(tag, "min(alpha - 1) = %.3f  min(nu) = %.3f" % (am1, nu))
    # the extreme case
    tag, (I, O, H, B) = "dlx", head_ref.DLX_CASE
    mod = G.ref_deer.DEERLayer(I, output_dim=O, hidden_dim=H, dropout=0.0).eval()
    names[tag] = {k: list(v.shape) for k, v in mod.state_dict().items()}
    sd = head_ref.extreme_state(synth.module_fill(tag, {k: tuple(v) for k, v in names[tag].items()}))
    mod.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    x = synth.normal(1200, B * I).reshape(B, I).astype(np.float32)
    with torch.no_grad():
        o = mod(torch.from_numpy(x))
    out[f"{tag}.input"] = x
    for k, v in o.items():
        out[f"{tag}.out.{k}"] = G.tnp(v)
    for k in KEYS[4:]:
        u = out[f"{tag}.out.{k}"]
        assert np.isinf(u).any() and np.isfinite(u).any(), k
    assert (out[f"{tag}.out.alpha"][:, :2] == 1.0).all()
    return out, names


def main():
    out, names = capture()
    path = os.path.join(HERE, "deer_head.npz")
    np.savez_compressed(path, **out)
    with open(os.path.join(HERE, "deer_head_state_dict_names.json"), "w") as f:
        json.dump(names, f, indent=1)
        f.write("\n")
    print("deer_head.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
