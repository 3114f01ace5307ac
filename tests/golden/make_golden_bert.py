"""Golden vectors of the BERT trunk: ``transformers.BertModel`` built FROM A CONFIG (never from a pretrained name: that reaches for
the network), run on the CPU in float64 at a geometry small enough to commit.

    python tests/golden/make_golden_bert.py      # writes tests/golden/bert_tiny.npz and tests/golden/bert_state_dict_names.json

Geometry: hidden 128 / 2 heads / intermediate 256 / 2 layers / vocab 64 / 48 positions / 2 token types.  With transformers' own
std-0.02 initialisation every softmax is nearly flat and every LayerNorm trivial, which would prove little; so the weights are
drawn wider (query / key so that the scores have a spread of a few units, gamma in [0.5, 1.5], beta and the biases away from zero)
and rounded to multiples of 1 / 32 below 8 in magnitude: at most 8 significant bits, so every value is exact in bf16 (the bf16
path then reads the same model), and the file compresses.  They are stored as the uint16 bit patterns of their bf16 form; the
pooler's two tensors are left out (the trunk never reads them; the names file has them).
Inputs: B = 4, L = 37, one mask per sample -- all valid, a masked tail, one valid token, holes at every third position --
and token type ids that switch inside the sequence.  Stored: the embedding output and every layer's output (float64), so that a
failure names its layer."""
import json
import os

os.environ["HF_HUB_OFFLINE"] = "1"
os.environ["TRANSFORMERS_OFFLINE"] = "1"

import numpy as np  # noqa: E402
import torch  # noqa: E402
from transformers import BertConfig, BertModel  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
GEOMETRY = dict(vocab_size=64, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, max_position_embeddings=48,
                type_vocab_size=2, layer_norm_eps=1e-12, hidden_act="gelu")
B, L = 4, 37


STEP = 32


def grid(t):
    """to multiples of 1 / 32, |.| <= 255 / 32: exact in bf16"""
    return (t * STEP).round().clamp(-255, 255) / STEP


def draw(name, shape, gen):
    n = torch.randn(shape, generator=gen, dtype=torch.float64)
    u = torch.rand(shape, generator=gen, dtype=torch.float64)
    if "LayerNorm.weight" in name:
        return grid(0.5 + u)
    if "LayerNorm.bias" in name:
        return grid(0.6 * u - 0.3)
    if name.endswith(".bias"):
        return grid(0.1 * n)
    if "embeddings" in name:
        return grid(0.5 * n)
    if ".query." in name or ".key." in name:
        return grid(0.2 * n)                      # scores with a spread of a few units over hidden 128
    return grid(n / shape[1] ** 0.5)              # value, dense, intermediate, output, pooler: unit gain


def bf16_bits(t):
    b = t.to(torch.float32).to(torch.bfloat16)
    assert torch.equal(b.to(torch.float64), t), "not exact in bf16"
    return b.view(torch.int16).numpy().view(np.uint16)


def inputs():
    gen = torch.Generator().manual_seed(20)
    ids = torch.randint(0, GEOMETRY["vocab_size"], (B, L), generator=gen)
    ids[0, 0], ids[1, 1] = 0, GEOMETRY["vocab_size"] - 1
    mask = torch.ones(B, L, dtype=torch.int64)
    mask[1, 23:] = 0                              # a masked tail
    mask[2] = 0
    mask[2, 5] = 1                                # one valid token
    mask[3, 2::3] = 0                             # holes at every third position
    types = torch.zeros(B, L, dtype=torch.int64)
    types[:, 19:] = 1
    types[3] = 0
    return ids, mask, types


def main():
    cfg = BertConfig(**GEOMETRY, attn_implementation="eager")
    model = BertModel(cfg).double().eval()
    gen = torch.Generator().manual_seed(19)
    sd = {name: draw(name, tuple(v.shape), gen) for name, v in model.state_dict().items()}
    model.load_state_dict(sd, strict=True)
    ids, mask, types = inputs()
    with torch.no_grad():
        out = model(input_ids=ids, attention_mask=mask, token_type_ids=types, output_hidden_states=True)
    assert len(out.hidden_states) == GEOMETRY["num_hidden_layers"] + 1 and torch.equal(out.hidden_states[-1], out.last_hidden_state)
    arrays = {"w." + name: bf16_bits(v) for name, v in sd.items() if not name.startswith("pooler.")}
    arrays.update(ids=ids.numpy().astype(np.int16), mask=mask.numpy().astype(np.uint8), types=types.numpy().astype(np.uint8))
    for i, h in enumerate(out.hidden_states):
        arrays[f"hidden.{i}"] = h.numpy()
    np.savez_compressed(os.path.join(HERE, "bert_tiny.npz"), **arrays)
    with open(os.path.join(HERE, "bert_state_dict_names.json"), "w") as f:
        json.dump(list(model.state_dict().keys()), f, indent=0)
        f.write("\n")
    print(os.path.getsize(os.path.join(HERE, "bert_tiny.npz")), "bytes;", "last hidden state rms", float(out.last_hidden_state.pow(2).mean().sqrt()))


if __name__ == "__main__":
    main()
