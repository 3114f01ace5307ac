#!/usr/bin/env python3
"""Capture tests/golden/modality_encoder_state_dict_names.json from the IMPORTED reference (build container only).

Run from the repo root:  python tests/golden/make_golden_modality.py
encoders.ModalityEncoder (reference src/models/encoders.py:764-852) with its default config, its text encoder in the no-BERT
configuration: the names and shapes of its state_dict, and what get_encoder_output_dims returns for {} and for hidden_dim = 256.
Names and shapes only: the token table alone is 92 MB.

The reference builds a BertModel whenever `transformers` imports, and that constructor fetches weights.  This script therefore
puts None in sys.modules["transformers"] BEFORE the reference's encoders module is imported, so that the reference takes its own
ImportError branch, and asserts that it did (TRANSFORMERS_AVAILABLE is False, text_encoder.bert is None) before going on -- exactly
as make_golden_text.py does."""
import contextlib
import io
import json
import os
import sys
import types

sys.modules["transformers"] = None      # `import transformers` raises ImportError: the reference takes its no-BERT branch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as G  # noqa: E402,F401  (sets up the import paths of the reference and of mmdeer)


def capture():
    for missing in ("librosa", "cv2"):
        if missing not in sys.modules:
            m = types.ModuleType(missing)
            m.__spec__ = __import__("importlib.machinery").machinery.ModuleSpec(missing, None)
            sys.modules[missing] = m
    with contextlib.redirect_stdout(io.StringIO()):
        import encoders as ref_enc  # (reference)
        assert ref_enc.TRANSFORMERS_AVAILABLE is False
        enc = ref_enc.ModalityEncoder()
    assert enc.text_encoder.bert is None
    return {"state_dict": {k: list(v.shape) for k, v in enc.state_dict().items()},
            "output_dims": {"default": ref_enc.get_encoder_output_dims({}), "hidden_dim_256": ref_enc.get_encoder_output_dims({"hidden_dim": 256})}}


def main():
    path = os.path.join(HERE, "modality_encoder_state_dict_names.json")
    with open(path, "w") as f:
        json.dump(capture(), f, indent=1)
        f.write("\n")
    print("modality_encoder_state_dict_names.json", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
