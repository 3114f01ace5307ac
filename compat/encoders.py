"""`from encoders import AudioEncoder, VideoEncoder, TextEncoder` (run_multimodal_deer.py:77).  The raw-signal front ends
(librosa / cv2 / BERT) are out of scope; the pre-extracted-feature branch of EnhancedAudioEncoder (row a14) is real,
and EnhancedTextEncoder is the reference's no-BERT configuration on token ids and a mask (mmdeer.text; its
``forward_embeddings`` takes the caller's own contextual embeddings in place of BERT's last_hidden_state), or, constructed
with ``bert=BertEncoder(config)``, its BERT configuration: the trunk on HIP, frozen, or with ``finetune_layers=k`` its last k
layers trained as the reference trains layers 6-11 (mmdeer.bert; parameters named as transformers.BertModel's, so a checkpoint
of the reference's ``self.bert`` loads; ``dropout=True`` runs the reference's hidden and attention dropout inside the trunk in train(), off by default; tokenisation and pretrained weights stay outside).  EnhancedVideoEncoder is
the reference's encoder downstream of its spatial CNN, on (B, T, 512) per-frame features (mmdeer.video; frame tensors raise);
FrameVideoEncoder is the same encoder from frames, its Conv2d backbone run on HIP, forward only (mmdeer.frames).  ModalityEncoder,
create_encoders_from_config and get_encoder_output_dims are the reference's unified interface over the three (mmdeer.encoders: a
refusal of an encoder propagates where the reference substitutes zeros)."""
from mmdeer.side import EnhancedAudioEncoder  # noqa: F401
from mmdeer.bert import BertEncoder  # noqa: F401
from mmdeer.text import TemporalTextEncoder as EnhancedTextEncoder  # noqa: F401
from mmdeer.video import TemporalVideoEncoder as EnhancedVideoEncoder  # noqa: F401
from mmdeer.frames import FrameVideoEncoder  # noqa: F401
from mmdeer.encoders import ModalityEncoder, create_encoders_from_config, get_encoder_output_dims  # noqa: F401


def _out_of_scope(name):
    class _Stub:
        def __init__(self, *a, **k):
            raise NotImplementedError(f"encoders.{name}: raw-signal feature extraction is outside the mmdeer hot path (SURVEY.md 2); "
                                      "feed pre-extracted (B, 84) / (B, 256) / (B, 768) feature blocks")
    _Stub.__name__ = _Stub.__qualname__ = name
    return _Stub


AudioEncoder, VideoEncoder, TextEncoder = (_out_of_scope(n) for n in ("AudioEncoder", "VideoEncoder", "TextEncoder"))
