"""``encoders.ModalityEncoder`` (reference src/models/encoders.py:764-852), ``create_encoders_from_config`` (:936-946) and
``get_encoder_output_dims`` (:949-966): the three encoders of the package behind the reference's one interface, and ``EndToEndDEER``,
the model from raw batch entries to the NIG outputs and the loss.

Host logic only: every number comes from the encoders (``temporal.TemporalAudioEncoder``, ``frames.FrameVideoEncoder``,
``text.TemporalTextEncoder``), a fusion module and ``head.MultiDimensionalDEER``, each a sequence of HIP launches on the current
stream.  The three encoders run one after the other on that stream: a training step through ``EndToEndDEER`` is one linear chain of
launches, and ``mmdeer.train_graph.capture_train_step`` replays it as one HIP graph (every module with dropout here follows the
step-counter protocol of ``stepcount.py``).  No CPU path: CPU tensors raise."""
from __future__ import annotations

from typing import Dict, Optional

import torch
from torch import nn

from .bert import BertEncoder
from .frames import FrameVideoEncoder
from .head import ComposedDEER, MultiDimensionalDEER
from .temporal import TemporalAudioEncoder
from .text import TemporalTextEncoder


class ModalityEncoder(nn.Module):
    """``encoders.ModalityEncoder``: ``audio_encoder`` (``TemporalAudioEncoder``: (B, 84) or (B, T, 84) features), ``video_encoder``
    (``FrameVideoEncoder``: (B, T, 3, H, W) or (B, 3, H, W) frames, or (B, T, 512) / (B, 512) per-frame features) and
    ``text_encoder`` (``TemporalTextEncoder``: (B, L) ids and mask; with ``bert=BertEncoder(...)`` the reference's BERT configuration,
    else its no-BERT branch), all three built from the one ``config`` as in the reference, each -> (B, ``hidden_dim``) fp32.  The
    ``state_dict`` has the reference class's names and shapes, so its checkpoints load with ``strict=True`` (with a trunk:
    ``text_encoder.bert.*`` named as ``transformers.BertModel`` names them, and no embedding tables).

    ``forward(dict) -> dict`` encodes the modalities that are present: ``audio`` -> ``audio``, ``video`` -> ``video``,
    ``text_input_ids`` and ``text_attention_mask`` (both) -> ``text``; an absent modality gives an absent key.  The optional key
    ``audio_lengths`` ((B,) valid steps of a padded ``audio`` batch) goes to ``TemporalAudioEncoder.forward(audio, lengths=...)``.

    One deviation from the reference: it catches ANY exception of an encoder, logs a warning and substitutes zeros.  Here a refusal
    (``ValueError``, ``NotImplementedError``, a CPU tensor) propagates: a batch the kernels do not take is an error, not a silent
    row of zeros to train on."""

    def __init__(self, config: Optional[Dict] = None, compute_dtype: str = "fp32", bert: Optional[BertEncoder] = None):
        super().__init__()
        config = {} if config is None else config
        self.config = config
        self.hidden_dim = config.get("hidden_dim", 512)
        self.compute_dtype = compute_dtype
        self.audio_encoder = TemporalAudioEncoder(config, compute_dtype)
        self.video_encoder = FrameVideoEncoder(config, compute_dtype)
        self.text_encoder = TemporalTextEncoder(config, compute_dtype, bert=bert)

    def encode_audio(self, audio_input: torch.Tensor, lengths=None) -> torch.Tensor:
        if lengths is None:
            return self.audio_encoder(audio_input)
        return self.audio_encoder(audio_input, lengths=lengths)

    def encode_video(self, video_input: torch.Tensor) -> torch.Tensor:
        return self.video_encoder(video_input)

    def encode_text(self, input_ids: torch.Tensor, attention_mask: torch.Tensor) -> torch.Tensor:
        return self.text_encoder(input_ids, attention_mask)

    def forward(self, multimodal_input: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        encoded: Dict[str, torch.Tensor] = {}
        if "audio" in multimodal_input and multimodal_input.get("audio_lengths") is not None:
            encoded["audio"] = self.encode_audio(multimodal_input["audio"], lengths=multimodal_input["audio_lengths"])
        elif "audio" in multimodal_input:
            encoded["audio"] = self.encode_audio(multimodal_input["audio"])
        if "video" in multimodal_input:
            encoded["video"] = self.encode_video(multimodal_input["video"])
        if "text_input_ids" in multimodal_input and "text_attention_mask" in multimodal_input:
            encoded["text"] = self.encode_text(multimodal_input["text_input_ids"], multimodal_input["text_attention_mask"])
        return encoded


def create_encoders_from_config(config: Dict, compute_dtype: str = "fp32", bert: Optional[BertEncoder] = None) -> ModalityEncoder:
    """``encoders.create_encoders_from_config``: ``ModalityEncoder(config)``."""
    return ModalityEncoder(config, compute_dtype, bert)


def get_encoder_output_dims(config: Dict) -> Dict[str, int]:
    """``encoders.get_encoder_output_dims``: ``hidden_dim`` (default 512) under 'audio', 'video', 'text' and 'unified'."""
    hidden_dim = config.get("hidden_dim", 512)
    return {"audio": hidden_dim, "video": hidden_dim, "text": hidden_dim, "unified": hidden_dim}


class EndToEndDEER(nn.Module):
    """Raw batch entries -> NIG outputs and loss: ``encoders`` (a ``ModalityEncoder``), then ``ComposedDEER(fusion, head, loss)`` on
    the three (B, 512) features, e.g. ``EndToEndDEER(ModalityEncoder(cfg, bert=BertEncoder(bert_cfg, finetune_layers=6,
    dropout=True)), HierarchicalMultimodalFusion(512, 512, 512), MultiDimensionalDEER(512))``.

    ``forward(batch)`` takes ``ModalityEncoder.forward``'s dictionary (all three modalities are required) and returns
    ``ComposedDEER``'s keys plus ``encoded_features`` (the encoders' dictionary).  ``compute_loss`` and
    ``get_predictions_and_uncertainties`` are ``ComposedDEER``'s.  It trains through autograd, e.g. under
    ``ModuleAdamW.for_module(model, ..., capturable=True)``, which finds the trunk's packed operands as it does for the text model;
    ``train_graph.capture_train_step`` then replays the whole step as one HIP graph."""

    def __init__(self, encoders: ModalityEncoder, fusion: nn.Module, head: MultiDimensionalDEER, loss: Optional[nn.Module] = None):
        super().__init__()
        self.encoders = encoders
        self.composed = ComposedDEER(fusion, head, loss)

    @property
    def fusion(self) -> nn.Module:
        return self.composed.fusion

    @property
    def head(self) -> MultiDimensionalDEER:
        return self.composed.head

    def forward(self, batch: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        encoded = self.encoders(batch)
        missing = [k for k in ("audio", "video", "text") if k not in encoded]
        if missing:
            raise ValueError(f"EndToEndDEER: the batch lacks the {', '.join(missing)} modality (keys 'audio', 'video', "
                             "'text_input_ids' + 'text_attention_mask')")
        out = self.composed(encoded["audio"], encoded["video"], encoded["text"])
        out["encoded_features"] = encoded
        return out

    def compute_loss(self, predictions: Dict[str, torch.Tensor], targets: torch.Tensor) -> Dict[str, torch.Tensor]:
        return self.composed.compute_loss(predictions, targets)

    def get_predictions_and_uncertainties(self, outputs: Dict[str, torch.Tensor]):
        return self.composed.get_predictions_and_uncertainties(outputs)
