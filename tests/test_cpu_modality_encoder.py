"""ModalityEncoder, its two companions, EndToEndDEER and the dropout step-counter protocol without a GPU: the state_dict against the
reference's names and shapes (tests/golden/modality_encoder_state_dict_names.json, written by tests/golden/make_golden_modality.py from
the imported reference class in its no-BERT branch), the BERT configuration's names, get_encoder_output_dims, the compat names, the
refusal of CPU tensors, the protocol's methods on every module with dropout, and the three device-counter entries of
include/mmdeer_drop_dev.h through the strict parser with their host-side refusals."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest
import torch

from mmdeer import _header, _lib, bert, build, encoders, frames, fusions, generic_fusion, head, model, side, stepcount, temporal, video

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "modality_encoder_state_dict_names.json")
BERT_NAMES = os.path.join(HERE, "golden", "bert_state_dict_names.json")
WIDE = dict(vocab_size=64, hidden_size=768, num_hidden_layers=2, num_attention_heads=12, intermediate_size=256, max_position_embeddings=48,
            type_vocab_size=2)


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


# ------------------------------------------------------------------------------------------------ ModalityEncoder
def test_state_dict_has_the_reference_names_and_shapes():
    m = encoders.ModalityEncoder()
    want = golden()["state_dict"]
    got = {k: list(v.shape) for k, v in m.state_dict().items()}
    assert list(got) == list(want), sorted(set(got) ^ set(want))
    assert got == want
    assert isinstance(m.audio_encoder, temporal.TemporalAudioEncoder) and isinstance(m.video_encoder, frames.FrameVideoEncoder)
    assert m.text_encoder.bert is None and m.hidden_dim == 512
    # a checkpoint of those names and shapes loads strictly
    m.load_state_dict({k: torch.zeros(s) for k, s in want.items()}, strict=True)


def test_one_config_builds_all_three():
    cfg = {"dropout": 0.25, "dropout_seed": 9, "train_backbone": True, "max_text_length": 64}
    m = encoders.ModalityEncoder(cfg, "bf16")
    assert m.config is cfg
    assert (m.audio_encoder.dropout, m.video_encoder.dropout, m.text_encoder.dropout) == (0.25, 0.25, 0.25)
    assert (m.audio_encoder.dropout_seed, m.video_encoder.dropout_seed, m.text_encoder.dropout_seed) == (9, 9, 9)
    assert m.video_encoder.train_backbone and m.text_encoder.max_length == 64
    assert {m.audio_encoder.compute_dtype, m.video_encoder.compute_dtype, m.text_encoder.compute_dtype} == {"bf16"}
    assert isinstance(encoders.create_encoders_from_config(cfg), encoders.ModalityEncoder)


def test_with_a_trunk_the_names_are_the_reference_bert_names_and_the_tables_are_absent():
    with open(BERT_NAMES) as f:
        names = json.load(f)
    m = encoders.ModalityEncoder(bert=bert.BertEncoder(WIDE))
    sd = list(m.state_dict())
    assert [k for k in sd if k.startswith("text_encoder.bert.")] == ["text_encoder.bert." + n for n in names]
    assert "text_encoder.embedding.weight" not in sd and "text_encoder.positional_encoding.weight" not in sd
    rest = [k for k in golden()["state_dict"] if k not in ("text_encoder.embedding.weight", "text_encoder.positional_encoding.weight")]
    assert [k for k in sd if not k.startswith("text_encoder.bert.")] == rest
    with pytest.raises(TypeError):
        encoders.ModalityEncoder(bert=torch.nn.Linear(4, 4))


def test_get_encoder_output_dims_is_the_reference():
    want = golden()["output_dims"]
    assert encoders.get_encoder_output_dims({}) == want["default"]
    assert encoders.get_encoder_output_dims({"hidden_dim": 256}) == want["hidden_dim_256"]


def test_compat_names_resolve():
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import encoders as E, mmdeer.encoders as M\n"
            "assert E.ModalityEncoder is M.ModalityEncoder and E.create_encoders_from_config is M.create_encoders_from_config\n"
            "assert E.get_encoder_output_dims is M.get_encoder_output_dims\n"
            "import mmdeer.side, mmdeer.text, mmdeer.video, mmdeer.frames, mmdeer.bert\n"
            "assert E.EnhancedAudioEncoder is mmdeer.side.EnhancedAudioEncoder and E.EnhancedTextEncoder is mmdeer.text.TemporalTextEncoder\n"
            "assert E.EnhancedVideoEncoder is mmdeer.video.TemporalVideoEncoder and E.FrameVideoEncoder is mmdeer.frames.FrameVideoEncoder\n"
            "assert E.BertEncoder is mmdeer.bert.BertEncoder\n" % (ROOT, os.path.join(ROOT, "compat")))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_cpu_tensors_are_refused_and_an_absent_modality_is_an_absent_key():
    m = encoders.ModalityEncoder()
    ids = torch.ones(2, 4, dtype=torch.int64)
    for batch in ({"audio": torch.zeros(2, 84)}, {"video": torch.zeros(2, 3, 512)}, {"video": torch.zeros(2, 1, 3, 8, 8)},
                  {"text_input_ids": ids, "text_attention_mask": ids}):
        with pytest.raises(RuntimeError, match="GPU tensors"):          # the reference would log a warning and return zeros
            m(batch)
    assert m({}) == {} and m({"text_input_ids": ids}) == {}            # ids without a mask: no text, as in the reference
    with pytest.raises(NotImplementedError):
        m({"audio": torch.zeros(2, 16000)})                             # a raw waveform: the refusal propagates too
    e2e = encoders.EndToEndDEER(m, model.HierarchicalMultimodalFusion(512, 512, 512), head.MultiDimensionalDEER(512))
    assert e2e.fusion is e2e.composed.fusion and e2e.head is e2e.composed.head
    with pytest.raises(ValueError, match="lacks the audio, video, text"):
        e2e({})


# ------------------------------------------------------------------------------------------------ the step-counter protocol
def protocol_modules():
    return {
        "EnhancedAudioEncoder": side.EnhancedAudioEncoder(),
        "TemporalAudioEncoder": temporal.TemporalAudioEncoder(),
        "TemporalVideoEncoder": video.TemporalVideoEncoder(),
        "FrameVideoEncoder": frames.FrameVideoEncoder(),
        "DEERLayer": head.DEERLayer(16),
        "MultiDimensionalDEER": head.MultiDimensionalDEER(16, hidden_dim=32),
        "GenericHierarchicalFusion": generic_fusion.GenericHierarchicalFusion(16, 16, 16),
        "HierarchicalMultimodalFusion": model.HierarchicalMultimodalFusion(16, 16, 16),
        "AdaptiveFusionGating": fusions.AdaptiveFusionGating([8, 8], ["attention"], hidden_dim=16),
        "ConcatFusion": fusions.ConcatFusion(16, 256),
    }


@pytest.mark.parametrize("name", sorted(protocol_modules()))
def test_protocol_methods_exist_and_refuse_a_wrong_counter(name):
    m = protocol_modules()[name]
    assert m._train_step == 0 and m.take_step_count() == 0
    for bad in (torch.zeros(1, dtype=torch.int32), torch.zeros(1), torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=torch.int64, device="meta"),
                3, [0]):
        with pytest.raises(ValueError, match="one-element int64 tensor"):
            m.set_step_counter(bad)
    m.set_step_counter(None)
    t = torch.zeros(1, dtype=torch.int64)
    m.set_step_counter(t)                                  # right dtype, shape and device (the module is on the CPU here)
    m.set_step_counter(None)
    assert m._train_step == 0 and m.take_step_count() == 0


def test_the_tuple_with_and_without_a_counter():
    m = head.MultiDimensionalDEER(16, hidden_dim=32, seed=4).train()
    assert isinstance(m, stepcount.DropOwner)
    assert m._drop.next(m, 0.3) == (0.3, 4, 0) and m._drop.next(m, 0.3) == (0.3, 4, 1) and m._train_step == m._drop.step == 2
    t = torch.full((1,), 7, dtype=torch.int64)
    m.set_step_counter(t)
    d0, d1 = m._drop.next(m, 0.3), m._drop.next(m, 0.3)
    assert d0[:3] == (0.3, 4, 0) and d0[3] is t and d1[:3] == (0.3, 4, 1) and m._train_step == 2      # the host step stands still
    assert m.take_step_count() == 2 and m.take_step_count() == 0
    m.set_step_counter(None)
    assert m._drop.next(m, 0.3) == (0.3, 4, 2)             # ... and continues where it was
    assert m.eval()._drop.next(m, 0.3) is None and m._train_step == 3
    m._train_step = 9
    assert m._drop.step == 9
    a = temporal.TemporalAudioEncoder({"dropout_seed": 6})
    assert a._drop_step(0.3, a.dropout_seed) == (0.3, 6, 0) and a._train_step == 1
    # the default geometry of the hierarchical fusion runs MultimodalDEER's fused pass: a device counter is refused there
    f = model.HierarchicalMultimodalFusion(84, 256, 768)
    f.set_step_counter(None)
    with pytest.raises(NotImplementedError):
        f.set_step_counter(t)


# ------------------------------------------------------------------------------------------------ the C ABI additions
DEV_SYMBOLS = {"mmdeer_dropout_mask_dev": "mmdeer_dropout_mask", "mmdeer_trimodal_attn_fwd_dev": "mmdeer_trimodal_attn_fwd",
               "mmdeer_trimodal_attn_bwd_dev": "mmdeer_trimodal_attn_bwd"}
A = 1 << 20     # a plausible, aligned address: never dereferenced by the host checks


def test_the_three_entries_are_declared_bound_and_exported():
    lib = _lib.load()
    plain = {n: args for n, _, args in _lib.SYMBOLS}
    got = {n: (res, args) for n, res, args in _lib.DROP_DEV_SYMBOLS}
    assert set(got) == set(DEV_SYMBOLS) and _lib.DROP_DEV_CONSTANTS == {} and _lib._DROP_DEV_CLASSES == {}
    for name, (res, args) in got.items():
        assert res is C.c_int32 and args == plain[DEV_SYMBOLS[name]] + [C.c_void_p], name      # the plain entry's arguments + offset_dev
        fn = getattr(lib, name)
        assert fn.restype is res and fn.argtypes == args
    assert _header.DROP_DEV_HEADER_PATH == build.DROP_DEV_HEADER_PATH
    assert os.path.samefile(build.DROP_DEV_HEADER_PATH, os.path.join(ROOT, "include", "mmdeer_drop_dev.h"))
    src = _header.read(_header.DROP_DEV_HEADER_PATH)
    for bad in (src.replace("int mmdeer_dropout_mask_dev(", "int mmdeer_dropout_mask_dev(uint16_t f, "),
                src.replace("#include <stdint.h>", "#include <stdint.h>\n#if 0\n#endif")):
        assert bad != src
        with pytest.raises(_header.HeaderError):
            _header.parse(bad, {}, {})


def refused(rc, match):
    assert rc == -1
    msg = _lib.load().mmdeer_last_error().decode()
    assert match in msg, msg


def test_a_misaligned_counter_is_refused_on_the_host_and_the_plain_refusals_stand():
    lib = _lib.load()
    for off in (1, 2, 4, 7):
        refused(lib.mmdeer_dropout_mask_dev(1, 8, 8, 0.3, 0, 0, A, None, A + off), "dropout_mask: offset_dev must be 8-byte aligned")
        refused(lib.mmdeer_trimodal_attn_fwd_dev(A, A, A, None, None, 4, 1, 1, 0.3, 0, 0, None, A + off), "trimodal_attn_fwd: offset_dev must be 8-byte aligned")
        refused(lib.mmdeer_trimodal_attn_bwd_dev(A, A, A, A, 4, 1, 1, 0.3, 0, 0, None, A + off), "trimodal_attn_bwd: offset_dev must be 8-byte aligned")
    # whatever p and training are
    refused(lib.mmdeer_dropout_mask_dev(1, 8, 8, 0.0, 0, 0, A, None, A + 4), "offset_dev must be 8-byte aligned")
    refused(lib.mmdeer_trimodal_attn_fwd_dev(A, A, A, None, None, 4, 1, 0, 0.0, 0, 0, None, A + 4), "offset_dev must be 8-byte aligned")
    # the plain entries' refusals, with their text, with and without a counter
    for ctr in (None, A):
        refused(lib.mmdeer_dropout_mask_dev(1, -1, 8, 0.3, 0, 0, A, None, ctr), "dropout_mask: rows and cols must be >= 0")
        refused(lib.mmdeer_dropout_mask_dev(1, 8, 8, 0.3, 0, 0, None, None, ctr), "dropout_mask: out is NULL")
        refused(lib.mmdeer_trimodal_attn_fwd_dev(A, A, A, None, None, -1, 1, 0, 0.0, 0, 0, None, ctr), "trimodal_attn_fwd: batch must be >= 0")
        refused(lib.mmdeer_trimodal_attn_fwd_dev(None, A, A, None, None, 4, 1, 0, 0.0, 0, 0, None, ctr), "trimodal_attn_fwd: NULL")
        refused(lib.mmdeer_trimodal_attn_bwd_dev(A, A, A, None, 4, 0, 1, 0.3, 0, 0, None, ctr), "trimodal_attn_bwd: NULL")
        # nothing to do: no launch, no error
        assert lib.mmdeer_dropout_mask_dev(1, 0, 8, 0.3, 0, 0, A, None, ctr) == 0
        assert lib.mmdeer_trimodal_attn_fwd_dev(None, None, None, None, None, 0, 1, 1, 0.3, 0, 0, None, ctr) == 0
        assert lib.mmdeer_trimodal_attn_bwd_dev(None, None, None, None, 0, 0, 1, 0.3, 0, 0, None, ctr) == 0
