"""ModalityEncoder on the GPU, and the END-TO-END training step replayed as ONE HIP graph (mmdeer.train_graph.capture_train_step)
against the same step run eagerly.  The model of this file is tests/test_gpu_bert_train_graph.py, whose ``everything`` /
``first_difference`` records it reuses.

The model is EndToEndDEER(ModalityEncoder(cfg, bert=BertEncoder(WIDE, finetune_layers=2, dropout=True)),
HierarchicalMultimodalFusion(512, 512, 512), MultiDimensionalDEER(512)) with MultiTaskDEERLoss, under
ModuleAdamW.for_module(capturable=True, max_grad_norm=1.0) with decay 0 on the one-dimensional parameters; WIDE is that file's trunk
(768 wide, 12 heads, 3 layers).  Inputs: B = 2, audio (2, 3, 84), frames (2, 2, 3, 16, 16), L = 5 with the second row's mask cut to 3
tokens, targets (2, 3).  fp32 and bf16 with ``train_backbone``, bf16 without.

Everything is bit for bit: a replay launches the kernels of the eager step on the same inputs, every dropout step comes from a device
counter instead of the host's (tests/test_gpu_module_drop_counters.py, tests/test_gpu_bert_drop_counter.py: the same masks), Adam's
step from the optimiser's device records, and nothing is atomic.  That presupposes an eager step that is itself run-to-run
deterministic, so the first test runs it twice from one state and asserts equal bits."""
import pytest
import torch

from mmdeer import bert, encoders, frames, head, temporal, text
from mmdeer.model import HierarchicalMultimodalFusion
from mmdeer.optim import ModuleAdamW
from mmdeer.train_graph import capture_train_step

from .test_gpu_bert_train_graph import WIDE, everything, first_difference

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B, L = 2, 5
CONFIGS = [("fp32", True), ("bf16", True), ("bf16", False)]


def make(compute, train_backbone, state=None):
    torch.manual_seed(3)
    trunk = bert.BertEncoder(WIDE, compute, finetune_layers=2, dropout=True, dropout_seed=11)
    enc = encoders.ModalityEncoder({"dropout_seed": 5, "train_backbone": train_backbone}, compute, bert=trunk)
    m = encoders.EndToEndDEER(enc, HierarchicalMultimodalFusion(512, 512, 512, compute_dtype=compute, seed=1),
                              head.MultiDimensionalDEER(512, compute_dtype=compute, seed=2)).to(DEV).train()
    if state is not None:
        m.load_state_dict(state)
    named = [(n, p) for n, p in m.named_parameters() if p.requires_grad]
    groups = [{"params": [p for n, p in named if p.ndim >= 2], "weight_decay": 0.01},
              {"params": [p for n, p in named if p.ndim < 2], "weight_decay": 0.0}]          # LayerNorm, BatchNorm and biases
    return m, ModuleAdamW.for_module(m, groups, lr=1e-3, capturable=True, max_grad_norm=1.0)


def batches(n=3):
    """(audio, frames, ids, mask, targets) x n, drawn once per call from one seed"""
    g = torch.Generator().manual_seed(77)
    out = []
    for _ in range(n):
        mask = torch.ones(B, L, dtype=torch.int64)
        mask[1, 3:] = 0
        out.append(tuple(t.to(DEV) for t in (torch.randn(B, 3, 84, generator=g), torch.randn(B, 2, 3, 16, 16, generator=g),
                                             torch.randint(1, 50, (B, L), generator=g), mask, torch.rand(B, 3, generator=g) * 2 - 1)))
    return out


def step_fn_of(m):
    def step_fn(audio, video, ids, mask, targets):
        out = m({"audio": audio, "video": video, "text_input_ids": ids, "text_attention_mask": mask})
        return m.compute_loss(out, targets)["total_loss"]
    return step_fn


def eager_step(m, opt, batch):
    for p in m.parameters():
        p.grad = None
    loss = step_fn_of(m)(*batch)
    loss.backward()
    opt.step()
    return loss.detach().clone()


def counted(m):
    return [x for x in m.modules() if hasattr(x, "set_step_counter")]


def operands_are_a_fresh_pack(compute, train_backbone, m):
    fresh, _ = make(compute, train_backbone, m.state_dict())
    want, got = fresh.encoders.text_encoder.bert._operands(), m.encoders.text_encoder.bert._operands()
    for a, b in zip(got["emb"], want["emb"]):
        assert torch.equal(a, b), "embedding operands"
    for i, (lg, lw) in enumerate(zip(got["layers"], want["layers"])):
        for k in lw:
            assert lg[k].dtype == lw[k].dtype and torch.equal(lg[k], lw[k]), f"packed operand {k} of layer {i}"


# ------------------------------------------------------------------------------------------------ ModalityEncoder
@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_modality_encoder_is_its_three_encoders_and_an_absent_modality_is_an_absent_key(compute):
    torch.manual_seed(4)
    cfg = {"dropout_seed": 5}
    m = encoders.ModalityEncoder(cfg, compute, bert=bert.BertEncoder(WIDE, compute)).to(DEV).eval()
    audio, video, ids, mask, _ = batches(1)[0]
    feats = torch.randn(B, 3, 512, generator=torch.Generator().manual_seed(5)).to(DEV)
    alone = {"audio": temporal.TemporalAudioEncoder(cfg, compute), "video": frames.FrameVideoEncoder(cfg, compute),
             "text": text.TemporalTextEncoder(cfg, compute, bert=bert.BertEncoder(WIDE, compute))}
    for k, e in alone.items():
        e.load_state_dict(getattr(m, f"{k}_encoder").state_dict())
        e.to(DEV).eval()
    with torch.no_grad():
        got = m({"audio": audio, "video": video, "text_input_ids": ids, "text_attention_mask": mask})
        assert set(got) == {"audio", "video", "text"} and all(v.shape == (B, 512) and v.dtype == torch.float32 for v in got.values())
        assert torch.equal(got["audio"], alone["audio"](audio)) and torch.equal(got["audio"], m.encode_audio(audio))
        assert torch.equal(got["video"], alone["video"](video)) and torch.equal(got["video"], m.encode_video(video))
        assert torch.equal(got["text"], alone["text"](ids, mask)) and torch.equal(got["text"], m.encode_text(ids, mask))
        assert bool(torch.isfinite(torch.cat(list(got.values()))).all()) and float(got["video"].abs().sum()) > 0
        # other forms of the same modalities; one modality; none
        got = m({"audio": audio[:, 0], "video": feats})
        assert set(got) == {"audio", "video"} and torch.equal(got["audio"], alone["audio"](audio[:, 0])) and torch.equal(got["video"], alone["video"](feats))
        assert set(m({"text_input_ids": ids, "text_attention_mask": mask})) == {"text"}
        assert m({"text_input_ids": ids}) == {} and m({}) == {}
    with pytest.raises(RuntimeError, match="GPU tensors"):
        m({"audio": audio.cpu()})
    with pytest.raises(ValueError):
        m({"video": video[:, :, :2]})                      # two channels: the refusal propagates, no row of zeros


# ------------------------------------------------------------------------------------------------ the captured step
@pytest.mark.parametrize("compute,train_backbone", CONFIGS)
def test_the_eager_step_is_run_to_run_deterministic(compute, train_backbone):
    """what the bit-for-bit comparisons below presuppose: two eager steps from one state, equal bits"""
    data = batches()
    runs = []
    for _ in range(2):
        m, opt = make(compute, train_backbone)
        losses = [eager_step(m, opt, b) for b in data[:2]]
        runs.append((losses, everything(m, opt)))
    torch.cuda.synchronize()
    for r, (a, b) in enumerate(zip(runs[0][0], runs[1][0])):
        assert torch.equal(a, b), f"loss of step {r}: {float(a)!r} against {float(b)!r}"
    diff = first_difference(runs[0][1], runs[1][1])
    assert diff is None, diff
    assert bool(torch.isfinite(torch.stack(runs[0][0])).all())


@pytest.mark.parametrize("compute,train_backbone", CONFIGS)
def test_three_replays_are_three_eager_steps(compute, train_backbone):
    eager, eopt = make(compute, train_backbone)
    start = {k: v.detach().clone() for k, v in eager.state_dict().items()}
    model, opt = make(compute, train_backbone, start)
    data = batches()
    before = everything(model, opt)
    static = [t.clone() for t in data[0]]
    replay = capture_train_step(step_fn_of(model), opt, static)
    # capturing is no training step
    after = everything(model, opt)
    assert first_difference(after, before) is None, first_difference(after, before)
    assert after["drop"] == before["drop"] and [int(t) for _, t in replay.counters] == before["drop"]
    assert [m for m, _ in replay.counters] == counted(model) and isinstance(replay.graph, torch.cuda.CUDAGraph)
    kinds = {type(m).__name__ for m, _ in replay.counters}
    assert {"TemporalAudioEncoder", "FrameVideoEncoder", "TemporalTextEncoder", "BertEncoder", "HierarchicalMultimodalFusion",
            "MultiDimensionalDEER", "DEERLayer"} <= kinds, kinds
    want = [eager_step(eager, eopt, b) for b in data]
    got = [replay(*b).clone() for b in data]
    torch.cuda.synchronize()
    for r, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), f"loss of step {r}: replay {float(a)!r}, eager {float(b)!r}"
    # parameters, buffers (the BatchNorm running statistics and num_batches_tracked among them), moments, step counts
    diff = first_difference(everything(model, opt), everything(eager, eopt))
    assert diff is None, diff
    assert opt.class_buffer[:, 2].tolist() == [3, 3]
    nbt = [k for k in model.state_dict() if k.endswith("num_batches_tracked")]
    assert len(nbt) == 6 and all(int(model.state_dict()[k]) == 3 for k in nbt)
    backbone = [p for n, p in model.named_parameters() if ".spatial_backbone." in n]
    assert all((p.grad is not None) == train_backbone for p in backbone)
    # the dropout steps: each device counter holds what the eager twin's host counter reached
    assert [int(t) for _, t in replay.counters] == [x._train_step for x in counted(eager)]
    live = {type(m).__name__: int(t) for m, t in replay.counters}
    assert all(live[k] == 3 for k in kinds - {"DEERLayer"}) and live["DEERLayer"] == 0          # the heads are run by their owner
    operands_are_a_fresh_pack(compute, train_backbone, model)
    operands_are_a_fresh_pack(compute, train_backbone, eager)


def test_replays_draw_fresh_masks_and_the_second_is_the_eager_step_1():
    eager, eopt = make("bf16", True)
    model, opt = make("bf16", True, eager.state_dict())
    batch = batches(1)[0]
    replay = capture_train_step(step_fn_of(model), opt, [t.clone() for t in batch])
    got = [replay(None, None, None, None, None).clone() for _ in range(2)]            # None keeps what the static inputs hold
    want = [eager_step(eager, eopt, batch) for _ in range(2)]
    assert not torch.equal(got[0], got[1]), "two replays on one batch gave the same loss: the masks are not fresh"
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (got, want)
    assert first_difference(everything(model, opt), everything(eager, eopt)) is None
