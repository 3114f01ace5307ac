"""The BERT fine-tuning step replayed as ONE HIP graph (mmdeer.train_graph.capture_train_step) against the same step run eagerly.

Everything is bit for bit: a replay launches the kernels of the eager step on the same inputs, the dropout step comes from a device
counter instead of the host's (tests/test_gpu_bert_drop_counter.py: the same masks), Adam's step from the optimiser's device records
(tests/test_gpu_module_adamw_capturable.py), and nothing is atomic.  From one saved start, three replays on three batches are
compared with three eager steps -- host counters, a capturable optimiser -- on those batches: the losses, every parameter, the trunk's
packed operands against a fresh encoder's pack of the final state dict, the moments, the step counts and the modules' dropout steps.

The model is TemporalTextEncoder(bert=BertEncoder(finetune_layers=2, dropout=True)) + nn.Linear(512, 3) + MSE under
ModuleAdamW.for_module(capturable=True, max_grad_norm=1.0) with decay 0 on LayerNorm and biases; B = 2 with the second row's mask cut to
3 valid tokens; L = 5 and L = 33 (across the attention kernels' 32-key block); fp32 and bf16.  TemporalTextEncoder takes a trunk of
hidden size 768 only (tests/test_cpu_bert.py pins the refusal of any other), so ITS trunk is 768 wide with 12 heads and otherwise the
tiny geometry (3 layers, intermediate 256, vocabulary 50, 40 positions); BertEncoder alone, with dropout=False, runs the tiny geometry
itself: hidden 128, 2 heads."""
import pytest
import torch
from torch import nn

from mmdeer import bert, text
from mmdeer.optim import ModuleAdamW
from mmdeer.train_graph import capture_train_step

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TINY = dict(vocab_size=50, hidden_size=128, num_hidden_layers=3, num_attention_heads=2, intermediate_size=256, max_position_embeddings=40)
WIDE = dict(TINY, hidden_size=768, num_attention_heads=12)
B = 2


class TextModel(nn.Module):
    def __init__(self, compute):
        super().__init__()
        trunk = bert.BertEncoder(WIDE, compute, finetune_layers=2, dropout=True, dropout_seed=11)
        self.enc = text.TemporalTextEncoder({"hidden_dim": 512, "dropout_seed": 5}, compute, bert=trunk)
        self.head = nn.Linear(512, 3)

    def trunk(self):
        return self.enc.bert

    def forward(self, ids, mask, target):
        return nn.functional.mse_loss(self.head(self.enc(ids, mask)), target)


class TrunkModel(nn.Module):
    """BertEncoder alone, no dropout: the optimiser half without masks"""

    def __init__(self, compute):
        super().__init__()
        self.bert = bert.BertEncoder(TINY, compute, finetune_layers=2, dropout=False)

    def trunk(self):
        return self.bert

    def forward(self, ids, mask, target):
        return nn.functional.mse_loss(self.bert(ids, mask).last_hidden_state.float(), target)


def make(kind, compute, state=None):
    torch.manual_seed(3)
    m = (TextModel if kind == "text" else TrunkModel)(compute).to(DEV).train()
    if state is not None:
        m.load_state_dict(state)
    named = [(n, p) for n, p in m.named_parameters() if p.requires_grad]
    groups = [{"params": [p for n, p in named if p.ndim >= 2], "weight_decay": 0.01},
              {"params": [p for n, p in named if p.ndim < 2], "weight_decay": 0.0}]          # LayerNorm and biases
    opt = ModuleAdamW.for_module(m, groups, lr=1e-3, capturable=True, max_grad_norm=1.0)
    return m, opt


def batches(kind, L, n=3):
    g = torch.Generator().manual_seed(40 + L)
    out = []
    for _ in range(n):
        mask = torch.ones(B, L, dtype=torch.int64)
        mask[1, 3:] = 0
        target = torch.randn(B, 3, generator=g) if kind == "text" else torch.randn(B, L, TINY["hidden_size"], generator=g)
        out.append((torch.randint(1, 50, (B, L), generator=g).to(DEV), mask.to(DEV), target.to(DEV)))
    return out


def eager_step(m, opt, batch):
    for p in m.parameters():
        p.grad = None
    loss = m(*batch)
    loss.backward()
    opt.step()
    return loss.detach().clone()


def counted(m):
    return [x for x in m.modules() if hasattr(x, "set_step_counter")]


def everything(m, opt):
    """what a training step changes, cloned: parameters, buffers, moments, step counts, dropout steps"""
    sd = opt.state_dict()["state"]
    params = [p for g in opt.param_groups for p in g["params"]]
    zero = lambda p: (torch.zeros_like(p), torch.zeros_like(p), 0.0)       # noqa: E731  (no state yet IS zero moments and no step done:
    # the capture itself leaves such entries behind, because the replays, which run no host code, update the buffers they view)
    return {"params": {n: p.detach().clone() for n, p in m.state_dict().items()},
            "moments": {k: (sd[k]["exp_avg"].clone(), sd[k]["exp_avg_sq"].clone(), float(sd[k]["step"])) if k in sd else zero(p)
                        for k, p in enumerate(params)},
            "steps": [0, 0] if opt.class_buffer is None else opt.class_buffer[:, 2].tolist(),       # no record yet: no step done
            "drop": [x._train_step for x in counted(m)]}


def first_difference(a, b):
    """the first tensor that differs between two everything() records, or None"""
    for n in a["params"]:
        if not torch.equal(a["params"][n], b["params"][n]):
            return f"parameter {n}: {int((a['params'][n] != b['params'][n]).sum())} of {a['params'][n].numel()} elements"
    if a["moments"].keys() != b["moments"].keys():
        return f"state of {sorted(a['moments'])} against {sorted(b['moments'])}"
    for k in a["moments"]:
        for j, what in enumerate(("exp_avg", "exp_avg_sq")):
            if not torch.equal(a["moments"][k][j], b["moments"][k][j]):
                return f"{what} of parameter {k}"
        if a["moments"][k][2] != b["moments"][k][2]:
            return f"step of parameter {k}: {a['moments'][k][2]} against {b['moments'][k][2]}"
    if a["steps"] != b["steps"]:
        return f"device step counts {a['steps']} against {b['steps']}"
    return None


def operands_are_a_fresh_pack(kind, compute, m):
    fresh, _ = make(kind, compute, m.state_dict())
    want, got = fresh.trunk()._operands(), m.trunk()._operands()
    for a, b in zip(got["emb"], want["emb"]):
        assert torch.equal(a, b), "embedding operands"
    for i, (lg, lw) in enumerate(zip(got["layers"], want["layers"])):
        for k in lw:
            assert lg[k].dtype == lw[k].dtype and torch.equal(lg[k], lw[k]), f"packed operand {k} of layer {i}"


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
@pytest.mark.parametrize("L", [5, 33])
@pytest.mark.parametrize("kind", ["text", "trunk"])
def test_three_replays_are_three_eager_steps(kind, L, compute):
    """(a) with the text encoder and dropout, (d) with the trunk alone and no dropout; (c) on the way: capturing is no training step"""
    eager, eopt = make(kind, compute)
    start = {k: v.detach().clone() for k, v in eager.state_dict().items()}
    model, opt = make(kind, compute, start)
    data = batches(kind, L)
    before = everything(model, opt)
    static = [t.clone() for t in data[0]]
    replay = capture_train_step(model, opt, static)
    assert first_difference(everything(model, opt), before) is None, first_difference(everything(model, opt), before)        # (c)
    assert everything(model, opt)["drop"] == before["drop"] and [int(t) for _, t in replay.counters] == before["drop"]
    assert [m for m, _ in replay.counters] == counted(model) and len(counted(model)) == (2 if kind == "text" else 1)
    assert replay.static_inputs[0] is static[0] and isinstance(replay.graph, torch.cuda.CUDAGraph)
    want = [eager_step(eager, eopt, b) for b in data]
    got = [replay(*b).clone() for b in data]
    torch.cuda.synchronize()
    for r, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), f"loss of step {r}: replay {float(a)!r}, eager {float(b)!r}"
    diff = first_difference(everything(model, opt), everything(eager, eopt))
    assert diff is None, diff
    assert opt.class_buffer[:, 2].tolist() == [3, 3]
    # the dropout steps: the device counters hold what the eager modules' host counters reached
    live = 3 if kind == "text" else 0
    assert [int(t) for _, t in replay.counters] == [x._train_step for x in counted(eager)] == [live] * len(replay.counters)
    operands_are_a_fresh_pack(kind, compute, model)
    operands_are_a_fresh_pack(kind, compute, eager)


def test_replays_draw_fresh_masks_and_the_second_is_the_eager_step_1():
    """(b)"""
    eager, eopt = make("text", "bf16")
    model, opt = make("text", "bf16", eager.state_dict())
    batch = batches("text", 33, 1)[0]
    replay = capture_train_step(model, opt, [t.clone() for t in batch])
    got = [replay(None, None, None).clone() for _ in range(2)]            # None keeps what the static inputs hold
    want = [eager_step(eager, eopt, batch) for _ in range(2)]
    assert not torch.equal(got[0], got[1]), "two replays on one batch gave the same loss: the masks are not fresh"
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (got, want)
    assert first_difference(everything(model, opt), everything(eager, eopt)) is None
    # the same batch under frozen masks and frozen parameters would repeat the loss: eval() has no dropout
    model.eval()
    with torch.no_grad():
        assert torch.equal(model(*batch), model(*batch))


def test_capturing_after_training_steps_leaves_everything_as_it_was():
    """(c) from a state with moments, step counts and advanced dropout steps"""
    model, opt = make("text", "fp32")
    data = batches("text", 5)
    eager_step(model, opt, data[0])
    eager_step(model, opt, data[1])
    before = everything(model, opt)
    assert before["steps"] == [2, 2] and before["drop"] == [2, 2]
    replay = capture_train_step(model, opt, [t.clone() for t in data[2]], warmup=3)
    after = everything(model, opt)
    assert first_difference(after, before) is None, first_difference(after, before)
    assert after["drop"] == before["drop"] and [int(t) for _, t in replay.counters] == [2, 2]
    operands_are_a_fresh_pack("text", "fp32", model)
    # ... and the replay is the third step
    twin, topt = make("text", "fp32")
    for b in data:
        want = eager_step(twin, topt, b)
    assert torch.equal(replay(*data[2]), want)
    assert first_difference(everything(model, opt), everything(twin, topt)) is None


def test_replay_refuses_another_shape_dtype_or_count():
    """(e)"""
    model, opt = make("trunk", "fp32")
    ids, mask, target = batches("trunk", 5, 1)[0]
    replay = capture_train_step(model, opt, [ids.clone(), mask.clone(), target.clone()])
    steps = opt.class_buffer[:, 2].tolist()
    for bad in ((ids[:, :4], mask, target), (ids, mask, target[:1]), (ids.int(), mask, target), (ids, mask), (ids, mask, target, target),
                (ids, mask, 3.0)):
        with pytest.raises(ValueError, match="replay"):
            replay(*bad)
    assert opt.class_buffer[:, 2].tolist() == steps          # nothing ran
    assert replay(ids, mask, target) is replay.loss
