"""The dropout step-counter protocol (mmdeer/stepcount.py) of every module with dropout outside the BERT trunk, on the GPU: from one
state, training forward number k on the HOST counter against the same forward with a DEVICE counter holding k, for k in {0, 3}.

Everything is bit for bit -- every output (the reported attention weights included) and every parameter gradient: with a counter the
launches carry (p, seed, 0, counter) instead of (p, seed, k), the GEMM / BatchNorm / LayerNorm launches read it through their
argument structs' offset_dev, and the three by-value entries run as their _dev twins (tests/test_gpu_drop_counter_ops.py).  The host
step stands still while a counter is set; after set_step_counter(None) the host path continues where it was.  The model of this
file is tests/test_gpu_bert_drop_counter.py.

Shapes: audio (2, 84) and (2, 3, 84) (the T = 1 path with side._DropoutFn's mask between the LSTM layers, and the sequence path);
video features (2, 3, 512) (the temporal CNN's BatchNorm dropout site included); the head and the fusion modules at B = 3."""
import copy

import pytest
import torch

from mmdeer import frames, fusions, generic_fusion, head, model, side, temporal, video

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(DEV)


def tri(seed, B, dims):
    return tuple(randn(seed + i, B, d) for i, d in enumerate(dims))


# name -> (constructor, the forward's positional inputs)
CASES = {
    "EnhancedAudioEncoder (2, 84)": (lambda c: side.EnhancedAudioEncoder({"dropout_seed": 3}, c), lambda: (randn(1, 2, 84),)),
    "TemporalAudioEncoder (2, 84)": (lambda c: temporal.TemporalAudioEncoder({"dropout_seed": 3}, c), lambda: (randn(1, 2, 84),)),
    "TemporalAudioEncoder (2, 3, 84)": (lambda c: temporal.TemporalAudioEncoder({"dropout_seed": 3}, c), lambda: (randn(2, 2, 3, 84),)),
    "TemporalVideoEncoder (2, 3, 512)": (lambda c: video.TemporalVideoEncoder({"dropout_seed": 4}, c), lambda: (randn(3, 2, 3, 512),)),
    "FrameVideoEncoder (2, 3, 512)": (lambda c: frames.FrameVideoEncoder({"dropout_seed": 4}, c), lambda: (randn(3, 2, 3, 512),)),
    "DEERLayer": (lambda c: head.DEERLayer(64, 2, 64, compute_dtype=c, seed=5), lambda: (randn(4, 3, 64),)),
    "MultiDimensionalDEER": (lambda c: head.MultiDimensionalDEER(64, hidden_dim=64, compute_dtype=c, seed=6), lambda: (randn(5, 3, 64),)),
    "GenericHierarchicalFusion": (lambda c: generic_fusion.GenericHierarchicalFusion(40, 128, 300, compute_dtype=c, seed=7),
                                  lambda: tri(10, 3, (40, 128, 300))),
    "HierarchicalMultimodalFusion (operator path)": (lambda c: model.HierarchicalMultimodalFusion(40, 128, 300, compute_dtype=c, seed=7),
                                                     lambda: tri(10, 3, (40, 128, 300))),
    "AdaptiveFusionGating": (lambda c: fusions.AdaptiveFusionGating([16, 32], ["attention", "bilinear"], hidden_dim=64, compute_dtype=c, dropout_seed=8),
                             lambda: tri(20, 3, (16, 32))),
    "ConcatFusion": (lambda c: fusions.ConcatFusion(48, 256, compute_dtype=c, dropout_seed=9), lambda: (randn(30, 3, 48),)),
}


def leaves(out, prefix=""):
    """the tensors of an output (a tensor, or a dictionary of tensors, dictionaries and None), by name"""
    if torch.is_tensor(out):
        return {prefix or "out": out}
    found = {}
    for k, v in (out or {}).items():
        found.update(leaves(v, f"{prefix}{k}.") if isinstance(v, dict) else ({f"{prefix}{k}": v} if torch.is_tensor(v) else {}))
    return found


def set_host_step(m, k):
    """the module's host step (and, for the wrapper, the step of the fusion it runs)"""
    (m._generic if isinstance(m, model.HierarchicalMultimodalFusion) else m)._train_step = k


def run(m, inputs):
    """one training forward and backward -> (outputs, parameter gradients), cloned"""
    for p in m.parameters():
        p.grad = None
    out = leaves(m(*inputs))
    loss = sum((v * torch.linspace(-1.0, 1.0, v.numel(), device=DEV).view(v.shape)).sum() for v in out.values() if v.requires_grad)
    loss.backward()
    torch.cuda.synchronize()
    return {k: v.detach().clone() for k, v in out.items()}, {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}


def same(got, want, what):
    assert set(got[0]) == set(want[0]) and set(got[1]) == set(want[1]), what
    for kind, g, w in (("output", got[0], want[0]), ("gradient of", got[1], want[1])):
        for k in w:
            assert torch.equal(g[k], w[k]), f"{what}: {kind} {k} differs in {int((g[k] != w[k]).sum())} of {g[k].numel()} elements"


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_a_device_counter_holding_k_is_host_step_k(name, compute):
    make, make_inputs = CASES[name]
    torch.manual_seed(2)
    host = make(compute).to(DEV).train()
    inputs = make_inputs()
    want = {}
    for k in (0, 2, 3):
        set_host_step(host, k)
        want[k] = run(host, inputs)
        assert host._train_step == k + 1
    assert any(not torch.equal(want[0][0][n], want[3][0][n]) for n in want[0][0]), "the step does not reach the masks"
    assert want[0][1], "no parameter received a gradient"
    for k in (0, 3):
        dev = copy.deepcopy(host)
        for p in dev.parameters():
            p.grad = None
        set_host_step(dev, 2)
        counter = torch.tensor([k], dtype=torch.int64, device=DEV)
        dev.set_step_counter(counter)
        same(run(dev, inputs), want[k], f"{name}, {compute}: device counter {k}")
        assert int(counter) == k, "a launch wrote the counter"
        assert dev._train_step == 2, "the host step moved under a device counter"
        assert dev.take_step_count() == 1 and dev.take_step_count() == 0
        # the second live forward since the count was taken is forward 0 again: k + *counter with k restarted
        same(run(dev, inputs), want[k], f"{name}, {compute}: device counter {k}, after take_step_count")
        counter.fill_(1)
        counter.add_(1)                                     # what the owner of a graph does between replays
        dev.take_step_count()
        same(run(dev, inputs), want[2], f"{name}, {compute}: the counter advanced to 2")
        dev.set_step_counter(None)
        assert dev._train_step == 2
        same(run(dev, inputs), want[2], f"{name}, {compute}: back on the host counter, where it was")
        assert dev._train_step == 3


def test_eval_draws_nothing_with_a_counter_set():
    m = head.MultiDimensionalDEER(64, hidden_dim=64, seed=6).to(DEV).eval()
    x = randn(5, 3, 64)
    with torch.no_grad():
        want = m(x)["mu_all"].clone()
        m.set_step_counter(torch.tensor([5], dtype=torch.int64, device=DEV))
        assert torch.equal(m(x)["mu_all"], want) and m.take_step_count() == 0 and m._train_step == 0
