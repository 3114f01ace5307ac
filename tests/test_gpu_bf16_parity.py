"""Tight parity of the bf16 path: the HIP step against the oracle with bf16 rounding emulated
at exactly the kernels' storage points (oracle.train_step(emulate_bf16=True)).  The first test IS the benchmark
configuration: B = 4096, bf16 feature blocks, dropout 0.3 with the masks exported from the kernels' counter hash, fused
projection + attention plan (the default).

What bounds the tolerance.  A chain of ~12 layers that round every stored activation AND activation-gradient to 8
significant bits is chaotic at the rounding level: one element that rounds the other way (because an fp32 sum was taken in
another order) moves every output of the next layer by a fraction of a bf16 ulp and flips a few per cent of THOSE.  The
oracle shows it on its own: perturb its fp32 biases by 1e-7 (the size of an fp32 summation-order difference) and its
gradients move by 1-6 % (relative l2; 4 % of the stored `fused` elements differ), its outputs by up to 9e-3, its loss by
3e-6 relative.  The tests therefore run the oracle TWICE (as is, and with that perturbation) and require the HIP step to sit
no farther from the oracle than `SLACK` times the oracle's distance from itself, tensor by tensor, and 1.75 times in the
root mean square over the tensors -- measured at B = 4096: HIP-vs-oracle within 1.05 of the oracle's self-distance on every
gradient tensor (each test prints its figures), cosine >= 0.9989, loss relative 3.6e-6.  For comparison the same HIP step against the UN-rounded fp32 oracle sits at cosine 0.979 / relative l2 20 %
(tests/test_gpu_model.py::test_bf16_forward_and_step_track_the_fp32_cpu_path keeps that looser, independent statement).
Layer by layer, with every kernel fed its own stored inputs, the comparison is exact to one bf16 ulp:
tests/test_gpu_bf16_layers.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mmdeer import synth  # noqa: E402
from mmdeer.model import ModelConfig, MultimodalDEER  # noqa: E402
from mmdeer.spec import DIM_NAMES, param_table  # noqa: E402
from oracle import deer_oracle as O  # noqa: E402

from .test_gpu_model import dump_masks  # noqa: E402

DEV = "cuda:0"
EDGES = np.array(O.ECE_EDGES_10, dtype=np.float32)


def batch(B, seed, zero=()):
    b = synth.make_batch(B, seed=seed)
    for z in zero:
        b[z] = np.zeros_like(b[z])
    return {k: torch.from_numpy(v) for k, v in b.items()}


def run_pair(B, dropout, seed, zero=(), init="reference", step=None):
    """One HIP train step (bf16 compute, bf16 feature blocks) and the bf16-emulating oracle step on the same inputs,
    parameters and dropout masks.  `step(model, audio, video, text, targets)` performs the HIP step (default: train_step)."""
    b = batch(B, seed=seed, zero=zero)
    m = MultimodalDEER(ModelConfig(compute_dtype="bf16", dropout=dropout, seed=seed + 1), init=init).to(DEV).train()
    a, v, t = (b[k].to(DEV).bfloat16() for k in ("audio", "video", "text"))
    y = b["targets"].to(DEV)
    ld = m.train_step(a, v, t, y) if step is None else step(m, a, v, t, y)
    masks = dump_masks(m, B, m._step) if dropout > 0 else None
    P = O.to_params({k: w.detach().cpu() for k, w in m.state_dict().items()}, torch.float32, requires_grad=True)
    args = (a.float().cpu(), v.float().cpu(), t.float().cpu(), b["targets"])
    fo, ho, ldo, grads = O.train_step(P, *args, masks=masks, p=dropout, emulate_bf16=True)
    grads = {k: g.clone() for k, g in grads.items()}
    # the oracle's distance from itself under an fp32-rounding-sized perturbation (module docstring)
    rng = np.random.default_rng(seed)
    P2 = {k: (w.detach() + torch.from_numpy(1e-7 * rng.standard_normal(tuple(w.shape)).astype(np.float32))).requires_grad_(True)
          if k.endswith(".bias") else w.detach().clone().requires_grad_(True) for k, w in P.items()}
    _, ho2, ldo2, grads2 = O.train_step(P2, *args, masks=masks, p=dropout, emulate_bf16=True)
    return m, ld, ho, ldo, grads, (ho2, ldo2, grads2)


SLACK = 2.0       # HIP-vs-oracle may be this many times the oracle's self-distance (measured: 0.8-0.9)


def check_pair(m, ld, ho, ldo, grads, self_run, B, tag, loss_rel=1e-4, cos_min=0.998):
    ho2, ldo2, grads2 = self_run
    nig = ld["_outputs"]["_nig"].cpu()
    cat = lambda h, k: torch.cat([h[f"{d}_{k}"] for d in DIM_NAMES], dim=1).detach()
    ref = {k: cat(ho, k) for k in ("mu", "nu", "alpha", "beta")}
    worst_out = 0.0
    for i, k in enumerate(("mu", "nu", "alpha", "beta")):
        d_gpu, d_self = (nig[i] - ref[k]).abs(), (cat(ho2, k) - ref[k]).abs()
        worst_out = max(worst_out, d_gpu.max().item())
        assert d_gpu.mean().item() <= SLACK * d_self.mean().item() + 1e-5, (tag, k, d_gpu.mean().item(), d_self.mean().item())
        assert d_gpu.max().item() <= 3.0 * d_self.max().item() + 1e-3, (tag, k, d_gpu.max().item(), d_self.max().item())
        assert d_gpu.max().item() <= 3e-2, (tag, k)
    lg, lo = float(ld["total_loss"]), float(ldo["total_loss"])
    assert abs(lg - lo) <= loss_rel * max(abs(lo), 1e-3), (tag, lg, lo)
    named = dict(m.named_parameters())
    rels, selfs, min_cos = {}, {}, 1.0
    for name, shape, _ in param_table():
        ref_g = grads[name].double()
        got = named[name].grad
        if float(ref_g.abs().max()) == 0.0:                     # dead slices / zeroed modalities: exact zeros on both sides
            assert got is None or float(got.abs().max()) == 0.0, (tag, name)
            continue
        got = got.cpu().double()
        rels[name] = float((got - ref_g).norm() / ref_g.norm())
        selfs[name] = float((grads2[name].double() - ref_g).norm() / ref_g.norm())
        if ref_g.numel() >= 64:
            cos = float((got.flatten() @ ref_g.flatten()) / (got.norm() * ref_g.norm() + 1e-300))
            min_cos = min(min_cos, cos)
            assert cos >= cos_min, (tag, name, cos)
    # which element rounds the other way is chance: a single tensor's self-distance fluctuates (small batches most), so the
    # per-tensor bound also admits the root-mean-square self-distance over all tensors, and the aggregate is held tighter
    rms = lambda d: float(np.sqrt(np.mean(np.square(list(d.values())))))
    rms_gpu, rms_self = rms(rels), rms(selfs)
    assert rms_gpu <= 1.75 * rms_self + 1e-3, (tag, rms_gpu, rms_self)
    for name, rel in rels.items():
        assert rel <= SLACK * max(selfs[name], rms_self) + 2e-3, (tag, name, rel, selfs[name], rms_self)
        assert rel <= 0.15, (tag, name, rel)
    worst_name = max(rels, key=rels.get)
    worst = rels[worst_name]
    # ECE bin populations (integer work).  (1) The kernel's counts are EXACTLY the (lo, hi] masks (losses.py:215) of its own
    # fp32 confidences -- recomputed here from the alpha / beta it returned; only a sample whose confidence lies within one
    # fp32 ulp of an edge may sit on the other side (division vs reciprocal).  (2) Against the oracle: a sample whose oracle
    # confidence is farther from every edge than the largest confidence difference between the two sits in the same bin;
    # in aggregate far_k <= count_k <= far_k + near_k for every (dimension, bin).
    counts = ld["ece_bin_counts"].cpu().numpy().reshape(3, 10)
    assert counts.sum() == 3 * B
    one, eps = np.float32(1), np.float32(1e-8)
    for d in range(3):
        al_o, be_o = ref["alpha"][:, d].numpy(), ref["beta"][:, d].numpy()
        al_g, be_g = nig[2][:, d].numpy(), nig[3][:, d].numpy()
        conf_o = (one / (one + be_o / (al_o - one + eps))).astype(np.float32)
        conf_g = (one / (one + be_g / (al_g - one + eps))).astype(np.float32)
        margin = float(np.abs(conf_o - conf_g).max()) + 1e-6
        assert margin < 1e-2, (tag, d, margin)
        dist = np.abs(conf_o[:, None] - EDGES[None, :]).min(axis=1)
        for k in range(10):
            own = int(((conf_g > EDGES[k]) & (conf_g <= EDGES[k + 1])).sum())
            tie = int((np.abs(conf_g[:, None] - EDGES[None, k:k + 2]).min(axis=1) < 2e-7).sum())
            assert abs(int(counts[d, k]) - own) <= tie, (tag, d, k, own, int(counts[d, k]))
            in_bin = (conf_o > EDGES[k]) & (conf_o <= EDGES[k + 1])
            far = int((in_bin & (dist >= margin)).sum())
            near = int(((dist < margin) & (conf_o > EDGES[k] - margin) & (conf_o <= EDGES[k + 1] + margin)).sum())
            assert far <= counts[d, k] <= far + near, (tag, d, k, far, near, int(counts[d, k]))
    print(f"bf16 parity [{tag}] B={B}: max|out - oracle| {worst_out:.2e}, loss {lg:.6f} vs {lo:.6f} (rel {abs(lg - lo) / max(abs(lo), 1e-3):.1e}), "
          f"gradient rel-l2: worst {worst:.2e} ({worst_name}), rms over tensors {rms_gpu:.2e} vs the oracle's self-distance {rms_self:.2e}, min cosine {min_cos:.5f}")
    return worst_out, worst, min_cos


def test_bench_configuration_B4096_bf16_dropout_matches_the_bf16_oracle():
    """BASELINE configs[2] exactly as bench.py runs it: B = 4096, bf16, dropout 0.3, fused plan, random-init weights."""
    B = 4096
    check_pair(*run_pair(B, dropout=0.3, seed=42), B, "configs[2]")


@pytest.mark.parametrize("B", [64, 515])
def test_small_and_ragged_batches_match_the_bf16_oracle(B):
    check_pair(*run_pair(B, dropout=0.3, seed=7 + B), B, f"ragged B={B}")


def test_no_dropout_matches_the_bf16_oracle():
    check_pair(*run_pair(512, dropout=0.0, seed=3), 512, "dropout 0")


@pytest.mark.parametrize("tag,zero", [("audio_only", ("video", "text")), ("text_only", ("audio", "video"))])
def test_config5_B8192_missing_modality_matches_the_bf16_oracle(tag, zero):
    """BASELINE configs[4] per-GPU shape (B = 8192, bf16, zero-filled missing modalities) with dropout live."""
    check_pair(*run_pair(8192, dropout=0.3, seed=29, zero=zero), 8192, f"configs[4] {tag}")
