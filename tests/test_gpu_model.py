"""GPU parity of the whole fusion + DEER path (MultimodalDEER through the C ABI) against
the CPU oracle and the golden vectors captured from the reference.

Tolerances: fp32 config <= 1e-4 abs on mu / nu / alpha / beta (BASELINE north star);
bf16 config gated on CCC >= 0.999 and a documented absolute band (SURVEY 7 "hard parts").
"""
import json
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mmdeer import _lib, synth  # noqa: E402
from mmdeer.model import ModelConfig, MultimodalDEER  # noqa: E402
from mmdeer.spec import DIM_NAMES, param_table  # noqa: E402
from oracle import deer_oracle as O  # noqa: E402

DEV = "cuda:0"
GRAD_SLICE = 48


def make_model(dtype="fp32", dropout=0.3, closed_form=True, seed=42):
    m = MultimodalDEER(ModelConfig(compute_dtype=dtype, dropout=dropout, seed=seed),
                       init="closed_form" if closed_form else "reference")
    return m.to(DEV)


def batch(B, seed=42, zero=()):
    b = synth.make_batch(B, seed=seed)
    for z in zero:
        b[z] = np.zeros_like(b[z])
    return {k: torch.from_numpy(v) for k, v in b.items()}


def oracle_params(model, dtype=torch.float32, requires_grad=False):
    return O.to_params({k: v.detach().cpu() for k, v in model.state_dict().items()}, dtype, requires_grad)


@pytest.mark.parametrize("B", [1, 7, 32])
def test_forward_fp32_matches_golden_and_oracle(golden_dir, B):
    g = dict(np.load(os.path.join(golden_dir, f"stackc_B{B}.npz")))
    m = make_model().eval()
    b = batch(B)
    with torch.no_grad():
        out = m(b["audio"].to(DEV), b["video"].to(DEV), b["text"].to(DEV))
    torch.cuda.synchronize()
    for k in ("fused_features", "audiovisual_features", "trimodal_features", "trimodal_attention_weights", "mu_all",
              "uncertainty_all"):
        np.testing.assert_allclose(out[k].cpu().numpy(), g["eval." + k], rtol=1e-4, atol=1e-4, err_msg=k)
    for d in DIM_NAMES:
        for key in ("mu", "nu", "alpha", "beta", "aleatoric_uncertainty", "epistemic_uncertainty", "uncertainty"):
            v = out[f"{d}_{key}"]
            assert v.shape == (B, 1)
            np.testing.assert_allclose(v.cpu().numpy(), g[f"eval.{d}_{key}"], rtol=1e-4, atol=1e-4, err_msg=f"{d}_{key}")
    assert torch.equal(out["av_attention_weights"]["audio_to_video"].cpu(), torch.ones(B, 1))
    assert out["uncertainty_weights"] is None
    assert out["gamma"].shape == (B, 3) and out["predictions"] is out["mu"]


def test_config2_fp32_B1024_vs_cpu_oracle():
    """BASELINE config 2: B=1024 fp32 eval forward, all outputs within 1e-4 of the CPU path; CCC per dimension."""
    m = make_model(closed_form=False).eval()
    b = batch(1024, seed=42)
    with torch.no_grad():
        out = m(b["audio"].to(DEV), b["video"].to(DEV), b["text"].to(DEV))
        P = oracle_params(m)
        fo, ho = O.model_forward(P, b["audio"], b["video"], b["text"])
    for k in ("mu", "nu", "alpha", "beta"):
        ref = torch.cat([ho[f"{d}_{k}"] for d in DIM_NAMES], dim=1)
        err = (out[{"mu": "gamma"}.get(k, k)].cpu() - ref).abs().max().item()
        assert err < 1e-4, (k, err)
    assert (out["fused_features"].cpu() - fo["fused_features"]).abs().max().item() < 1e-4
    for i in range(3):
        assert O.ccc(out["mu_all"][:, i].cpu(), ho["mu_all"][:, i]) > 0.9999


@pytest.mark.parametrize("B", [1, 7, 32])
def test_train_step_fp32_grads_match_golden(golden_dir, B):
    g = dict(np.load(os.path.join(golden_dir, f"stackc_B{B}.npz")))
    m = make_model(dropout=0.0).train()
    b = batch(B)
    ld = m.train_step(b["audio"].to(DEV), b["video"].to(DEV), b["text"].to(DEV), b["targets"].to(DEV))
    torch.cuda.synchronize()
    for k in ("total_loss", "cross_dim_loss", "valence_nll_loss", "arousal_reg_loss", "dominance_kl_loss", "valence_ece_loss",
              "arousal_total_loss"):
        assert float(ld[k]) == pytest.approx(float(g["loss." + k]), rel=2e-4, abs=2e-5), k
    named = dict(m.named_parameters())
    for name, _, _ in param_table():
        gr = named[name].grad
        assert gr is not None, name
        gr = gr.detach().cpu()
        ref_norm = float(g["gnorm." + name])
        assert float(gr.double().norm()) == pytest.approx(ref_norm, rel=2e-3, abs=1e-6), name
        flat = gr.numpy().reshape(-1)
        tol = 2e-4 * max(ref_norm, 1e-3)
        np.testing.assert_allclose(flat[:GRAD_SLICE], g["ghead." + name], rtol=2e-3, atol=tol, err_msg=name)
        np.testing.assert_allclose(flat[-GRAD_SLICE:], g["gtail." + name], rtol=2e-3, atol=tol, err_msg=name)
    w = named["fusion.audio_visual_fusion.cross_attention.in_proj_weight"].grad
    assert float(w[:512].abs().max()) == 0.0          # dead q/k rows: exact zeros
    for n, p in m.named_parameters():
        if "uncertainty_gate" in n:
            assert p.grad is None


def test_autograd_path_equals_fused_step():
    """compute_loss(model(a,v,t), y)['total_loss'].backward() == train_step()."""
    b = batch(48, seed=5)
    a, v, t, y = (b[k].to(DEV) for k in ("audio", "video", "text", "targets"))
    m1 = make_model(dropout=0.3, seed=9).train()
    m2 = make_model(dropout=0.3, seed=9).train()
    ld1 = m1.train_step(a, v, t, y)
    out = m2(a, v, t)
    ld2 = m2.compute_loss(out, y)
    ld2["total_loss"].backward()
    torch.cuda.synchronize()
    assert float(ld1["total_loss"]) == pytest.approx(float(ld2["total_loss"]), rel=1e-6)
    for (n1, p1), (n2, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        if p1.grad is None:
            assert p2.grad is None
            continue
        d = (p1.grad - p2.grad).abs()
        # same kernels either way; the two entry points differ only in fp32 evaluation order of the loss gradient
        assert float(d.max()) <= 2e-6 * max(float(p1.grad.abs().max()), 1e-6), (n1, float(d.max()), int(d.argmax()),
                                                                         float(p1.grad.abs().max()), bool(torch.isnan(p2.grad).any()))
    assert torch.equal(ld1["ece_bin_counts"], ld2["ece_bin_counts"])


def dump_masks(m, B, offset):
    """Regenerate the keep-masks of a training forward (seed, offset) for the oracle."""
    lib = _lib.load()
    p, seed = m.dims.dropout, m.dropout_seed
    s = torch.cuda.current_stream().cuda_stream

    def mask(site, rows, cols):
        t = torch.empty(rows, cols, dtype=torch.uint8, device=DEV)
        _lib.check(lib.mmdeer_dropout_mask(site, rows, cols, p, seed, offset, t.data_ptr(), s))
        return t
    av = mask(1, 2 * B, 8)
    masks = {
        "av_attn_a2v": av[:B], "av_attn_v2a": av[B:],
        "av_fuse": mask(2, B, 256), "tri_attn": mask(3, B, 32).view(B, 8, 2, 2), "tri_fuse": mask(4, B, 512),
        "out_proj": mask(5, B, 512), "fp0": mask(6, B, 256), "fp1": mask(7, B, 256),
        "ev0": mask(8, B, 384).view(B, 3, 128), "ev1": mask(9, B, 192).view(B, 3, 64),
    }
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in masks.items()}


def test_training_with_dropout_matches_oracle_given_the_same_masks():
    B = 40
    m = make_model(dropout=0.3, seed=123).train()
    b = batch(B, seed=11)
    ld = m.train_step(b["audio"].to(DEV), b["video"].to(DEV), b["text"].to(DEV), b["targets"].to(DEV), return_features=True)
    masks = dump_masks(m, B, m._step)
    P = oracle_params(m, torch.float64, requires_grad=True)
    fo, ho, ldo, grads = O.train_step(P, b["audio"].double(), b["video"].double(), b["text"].double(),
                                      b["targets"].double(), masks=masks, p=0.3)
    out = ld["_outputs"]
    assert (out["fused_features"].cpu().double() - fo["fused_features"]).abs().max().item() < 1e-4
    assert (out["trimodal_attention"].cpu().double() - fo["trimodal_attention_weights"]).abs().max().item() < 1e-5
    assert (out["av_attention"][:, 0:1].cpu().double() - fo["av_attention_weights"]["audio_to_video"]).abs().max().item() < 1e-6
    assert float(ld["total_loss"]) == pytest.approx(float(ldo["total_loss"]), rel=2e-4)
    named = dict(m.named_parameters())
    for name, _, _ in param_table():
        got, ref = named[name].grad.cpu().double(), grads[name]
        scale = max(float(ref.abs().max()), 1e-6)
        assert (got - ref).abs().max().item() < 2e-3 * scale + 1e-7, name
    keep = np.mean([float(v.float().mean()) for v in masks.values()])
    assert abs(keep - 0.7) < 0.03


@pytest.mark.parametrize("tag,zero", [("audio_only", ("video", "text")), ("text_only", ("audio", "video"))])
def test_missing_modalities(golden_dir, tag, zero):
    """BASELINE config 5 semantics: a missing modality is an all-zero feature block."""
    g = dict(np.load(os.path.join(golden_dir, "stackc_missing.npz")))
    m = make_model().eval()
    b = batch(8, seed=43, zero=zero)
    with torch.no_grad():
        out = m({"audio": b["audio"].to(DEV), "video": b["video"].to(DEV), "text": b["text"].to(DEV)})
    np.testing.assert_allclose(out["mu_all"].cpu().numpy(), g[f"{tag}/eval.mu_all"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(out["uncertainty_all"].cpu().numpy(), g[f"{tag}/eval.uncertainty_all"], rtol=1e-4, atol=1e-4)


def test_bf16_forward_and_step_track_the_fp32_cpu_path():
    B = 512
    b = batch(B, seed=3)
    m = make_model("bf16", closed_form=False, dropout=0.0).train()
    a, v, t, y = (b[k].to(DEV) for k in ("audio", "video", "text", "targets"))
    ld = m.train_step(a, v, t, y)
    P = oracle_params(m, torch.float32, requires_grad=True)
    fo, ho, ldo, grads = O.train_step(P, b["audio"], b["video"], b["text"], b["targets"])
    out = ld["_outputs"]["_nig"].cpu()
    ref = {k: torch.cat([ho[f"{d}_{k}"] for d in DIM_NAMES], dim=1).detach() for k in ("mu", "nu", "alpha", "beta")}
    for i, k in enumerate(("mu", "nu", "alpha", "beta")):
        assert (out[i] - ref[k]).abs().max().item() < 5e-2, k
    for i in range(3):
        assert O.ccc(out[0][:, i], ref["mu"][:, i]) > 0.999
    assert float(ld["total_loss"]) == pytest.approx(float(ldo["total_loss"]), rel=2e-2)
    # gradient direction: cosine similarity per large tensor
    named = dict(m.named_parameters())
    for name, shape, _ in param_table():
        if len(shape) != 2 or "in_proj_weight" in name and "cross_attention" in name:
            continue
        gg, rr = named[name].grad.cpu().double().flatten(), grads[name].double().flatten()
        cos = float((gg @ rr) / (gg.norm() * rr.norm() + 1e-30))
        print(f"bf16 grad cosine {name}: {cos:.4f}")
        # activations AND activation-gradients are stored in bf16 (8 significant bits) through ~12 layers:
        # the deepest weights see the accumulated rounding noise of the whole chain
        assert cos > 0.95, (name, cos)
    # bf16 user inputs are accepted as-is
    m.eval()
    with torch.no_grad():
        o2 = m(a.bfloat16(), v.bfloat16(), t.bfloat16())
    assert (o2["mu_all"].cpu() - ref["mu"]).abs().max().item() < 8e-2


def test_full_size_properties_B4096():
    """Size-independent properties at the BASELINE batch size (no oracle run at this size):
    permutation equivariance over the batch and determinism of the fused step."""
    B = 4096
    b = batch(B, seed=8)
    a, v, t, y = (b[k].to(DEV) for k in ("audio", "video", "text", "targets"))
    m = make_model("bf16", closed_form=False).eval()
    with torch.no_grad():
        o1 = m(a, v, t)["mu_all"].clone()
        perm = torch.randperm(B, device=DEV)
        o2 = m(a[perm], v[perm], t[perm])["mu_all"]
    assert torch.equal(o1[perm], o2)
    m.train()
    step0 = m._step
    l1 = m.train_step(a, v, t, y)
    g1 = m.flat_grad().clone()
    loss1 = float(l1["total_loss"])
    m._step = step0
    l2 = m.train_step(a, v, t, y)
    assert torch.equal(g1, m.flat_grad())                       # no atomics anywhere: bit-identical reruns
    assert loss1 == float(l2["total_loss"])
    assert int(l1["ece_bin_counts"].sum()) == 3 * B
    assert torch.isfinite(g1).all()


def test_empty_batch_and_errors():
    m = make_model().eval()
    with torch.no_grad():
        out = m(torch.empty(0, 84, device=DEV), torch.empty(0, 256, device=DEV), torch.empty(0, 768, device=DEV))
    assert out["mu_all"].shape == (0, 3)
    with pytest.raises(ValueError):
        m(torch.zeros(2, 83, device=DEV), torch.zeros(2, 256, device=DEV), torch.zeros(2, 768, device=DEV))
    with pytest.raises(RuntimeError):
        m(torch.zeros(2, 84), torch.zeros(2, 256), torch.zeros(2, 768))   # CPU tensors: no fallback


def test_state_dict_roundtrip_and_repack():
    m1 = make_model(closed_form=False, seed=1).eval()
    m2 = make_model(closed_form=False, seed=2).eval()
    b = batch(16)
    a, v, t = (b[k].to(DEV) for k in ("audio", "video", "text"))
    with torch.no_grad():
        o1 = m1(a, v, t)["mu_all"].clone()
        assert not torch.allclose(o1, m2(a, v, t)["mu_all"])
        m2.load_state_dict(m1.state_dict())          # in-place copy_ bumps versions -> repack
        assert torch.equal(o1, m2(a, v, t)["mu_all"])


def test_graph_captured_train_step_matches_eager():
    """capture_train_step (HIP graph, dropout counter on the device) reproduces the eager steps: same losses and
    gradients step by step, fresh masks on every replay."""
    import copy

    m1 = MultimodalDEER(ModelConfig(compute_dtype="bf16", seed=11)).to("cuda:0").train()
    m2 = copy.deepcopy(m1)
    b = synth.make_batch(256, seed=9)
    a, v, t, y = (torch.from_numpy(b[k]).to("cuda:0") for k in ("audio", "video", "text", "targets"))
    replay = m1.capture_train_step(a, v, t, y)       # runs one eager warm-up step (dropout step 1) before capturing
    m2.train_step(a, v, t, y)                        # keep the eager twin's step counter in sync
    losses = []
    for _ in range(3):
        d1 = replay()
        d2 = m2.train_step(a, v, t, y)
        assert float(d1["total_loss"]) == float(d2["total_loss"])
        assert torch.equal(m1.flat_grad(), m2.flat_grad())
        losses.append(float(d1["total_loss"]))
    assert len(set(losses)) == 3                     # different dropout masks each replay
    # new data goes in through the captured tensors
    b2 = synth.make_batch(256, seed=10)
    a.copy_(torch.from_numpy(b2["audio"])); v.copy_(torch.from_numpy(b2["video"]))
    t.copy_(torch.from_numpy(b2["text"])); y.copy_(torch.from_numpy(b2["targets"]))
    d1, d2 = replay(), m2.train_step(a, v, t, y)
    assert float(d1["total_loss"]) == float(d2["total_loss"])


def test_attention_launch_plans_match_each_other():
    """The three plans of the trimodal attention block -- fused projection + attention with the backward recomputing q|k|v
    (default), fused forward that also stores q|k|v for the unfused backward kernel (option qkv_recompute = 0), and the
    unfused pair (fused_attn = 0) -- give the same training step up to the bf16 rounding of q, k, v.  The plans are
    switched in-process through mmdeer_set_option (the library reads no environment variable)."""
    b = synth.make_batch(300, seed=3)
    a, v, t, y = (torch.from_numpy(b[k]).to(DEV) for k in ("audio", "video", "text", "targets"))
    outs = {}
    for mode, opts in (("default", {}), ("store_qkv", {"qkv_recompute": 0}), ("unfused", {"fused_attn": 0})):
        m = MultimodalDEER(ModelConfig(compute_dtype="bf16", seed=5)).to(DEV).train()
        with _lib.options(**opts):
            d = m.train_step(a, v, t, y)
            torch.cuda.synchronize()
        outs[mode] = (float(d["total_loss"]), m.flat_grad().double().clone())
    assert _lib.get_option("fused_attn") == 1 and _lib.get_option("qkv_recompute") == 1      # restored
    with pytest.raises(RuntimeError, match="unknown option"):
        _lib.set_option("no_such_option", 1)
    g0 = outs["default"][1]
    for mode in ("store_qkv", "unfused"):
        loss, g = outs[mode]
        assert outs["default"][0] == pytest.approx(loss, rel=2e-3), mode
        assert not torch.equal(g, g0), mode                      # another plan really ran
        cos = float((g @ g0) / (g.norm() * g0.norm()))
        # the unfused plan stores q|k|v (v rounded to bf16 too): another rounding pattern, and a bf16 chain amplifies that
        # to ~1 % of the gradient (tests/test_gpu_bf16_parity.py) -- measured 0.990 (unfused), 0.99x (store_qkv)
        assert cos > 0.98, (mode, cos)
        assert float(g.abs().sum()) == pytest.approx(float(g0.abs().sum()), rel=2e-2), mode


def _chain_step(B, **opts):
    b = synth.make_batch(B, seed=21)
    a, v, t, y = (torch.from_numpy(b[k]).to(DEV) for k in ("audio", "video", "text", "targets"))
    m = MultimodalDEER(ModelConfig(compute_dtype="bf16", seed=6)).to(DEV).train()
    with _lib.options(chain_min=1, **opts):         # the library takes the chains from B = 512 on: here at every size
        d = m.train_step(a, v, t, y)
        torch.cuda.synchronize()
    return float(d["total_loss"]), m.flat_grad().clone(), {k: d[k].clone() for k in ("gamma", "nu", "alpha", "beta") if k in d}


@pytest.mark.parametrize("B", [300, 2500, 4096, 5000, 8192])
def test_layer_chain_launch_is_bit_identical_to_the_separate_launches(B):
    """chain.hip walks F2..F6 (the AV value / output projections, fusion layer, LayerNorm, token-0 projection) and F9..F17
    (five Linear+ReLU+Dropout layers, two LayerNorms, the stacked evidence heads) as ONE launch each with the rows resident in LDS.
    Same accumulation order, same rounding points, same dropout decisions as the stand-alone
    GEMM / fused-LayerNorm launches: the training step must come out bit for bit (B = 300 and 2500: ragged 16-sample blocks;
    the library
    uses 16-sample workgroups up to B = 4096 and 32-sample ones, forward chains only, up to 8192: B = 5000 and 8192).  The backward
    chains are switched off here: see the next test."""
    on, off = _chain_step(B, chain=1, chain_bwd=0), _chain_step(B, chain=0)
    assert on[0] == off[0]
    assert torch.equal(on[1], off[1])
    for k in on[2]:
        assert torch.equal(on[2][k], off[2][k]), k


def _input_chain_step(B, **opts):
    """A training step on bf16 feature blocks (the bench's inputs) + the workspace buffers the input projections leave behind."""
    lib = _lib.load()
    b = synth.make_batch(B, seed=23)
    a, v, t = (torch.from_numpy(b[k]).to(DEV).bfloat16() for k in ("audio", "video", "text"))
    y = torch.from_numpy(b["targets"]).to(DEV)
    m = MultimodalDEER(ModelConfig(compute_dtype="bf16", seed=6)).to(DEV).train()
    with _lib.options(chain_min=1, **opts):
        d = m.train_step(a, v, t, y)
        torch.cuda.synchronize()
    ws = m._workspace(B, torch.device(DEV)).view(torch.uint8)
    bufs = {}
    for name, nbytes in (("avin", 2 * B * 256 * 2), ("xtok", 2 * B * 512 * 2), ("audio_pad", B * 128 * 2)):
        off = lib.mmdeer_workspace_offset(B, 0, name.encode())
        bufs[name] = ws[off:off + nbytes].clone()
    return float(d["total_loss"]), m.flat_grad().clone(), {k: d[k].clone() for k in ("gamma", "nu", "alpha", "beta") if k in d}, bufs


@pytest.mark.parametrize("B", [300, 2500, 4096])
def test_input_chain_is_bit_identical_to_the_pad_and_projection_launches(B):
    """Option chain_in (bf16 feature blocks, B <= 4096): the audio-visual chain's launch starts from the raw text / video / 84-wide
    audio rows -- text_projection, video_projection and audio_projection (on rows it pads in LDS) are its first two layers -- instead
    of reading what a pad launch and the three-problem projection launch left.  Same k order in the MFMAs, same bias add: the stacked
    attention input, token 1 of xtok, the padded audio copy the weight-gradient launch reads, the loss, the outputs and every
    gradient must come out bit for bit (B = 300, 2500: ragged 16-sample blocks)."""
    on, off = _input_chain_step(B, chain_in=1), _input_chain_step(B, chain_in=0)
    for name in on[3]:
        assert torch.equal(on[3][name], off[3][name]), name
    assert on[0] == off[0]
    for k in on[2]:
        assert torch.equal(on[2][k], off[2][k]), k
    assert torch.equal(on[1], off[1])


def test_input_chain_graph_replay_matches_eager():
    """The device-side dropout counter is advanced by the forward's last kernel (the NIG head) now that no pad launch precedes the
    first mask: captured replays of the input-chain plan reproduce eager steps, loss and gradient, with fresh masks per replay."""
    import copy
    B = 600
    with _lib.options(chain_min=1):
        m1 = MultimodalDEER(ModelConfig(compute_dtype="bf16", seed=12)).to(DEV).train()
        m2 = copy.deepcopy(m1)
        b = synth.make_batch(B, seed=9)
        a, v, t = (torch.from_numpy(b[k]).to(DEV).bfloat16() for k in ("audio", "video", "text"))
        y = torch.from_numpy(b["targets"]).to(DEV)
        replay = m1.capture_train_step(a, v, t, y)
        m2.train_step(a, v, t, y)
        losses = []
        for _ in range(3):
            d1 = replay()
            d2 = m2.train_step(a, v, t, y)
            assert float(d1["total_loss"]) == float(d2["total_loss"])
            assert torch.equal(m1.flat_grad(), m2.flat_grad())
            losses.append(float(d1["total_loss"]))
        assert len(set(losses)) == 3


@pytest.mark.parametrize("B", [300, 2500, 4096, 5000, 8192])
def test_backward_chain_matches_the_separate_launches(B):
    """The backward's head / trimodal run (7 dX products with their (Y > 0) masks, two LayerNorm backwards with gamma / beta
    partials) as one chain launch.  The dX products are bit-identical to the GEMM launches; the LayerNorm backward sums a row in
    another order than rowops.hip's kernel, so dz differs by a bf16 rounding now and then and the gradients upstream of it by what
    a bf16 chain makes of that (tests/test_gpu_bf16_parity.py): the forward results must be identical, the gradient must agree to
    a small fraction of its norm, and every launch of the plan is checked to 1 ulp by tests/test_gpu_bf16_layers.py."""
    on, off = _chain_step(B, chain=1, chain_bwd=1), _chain_step(B, chain=1, chain_bwd=0)
    assert on[0] == off[0]
    for k in on[2]:
        assert torch.equal(on[2][k], off[2][k]), k
    g1, g0 = on[1].double(), off[1].double()
    assert not torch.equal(g1, g0)                       # the other plan really ran
    rel = float((g1 - g0).norm() / g0.norm())
    cos = float((g1 @ g0) / (g1.norm() * g0.norm()))
    assert rel < 2e-2 and cos > 0.9998, (rel, cos)       # measured: see DESIGN.md


@pytest.mark.parametrize("B", [300, 4096, 5000, 8192])
def test_head_backward_in_the_chain_prologue_matches_its_own_launch(B):
    """Option chain_nig: the backward chain computes the head's last-layer backward and the loss gradient in its prologue instead
    of reading what nig_bwd_kernel left (one launch fewer).  Same arithmetic per (sample, dimension): the loss record, d e2 and so
    every gradient upstream come out bit for bit; only dW3 / db3 of the three heads' last layers are summed over other partial
    blocks (16- or 32-sample workgroups instead of 64-sample ones)."""
    from mmdeer.spec import param_offsets
    lo = min(o for (name, _s, _i), o in zip(param_table(), param_offsets()[0]) if ".evidence_net.6." in name)
    on, off = _chain_step(B, chain_nig=1), _chain_step(B, chain_nig=0)
    assert on[0] == off[0]
    for k in on[2]:
        assert torch.equal(on[2][k], off[2][k]), k
    assert torch.equal(on[1][:lo], off[1][:lo])
    assert not torch.equal(on[1][lo:], off[1][lo:])       # the other plan really ran
    d = (on[1][lo:].double() - off[1][lo:].double()).norm() / off[1][lo:].double().norm()
    assert float(d) < 1e-5, float(d)


@pytest.mark.parametrize("B", [300, 1000, 4096, 5000, 8192])
def test_nig_head_in_the_forward_chain_tail_matches_its_own_launch(B):
    """Option chain_nigf: the forward head chain ends in the NIG head -- last layer, activations, uncertainties and the loss statistics as
    WAVE partials (16 samples each) that the consumers combine four to a block in nig_fwd_kernel's own order.  Loss record, outputs, ECE
    bin counts and the whole flat gradient must come out bit for bit as with the separate nig_fwd launch (ragged batches: the last
    block's absent waves count as the zeros an inactive wave contributes; 32-sample workgroups: two row blocks per workgroup)."""
    on, off = _chain_step(B, chain_nigf=1), _chain_step(B, chain_nigf=0)
    assert on[0] == off[0]
    for k in on[2]:
        assert torch.equal(on[2][k], off[2][k]), k
    assert torch.equal(on[1], off[1])
    # ... also with the head's backward as a launch of its own (nig_bwd_kernel reads the wave partials) and in exact-global mode
    on2, off2 = _chain_step(B, chain_nigf=1, chain_nig=0), _chain_step(B, chain_nigf=0, chain_nig=0)
    assert on2[0] == off2[0] and torch.equal(on2[1], off2[1])


@pytest.mark.parametrize("opts", [dict(dw_tile=3), dict(dw_tile=4), dict(dw_kg=1), dict(ln_fused=0, chain=0), dict(chain=0, dw_tile=3),
                                  dict(splitk_max=2), dict(ksteps=8), dict(chain_nig=0)])
def test_weight_gradient_and_launch_plan_options_agree(opts):
    """Every launch plan the options select computes the same training step: the weight-gradient kernel on 128x128 tiles (default,
    K-slices of B rows, the workgroup's halves splitting 64-row stages), 256x256 tiles with split-K slabs (rounds 1-2), 256x128
    tiles, other slice lengths; chains and fused LayerNorms on or off.  Weight gradients are fp32 sums of the same bf16 products in
    another order: plans that leave the activations alone must agree to 1e-5 of the gradient's norm; plans that change a LayerNorm's
    summation order move a bf16 rounding now and then (bounded like the backward-chain test)."""
    B = 4096
    base = _chain_step(B)                      # helper lowers chain_min to 1: chains run as in the default plan at this size
    other = _chain_step(B, **opts)
    exact_acts = not ({"ln_fused", "chain"} & set(opts))
    g1, g0 = other[1].double(), base[1].double()
    rel = float((g1 - g0).norm() / g0.norm())
    if exact_acts:
        assert other[0] == base[0]
        for k in base[2]:
            assert torch.equal(other[2][k], base[2][k]), k
        assert rel < 1e-5, rel
    else:
        assert other[0] == pytest.approx(base[0], rel=1e-4)
        assert rel < 2e-2, rel


@pytest.mark.parametrize("B,opts", [(300, {}), (300, dict(chain_min=1)), (5000, {}), (5000, dict(chain=0)), (8192, {})])
def test_training_step_reads_nothing_stale_from_the_workspace(B, opts):
    """Every workspace buffer a step reads is written earlier in the same step -- in particular the per-workgroup partial slabs the
    fold sums (a layer chain over 4096 < B < 8192 samples runs fewer workgroups than the LayerNorm-backward kernel it replaces:
    the fold must take the chain's count).  The workspace is filled with NaN bit patterns before the step; the step must come out
    bit for bit as on a fresh model."""
    b = synth.make_batch(B, seed=23)
    a, v, t, y = (torch.from_numpy(b[k]).to(DEV) for k in ("audio", "video", "text", "targets"))
    res = []
    for poison in (False, True):
        m = MultimodalDEER(ModelConfig(compute_dtype="bf16", seed=8)).to(DEV).train()
        with _lib.options(**opts):
            if poison:
                m._workspace(B, torch.device(DEV)).fill_(0xFF)
            d = m.train_step(a, v, t, y)
            torch.cuda.synchronize()
        res.append((float(d["total_loss"]), m.flat_grad().clone()))
    assert math.isfinite(res[1][0]) and res[0][0] == res[1][0]
    assert bool(torch.isfinite(res[1][1]).all())
    assert torch.equal(res[0][1], res[1][1])


@pytest.mark.parametrize("B,dtype", [(5000, "bf16"), (4096, "bf16"), (200, "fp32")])
def test_two_call_backward_reads_nothing_stale_from_the_workspace(B, dtype):
    """The same for the data-parallel overlap plan (mmdeer_backward phase 1, then 2) and for the fp32 configuration."""
    b = synth.make_batch(B, seed=29)
    a, v, t, y = (torch.from_numpy(b[k]).to(DEV) for k in ("audio", "video", "text", "targets"))
    res = []
    for poison in (False, True):
        m = MultimodalDEER(ModelConfig(compute_dtype=dtype, seed=8)).to(DEV).train()
        m.train_step(a, v, t, y)                      # allocates the workspace, packs the weights
        if poison:
            m._workspace(B, torch.device(DEV)).fill_(0xFF)
        o = m._launch_forward(a, v, t, y, want_features=False)
        meta = o["_meta"]
        flat = torch.zeros_like(m.flat_grad())
        loss = torch.empty(_lib.LOSS_OUT, device=DEV)
        m._launch_backward(meta, meta["targets"], loss_out=loss, flat=flat, want_views=False, phase=1)
        m._launch_backward(meta, meta["targets"], loss_out=loss, flat=flat, want_views=False, phase=2)
        torch.cuda.synchronize()
        res.append((loss.clone(), flat.clone()))
    assert bool(torch.isfinite(res[1][0]).all()) and bool(torch.isfinite(res[1][1]).all())
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def test_autotune_launch_plan_picks_a_plan_and_keeps_the_results():
    """MultimodalDEER.autotune_launch_plan times the captured step under the three launch plans on this GPU and sets the library's
    options to the fastest (bench.py does that before its warm-up).  Whatever it picks, the forward results are those of the
    default plan bit for bit; outside the chains' range nothing is timed."""
    saved = {k: _lib.get_option(k) for k in ("chain", "chain_bwd")}
    try:
        b = synth.make_batch(4096, seed=31)
        a, v, t, y = (torch.from_numpy(b[k]).to(DEV) for k in ("audio", "video", "text", "targets"))
        m = MultimodalDEER(ModelConfig(compute_dtype="bf16", seed=9)).to(DEV).train()
        calls = []
        plan = m.autotune_launch_plan(a, v, t, y, replays=5, reduce_max=lambda x: calls.append(x) or x)
        names = [n for n, _ in MultimodalDEER.LAUNCH_PLANS]
        assert plan["plan"] in names and sorted(plan["ms"]) == sorted(names) and len(calls) == 6
        assert all(0.05 < ms < 5.0 for ms in plan["ms"].values()), plan
        assert plan["ms"][plan["plan"]] == min(plan["ms"].values())
        for k, val in plan["options"].items():
            assert _lib.get_option(k) == val
        m2 = MultimodalDEER(ModelConfig(compute_dtype="bf16", seed=9)).to(DEV).train()
        d_tuned = m2.train_step(a, v, t, y)
        for k, val in saved.items():
            _lib.set_option(k, val)
        m3 = MultimodalDEER(ModelConfig(compute_dtype="bf16", seed=9)).to(DEV).train()
        d_default = m3.train_step(a, v, t, y)
        torch.cuda.synchronize()
        for k in d_default:
            if torch.is_tensor(d_default[k]):
                assert torch.equal(d_tuned[k], d_default[k]), k
        assert float(d_tuned["total_loss"]) == float(d_default["total_loss"])
        # fp32 / small batches: the chains do not apply, nothing to choose
        small = m.autotune_launch_plan(a[:64], v[:64], t[:64], y[:64])
        assert small["ms"] == {} and small["plan"] == "separate launches"
    finally:
        for k, val in saved.items():
            _lib.set_option(k, val)


def test_eval_forward_with_chains_is_bit_identical():
    """The inference path takes the forward chains as well (no dropout: every site is off): all outputs of forward() in eval mode
    must equal the separate-launch plan's bit for bit, also on a ragged batch."""
    B = 2500
    b = synth.make_batch(B, seed=23)
    a, v, t = (torch.from_numpy(b[k]).to(DEV) for k in ("audio", "video", "text"))
    m = MultimodalDEER(ModelConfig(compute_dtype="bf16", seed=4)).to(DEV).eval()
    outs = {}
    for chain in (1, 0):
        with _lib.options(chain=chain, chain_min=1), torch.no_grad():
            o = m(a, v, t)
            torch.cuda.synchronize()
        outs[chain] = {k: x.clone() for k, x in o.items() if torch.is_tensor(x)}
    assert set(outs[1]) == set(outs[0]) and len(outs[1]) >= 5
    for k in outs[1]:
        assert torch.equal(outs[1][k], outs[0][k]), k


def test_two_phase_backward_equals_single_call():
    """mmdeer_backward with phase = 1 then 2 (the data-parallel overlap plan) fills the flat gradient buffer with
    what the single call produces (buckets 0-1 bit for bit, bucket 2 up to the fp32 summation order); after phase 1 buckets 0-1 are
    final and bucket 2 is still untouched.  (B = 500: below chain_min, both modes run the separate launches -- with the chains the
    single call walks the audio-visual run as a chain, whose LayerNorm backward sums in another order than the stand-alone kernel.)"""
    lib = _lib.load()
    m = MultimodalDEER(ModelConfig(compute_dtype="bf16", seed=8)).to(DEV).train()
    b = batch(500, seed=13)
    a, v, t, y = (b[k].to(DEV) for k in ("audio", "video", "text", "targets"))
    m.train_step(a, v, t, y)
    ref = m.flat_grad().clone()
    lo = int(lib.mmdeer_bucket_end(2))

    o = m._launch_forward(a, v, t, y, want_features=False)
    meta = o["_meta"]
    meta["offset"] = meta["offset"]            # same dropout step as the forward just run
    # re-run the reference with the SAME dropout step for a bitwise comparison
    flat0 = torch.zeros_like(ref)
    loss0 = torch.empty(_lib.LOSS_OUT, device=DEV)
    m._launch_backward(meta, meta["targets"], loss_out=loss0, flat=flat0, want_views=False, phase=0)
    flat = torch.zeros_like(ref)
    loss = torch.empty(_lib.LOSS_OUT, device=DEV)
    m._launch_backward(meta, meta["targets"], loss_out=loss, flat=flat, want_views=False, phase=1)
    torch.cuda.synchronize()
    assert torch.equal(flat[lo:], flat0[lo:])
    assert float(flat[:lo].abs().sum()) == 0.0
    m._launch_backward(meta, meta["targets"], loss_out=loss, flat=flat, want_views=False, phase=2)
    torch.cuda.synchronize()
    assert torch.equal(flat[lo:], flat0[lo:])
    # the second call cuts the K of its five weight gradients into shorter slices (few problems: whole-reduction tiles would idle
    # the chip): the same bf16 products summed in fp32 in another order
    d = (flat[:lo].double() - flat0[:lo].double()).norm() / flat0[:lo].double().norm()
    assert float(d) < 1e-5, float(d)
    assert torch.equal(loss, loss0)


def test_exact_global_loss_over_two_shards_equals_the_global_batch():
    """SURVEY 8e, optional exact-global mode: with the 106 loss statistics summed across ranks between forward and
    backward, the loss every rank reports is the global batch's and the SUM of the ranks' gradients is its gradient
    (the default -- mean of per-shard losses -- is not: ECE and cross-dimension terms are non-linear in batch statistics).
    Two ranks are played by two shards of unequal size on the one GPU; the oracle runs on their union."""
    sizes = (48, 80)                                   # unequal, and ragged against the 64-row blocks of the head kernels
    b = batch(sum(sizes), seed=17)
    shards, lo = [], 0
    for n in sizes:
        shards.append({k: v[lo:lo + n].to(DEV) for k, v in b.items()})
        lo += n
    models = [make_model(dropout=0.0).train() for _ in sizes]       # identical closed-form parameters

    class Exchange:                                    # stands in for parallel.BucketedAllReduce on each "rank"
        active = True

        def __init__(self):
            self.seen, self.total = None, None

        def sum_small(self, t):
            self.seen = t.clone()
            if self.total is not None:
                t.copy_(self.total)

    ex = [Exchange() for _ in sizes]
    step = lambda m, s, e: m.train_step(s["audio"], s["video"], s["text"], s["targets"], stats_comm=e)
    local = [step(m, s, e) for m, s, e in zip(models, shards, ex)]          # pass 1: every rank's own statistics
    total = ex[0].seen + ex[1].seen
    assert float(total[105]) == sum(sizes) and float(ex[0].seen[105]) == sizes[0]
    for e in ex:
        e.total = total
    glob = [step(m, s, e) for m, s, e in zip(models, shards, ex)]           # pass 2: backward on the summed statistics
    torch.cuda.synchronize()

    P = oracle_params(models[0], requires_grad=True)
    fo, ho, ldo, grads = O.train_step(P, b["audio"], b["video"], b["text"], b["targets"])
    want = float(ldo["total_loss"])
    for d in glob:
        assert float(d["total_loss"]) == pytest.approx(want, rel=2e-5, abs=2e-6)
    assert float(glob[0]["total_loss"]) == float(glob[1]["total_loss"])
    assert abs(float(local[0]["total_loss"]) - want) > 1e-3                  # the shard's own loss is a different number
    assert torch.equal(glob[0]["ece_bin_counts"], glob[1]["ece_bin_counts"]) and int(glob[0]["ece_bin_counts"].sum()) == 3 * sum(sizes)
    g0, g1 = (dict(m.named_parameters()) for m in models)               # .grad of a live parameter is a view of the flat buffer
    checked = 0
    for name, ref in grads.items():
        if g0[name].grad is None:
            continue
        g = (g0[name].grad.double() + g1[name].grad.double()).cpu()
        scale = max(ref.abs().max().item(), 1e-12)
        assert (g - ref.double()).abs().max().item() / scale < 2e-3, name
        checked += 1
    assert checked >= 30


def test_exact_global_statistics_through_the_chain_prologue():
    """The exact-global mode with the head's backward inside the backward chain (bf16, option chain_nig): the summed statistics
    reach the chain's prologue instead of nig_bwd_kernel; loss record and every gradient upstream of the last head layer are bit
    for bit those of the stand-alone launch."""
    from mmdeer.spec import param_offsets
    lo = min(o for (name, _s, _i), o in zip(param_table(), param_offsets()[0]) if ".evidence_net.6." in name)
    sizes = (300, 420)
    b = synth.make_batch(sum(sizes), seed=37)

    class Exchange:
        active = True

        def __init__(self):
            self.seen, self.total = None, None

        def sum_small(self, t):
            self.seen = t.clone()
            if self.total is not None:
                t.copy_(self.total)

    res = {}
    for nig in (1, 0):
        with _lib.options(chain_min=1, chain_nig=nig):
            out, start = [], 0
            ex = [Exchange() for _ in sizes]
            models = [MultimodalDEER(ModelConfig(compute_dtype="bf16", seed=6)).to(DEV).train() for _ in sizes]
            shards = []
            for n in sizes:
                shards.append(tuple(torch.from_numpy(b[k][start:start + n]).to(DEV) for k in ("audio", "video", "text", "targets")))
                start += n
            for m, sh, e in zip(models, shards, ex):
                m.train_step(*sh, stats_comm=e)
            total = ex[0].seen + ex[1].seen
            for e in ex:
                e.total = total
            models = [MultimodalDEER(ModelConfig(compute_dtype="bf16", seed=6)).to(DEV).train() for _ in sizes]    # same dropout step
            for m, sh, e in zip(models, shards, ex):
                d = m.train_step(*sh, stats_comm=e)
                out.append((float(d["total_loss"]), m.flat_grad().clone()))
            torch.cuda.synchronize()
            res[nig] = out
    assert float(total[105]) == sum(sizes)
    for (l1, g1), (l0, g0) in zip(res[1], res[0]):
        assert l1 == l0 and math.isfinite(l1)
        assert torch.equal(g1[:lo], g0[:lo])
        d = (g1[lo:].double() - g0[lo:].double()).norm() / g0[lo:].double().norm()
        assert 0.0 < float(d) < 1e-5, float(d)
    assert res[1][0][0] == res[1][1][0]              # both "ranks" report the global batch's loss


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_gradient_through_fused_features_reaches_the_fusion_parameters(dtype):
    """fused_features is a differentiable output (fusion.py:164-171 hands it to whatever head the caller builds): a loss
    on it alone, and one on it plus the NIG outputs, give the oracle's gradients."""
    b = batch(40, seed=23)
    a, v, t = (b[k].to(DEV) for k in ("audio", "video", "text"))
    w = torch.from_numpy(synth.normal(999, 40 * 512).reshape(40, 512).astype(np.float32))
    for with_head in (False, True):
        m = make_model(dtype=dtype, dropout=0.0).train()
        out = m(a, v, t)
        loss = (out["fused_features"] * w.to(DEV)).sum()
        if with_head:
            loss = loss + (out["mu_all"] * 0.5).sum() + out["valence_uncertainty"].sum()
        loss.backward()
        P = oracle_params(m, requires_grad=True)
        fo, ho = O.model_forward(P, b["audio"], b["video"], b["text"])
        ref = (fo["fused_features"] * w).sum()
        if with_head:
            ref = ref + (ho["mu_all"] * 0.5).sum() + ho["valence_uncertainty"].sum()
        ref.backward()
        tol = 2e-3 if dtype == "fp32" else 8e-2
        close = abs(float(loss) - float(ref)) / max(abs(float(ref)), 1.0)
        assert close < (1e-4 if dtype == "fp32" else 3e-2)
        named = dict(m.named_parameters())
        checked = 0
        for name, p in P.items():
            if p.grad is None or named[name].grad is None:
                continue
            head = name.startswith("head.")
            if head and not with_head:
                assert float(named[name].grad.abs().max()) == 0.0, name      # nothing flows into the head
                continue
            g, r = named[name].grad.cpu().double().flatten(), p.grad.double().flatten()
            if dtype == "fp32":
                assert (g - r).abs().max().item() / max(r.abs().max().item(), 1e-12) < tol, name
            else:
                cos = float((g @ r) / (g.norm() * r.norm() + 1e-30))
                assert cos > 0.95, (name, cos)
            checked += 1
        assert checked >= (20 if with_head else 12)


def test_standalone_fusion_module_has_the_reference_protocol(golden_dir):
    """model.HierarchicalMultimodalFusion: the reference class's constructor, state_dict keys, output dictionary, values
    (golden eval forward) and a caller-owned head that trains the fusion through fused_features."""
    from mmdeer.model import HierarchicalMultimodalFusion
    f = HierarchicalMultimodalFusion(84, 256, 768, fusion_dim=512, intermediate_dim=256, num_attention_heads=8, dropout=0.0)
    names = json.load(open(os.path.join(golden_dir, "state_dict_names.json")))
    assert sorted(f.state_dict()) == sorted(names["fusion"])   # exactly the reference class's keys (no head.*, no prefix)
    state = synth.closed_form_state(include_gate=True)
    f.load_state_dict({k[len("fusion."):]: torch.from_numpy(v) for k, v in state.items() if k.startswith("fusion.")})
    f = f.to(DEV).eval()
    g = dict(np.load(os.path.join(golden_dir, "stackc_B7.npz")))
    b = batch(7)
    with torch.no_grad():
        out = f(b["audio"].to(DEV), b["video"].to(DEV), b["text"].to(DEV))
    assert set(out) == set(HierarchicalMultimodalFusion.KEYS) and out["uncertainty_weights"] is None
    for k in ("fused_features", "audiovisual_features", "trimodal_features", "trimodal_attention_weights"):
        np.testing.assert_allclose(out[k].cpu().numpy(), g["eval." + k], rtol=1e-4, atol=1e-4, err_msg=k)
    with pytest.raises(TypeError, match="keyword-only argument: 'uncertainties'"):      # the reference's own failure (fusion.py:148-150)
        f(b["audio"].to(DEV), b["video"].to(DEV), b["text"].to(DEV), uncertainties={"audio": None})
    # a caller's own head on fused_features: gradients reach the fusion parameters and match the oracle
    f.train()
    head = torch.nn.Linear(512, 2).to(DEV)
    out = f(b["audio"].to(DEV), b["video"].to(DEV), b["text"].to(DEV))
    head(out["fused_features"]).square().sum().backward()
    P = O.to_params({k: torch.from_numpy(v) for k, v in state.items()}, requires_grad=True)
    fo = O.fusion_forward(P, b["audio"], b["video"], b["text"])
    w, bb = head.weight.detach().cpu(), head.bias.detach().cpu()
    (fo["fused_features"] @ w.t() + bb).square().sum().backward()
    got = dict(f.named_parameters())
    checked = 0
    for name, p in P.items():
        key = name[len("fusion."):]
        if not name.startswith("fusion.") or p.grad is None or got[key].grad is None:
            continue
        scale = max(p.grad.abs().max().item(), 1e-12)
        assert (got[key].grad.cpu() - p.grad).abs().max().item() / scale < 2e-3, name
        checked += 1
    assert checked >= 12


def test_training_after_an_inference_call_on_the_same_parameters():
    """The W^T copies the backward GEMMs read are packed with every repack -- also when the call that triggers it is an
    inference call; gradients after eval -> train equal those of a model that trained first."""
    b = batch(7, seed=31)
    a, v, t, y = (b[k].to(DEV) for k in ("audio", "video", "text", "targets"))
    grads = []
    for first_eval in (False, True):
        junk = torch.full((64 << 20,), 7.0, device=DEV)      # dirty the allocator's free blocks: no lucky leftovers
        del junk
        m = make_model(dropout=0.0)
        if first_eval:
            m.eval()
            with torch.no_grad():
                m(a, v, t)
        m.train()
        m.compute_loss(m(a, v, t), y)["total_loss"].backward()
        grads.append([p.grad.clone() for p in m.live_parameters()])
    for g0, g1 in zip(*grads):
        assert torch.equal(g0, g1)
    assert float(grads[1][0].abs().sum()) > 0
    # gradients asked for in eval mode (dropout is 0 here, so they are the same numbers)
    m = make_model(dropout=0.0).eval()
    m.compute_loss(m(a, v, t), y)["total_loss"].backward()
    for g0, p in zip(grads[0], m.live_parameters()):
        assert torch.equal(g0, p.grad)


def test_mark_parameters_changed_after_a_write_through_data():
    m = make_model().eval()
    b = batch(5)
    a, v, t = (b[k].to(DEV) for k in ("audio", "video", "text"))
    with torch.no_grad():
        before = m(a, v, t)["mu_all"].clone()
        dict(m.named_parameters())["head.deer_heads.0.evidence_net.6.bias"].data[0] += 1.0   # .data: no version bump
        m.mark_parameters_changed()
        after = m(a, v, t)["mu_all"]
    np.testing.assert_allclose((after - before).cpu().numpy(), np.tile(np.float32([1, 0, 0]), (5, 1)), atol=1e-5)
