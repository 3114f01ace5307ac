"""The float64 restatement of MultiTaskDEERLoss (tests/nig_ref.py) is right, and the comparison the GPU tests make with it has teeth.

 * it agrees with oracle.deer_oracle.multitask_loss and its autograd (the oracle is pinned to the reference by
   tests/test_oracle_golden.py) on the rows of tests/golden/loss_cases.npz and on the random cases of the GPU tests;
 * the edge samples exist in float32 arithmetic: confidences ON every interior bin edge, the attainable ones next to it, 1, 0;
 * the same formulas in float32 on the CPU pass the comparison at the constants K of tests/test_gpu_nig_loss.py with the factor 2
   those constants were set with, and every seeded error is rejected.
"""
import os

import numpy as np
import pytest
import torch

from oracle import deer_oracle as O

from . import nig_ref as R
from . import test_gpu_nig_loss as T          # the cases, the constants K and the head's spread factors of the GPU tests

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "loss_cases.npz")
K_LOSS, K_GRAD, K_DW = T.K_LOSS, T.K_GRAD, T.K_DW
CASES = T.CASES
_REFS = {}


def _ref(tag):
    """The reference of a case, computed once (its conditions asserted) and left unchanged."""
    if tag not in _REFS:
        inputs, cfg, regular = CASES[tag]
        _REFS[tag] = R.checked_reference(tag, inputs, cfg, regular)
    return _REFS[tag]


def _oracle(inputs, cfg):
    g, n, a, b, y = inputs
    L = [t.double().requires_grad_(True) for t in (g, n, a, b)]
    pred = {f"{d}_{k}": L[j][:, i:i + 1] for i, d in enumerate(O.DIM_NAMES) for j, k in enumerate(("mu", "nu", "alpha", "beta"))}
    ld = O.multitask_loss(pred, y.double(), task_weights=cfg.task_w, cross_w=cfg.cross_w, reg_w=cfg.reg_w, kl_w=cfg.kl_w, ece_w=cfg.ece_w)
    ld["total_loss"].backward()
    ld = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in ld.items()}
    return ld, [t.grad if t.grad is not None else torch.zeros_like(t) for t in L]


def _agree(tag, inputs, cfg):
    g, n, a, b, y = inputs
    # the oracle in float64 decides membership on the float64 confidence: where that differs from the float32 rule -- only
    # within 1e-6 of an edge -- both sides take the same membership
    c32 = R.conf32(a, b)
    c64 = 1.0 / (1.0 + b.double() / (a.double() - 1 + 1e-8))
    e = R.EDGES32.double()
    m64 = (c64.unsqueeze(0) > e[:-1].view(-1, 1, 1)) & (c64.unsqueeze(0) <= e[1:].view(-1, 1, 1))
    m32 = R.bin_masks(c32)
    differ = (m64 != m32).any(0)
    near = ((c64.unsqueeze(0) - e.view(-1, 1, 1)).abs() < 1e-6).any(0)
    assert not (differ & ~near).any(), tag
    ref = R.reference(g, n, a, b, y, cfg, masks=m64 if differ.any() else None)
    ld, grads = _oracle(inputs, cfg)
    tol = lambda v: 1e-12 * max(1.0, abs(float(v)))
    for i, d in enumerate(O.DIM_NAMES):
        for j, k in enumerate(("total_loss", "nll_loss", "reg_loss", "kl_loss")):
            assert abs(float(ld[f"{d}_{k}"]) - float(ref.out[i * 5 + j])) <= tol(ref.out_scale[i * 5 + j]), (tag, d, k)
        if cfg.ece_w > 0:
            assert abs(float(ld[f"{d}_ece_loss"]) - float(ref.out[i * 5 + 4])) <= 1e-12, (tag, d)
            assert ld[f"{d}__bin_counts"] == ref.counts[i].tolist(), (tag, d)
    if cfg.cross_w > 0:
        assert abs(float(ld["cross_dim_loss"]) - float(ref.out[15])) <= tol(ref.out_scale[15]), tag
    assert abs(float(ld["total_loss"]) - float(ref.out[16])) <= tol(ref.out_scale[16]), tag
    for j in range(4):
        err = (grads[j] - ref.grads[j]).abs()
        assert bool((err <= 1e-12 * ref.grad_scale[j] + 1e-300).all()), (tag, j, float(err.max()))
        assert bool((ref.grad_scale[j] >= ref.grads[j].abs() * (1 - 1e-12)).all()), (tag, j)    # a scale is never below its value


@pytest.mark.parametrize("tag,sl", [("reg", slice(5, 64)), ("one", slice(7, 8)), ("two", slice(9, 11))])
def test_restatement_agrees_with_the_oracle_on_the_golden_rows(tag, sl):
    gold = dict(np.load(GOLDEN))
    mu, nu, alpha, beta, *_ = O.nig_activations(torch.from_numpy(gold["evidence"]))
    inputs = tuple(t[sl].contiguous() for t in (mu, nu, alpha, beta, torch.from_numpy(gold["targets"])))
    for cfg in (R.LossConfig(), R.LossConfig(reg_w=0.3, kl_w=0.07, ece_w=0.2, cross_w=0.4, task_w=(0.5, 1.0, 2.0))):
        _agree(tag, inputs, cfg)
    # the captured reference values themselves (float32 program): the restatement is within float32 rounding of them
    ref = R.reference(*inputs)
    for k, i in (("valence_total_loss", 0), ("arousal_ece_loss", 9), ("dominance_kl_loss", 13), ("cross_dim_loss", 15), ("total_loss", 16)):
        assert abs(float(gold[f"multitask.{tag}.{k}"]) - float(ref.out[i])) <= 64 * R.ULP * float(ref.out_scale[i]) + 1e-7, (tag, k)


# (conf == 0 exists in float32 only: in float64 that confidence is a tiny positive number of bin 0)
@pytest.mark.parametrize("tag", [t for t in CASES if not t.endswith("conf0")])
def test_restatement_agrees_with_the_oracle_on_the_gpu_cases(tag):
    inputs, cfg, _ = CASES[tag]
    _agree(tag, inputs, cfg)


def test_edge_samples_exist_in_float32():
    edges = R.edge_betas()
    assert [k for k, *_ in edges] == list(range(1, 10))
    two = torch.tensor([2.0], dtype=torch.float32)
    assert float(two - 1 + 1e-8) == 1.0                                    # alpha = 2: the denominator is exactly 1
    for k, b_on, b_below, b_above in edges:
        edge = float(R.EDGES32[k])
        c_on, c_below, c_above = (R._conf_of_beta(x) for x in (b_on, b_below, b_above))
        assert c_on == edge
        assert c_below < edge < c_above
        # the NEAREST attainable confidences: no float32 beta in between gives another one
        for lo, hi, c_far in ((b_on, b_below, c_below), (b_above, b_on, c_above)):
            x = R._next(lo, True)
            while x < hi:
                assert R._conf_of_beta(x) in (edge, c_far)
                x = R._next(x, True)
        assert c_below >= float(torch.nextafter(torch.tensor(edge), torch.tensor(0.0))) - 2 ** -24
        assert c_above <= edge + 2 ** -23
    g, n, a, b, y, expect = R.edge_case(True)
    assert len(expect) == 27 + 3
    conf = R.conf32(a, b)
    m = R.bin_masks(conf)
    for row, k in expect:
        got = int(m[:, row, 0].nonzero()[0]) if bool(m[:, row, 0].any()) else -1
        assert got == k, (row, k, got, float(conf[row, 0]))
    assert float(conf[-3, 0]) == 1.0 and float(a[-3, 0]) == 2.0            # tiny u: bin 9
    assert float(a[-2, 0]) == 1.0 and 0.0 < float(conf[-2, 0]) < 2e-8        # alpha == 1.0f, finite u near 1e8: bin 0
    assert float(conf[-1, 0]) == 0.0 and not bool(m[:, -1, 0].any())         # beta / 1e-8 overflows: no bin
    assert bool(torch.isinf(b[-1, 0] / (a[-1, 0] - 1 + 1e-8)))
    assert float(torch.nn.functional.softplus(torch.tensor(-18.0)) + 1.0) == 1.0   # how a head reaches alpha == 1.0f
    assert bool((conf[-1, 1:] > 0).all())                                    # the other dimensions of that row are ordinary


@pytest.mark.parametrize("tag", list(CASES))
def test_float32_evaluation_passes_with_the_margin_the_constants_were_set_with(tag):
    """K = twice the worst ratio of this comparison over all cases (and not below 8): so every case passes at K / 2."""
    inputs, cfg, regular = CASES[tag]
    ref = _ref(tag)
    out, counts, grads, stats = R.float32_eval(*inputs, cfg)
    R.compare_loss(out, counts, grads, ref, K_LOSS / 2, K_GRAD / 2, tag=tag)
    R.assert_close(f"{tag} sums", stats, ref.sums, ref.sums_scale, K_LOSS / 2)
    # non-finite values: only the one the conf == 0 sample makes (the mean of u of its dimension, hence the reported cross term)
    bad = (~torch.isfinite(ref.out.float())).nonzero().flatten().tolist()
    assert bad == ([15] if tag.endswith("conf0") else []), (tag, bad)
    assert bool(torch.isfinite(ref.grads.float()).all()) and bool(torch.isfinite(grads).all()), tag


def test_conf_zero_sample_carries_no_ece_gradient():
    inputs, cfg, _ = CASES["edges-alone-conf0"]
    with_ece = R.reference(*inputs, R.LossConfig(cross_w=0.0, ece_w=50.0))
    without = R.reference(*inputs, R.LossConfig(cross_w=0.0, ece_w=0.0))
    assert torch.equal(with_ece.grads[2:, -1, 0], without.grads[2:, -1, 0])    # alpha, beta of the conf == 0 sample


SEEDED = [("half_open_left", "edges-alone"), ("half_open_left", "edges-in-300-conf0"),
          ("ece_sign", "cfg-default-B513"), ("ece_sign", "fold-B8193"),
          ("kl_beta_factor", "cfg-default-B513"), ("kl_beta_factor", "cfg-kl_only-B8193"),
          ("cross_third", "cfg-default-B513"), ("cross_third", "cfg-cross_only-B8193"),
          ("no_upper_half", "fold-B257"), ("no_upper_half", "fold-B8193"),
          ("last_partial_twice", "fold-B1"), ("last_partial_twice", "fold-B513"), ("last_partial_twice", "fold-B8193"),
          ("task_w_ignored", "cfg-task_weights-B513"), ("task_w_ignored", "cfg-task_weights-B8193")]


@pytest.mark.parametrize("fault,tag", SEEDED)
def test_every_seeded_error_is_rejected(fault, tag):
    inputs, cfg, regular = CASES[tag]
    ref = _ref(tag)
    R.compare_loss(*R.float32_eval(*inputs, cfg)[:3], ref, K_LOSS, K_GRAD, tag=tag)           # the unmodified evaluation passes
    with pytest.raises(AssertionError):
        R.compare_loss(*R.float32_eval(*inputs, cfg, fault=fault)[:3], ref, K_LOSS, K_GRAD, tag=tag)
    assert set(f for f, _ in SEEDED) == set(R.FAULTS)


def test_seeded_gradient_errors_are_rejected_by_the_gradient_comparison_alone():
    """The faults that sit in the gradient formula only leave loss values and counts untouched: the gradient comparison catches them."""
    for fault, tag in (("ece_sign", "cfg-default-B513"), ("kl_beta_factor", "cfg-default-B513"), ("cross_third", "cfg-default-B513")):
        inputs, cfg, regular = CASES[tag]
        ref = _ref(tag)
        out, counts, grads, _ = R.float32_eval(*inputs, cfg, fault=fault)
        assert torch.equal(counts, ref.counts)
        assert R.worst_ratio(out, ref.out, ref.out_scale) <= K_LOSS
        assert R.worst_ratio(grads, ref.grads, ref.grad_scale) > 100 * K_GRAD, fault


def test_exact_global_statistics_of_the_own_batch_reproduce_the_own_loss():
    inputs, cfg, _ = CASES["fold-B513"]
    own = R.reference(*inputs, cfg)
    gs = torch.cat([own.sums, torch.tensor([513.0], dtype=torch.float64)]).float()
    back = R.reference(*inputs, cfg, global_stats=gs)
    assert R.worst_ratio(back.out, own.out, own.out_scale) <= 4
    assert R.worst_ratio(back.grads, own.grads, own.grad_scale) <= 4
    assert torch.equal(back.counts, own.counts)


def test_head_reference_is_the_chain_rule():
    torch.manual_seed(5)
    B = 37
    evid = (torch.randn(B, 3, 4) * torch.tensor([1.0, 2.0, 3.0, 3.0])).requires_grad_(True)
    e2 = torch.relu(torch.randn(B, 192)).requires_grad_(True)
    w3 = [torch.randn(4, 64).requires_grad_(True) for _ in range(3)]
    y = torch.tanh(torch.randn(B, 3))
    # forward in float64 autograd: evidence = e2 W^T + b -> activations -> the oracle's loss
    E2, W = e2.double(), [w.double() for w in w3]
    bias = [torch.zeros(4, dtype=torch.float64, requires_grad=True) for _ in range(3)]
    ev = torch.stack([E2[:, 64 * i:64 * i + 64] @ W[i].t() + bias[i] for i in range(3)], dim=1)
    ev = ev + (evid.double() - ev).detach()                                   # the stored evidence's values, the product's graph
    sp = torch.nn.functional.softplus
    vals, _ = R.nig_activations64(evid.detach())
    g32 = [v.float() for v in vals]                                           # the float32 activations the kernel would store
    st = lambda v, v32: v + (v32.double() - v).detach()                        # their values, the float64 activation's derivative
    pred = {}
    for i, d in enumerate(O.DIM_NAMES):
        pred[f"{d}_mu"], pred[f"{d}_nu"] = ev[:, i, 0:1], st(sp(ev[:, i, 1:2]) + 1e-6, g32[1][:, i:i + 1])
        pred[f"{d}_alpha"], pred[f"{d}_beta"] = st(sp(ev[:, i, 2:3]) + 1.0, g32[2][:, i:i + 1]), st(sp(ev[:, i, 3:4]) + 1e-6, g32[3][:, i:i + 1])
    O.multitask_loss(pred, y.double())["total_loss"].backward()
    ref = R.reference(*g32, y)
    H = R.head_reference(evid.detach(), e2.detach(), [w.detach() for w in w3], ref.grads, ref.grad_scale, mask_scale=1.0)
    dz_ref = e2.grad.double() * (e2.detach() > 0)                            # the ReLU mask belongs to the kernel's dz2
    assert float((H["dz2"][0] - dz_ref).abs().max()) <= 2e-7 * float(dz_ref.abs().max())     # .grad of a float32 leaf is rounded to float32
    for i in range(3):
        assert float((H["dW3"][0][i] - w3[i].grad.double()).abs().max()) <= 2e-7 * float(w3[i].grad.abs().max())
        assert float((H["db3"][0][i] - bias[i].grad).abs().max()) <= 1e-10 * float(bias[i].grad.abs().max())
    for k in ("dz2", "dW3", "db3"):
        assert bool((H[k][1] >= H[k][0].abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize("B", [129, 1025])
def test_float32_head_evaluation_passes_with_the_margin_the_constants_were_set_with(B):
    """The head cases of the GPU tests on the CPU: the oracle's forward of the model with the spread last layer, the loss and the
    last layer's backward in float32 (64-sample block partials) against the restatement, at K / 2."""
    from mmdeer import synth
    from mmdeer.model import ModelConfig, MultimodalDEER
    m = MultimodalDEER(ModelConfig(compute_dtype="fp32", dropout=0.0, seed=T.MODEL_SEED))
    P = {k: v.detach().clone() for k, v in m.state_dict().items()}
    T.spread_head(P)
    b = {k: torch.from_numpy(v) for k, v in synth.make_batch(B, seed=T.batch_seed(B)).items()}
    with torch.no_grad():
        fused = O.fusion_forward(P, b["audio"], b["video"], b["text"], None, 0.0)["fused_features"]
        h = torch.relu(O._lin(torch.relu(O._lin(fused, P, "head.feature_processor.0")), P, "head.feature_processor.3"))
        e2s, evs = [], []
        for i in range(3):
            pre = f"head.deer_heads.{i}.evidence_net"
            e = torch.relu(O._lin(torch.relu(O._lin(h, P, pre + ".0")), P, pre + ".3"))
            e2s.append(e)
            evs.append(O._lin(e, P, pre + ".6"))
    e2, evid = torch.cat(e2s, dim=1), torch.stack(evs, dim=1)
    vals, scales = R.nig_activations64(evid)
    mu, nu, alpha, beta, *_ = O.nig_activations(evid)
    for got, v, s_ in zip((mu, nu, alpha, beta), vals, scales):
        R.assert_close("activation", got, v, s_, K_LOSS / 2)
    inputs = (mu.contiguous(), nu, alpha, beta, b["targets"])
    ref = R.checked_reference(f"head-B{B}", inputs, R.LossConfig(), True)
    out, counts, grads, stats = R.float32_eval(*inputs, block=64)
    R.compare_loss(out, counts, grads, ref, K_LOSS / 2, K_GRAD / 2)
    R.assert_close("stats", stats, ref.sums, ref.sums_scale, K_LOSS / 2)
    w3 = [P[f"head.deer_heads.{i}.evidence_net.6.weight"] for i in range(3)]
    H = R.head_reference(evid, e2, w3, ref.grads, ref.grad_scale)
    chain = torch.stack([torch.ones(B, 3), *(torch.sigmoid(evid[..., c]) for c in (1, 2, 3))], dim=2)
    dE = grads.permute(1, 2, 0) * chain
    R.assert_close("dz2", torch.cat([dE[:, i] @ w3[i] for i in range(3)], dim=1) * (e2 > 0), *H["dz2"], K_GRAD / 2)
    R.assert_close("dW3", torch.stack([dE[:, i].t() @ e2[:, 64 * i:64 * i + 64] for i in range(3)]), *H["dW3"], K_DW / 2)
    R.assert_close("db3", dE.sum(0), *H["db3"], K_DW / 2)


def test_loss_dictionary_reports_no_ece_without_its_weight():
    """losses.py:118: with ece_weight = 0 the reference does not evaluate the ECE and reports 0; the kernel always computes it."""
    from mmdeer.model import loss_dict_from
    record = torch.arange(20, dtype=torch.float32)
    assert [float(loss_dict_from(record, 5, 0.0)[f"{d}_ece_loss"]) for d in O.DIM_NAMES] == [0.0, 0.0, 0.0]
    assert [float(loss_dict_from(record, 5, 0.05)[f"{d}_ece_loss"]) for d in O.DIM_NAMES] == [4.0, 9.0, 14.0]
    assert float(loss_dict_from(record, 5)["arousal_ece_loss"]) == 9.0
    assert float(loss_dict_from(record, 5, 0.0)["total_loss"]) == 16.0
