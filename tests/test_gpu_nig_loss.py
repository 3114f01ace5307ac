"""The NIG head and MultiTaskDEERLoss kernels (csrc/nig_dev.h, csrc/nig.hip, the prologue and tail of csrc/chain.hip) at their edges
against the float64 restatement of tests/nig_ref.py.

The stand-alone operator mmdeer_nig_loss: every width of compute_finals' fold over the 256-sample block partials (1 block to 65:
empty upper half, halves of unequal length, a second and third batch of 16 clamped loads), every branch of the loss configuration,
confidences on, next to and outside the ECE bin edges, the host classes, the refusals.  The head kernels (nig_fwd_kernel,
nig_bwd_kernel, the chain prologue / tail): one training step on a model whose last head layer is scaled so that the stored evidence
populates all ten bins of every dimension, restated from the kernel's OWN stored inputs (mmdeer_workspace_offset), at every block
count of the 64-sample head kernels; the launch plans bit for bit against each other on that data; the exact-global mode.

Tolerance: |got - ref| <= K * 2^-24 * scale, the scale being the float64 sum of the absolute values of the pieces that form the
value (tests/nig_ref.py).  The constants are twice the worst ratio the SAME formulas in float32 on the CPU show against the
restatement over all cases of this file (never below 8); the factor 2 is for the device's lgammaf / logf / expf and the series
digamma.  Measured on the CPU (float32 torch against the restatement):
    loss values and sums   worst 4.17 (stand-alone cases), 3.17 (head cases)        -> K_LOSS = 9
    gradients, dz2         worst 6.73 (stand-alone cases), 5.55 (head cases)        -> K_GRAD = 14
    dW3 / db3              worst 6.07 (head cases, B = 129)                         -> K_DW   = 13
Worst ratios seen on an MI355X over this file: 5.04 (K_LOSS: the 105 sums at B = 4097), 6.73 (K_GRAD: fold-B8449), 5.12 (K_DW).
Bin counts and stats[105] (the batch size) are exact.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mmdeer import _lib, losses, synth  # noqa: E402
from mmdeer.model import ModelConfig, MultimodalDEER, make_loss_cfg  # noqa: E402
from mmdeer.spec import DIM_NAMES, param_offsets, param_table  # noqa: E402
from oracle import deer_oracle as O  # noqa: E402

from . import nig_ref as R  # noqa: E402

DEV = "cuda:0"
K_LOSS, K_GRAD, K_DW = 9.0, 14.0, 13.0
CASES = {tag: (inputs, cfg, regular) for tag, inputs, cfg, regular in R.loss_cases()}
WORST = {}          # name of a K -> worst ratio seen in this run (printed by the tests, pytest -s)


def _note(kind, log):
    for name, r in log:
        WORST[kind] = max(WORST.get(kind, 0.0), r)
    print("   " + "  ".join(f"{name}: {r:.2f}" for name, r in log) + f"   [worst so far {kind}: {WORST.get(kind, 0.0):.2f}]")


def _cfg(c: R.LossConfig):
    return make_loss_cfg(c.reg_w, c.kl_w, c.ece_w, c.cross_w, c.task_w)


def nig_loss(inputs, cfg: R.LossConfig, want_grads=True, sentinel=None, batch=None):
    """mmdeer_nig_loss through the C ABI: (rc, loss_out [20], bin_counts [30], grads [4, B, 3]) as CPU tensors."""
    lib = _lib.load()
    g, n, a, b, y = (t.to(DEV).contiguous() for t in inputs)
    B = g.shape[0] if batch is None else batch
    stats = torch.empty(max(1, int(lib.mmdeer_nig_stats_elems(max(B, 1)))), dtype=torch.float32, device=DEV)
    fill = float("nan") if sentinel is None else sentinel
    grads = torch.full((4, g.shape[0], 3), fill, dtype=torch.float32, device=DEV)
    out = torch.full((_lib.LOSS_OUT,), fill, dtype=torch.float32, device=DEV)
    bins = torch.full((30,), -7, dtype=torch.int32, device=DEV)
    gp = [grads[i].data_ptr() if want_grads else None for i in range(4)]
    rc = lib.mmdeer_nig_loss(g.data_ptr(), n.data_ptr(), a.data_ptr(), b.data_ptr(), y.data_ptr(), stats.data_ptr(), *gp,
                             out.data_ptr(), bins.data_ptr(), B, C.byref(_cfg(cfg)), _lib.current_stream())
    torch.cuda.synchronize()
    return rc, out.cpu(), bins.cpu(), grads.cpu()


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# =========================================================================== 3. the stand-alone operator
@pytest.mark.parametrize("tag", list(CASES))
def test_nig_loss_operator_against_float64(tag):
    inputs, cfg, regular = CASES[tag]
    ref = R.checked_reference(tag, inputs, cfg, regular)
    rc, out, bins, grads = nig_loss(inputs, cfg)
    assert rc == 0
    log = []
    print(f"\n{tag}: B = {inputs[0].shape[0]}, smallest bin {int(ref.bin_population.min())}, smallest gap {ref.min_gap:.3g}")
    try:
        R.compare_loss(out, bins, grads, ref, K_LOSS, K_GRAD, log, tag)
    finally:
        _note("K_LOSS", [x for x in log if "loss_out" in x[0]])
        _note("K_GRAD", [x for x in log if "gradients" in x[0]])
    # values only (no gradient outputs): the same record
    rc, out_v, bins_v, _ = nig_loss(inputs, cfg, want_grads=False)
    assert rc == 0 and _same_bits(out_v, out) and torch.equal(bins_v, bins)
    # a second call: identical bits
    rc, out2, bins2, grads2 = nig_loss(inputs, cfg)
    assert rc == 0 and _same_bits(out2, out) and torch.equal(bins2, bins) and _same_bits(grads2, grads)


@pytest.mark.parametrize("with_conf0", [True, False])
@pytest.mark.parametrize("mixed", [False, True])
def test_bin_membership_on_next_to_and_outside_the_edges(with_conf0, mixed):
    g, n, a, b, y, expect = R.mixed_edge_case(with_conf0) if mixed else R.edge_case(with_conf0)
    cfg = R.LossConfig(cross_w=0.0) if with_conf0 else R.LossConfig()
    masks = R.bin_masks(R.conf32(a, b))                                    # the float32 CPU masks
    for row, k in expect:                                                  # ... put every edge sample where it was built to go
        assert (int(masks[:, row, 0].nonzero()[0]) if bool(masks[:, row, 0].any()) else -1) == k
    rc, out, bins, grads = nig_loss((g, n, a, b, y), cfg)
    assert rc == 0
    assert torch.equal(bins.view(3, 10).to(torch.int64), masks.sum(1).t().to(torch.int64))
    assert int(bins.view(3, 10)[0].sum()) == g.shape[0] - (1 if with_conf0 else 0)      # conf == 0 is in no bin
    assert bool(torch.isfinite(grads).all())
    if with_conf0:
        row = expect[-1][0]
        assert expect[-1][1] == -1
        # the sample outside every bin carries no ECE gradient: its gradient does not move with the ECE weight
        hi = nig_loss((g, n, a, b, y), R.LossConfig(cross_w=0.0, ece_w=50.0))[3]
        lo = nig_loss((g, n, a, b, y), R.LossConfig(cross_w=0.0, ece_w=0.0))[3]
        assert _same_bits(hi[:, row, 0], lo[:, row, 0]) and _same_bits(grads[:, row, 0], lo[:, row, 0])
        assert not _same_bits(hi[:, row - 1, 0], lo[:, row - 1, 0])         # its neighbour (alpha == 1.0f, bin 0) does carry one
        assert float(out[15]) == float("inf")                              # mean u of dimension 0 is inf: so is the reported cross term


def test_host_deer_loss_on_15000_flattened_elements():
    """losses.DEERLoss on (B, D) = (3000, 5): one dimension of the kernel over 15000 elements (59 blocks)."""
    B, D = 3000, 5
    gen = torch.Generator().manual_seed(11)
    e = torch.randn(B, D, 4, generator=gen) * torch.tensor([1.0, 2.0, 3.0, 3.0])
    mu, nu, alpha, beta, *_ = O.nig_activations(e)
    y = torch.tanh(torch.randn(B, D, generator=gen))
    mod = losses.DEERLoss(reg_weight=0.2, kl_weight=0.03, ece_weight=0.4)
    leaves = [t.clone().to(DEV).requires_grad_(True) for t in (mu, nu, alpha, beta)]
    got = mod({"gamma": leaves[0], "nu": leaves[1], "alpha": leaves[2], "beta": leaves[3]}, y.to(DEV))
    got["total_loss"].backward()
    # the host runs dimension 0 of the multi-task kernel with task weights (3, 0, 0) and no cross term
    three = tuple(t.reshape(-1, 1).expand(-1, 3).contiguous() for t in (mu, nu, alpha, beta, y))
    cfg = R.LossConfig(reg_w=0.2, kl_w=0.03, ece_w=0.4, cross_w=0.0, task_w=(3.0, 0.0, 0.0))
    ref = R.checked_reference("DEERLoss", three, cfg, True)
    log = []
    for key, i in (("total_loss", 16), ("nll_loss", 1), ("reg_loss", 2), ("kl_loss", 3), ("ece_loss", 4)):
        R.assert_close(key, got[key].detach().reshape(1), ref.out[i:i + 1], ref.out_scale[i:i + 1], K_LOSS, log)
    assert got["batch_size"] == B
    _note("K_LOSS", log)
    log = []
    for j, name in enumerate(("gamma", "nu", "alpha", "beta")):
        R.assert_close("d/d" + name, leaves[j].grad.reshape(-1), ref.grads[j].sum(1), ref.grad_scale[j].sum(1), K_GRAD, log)
    _note("K_GRAD", log)
    assert float(losses.DEERLoss(ece_weight=0.0)({"gamma": leaves[0], "nu": leaves[1], "alpha": leaves[2], "beta": leaves[3]},
                                                 y.to(DEV))["ece_loss"]) == 0.0


def test_host_multitask_loss_with_task_weights_and_reports_no_ece_without_its_weight():
    inputs, _, _ = CASES["fold-B513"]
    cfg = R.LossConfig(reg_w=0.2, kl_w=0.03, ece_w=0.4, cross_w=0.3, task_w=(0.5, 1.0, 2.0))
    ref = R.checked_reference("MultiTaskDEERLoss", inputs, cfg, True)
    tw = dict(zip(DIM_NAMES, cfg.task_w))
    mod = losses.MultiTaskDEERLoss(task_weights=tw, cross_dim_weight=cfg.cross_w, reg_weight=cfg.reg_w, kl_weight=cfg.kl_w, ece_weight=cfg.ece_w)
    leaves = [t.clone().to(DEV).requires_grad_(True) for t in inputs[:4]]
    pred = {f"{d}_{k}": leaves[j][:, i:i + 1] for i, d in enumerate(DIM_NAMES) for j, k in enumerate(("mu", "nu", "alpha", "beta"))}
    got = mod(pred, inputs[4].to(DEV))
    got["total_loss"].backward()
    vec = [got[f"{d}_{k}"] for d in DIM_NAMES for k in ("total_loss", "nll_loss", "reg_loss", "kl_loss", "ece_loss")]
    vec += [got["cross_dim_loss"], got["total_loss"], got["nll_loss"], got["evidence_reg"], got["kl_reg"]]
    log = []
    R.assert_close("loss dictionary", torch.stack([v.detach() for v in vec]), ref.out, ref.out_scale, K_LOSS, log)
    assert torch.equal(got["ece_bin_counts"].cpu().to(torch.int64), ref.counts)
    _note("K_LOSS", log)
    log = []
    R.assert_close("gradients", torch.stack([t.grad for t in leaves]), ref.grads, ref.grad_scale, K_GRAD, log)
    _note("K_GRAD", log)
    # ece_weight = 0: the reference does not evaluate the ECE and reports 0 (losses.py:118); the total is the kernel's
    cfg0 = R.LossConfig(ece_w=0.0, task_w=cfg.task_w)
    ref0 = R.reference(*inputs, cfg0)
    got0 = losses.MultiTaskDEERLoss(task_weights=tw, ece_weight=0.0)(pred, inputs[4].to(DEV))
    for d in DIM_NAMES:
        assert float(got0[f"{d}_ece_loss"]) == 0.0
    assert float(ref0.out[4]) > 1e-3                                        # (the kernel's own value is not 0)
    R.assert_close("total without ECE", got0["total_loss"].detach().reshape(1), ref0.out[16:17], ref0.out_scale[16:17], K_LOSS)


def test_refusals_write_nothing():
    lib = _lib.load()
    inputs, cfg, _ = CASES["fold-B2"]
    rc, out, bins, grads = nig_loss(inputs, cfg, sentinel=-123.0, batch=0)          # valid pointers, B = 0
    assert rc == -1 and len(lib.mmdeer_last_error()) > 0
    assert bool((out == -123.0).all()) and bool((bins == -7).all()) and bool((grads == -123.0).all())
    # one gradient pointer of four missing
    g, n, a, b, y = (t.to(DEV) for t in inputs)
    stats = torch.full((int(lib.mmdeer_nig_stats_elems(2)),), -123.0, device=DEV)
    grads = torch.full((4, 2, 3), -123.0, device=DEV)
    out = torch.full((_lib.LOSS_OUT,), -123.0, device=DEV)
    bins = torch.full((30,), -7, dtype=torch.int32, device=DEV)
    for missing in range(4):
        gp = [None if i == missing else grads[i].data_ptr() for i in range(4)]
        rc = lib.mmdeer_nig_loss(g.data_ptr(), n.data_ptr(), a.data_ptr(), b.data_ptr(), y.data_ptr(), stats.data_ptr(), *gp,
                                 out.data_ptr(), bins.data_ptr(), 2, C.byref(_cfg(cfg)), _lib.current_stream())
        assert rc == -1 and b"gradient" in lib.mmdeer_last_error()
    torch.cuda.synchronize()
    assert bool((out == -123.0).all()) and bool((bins == -7).all()) and bool((grads == -123.0).all()) and bool((stats == -123.0).all())


# =========================================================================== 4. the head kernels on their own stored inputs
# A freshly initialised head leaves the evidence near zero (every sample in one or two bins).  The rows of the last layer of head i
# are scaled by HEAD_SCALE[i] and its bias set to HEAD_BIAS[i]: chosen on the CPU with oracle.model_forward (model seed 43, the
# batches of mmdeer.synth) so that the evidence of dimension i is roughly randn * (1, 2, 3, 3) x a per-dimension variation around 0.
HEAD_SCALE = ((14.0, 22.0, 37.0, 29.0), (11.0, 17.0, 32.0, 42.0), (11.0, 26.0, 35.0, 26.0))
HEAD_BIAS = ((-2.0, 1.4, -2.0, 4.5), (-0.8, -2.6, 1.0, -7.0), (-2.9, -1.25, 2.7, -1.4))
MODEL_SEED = 43
# batch seeds at which the reference meets the conditions (every bin populated from B = 255, bin gaps >= 1e-3), searched on the CPU
BATCH_SEED = {129: 43, 2049: 43}


def batch_seed(B):
    return BATCH_SEED.get(B, 42)


def spread_head(state):
    """state: a dict of tensors keyed like the model's state_dict (modified in place)."""
    for i in range(3):
        w = state[f"head.deer_heads.{i}.evidence_net.6.weight"]
        w.mul_(torch.tensor(HEAD_SCALE[i], dtype=w.dtype, device=w.device).view(4, 1))
        state[f"head.deer_heads.{i}.evidence_net.6.bias"].copy_(torch.tensor(HEAD_BIAS[i], dtype=w.dtype, device=w.device))


def spread_model(dtype, dropout, B):
    m = MultimodalDEER(ModelConfig(compute_dtype=dtype, dropout=dropout, seed=MODEL_SEED)).to(DEV).train()
    with torch.no_grad():
        spread_head(dict(m.named_parameters()))
    m.mark_parameters_changed()
    b = synth.make_batch(B, seed=batch_seed(B))
    x = [torch.from_numpy(b[k]).to(DEV) for k in ("audio", "video", "text")]
    if dtype == "bf16":
        x = [t.bfloat16() for t in x]
    return m, x, torch.from_numpy(b["targets"])


def _loss_vector(d):
    vec = [d[f"{dim}_{k}"] for dim in DIM_NAMES for k in ("total_loss", "nll_loss", "reg_loss", "kl_loss", "ece_loss")]
    vec += [d["cross_dim_loss"], d["total_loss"], d["nll_loss"], d["evidence_reg"], d["kl_reg"]]
    return torch.stack([v.detach() for v in vec]).cpu()


def _workspace_reader(m, B, f32):
    lib = _lib.load()
    ws = m._workspace(B, torch.device(DEV))

    def buf(name, shape, dtype):
        off = lib.mmdeer_workspace_offset(B, f32, name.encode())
        assert off >= 0, name
        nbytes = int(np.prod(shape)) * (2 if dtype == torch.bfloat16 else 4)
        return ws[off:off + nbytes].view(dtype).view(*shape).float().cpu()
    return buf, ws


class _OwnStatistics:
    """stats_comm of train_step that exchanges nothing: the step then runs in exact-global mode on the rank's own statistics."""
    active = True

    def __init__(self):
        self.seen = None

    def sum_small(self, t):
        self.seen = t.clone()


def _check_head_step(tag, dtype, dropout, B, options, exact_global=False):
    f32 = int(dtype == "fp32")
    act = torch.float32 if f32 else torch.bfloat16
    m, x, y = spread_model(dtype, dropout, B)
    comm = _OwnStatistics() if exact_global else None
    with _lib.options(**options):
        d = m.train_step(*x, y.to(DEV), stats_comm=comm)
        torch.cuda.synchronize()
        lib = _lib.load()
        buf, ws = _workspace_reader(m, B, f32)
        stats = torch.full((106,), float("nan"), dtype=torch.float32, device=DEV)
        _lib.check(lib.mmdeer_loss_stats(ws.data_ptr(), ws.numel(), B, f32, stats.data_ptr(), _lib.current_stream()))
        torch.cuda.synchronize()
    stats = stats.cpu()
    evid, e2, dz2 = buf("evid", (B, 3, 4), torch.float32), buf("e2", (B, 192), act), buf("dz2", (B, 192), act)
    nig = d["_outputs"]["_nig"].cpu()                                         # [7, B, 3]
    log_l, log_g, log_w = [], [], []
    try:
        # the activations (deer.py:90-93) from the stored evidence, the uncertainties (:96-98) from the stored activations
        vals, scales = R.nig_activations64(evid)
        for j, name in enumerate(("mu", "nu", "alpha", "beta")):
            R.assert_close(f"nig_out {name}", nig[j], vals[j], scales[j], K_LOSS, log_l)
        uv, us = R.uncertainties64(nig[1], nig[2], nig[3])
        for j, name in enumerate(("aleatoric", "epistemic", "total")):
            R.assert_close(f"nig_out {name}", nig[4 + j], uv[j], us[j], K_LOSS, log_l)
        # the loss on the kernel's own float32 activations
        inputs = (nig[0].contiguous(), nig[1].contiguous(), nig[2].contiguous(), nig[3].contiguous(), y)
        gs = stats if exact_global else None
        ref = R.checked_reference(tag, inputs, R.LossConfig(), True, global_stats=gs)
        print(f"\n{tag}: smallest bin {int(ref.bin_population.min())}, smallest gap {ref.min_gap:.3g}, loss {float(ref.out[16]):.4f}")
        R.assert_close("loss dictionary", _loss_vector(d), ref.out, ref.out_scale, K_LOSS, log_l)
        assert torch.equal(d["ece_bin_counts"].cpu().to(torch.int64), ref.counts), tag
        R.assert_close("stats", stats[:105], ref.sums, ref.sums_scale, K_LOSS, log_l)
        assert float(stats[105]) == float(B)
        if exact_global:
            assert _same_bits(comm.seen.cpu(), stats)
        # the last layer's backward
        w3 = [dict(m.named_parameters())[f"head.deer_heads.{i}.evidence_net.6.weight"].detach().cpu() for i in range(3)]
        scale = O.drop_scale(dropout) if dropout > 0 else 1.0
        H = R.head_reference(evid, e2, w3, ref.grads, ref.grad_scale, mask_scale=scale, w3_read=None if f32 else O._bf16_round)
        if f32:
            R.assert_close("dz2", dz2, H["dz2"][0], H["dz2"][1], K_GRAD, log_g)
        else:
            from .test_gpu_bf16_layers import Report
            rep = Report()
            rep.bf16("dz2", dz2, O._bf16_round(H["dz2"][0].float()))
            print("\n".join(rep.rows))
        P = dict(m.named_parameters())
        gw = torch.stack([P[f"head.deer_heads.{i}.evidence_net.6.weight"].grad.detach().cpu() for i in range(3)])
        gb = torch.stack([P[f"head.deer_heads.{i}.evidence_net.6.bias"].grad.detach().cpu() for i in range(3)])
        R.assert_close("dW3", gw, H["dW3"][0], H["dW3"][1], K_DW, log_w)
        R.assert_close("db3", gb, H["db3"][0], H["db3"][1], K_DW, log_w)
    finally:
        _note("K_LOSS", log_l); _note("K_GRAD", log_g); _note("K_DW", log_w)


HEAD_B = (1, 63, 64, 65, 129, 1024, 1025, 2049, 4097)     # 1, 1, 1, 2, 3, 16, 17, 33, 65 blocks of the 64-sample head kernels


@pytest.mark.parametrize("B", HEAD_B)
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_head_kernels_on_their_own_stored_inputs(dtype, B):
    _check_head_step(f"head-{dtype}-B{B}", dtype, 0.0, B, {} if dtype == "fp32" else dict(chain=0))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_head_kernels_with_dropout(dtype):
    """The stored e2 already carries the dropout mask; dz2 is scaled by 1 / 0.7."""
    _check_head_step(f"head-{dtype}-B1025-dropout", dtype, 0.3, 1025, {} if dtype == "fp32" else dict(chain=0))


def test_exact_global_mode_on_the_own_statistics():
    """A rank's own mmdeer_loss_stats vector handed back as global_stats reproduces its loss and gradients to rounding (not bit
    for bit: nig_stats_sum_kernel adds the partials one after the other, compute_finals in a tree)."""
    _check_head_step("head-fp32-B1025-global", "fp32", 0.0, 1025, {}, exact_global=True)


def _plan_step(B, **opts):
    m, x, y = spread_model("bf16", 0.3, B)
    with _lib.options(chain_min=1, **opts):
        d = m.train_step(*x, y.to(DEV))
        torch.cuda.synchronize()
    return _loss_vector(d), d["ece_bin_counts"].cpu().clone(), d["_outputs"]["_nig"].cpu().clone(), m.flat_grad().cpu().clone()


@pytest.mark.parametrize("B", [300, 2049, 8192])
def test_launch_plans_keep_their_bit_for_bit_relations_on_spread_evidence(B):
    """What tests/test_gpu_model.py asserts on near-zero evidence (chain_nig, chain_nigf), with all ten bins of every dimension populated."""
    lo = min(o for (name, _s, _i), o in zip(param_table(), param_offsets()[0]) if ".evidence_net.6." in name)
    base = _plan_step(B, chain_nig=0, chain_nigf=0)
    assert int(base[1].min()) > 0 and int(base[1].sum()) == 3 * B          # every bin of every dimension is populated
    assert bool(torch.isfinite(base[0]).all()) and bool(torch.isfinite(base[3]).all())

    def same_record(a, b):
        assert _same_bits(a[0], b[0]) and torch.equal(a[1], b[1]) and _same_bits(a[2], b[2])

    nig = _plan_step(B, chain_nig=1, chain_nigf=0)                           # the head's backward in the backward chain's prologue
    same_record(nig, base)
    assert _same_bits(nig[3][:lo], base[3][:lo])
    assert not _same_bits(nig[3][lo:], base[3][lo:])                         # the other plan really ran
    rel = (nig[3][lo:].double() - base[3][lo:].double()).norm() / base[3][lo:].double().norm()
    assert float(rel) < 1e-5, float(rel)                                    # dW3 / db3: other partial blocks
    nigf = _plan_step(B, chain_nigf=1, chain_nig=1)                          # the head as the forward chain's tail
    same_record(nigf, nig)
    assert _same_bits(nigf[3], nig[3])
    nigf0 = _plan_step(B, chain_nigf=1, chain_nig=0)                         # ... with the stand-alone backward reading wave partials
    same_record(nigf0, base)
    assert _same_bits(nigf0[3], base[3])
