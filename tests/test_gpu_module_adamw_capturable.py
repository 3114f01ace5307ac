"""ModuleAdamW(capturable=True) / mmdeer_adamw_multi_dev (include/mmdeer_graph.h) on the GPU: three steps against the float64
restatement (tests/optim_multi_ref.py, optim_ref.K's factors -- POW_ULPS already allows for the power in the bias corrections, and
tests/test_cpu_train_graph.py holds the device's power to it), the device step counts, an lr changed between steps, state_dict moves
to torch.optim.AdamW and to a non-capturable ModuleAdamW and back, and a HIP graph of step() alone against eager steps, bit for bit.

Tensors: 1, 5, 1025 and 2051 elements, each one element into a larger buffer (4-byte, not 16-byte aligned: the head / tail path and
the chunk boundary at 1024), and 130 small tensors, dealt to two groups: 134 records are three batches of the table-writing kernel.
The distance between the capturable and the non-capturable step is measured and printed, not asserted: both are held to float64."""
import copy

import numpy as np
import pytest
import torch

from mmdeer import _lib
from mmdeer.optim import ModuleAdamW

from . import optim_multi_ref as R
from .test_gpu_module_adamw import BETAS, EPS32, held_to_torch, snapshot

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES = [1, 5, 1025, 2051] + [1 + (37 * i) % 70 for i in range(130)]
LR, WD = (1e-3, 2.5e-4), (0.01, 0.0)
MAXN = 0.5


def make_params(seed=0):
    gen = torch.Generator().manual_seed(seed)
    P, keep = [], []
    for i, n in enumerate(SIZES):
        if i < 4:                                       # an odd start
            buf = torch.randn(n + 8, generator=gen).to(DEV)
            keep.append(buf)
            P.append(torch.nn.Parameter(buf[1:1 + n]))
            assert P[-1].data_ptr() % 16 == 4
        else:
            P.append(torch.nn.Parameter(torch.randn(n, generator=gen).to(DEV)))
    return P, keep


def clones(P):
    """the same values at the same alignment"""
    out = []
    for i, p in enumerate(P):
        if i < 4:
            out.append(torch.nn.Parameter(torch.cat([torch.zeros(1, device=DEV), p.detach(), torch.zeros(7, device=DEV)])[1:1 + p.numel()]))
        else:
            out.append(torch.nn.Parameter(p.detach().clone()))
    return out


def groups_of(P, lr=LR):
    return [{"params": P[c::2], "lr": lr[c], "weight_decay": WD[c]} for c in range(2)]


def group_of(i):
    return i % 2


def draw_grads(seed):
    gen = torch.Generator().manual_seed(1000 + seed)
    return [(torch.randn(n, generator=gen) * 10.0 ** torch.empty(n).uniform_(-6, 1, generator=gen)).to(DEV) for n in SIZES]


def give(P, G):
    """the values of G into the gradients of P, in place where they exist (their addresses stay)"""
    for p, g in zip(P, G):
        if p.grad is None:
            p.grad = g.clone()
        else:
            p.grad.copy_(g)


def state_of(opt, P):
    return [(p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()) for p in P]


def against_float64(tag, before, G, after, norm, lrs, step):
    T = [{"p": b[0].double().cpu().numpy(), "m": b[1].double().cpu().numpy(), "v": b[2].double().cpu().numpy(), "g": g.double().cpu().numpy(),
          "cls": group_of(i), "skip": False} for i, (b, g) in enumerate(zip(before, G))]
    classes = [(R.f32(lrs[c]), R.f32(WD[c]), step) for c in range(2)]
    ref = R.adamw_multi_ref(T, classes, R.BETA1, R.BETA2, R.EPS, MAXN, 1.0, norm=norm)
    got = {"norm": norm, "tensors": [{"p": a[0].cpu().numpy(), "exp_avg": a[1].cpu().numpy(), "exp_avg_sq": a[2].cpu().numpy()} for a in after]}
    worst = R.ratios(got, ref)
    print(f"\n  {tag}: " + "  ".join(f"{f} {x:.3f} (K {R.K[f]})" for f, x in worst.items()), end="")
    for f, x in worst.items():
        assert x <= R.K[f], (tag, f, x)
    return ref


def test_three_capturable_steps_against_float64_and_the_device_step_count():
    lib = _lib.load()
    P, _ = make_params()
    Q = clones(P)
    opt = ModuleAdamW(groups_of(P), betas=BETAS, eps=EPS32, max_grad_norm=MAXN, capturable=True)
    plain = ModuleAdamW(groups_of(Q), betas=BETAS, eps=EPS32, max_grad_norm=MAXN)
    lrs = list(LR)
    blocking, uploads, dev_uploads = lib.mmdeer_adamw_multi_blocking_calls(), lib.mmdeer_adamw_multi_uploads(), lib.mmdeer_adamw_multi_dev_uploads()
    for step in (1, 2, 3):
        if step == 3:                                   # an lr changed through param_groups between steps is the one used
            lrs[0] = 4e-3
            opt.param_groups[0]["lr"] = plain.param_groups[0]["lr"] = 4e-3
        G = draw_grads(step)
        give(P, G)
        give(Q, G)
        z = [(p.detach().clone(), torch.zeros_like(p), torch.zeros_like(p)) for p in P]
        before = state_of(opt, P) if step > 1 else z
        versions = [p._version for p in P]
        norm = opt.step()
        assert norm is opt.last_grad_norm and float(norm) > MAXN                     # the clip is live
        after = state_of(opt, P)
        against_float64(f"capturable step {step}", before, G, after, float(norm), lrs, step)
        assert all(p._version > v for p, v in zip(P, versions))
        for p in P:
            s = opt.state[p]["step"]
            assert s.is_cuda and s.dim() == 0 and int(s) == step                     # a device scalar that reads 1, 2, 3
        assert opt.class_buffer[:, 2].tolist() == [step, step]
        # the non-capturable step from the same state and gradients: the distance is the power's last bit, measured here
        plain.step()
        other = state_of(plain, Q)
        ndiff = sum(int((a[0] != b[0]).sum()) for a, b in zip(after, other))
        worst = max(float(((a[0] - b[0]).abs() / b[0].abs().clamp_min(1e-30)).max()) for a, b in zip(after, other))
        assert all(torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) for a, b in zip(after, other)), "the moments do not see the bias corrections"
        print(f"\n  step {step}: capturable vs non-capturable parameters differ in {ndiff} of {sum(SIZES)} elements, worst relative {worst:.3e}", end="")
        for p, q in zip(P, Q):                         # keep the two on one trajectory: each step is compared from the same start
            q.data.copy_(p.data)
    assert opt.table_uploads == 1 and lib.mmdeer_adamw_multi_dev_uploads() == dev_uploads + 1
    assert lib.mmdeer_adamw_multi_uploads() == uploads + 1                           # the non-capturable twin's one upload ...
    assert lib.mmdeer_adamw_multi_blocking_calls() == blocking + 1                   # ... and its wait; the capturable step made none


def test_state_dict_moves_to_torch_and_to_the_non_capturable_optimiser_and_back():
    P, _ = make_params(1)
    opt = ModuleAdamW(groups_of(P), betas=BETAS, eps=EPS32, max_grad_norm=MAXN, capturable=True)
    for step in (1, 2):
        give(P, draw_grads(10 + step))
        opt.step()
    group = [(LR[group_of(i)], WD[group_of(i)]) for i in range(len(P))]

    def both(tag, seed, a_opt, a_P, b_opt, b_P, step, b_is_torch):
        G = draw_grads(seed)
        give(a_P, G)
        give(b_P, G)
        before, mom = [p.detach().clone() for p in a_P], [(m, v) for _, m, v in snapshot(a_opt, a_P)]
        norm = a_opt.step()
        if b_is_torch:
            torch.nn.utils.clip_grad_norm_(b_P, MAXN)
        b_opt.step()
        held_to_torch(tag, snapshot(a_opt, a_P), snapshot(b_opt, b_P), before, G, mom, group, [step] * len(a_P), float(norm), MAXN)

    sd = opt.state_dict()
    assert all(float(st["step"]) == 2.0 and not st["step"].is_cuda for st in sd["state"].values())       # torch.optim.AdamW's format
    Q = clones(P)
    theirs = torch.optim.AdamW(groups_of(Q), betas=BETAS, eps=EPS32)
    theirs.load_state_dict(copy.deepcopy(sd))
    both("capturable -> torch, one more step", 21, opt, P, theirs, Q, 3, True)
    assert all(int(st["step"]) == 3 for st in theirs.state.values()) and int(opt.state[P[0]]["step"]) == 3
    P2 = clones(P)
    plain = ModuleAdamW(groups_of(P2), betas=BETAS, eps=EPS32, max_grad_norm=MAXN)
    plain.load_state_dict(copy.deepcopy(opt.state_dict()))
    both("capturable -> non-capturable, one more step", 22, opt, P, plain, P2, 4, False)
    P3 = clones(P2)
    again = ModuleAdamW(groups_of(P3), betas=BETAS, eps=EPS32, max_grad_norm=MAXN, capturable=True)
    again.load_state_dict(copy.deepcopy(plain.state_dict()))
    both("non-capturable -> capturable, one more step", 23, again, P3, plain, P2, 5, False)
    assert again.class_buffer[:, 2].tolist() == [5, 5] and int(again.state[P3[3]]["step"]) == 5
    assert all(float(st["step"]) == 5.0 for st in again.state_dict()["state"].values())
    # from torch into the capturable one
    P4 = clones(Q)
    last = ModuleAdamW(groups_of(P4), betas=BETAS, eps=EPS32, max_grad_norm=MAXN, capturable=True)
    last.load_state_dict(copy.deepcopy(theirs.state_dict()))
    both("torch -> capturable, one more step", 24, last, P4, theirs, Q, 4, True)
    assert last.class_buffer[:, 2].tolist() == [4, 4]


def test_a_graph_of_step_replayed_three_times_is_three_eager_steps():
    lib = _lib.load()
    P, _ = make_params(2)
    Q = clones(P)
    opt = ModuleAdamW(groups_of(P), betas=BETAS, eps=EPS32, max_grad_norm=MAXN, capturable=True)
    eager = ModuleAdamW(groups_of(Q), betas=BETAS, eps=EPS32, max_grad_norm=MAXN, capturable=True)
    start = [p.detach().clone() for p in P]
    snap = opt.snapshot()
    give(P, draw_grads(30))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        opt.step()                                      # the warm-up: buffers, device records, table
    torch.cuda.current_stream().wait_stream(side)
    with torch.no_grad():
        for p, s in zip(P, start):
            p.copy_(s)
    opt.restore(snap)
    assert opt.class_buffer[:, 2].tolist() == [0, 0] and not opt.state
    for p in P:
        p.grad = p.grad.clone()                         # static gradients at NEW addresses: the captured step must upload the table
    torch.cuda.synchronize()
    counts = lambda: (lib.mmdeer_adamw_multi_uploads(), lib.mmdeer_adamw_multi_blocking_calls(), lib.mmdeer_adamw_multi_dev_uploads())      # noqa: E731
    before = counts()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        norm = opt.step()
    after = counts()
    assert after[:2] == before[:2], "a copy or a wait inside the capture"
    assert after[2] == before[2] + 1, "the captured step did not upload the table"
    assert opt.class_buffer[:, 2].tolist() == [0, 0]    # recorded, not run
    norms = []
    for r in range(3):
        G = draw_grads(31 + r)
        give(P, G)
        give(Q, G)
        if r == 2:                                      # an LR scheduler between replays
            opt.param_groups[1]["lr"] = eager.param_groups[1]["lr"] = 1e-2
            opt.refresh_hyper()
        graph.replay()
        norms.append((float(norm), float(eager.step())))
    assert all(a == b for a, b in norms), norms
    assert opt.class_buffer[:, 2].tolist() == eager.class_buffer[:, 2].tolist() == [3, 3]
    for i, (p, q) in enumerate(zip(P, Q)):
        assert torch.equal(p, q), f"parameter {i} ({SIZES[i]} elements)"
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(opt.state[p][k], eager.state[q][k]), (i, k)
    assert not np.array_equal(P[3].detach().cpu().numpy(), start[3].cpu().numpy())
