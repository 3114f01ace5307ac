"""mmdeer_adamw_multi and optim.ModuleAdamW on the GPU.

1. the entry itself on the cases of tests/optim_multi_ref.py (tensor sizes around the 1024-element chunk, odd starts, 130 small tensors
   in two classes, 300,000 elements, more chunks than either grid has blocks): p, exp_avg, exp_avg_sq and the norm within K of the
   float64 restatement (the clip teacher-forced with the kernel's own norm); skipped tensors, their moments and every canary element
   around a parameter, a moment range and a mirror exactly as they were; mirrors exactly the rounded parameter; a second run from the
   same state bit-equal, and with unchanged pointers without another table upload
2. ModuleAdamW against clip_grad_norm_ + torch.optim.AdamW on a CUDA copy, version counters, state_dict in both directions
3. BertEncoder: after a step of ModuleAdamW.for_module the packed operands are the same objects, equal to a fresh encoder's pack of
   the updated parameters, and four steps lower the loss of the text encoder's end-to-end case
4. DEERTrainer with module_optimizer on a ComposedDEER"""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mmdeer import _lib, bert, head, synth, text  # noqa: E402
from mmdeer.model import HierarchicalMultimodalFusion  # noqa: E402
from mmdeer.optim import ModuleAdamW  # noqa: E402

from . import optim_multi_ref as R  # noqa: E402
from .test_cpu_bert import TINY, golden  # noqa: E402
from .test_gpu_bert import BIG, big_model  # noqa: E402

DEV = "cuda:0"
PAD = 4                      # canary elements on each side of every tensor (a multiple of 4: the heads are what the layout says)
CAN_P, CAN_M, CAN_V, CAN_F32 = 7.25, 5.0, 6.0, 9.5
CAN_BF16 = 0x5AA5            # no plausible bf16 value of the data (~ 2.3e16)


# ================================================================================================ 1. the entry
class Harness:
    """One case in device buffers: every tensor inside one buffer per stream with canaries around it.  The gradient buffer's canaries
    (and the gradients of skipped tensors) are NaN: a read outside the listed tensors poisons the norm."""

    def __init__(self, name):
        self.tensors, self.classes, self.hyper, _ = R.case_inputs(name)
        cur, self.off, self.goff = PAD, [], []
        for t in self.tensors:
            n = len(t["p"])
            self.off.append(cur + t["head"])
            self.goff.append(cur + t["ghead"])
            cur = (cur + max(t["head"], t["ghead"]) + n + 3) // 4 * 4 + PAD
        self.total = cur
        host = {"p": np.full(cur, CAN_P, np.float32), "g": np.full(cur, np.nan, np.float32), "m": np.full(cur, CAN_M, np.float32),
                "v": np.full(cur, CAN_V, np.float32), "f32": np.full(cur, CAN_F32, np.float32), "bf16": np.full(cur, CAN_BF16, np.uint16)}
        for t, o, go in zip(self.tensors, self.off, self.goff):
            n = len(t["p"])
            host["p"][o:o + n], host["m"][o:o + n], host["v"][o:o + n] = t["p"], t["m"], t["v"]
            if not t["skip"]:
                host["g"][go:go + n] = t["g"]
        self.host = host
        self.dev = {k: torch.from_numpy(v.view(np.int16) if k == "bf16" else v).to(DEV) for k, v in host.items()}
        self.live = [i for i, t in enumerate(self.tensors) if not t["skip"]]
        rec = (_lib.AdamWMultiTensor * len(self.live))()
        for r, i in zip(rec, self.live):
            t, o = self.tensors[i], self.off[i]
            r.param, r.grad = self.dev["p"].data_ptr() + 4 * o, self.dev["g"].data_ptr() + 4 * self.goff[i]
            r.count, r.moment_off, r.cls = len(t["p"]), o, t["cls"]
            if t["mirror"] == "bf16":
                r.mirror, r.mirror_f32 = self.dev["bf16"].data_ptr() + 2 * o, 0
            elif t["mirror"] == "f32":
                r.mirror, r.mirror_f32 = self.dev["f32"].data_ptr() + 4 * o, 1
        self.rec = rec
        lib = _lib.load()
        self.table = torch.empty(lib.mmdeer_adamw_multi_table_bytes(rec, len(rec)), dtype=torch.uint8, device=DEV)
        self.scratch = torch.full((R.NPART,), float("nan"), device=DEV)
        self.norm = torch.zeros((), device=DEV)

    def reset(self):
        for k, v in self.host.items():
            self.dev[k].copy_(torch.from_numpy(v.view(np.int16) if k == "bf16" else v))

    def run(self, upload):
        lib = _lib.load()
        a = _lib.AdamWMultiArgs()
        a.tensors, a.ntensors, a.nclasses = self.rec, len(self.rec), len(self.classes)
        for c, (lr, wd, step) in enumerate(self.classes):
            a.classes[c].lr, a.classes[c].weight_decay, a.classes[c].step = lr, wd, step
        a.exp_avg, a.exp_avg_sq, a.moment_elems = self.dev["m"].data_ptr(), self.dev["v"].data_ptr(), self.total
        a.table, a.table_bytes, a.upload = self.table.data_ptr(), self.table.numel(), int(upload)
        a.scratch, a.grad_norm = self.scratch.data_ptr(), self.norm.data_ptr()
        h = self.hyper
        a.beta1, a.beta2, a.eps, a.max_grad_norm, a.grad_scale = h["beta1"], h["beta2"], h["eps"], h["max_norm"], h["grad_scale"]
        a.stream = _lib.current_stream()
        before = lib.mmdeer_adamw_multi_uploads()
        _lib.check(lib.mmdeer_adamw_multi(C.byref(a)))
        torch.cuda.synchronize()
        out = {k: (v.cpu().numpy().view(np.uint16) if k == "bf16" else v.cpu().numpy()) for k, v in self.dev.items()}
        out["norm"] = float(self.norm)
        return out, lib.mmdeer_adamw_multi_uploads() - before


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32 if x.dtype == np.float32 else np.uint16)


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_entry_against_float64(name):
    assert _lib.OPTIM_CONSTANTS["ADAMW_MULTI_CHUNK"] == R.CHUNK and _lib.OPTIM_CONSTANTS["ADAMW_MULTI_SCRATCH"] == R.NPART
    H = Harness(name)
    got, uploads = H.run(upload=True)
    assert uploads == 1
    ref = R.adamw_multi_ref(H.tensors, H.classes, **H.hyper, norm=got["norm"])
    per = [{"p": got["p"][o:o + len(t["p"])], "exp_avg": got["m"][o:o + len(t["p"])], "exp_avg_sq": got["v"][o:o + len(t["p"])]}
           for t, o in zip(H.tensors, H.off)]
    r = R.ratios({"norm": got["norm"], "tensors": per}, ref)
    print(f"\n  {name}: " + "  ".join(f"{f} {x:.3f} (K {R.K[f]})" for f, x in r.items()) + f"  norm {got['norm']:.9g} (float64 {ref['norm']:.9g})", end="")
    for f, x in r.items():
        assert x <= R.K[f], (name, f, x)
    # exact: everything outside the listed tensors is as it was -- canaries, skipped tensors and their moments, the gradients
    expect = {k: v.copy() for k, v in H.host.items()}
    for i in H.live:
        t, o, n = H.tensors[i], H.off[i], len(H.tensors[i]["p"])
        for k in ("p", "m", "v"):
            expect[k][o:o + n] = got[k][o:o + n]
        if t["mirror"] == "bf16":
            expect["bf16"][o:o + n] = R.bf16_rne(got["p"][o:o + n])          # what p.to(torch.bfloat16) stores
            assert torch.equal(torch.from_numpy(got["p"][o:o + n].copy()).to(torch.bfloat16).view(torch.int16),
                               torch.from_numpy(got["bf16"][o:o + n].view(np.int16).copy())), (name, i)
        elif t["mirror"] == "f32":
            expect["f32"][o:o + n] = got["p"][o:o + n]
    for k in expect:
        assert np.array_equal(bits(got[k]), bits(expect[k])), (name, k, np.flatnonzero(bits(got[k]) != bits(expect[k]))[:8])
    for i, t in enumerate(H.tensors):                                       # a live tensor did move
        if not t["skip"] and len(t["p"]) > 8:
            assert not np.array_equal(got["p"][H.off[i]:H.off[i] + len(t["p"])], t["p"]), (name, i)
    # the same state again, the pointers unchanged: no upload, the same bits
    H.reset()
    again, uploads = H.run(upload=False)
    assert uploads == 0
    assert again["norm"] == got["norm"] and all(np.array_equal(bits(again[k]), bits(got[k])) for k in expect), name


# ================================================================================================ 2. ModuleAdamW
# The C ABI takes betas and eps as float32.  torch forms 1 - beta in double: from the DEFAULT betas that is 0.001 where the library's
# 1.f - 0.999f is 0.00099998712 -- 1.3e-5 apart, a property of the ABI's number format and not of the kernel -- so both optimisers get
# the float32 values the library receives (1 - beta is then exact in either arithmetic).
BETAS, EPS32 = (R.f32(R.BETA1), R.f32(R.BETA2)), R.f32(R.EPS)


def module_params(seed=0):
    """two matrices, a scalar, a view one element into a larger buffer, a vector; the last one gets no gradient"""
    gen = torch.Generator().manual_seed(seed)
    buf = torch.randn(1200, generator=gen).to(DEV)
    P = [torch.nn.Parameter(torch.randn(33, 7, generator=gen).to(DEV)), torch.nn.Parameter(torch.randn(1, generator=gen).to(DEV)),
         torch.nn.Parameter(buf[1:1 + 1030]), torch.nn.Parameter(torch.randn(2 * R.CHUNK + 3, generator=gen).to(DEV)),
         torch.nn.Parameter(torch.randn(17, generator=gen).to(DEV))]
    assert P[2].data_ptr() % 16 == 4
    return P, buf


def groups_of(P):
    return [{"params": [P[0], P[2]], "lr": 1e-3, "weight_decay": 0.01}, {"params": [P[1], P[3], P[4]], "lr": 2.5e-4, "weight_decay": 0.0}]


def set_grads(P, seed, skip=(4,)):
    gen = torch.Generator().manual_seed(seed)
    for i, p in enumerate(P):
        p.grad = None if i in skip else (torch.randn(p.shape, generator=gen) * 10.0 ** torch.empty(p.shape).uniform_(-6, 1, generator=gen)).to(DEV)


def held_to_torch(tag, mine, theirs, before, grads, moments, group, steps, norm, max_norm, grad_scale=1.0, families=R.FAMILIES):
    """|mine - torch| <= K * U * magnitude, the magnitudes from the float64 restatement of this very step"""
    keys = {}
    T = []
    for i, (b, g) in enumerate(zip(before, grads)):
        m, v = moments[i]
        t = {"p": b.double().cpu().numpy().ravel(), "m": m.double().cpu().numpy().ravel(), "v": v.double().cpu().numpy().ravel(), "skip": g is None,
             "g": np.zeros(b.numel()) if g is None else g.double().cpu().numpy().ravel(), "cls": 0}
        if g is not None:
            t["cls"] = keys.setdefault((group[i][0], group[i][1], steps[i]), len(keys))
        T.append(t)
    ref = R.adamw_multi_ref(T, [(lr, wd, s) for lr, wd, s in keys], R.BETA1, R.BETA2, R.EPS, max_norm, grad_scale, norm=norm)
    worst = {}
    for i, rt in enumerate(ref["tensors"]):
        for f, a, b in (("p", mine[i][0], theirs[i][0]), ("exp_avg", mine[i][1], theirs[i][1]), ("exp_avg_sq", mine[i][2], theirs[i][2])):
            if f in families:
                x = R.ratio(a.double().cpu().numpy().ravel(), b.double().cpu().numpy().ravel(), rt["mag_" + f])
                worst[f] = max(worst.get(f, 0.0), x)
    print(f"\n  {tag}: ModuleAdamW against torch " + "  ".join(f"{f} {x:.3f} (K {R.K[f]})" for f, x in worst.items()), end="")
    for f, x in worst.items():
        assert x <= R.K[f], (tag, f, x)


def snapshot(opt, P):
    z = lambda p: torch.zeros_like(p)                      # noqa: E731
    return [(p.detach().clone(), opt.state[p]["exp_avg"].clone() if "exp_avg" in opt.state.get(p, {}) else z(p),
             opt.state[p]["exp_avg_sq"].clone() if "exp_avg_sq" in opt.state.get(p, {}) else z(p)) for p in P]


def test_module_adamw_against_torch_and_state_dict_round_trips():
    MAXN = 0.5
    P, _ = module_params()
    Q = [torch.nn.Parameter(p.detach().clone()) for p in P]
    mine, ref = ModuleAdamW(groups_of(P), betas=BETAS, eps=EPS32, max_grad_norm=MAXN), torch.optim.AdamW(groups_of(Q), betas=BETAS, eps=EPS32)
    group = [(1e-3, 0.01), (2.5e-4, 0.0), (1e-3, 0.01), (2.5e-4, 0.0), (2.5e-4, 0.0)]
    steps = [1, 1, 1, 1, 1]

    def both(seed, skip, tag, a_opt, a_P, b_opt, b_P):
        """one step of a_opt (a ModuleAdamW) on a_P and of b_opt (torch) on b_P from the same gradients"""
        set_grads(a_P, seed, skip)
        for p, q in zip(a_P, b_P):
            q.grad = None if p.grad is None else p.grad.clone()
        before, grads = [p.detach().clone() for p in a_P], [None if p.grad is None else p.grad.clone() for p in a_P]
        mom = [(m, v) for _, m, v in snapshot(a_opt, a_P)]
        versions = [p._version for p in a_P]
        norm = a_opt.step()
        tn = torch.nn.utils.clip_grad_norm_(b_P, MAXN)
        b_opt.step()
        assert norm is a_opt.last_grad_norm and norm.device.type == "cuda" and float(norm) == pytest.approx(float(tn), rel=1e-6)
        assert float(norm) > MAXN                                                    # the clip is live
        for i, p in enumerate(a_P):
            assert (p._version > versions[i]) == (i not in skip), i                  # advanced where updated, and only there
            if i in skip:
                assert torch.equal(p, before[i])
        held_to_torch(tag, snapshot(a_opt, a_P), snapshot(b_opt, b_P), before, grads, mom, group, steps, float(norm), MAXN)
        for i in range(len(a_P)):
            steps[i] += i not in skip

    both(1, (4,), "step 1", mine, P, ref, Q)
    assert mine.table_uploads == 1 and P[4] not in mine.state_dict()["state"] and len(mine.state_dict()["state"]) == 4
    assert [p.grad.data_ptr() for p in P[:4]] and mine.step() is not None and mine.table_uploads == 1      # the same gradients again: nothing uploaded
    ref.step()                                                                       # (keeps the two in step; Q's gradients are still the clipped ones)
    steps = [3, 3, 3, 3, 1]                                                          # the step each parameter takes next
    # torch -> ModuleAdamW -> one more step, against torch going on; parameter 4 joins: a class of its own (step 1 beside step 3)
    P2 = [torch.nn.Parameter(q.detach().clone()) for q in Q]
    P2[2] = torch.nn.Parameter(torch.cat([torch.zeros(1, device=DEV), Q[2].detach()])[1:])       # again one element into a buffer
    loaded = ModuleAdamW(groups_of(P2), betas=BETAS, eps=EPS32, max_grad_norm=MAXN)
    loaded.load_state_dict(ref.state_dict())
    both(2, (), "torch -> ModuleAdamW, one more step", loaded, P2, ref, Q)
    assert int(loaded.state_dict()["state"][0]["step"]) == 3 and int(loaded.state_dict()["state"][4]["step"]) == 1
    # ModuleAdamW -> torch -> one more step, against ModuleAdamW going on
    Q3 = [torch.nn.Parameter(p.detach().clone()) for p in P2]
    back = torch.optim.AdamW(groups_of(Q3), betas=BETAS, eps=EPS32)
    # (a copy, as a checkpoint file is: torch's load_state_dict keeps tensors that already have the parameter's dtype and device, and
    # the two optimisers must not share their moments here)
    back.load_state_dict(copy.deepcopy(loaded.state_dict()))
    both(3, (1,), "ModuleAdamW -> torch, one more step", loaded, P2, back, Q3)
    assert int(back.state[Q3[0]]["step"]) == 4 and int(back.state[Q3[1]]["step"]) == 3            # the skipped one stays a step behind


def test_a_reallocated_gradient_uploads_the_table_again_and_noncontiguous_gradients_raise():
    P, _ = module_params(3)
    opt = ModuleAdamW(P, lr=1e-3)
    set_grads(P, 5, ())
    opt.step()
    opt.step()
    assert opt.table_uploads == 1
    keep = P[0].grad                                        # held, so that the new one cannot land on its address
    P[0].grad = keep.clone()
    opt.step()
    assert opt.table_uploads == 2
    P[3].grad = None                                        # another set of parameters has gradients
    opt.step()
    assert opt.table_uploads == 3
    P[0].grad = torch.randn(7, 33, device=DEV).t()
    before = P[0].detach().clone()
    with pytest.raises(RuntimeError, match="contiguous"):
        opt.step()
    assert torch.equal(P[0], before)
    half = torch.nn.Parameter(torch.randn(8, device=DEV, dtype=torch.float16))
    o2 = ModuleAdamW([half])
    half.grad = torch.zeros_like(half)
    with pytest.raises(RuntimeError, match="fp32"):
        o2.step()


# ================================================================================================ 3. BertEncoder
def bert_case(which):
    if which == "tiny":
        sd, ids, mask, typ, _ = golden()
        return TINY, sd, ids[:2], mask[:2], typ[:2], 128
    sd, ids, mask, _ = big_model()
    return BIG, sd, ids[:2], mask[:2], None, 768


def make_encoder(config, sd, compute, k):
    enc = bert.BertEncoder(config, compute_dtype=compute, finetune_layers=k)
    enc.load_state_dict({n: v.float() for n, v in sd.items()}, strict=True)
    return enc.to(DEV)


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
@pytest.mark.parametrize("which,k", [("tiny", 1), ("tiny", 2), ("big", 1), ("big", 2)])
def test_bert_operands_are_written_by_the_step(which, k, compute):
    config, sd, ids, mask, typ, H = bert_case(which)
    assert tuple(ids.shape) == (2, 37)
    ids, mask, typ = ids.to(DEV), mask.to(DEV), None if typ is None else typ.to(DEV)
    enc = make_encoder(config, sd, compute, k)
    nl = config["num_hidden_layers"]
    opt = ModuleAdamW.for_module(enc, lr=1e-3, weight_decay=0.01, max_grad_norm=1.0)
    mirrors = enc.operand_mirrors()
    assert len(mirrors) == 16 * k and set(map(id, mirrors)) == {id(p) for p in enc.parameters() if p.requires_grad}
    gen = torch.Generator().manual_seed(2)
    up = torch.randn(2, 37, H, generator=gen).to(DEV)
    (enc(ids, mask, typ).last_hidden_state.float() * up).sum().backward()
    packed = enc._operands()
    ptrs = [{n: t.data_ptr() for n, t in lyr.items()} for lyr in packed["layers"]]
    old = [{n: t.clone() for n, t in lyr.items()} for lyr in packed["layers"]]
    versions = {n: p._version for n, p in enc.named_parameters()}
    opt.step()
    after = enc._operands()
    assert after is packed and after["emb"] is packed["emb"]                        # no rebuild: the same object ...
    assert all(a is b for a, b in zip(after["layers"], packed["layers"]))           # ... the frozen layers' entries included
    assert [{n: t.data_ptr() for n, t in lyr.items()} for lyr in after["layers"]] == ptrs
    for n, p in enc.named_parameters():
        assert (p._version > versions[n]) == p.requires_grad, n
    fresh = make_encoder(config, enc.state_dict(), compute, k)                      # packs the updated parameters from scratch
    want = fresh._operands()
    for li in range(nl):
        for n, t in after["layers"][li].items():
            assert t.dtype == want["layers"][li][n].dtype and torch.equal(t, want["layers"][li][n]), (li, n)
            assert torch.equal(t, old[li][n]) == (li < nl - k), (li, n)             # the tail moved, the frozen layers did not
    with torch.no_grad():
        assert torch.equal(enc(ids, mask, typ).last_hidden_state, fresh(ids, mask, typ).last_hidden_state)
    assert enc._operands() is packed and opt.table_uploads == 1


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_text_encoder_trains_the_trunks_tail_with_module_adamw(compute):
    """test_gpu_bert_backward's end-to-end case (TemporalTextEncoder over a one-layer trunk of width 768, B = 3, L = 9, eval mode) with
    ModuleAdamW.for_module on the trunk's tail in place of plain SGD: four steps lower the loss every time.  Adam moves every element
    by about lr per step whatever the gradient's size; lr = 2e-5 is 1/1800 of a weight's spread (768^-0.5), small enough for the
    first-order model to hold, and the first gradient gives the expected decrease lr * sum |g| per step."""
    torch.manual_seed(5)
    cfg = dict(vocab_size=97, hidden_size=768, num_hidden_layers=1, num_attention_heads=12, intermediate_size=3072, max_position_embeddings=16)
    trunk = bert.BertEncoder(cfg, compute_dtype=compute, finetune_layers=1)
    with torch.no_grad():
        for n, p in trunk.named_parameters():
            if "LayerNorm.weight" in n:
                p.copy_(0.5 + torch.rand_like(p))
            elif n.startswith("embeddings.") and n.endswith("weight"):
                p.copy_(0.5 * torch.randn_like(p))
            elif n.endswith("weight"):
                p.copy_(torch.randn_like(p) / p.shape[1] ** 0.5)
    enc = text.TemporalTextEncoder({"hidden_dim": 512}, compute, bert=trunk).to(DEV).eval()
    gen = torch.Generator().manual_seed(6)
    ids = torch.randint(1, 97, (3, 9), generator=gen).to(DEV)
    mask = torch.ones(3, 9)
    mask[1, 5:] = 0
    mask[2, 1::2] = 0
    mask = mask.to(DEV)
    target = torch.randn(3, 512, generator=gen).to(DEV)
    tail = [p for n, p in enc.named_parameters() if n.startswith("bert.encoder.layer.0.")]
    opt = ModuleAdamW.for_module(enc, params=tail, lr=2e-5, weight_decay=0.0, max_grad_norm=0.0)
    assert opt._owners == [enc.bert] and sum(t is not None for t in opt._mirrors) == 16
    packed = enc.bert._operands()
    losses = []
    for step in range(5):
        opt.zero_grad()
        loss = (enc(ids, mask) - target).square().mean()
        losses.append(float(loss.detach()))
        if step == 4:
            break
        loss.backward()
        opt.step()
        assert enc.bert._operands() is packed
    print(f"text encoder + trunk tail, {compute}: loss before and after each of four ModuleAdamW steps: " + ", ".join(f"{v:.6g}" for v in losses))
    assert all(b < a for a, b in zip(losses, losses[1:])), losses


# ================================================================================================ 4. the trainer
def test_trainer_module_optimizer_on_a_composed_model(tmp_path):
    from mmdeer.trainer import DEERTrainer, TrainingConfig

    def mk():
        torch.manual_seed(21)
        return head.ComposedDEER(HierarchicalMultimodalFusion(40, 128, 300, dropout=0.0), head.MultiDimensionalDEER(512, dropout=0.0))

    B = 64
    batch = {"audio_features": torch.from_numpy(synth.normal(911, B * 40).reshape(B, 40).astype(np.float32)),
             "video_features": torch.from_numpy(synth.normal(912, B * 128).reshape(B, 128).astype(np.float32)),
             "text_features": torch.from_numpy(synth.normal(913, B * 300).reshape(B, 300).astype(np.float32)),
             "targets": torch.from_numpy(np.tanh(synth.normal(914, B * 3).reshape(B, 3)).astype(np.float32))}
    cfg = dict(learning_rate=3e-4, batch_size=B, output_dir=str(tmp_path / "o"), log_dir=str(tmp_path / "l"), save_frequency=1000, num_epochs=2,
               checkpoint_dir=str(tmp_path / "c"))
    on, off = DEERTrainer(mk(), TrainingConfig(module_optimizer=True, **cfg), DEV), DEERTrainer(mk(), TrainingConfig(**cfg), DEV)
    assert on.generic and isinstance(on.optimizer, ModuleAdamW) and type(off.optimizer) is torch.optim.AdamW
    assert on.optimizer.max_grad_norm == 1.0 and [g["lr"] for g in on.optimizer.param_groups] == [g["lr"] for g in off.optimizer.param_groups]
    assert all(torch.equal(a, b) for a, b in zip(on.model.parameters(), off.model.parameters()))
    before = [p.detach().clone() for p in on.model.parameters()]
    loaders = {"ravdess": [batch]}                                                  # dataset weight 0.8: the loss scale reaches the gradients
    m_on, m_off = on.train_epoch(loaders), off.train_epoch(loaders)
    assert m_on["total_loss"] == pytest.approx(m_off["total_loss"], rel=1e-6) and m_on["grad_norm"] == pytest.approx(m_off["grad_norm"], rel=1e-6)
    params = list(on.model.parameters())
    grads = [None if p.grad is None else p.grad.clone() for p in params]             # unclipped: ModuleAdamW clips inside the step
    lr_wd = {id(p): (R.f32(g["lr"]), R.f32(g["weight_decay"])) for g in on.optimizer.param_groups for p in g["params"]}
    z = [(torch.zeros_like(p), torch.zeros_like(p)) for p in params]
    # the parameters (the trainer's torch.optim.AdamW keeps torch's default betas: see BETAS above for what that does to the moments)
    held_to_torch("trainer step 1", snapshot(on.optimizer, params), snapshot(off.optimizer, list(off.model.parameters())), before, grads, z,
                  [lr_wd[id(p)] for p in params], [1] * len(params), float(on.optimizer.last_grad_norm), 1.0, families=("p",))
    assert any(g is None for g in grads) or len(grads) > 30
    second = on.train_epoch(loaders)                                                 # and a second step
    assert np.isfinite(second["total_loss"]) and np.isfinite(second["grad_norm"])
    assert any(not torch.equal(p, b) for p, b in zip(params, before))
    assert all(bool(torch.isfinite(p).all()) for p in params)
