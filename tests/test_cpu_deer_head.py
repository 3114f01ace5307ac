"""The DEER head modules without a GPU: the compat import, the state_dict contract against the reference's recorded key order
and shapes, constructor signatures, every refusal that is decided on the host (module and C entry points), and the float64
restatement (tests/head_ref.py) against the vectors captured from the reference (tests/golden/deer_head.npz)."""
import ctypes as C
import inspect
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from mmdeer import _lib, head, synth

from . import head_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NAMES = json.load(open(os.path.join(GOLDEN, "deer_head_state_dict_names.json")))


def _state(tag, dtype=torch.float64):
    sd = synth.module_fill(tag, {k: tuple(v) for k, v in NAMES[tag].items()})
    if tag == "dlx":
        sd = R.extreme_state(sd)
    return {k: torch.from_numpy(v).to(dtype) for k, v in sd.items()}


def test_compat_deer_exports_the_head_modules():
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "from deer import MultiDimensionalDEER, CrossModalAttention, test_deer_implementation, DEERLayer\n"
            "import mmdeer.head as H\n"
            "assert MultiDimensionalDEER is H.MultiDimensionalDEER and DEERLayer is H.DEERLayer\n"
            "print('ok')\n") % (ROOT, os.path.join(ROOT, "compat"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-2000:]


def _build(tag):
    if tag in R.MD_CASES:
        I, D, H, _ = R.MD_CASES[tag]
        return head.MultiDimensionalDEER(I, emotion_dims=D, hidden_dim=H, dropout=0.0)
    I, O, H, _ = R.DL_CASES[tag] if tag in R.DL_CASES else R.DLX_CASE
    return head.DEERLayer(I, output_dim=O, hidden_dim=H, dropout=0.0)


@pytest.mark.parametrize("tag", list(NAMES))
def test_state_dict_is_the_references(tag):
    m = _build(tag)
    sd = m.state_dict()
    assert list(sd.keys()) == list(NAMES[tag].keys())
    assert {k: list(v.shape) for k, v in sd.items()} == NAMES[tag]
    m.load_state_dict(_state(tag, torch.float32), strict=True)


def test_default_geometry_parameter_count_and_initialisation():
    m = head.MultiDimensionalDEER(512)
    assert sum(p.numel() for p in m.parameters()) == 321356
    assert m.dimension_names == ["valence", "arousal", "dominance"] and m.emotion_dims == 3
    m.requires_grad_(False)
    for h in m.deer_heads:                                   # deer.py:61-66: Xavier-uniform weights, zero biases
        for lin in (h.evidence_net[0], h.evidence_net[3], h.evidence_net[6]):
            bound = (6.0 / (lin.in_features + lin.out_features)) ** 0.5
            assert float(lin.weight.abs().max()) <= bound and float(lin.weight.abs().max()) > 0.8 * bound
            assert float(lin.bias.abs().max()) == 0.0
    lin = m.feature_processor[0]                             # torch's default Linear init: both within 1 / sqrt(fan_in)
    assert float(lin.weight.abs().max()) <= 512 ** -0.5 and float(lin.bias.abs().max()) > 0.0
    a, b = head.MultiDimensionalDEER(64, hidden_dim=32, seed=3), head.MultiDimensionalDEER(64, hidden_dim=32, seed=3)
    assert all(torch.equal(p, q) for p, q in zip(a.parameters(), b.parameters()))
    c = head.MultiDimensionalDEER(64, hidden_dim=32, seed=4)
    assert not torch.equal(a.deer_heads[0].evidence_net[0].weight, c.deer_heads[0].evidence_net[0].weight)
    assert not torch.equal(a.deer_heads[0].evidence_net[0].weight, a.deer_heads[1].evidence_net[0].weight)


def test_constructor_signatures_are_the_references():
    """deer.py:33-34 and :201-202, then the two build-specific keyword arguments."""
    def sig(cls):
        return [(p.name, p.default) for p in list(inspect.signature(cls.__init__).parameters.values())[1:]]
    E = inspect.Parameter.empty
    assert sig(head.DEERLayer) == [("input_dim", E), ("output_dim", 1), ("hidden_dim", 256), ("dropout", 0.3),
                                   ("compute_dtype", "fp32"), ("seed", 0)]
    assert sig(head.MultiDimensionalDEER) == [("input_dim", E), ("emotion_dims", 3), ("hidden_dim", 256), ("dropout", 0.3),
                                              ("compute_dtype", "fp32"), ("seed", 0)]
    m = head.DEERLayer(16, 2, 32, 0.1)
    assert (m.input_dim, m.output_dim) == (16, 2)
    assert [type(x).__name__ for x in m.evidence_net] == ["Linear", "ReLU", "Dropout", "Linear", "ReLU", "Dropout", "Linear"]
    assert m.evidence_net[2].p == 0.1 and m.evidence_net[6].out_features == 8 and m.evidence_net[3].out_features == 16


def test_module_refusals_name_the_argument_and_need_no_library(monkeypatch):
    def no_library(*a, **k):
        raise AssertionError("a refusal must not reach the library")
    monkeypatch.setattr(_lib, "load", no_library)
    for kw, word in [(dict(input_dim=42), "input_dim"), (dict(input_dim=0), "input_dim"), (dict(input_dim=64, hidden_dim=24), "hidden_dim"),
                     (dict(input_dim=64, hidden_dim=1040), "hidden_dim"), (dict(input_dim=64, output_dim=0), "output_dim"),
                     (dict(input_dim=64, output_dim=9), "output_dim")]:
        with pytest.raises(NotImplementedError, match=word):
            head.DEERLayer(**kw)
    for kw, word in [(dict(input_dim=42), "input_dim"), (dict(input_dim=64, hidden_dim=48), "hidden_dim"),
                     (dict(input_dim=64, hidden_dim=2080), "hidden_dim"), (dict(input_dim=64, emotion_dims=0), "emotion_dims"),
                     (dict(input_dim=64, emotion_dims=4), "emotion_dims")]:
        with pytest.raises(NotImplementedError, match=word):
            head.MultiDimensionalDEER(**kw)
    with pytest.raises(ValueError):
        head.DEERLayer(64, compute_dtype="fp16")
    # the edges of the range build
    head.DEERLayer(4, 8, 1024)
    head.MultiDimensionalDEER(4, 1, 2048)
    # CPU tensors: no CPU fallback
    for m, x in ((head.DEERLayer(64, 2, 32), torch.zeros(3, 64)), (head.MultiDimensionalDEER(64, 3, 32), torch.zeros(3, 64))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m(x)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m(torch.zeros(0, 64))
        with pytest.raises(RuntimeError, match="expected"):
            m(torch.zeros(3, 60))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        head.evidence_tail(torch.zeros(2, 8), torch.zeros(1, 4, 8), torch.zeros(1, 4))


@pytest.mark.parametrize("tag", list(R.MD_CASES) + list(R.DL_CASES))
def test_restatement_reproduces_the_reference_capture(tag):
    """The distance is the reference's own fp32 rounding: tests/test_oracle_golden.py's bounds for the oracle's head
    (outputs rtol 1e-5, atol 2e-6; gradients rtol 2e-4, atol 2e-5 of each tensor's scale).  Measured worst output distance, in
    units of (atol + rtol |ref|): 0.04 ... 0.19 over the six cases, md768x3x512 (the 512-wide one) 0.04 -- every case is inside
    the project's bounds, so none has a bound of its own."""
    g = np.load(os.path.join(GOLDEN, "deer_head.npz"))
    P = {k: v.requires_grad_(True) for k, v in _state(tag).items()}
    x = torch.from_numpy(g[f"{tag}.input"]).double().requires_grad_(True)
    o = R.multi_dim(P, x, R.MD_CASES[tag][1]) if tag in R.MD_CASES else R.deer_layer(P, x)
    keys = [k[len(tag) + 5:] for k in g.files if k.startswith(tag + ".out.")]
    assert list(o.keys()) == keys
    worst = 0.0
    for k in keys:
        ref = g[f"{tag}.out.{k}"]
        assert tuple(o[k].shape) == ref.shape
        worst = max(worst, float((np.abs(o[k].detach().numpy() - ref) / (2e-6 + 1e-5 * np.abs(ref))).max()))
    print(tag, "worst output distance / bound = %.3f" % worst)
    for k in keys:
        np.testing.assert_allclose(o[k].detach().numpy(), g[f"{tag}.out.{k}"], rtol=1e-5, atol=2e-6, err_msg=k)
    sum((o[k] * torch.from_numpy(g[f"{tag}.w.{k}"]).double()).sum() for k in keys).backward()
    R.check_grads(g, tag, {k: v.grad for k, v in P.items()}, x.grad, rtol=2e-4, atol_frac=2e-5)


def test_restatement_reproduces_the_extreme_case():
    g = np.load(os.path.join(GOLDEN, "deer_head.npz"))
    P = _state("dlx")
    o = R.deer_layer(P, torch.from_numpy(g["dlx.input"]).double())
    for k in R.NIG_KEYS:
        ref, got = g[f"dlx.out.{k}"], o[k].numpy()
        assert np.array_equal(np.isinf(got), np.isinf(ref)), k
        fin = np.isfinite(ref)
        np.testing.assert_allclose(got[fin], ref[fin], rtol=1e-5, atol=2e-6, err_msg=k)
    assert np.isinf(g["dlx.out.uncertainty"][:, :2]).all() and np.isfinite(g["dlx.out.uncertainty"][:, 2:]).all()
    assert (g["dlx.out.alpha"][:, :2] == 1.0).all()


def test_restatement_tail_backward_equals_its_autograd():
    """tail_bwd's formulas (the ones the kernel is written from) against autograd through nig(), all planes and subsets."""
    B, G, K, O = 5, 2, 16, 3
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(B, G * K, dtype=torch.float64, generator=gen).requires_grad_(True)
    w = (0.3 * torch.randn(G, 4 * O, K, dtype=torch.float64, generator=gen)).requires_grad_(True)
    b = torch.randn(G, 4 * O, dtype=torch.float64, generator=gen).requires_grad_(True)
    gs = [torch.randn(B, G * O, dtype=torch.float64, generator=gen) for _ in range(7)]
    for use in [(1,) * 7, (1, 1, 1, 1, 0, 0, 0), (1, 0, 0, 0, 0, 0, 1), (0, 0, 0, 0, 1, 1, 0), (1, 1, 1, 1, 0, 0, 1)]:
        for t in (x, w, b):
            t.grad = None
        e = R.tail_evidence(x, w, b)
        outs = R.nig(e)
        sum((o * g).sum() for o, g, u in zip(outs, gs, use) if u).backward()
        devid, dx, dw, db = R.tail_bwd(x.detach(), w.detach(), e.detach(), [g if u else None for g, u in zip(gs, use)])
        for got, ref in ((dx, x.grad), (dw, w.grad), (db, b.grad)):
            torch.testing.assert_close(got, ref, rtol=1e-10, atol=1e-12)


A = 1 << 20     # a plausible, aligned address: never dereferenced by the host checks


def _tail(**kw):
    a = _lib.EvidenceTailArgs()
    a.x, a.ld_x, a.w, a.b, a.evid, a.nig_out = A, 192, A, A, A, A
    a.devid, a.dx, a.ld_dx, a.dw, a.db, a.scratch = A, A, 192, A, A, A
    a.B, a.G, a.K, a.O, a.act_f32 = 8, 3, 64, 1, 0
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("op", ["mmdeer_evidence_tail_fwd", "mmdeer_evidence_tail_bwd"])
def test_tail_operators_refuse_on_the_host(op):
    lib = _lib.load()
    f = getattr(lib, op)
    bwd = op.endswith("bwd")
    cases = [({"G": 0}, b"G must"), ({"G": 9}, b"G must"), ({"O": 0}, b"O must"), ({"O": 9}, b"O must"), ({"K": 0}, b"K must"),
             ({"K": 12}, b"K must"), ({"K": 520}, b"K must"), ({"B": -1}, b"B must"), ({"ld_x": 184}, b"ld_x"), ({"ld_x": 196}, b"ld_x"),
             ({"act_f32": 1, "ld_x": 194}, b"ld_x"), ({"x": A + 8}, b"x must"), ({"w": A + 2}, b"w must"), ({"evid": A + 4}, b"evid"),
             ({"x": None}, b"NULL"), ({"w": None}, b"NULL"), ({"evid": None}, b"evid")]
    if bwd:
        cases += [({"ld_dx": 184}, b"ld_dx"), ({"ld_dx": 196}, b"ld_dx"), ({"dx": A + 8}, b"dx must"), ({"scratch": A + 4}, b"scratch"),
                  ({"scratch": None}, b"scratch"), ({"devid": A + 4}, b"devid"), ({"dw": None}, b"NULL"), ({"db": None}, b"NULL")]
    else:
        cases += [({"b": None}, b"b must"), ({"b": A + 4}, b"b must"), ({"nig_out": None}, b"NULL")]
    for kw, msg in cases:
        assert f(C.byref(_tail(**kw))) == -1, kw
        assert msg in lib.mmdeer_last_error(), (kw, lib.mmdeer_last_error())
    assert f(None) == -1
    if not bwd:
        assert f(C.byref(_tail(B=0))) == 0                  # an empty batch launches nothing
    # fp32 rows may be multiples of 4; the edges of the range pass the shape checks (B = 0: nothing is launched)
    if not bwd:
        assert f(C.byref(_tail(B=0, act_f32=1, ld_x=196))) == 0
        assert f(C.byref(_tail(B=0, G=8, O=8, K=512, ld_x=4096))) == 0
        assert f(C.byref(_tail(B=0, G=1, O=1, K=8, ld_x=8))) == 0


def test_tail_scratch_size():
    lib = _lib.load()
    assert lib.mmdeer_evidence_tail_scratch(8, 9, 64, 1) == -1 and b"G must" in lib.mmdeer_last_error()
    assert lib.mmdeer_evidence_tail_scratch(8, 3, 60, 1) == -1 and b"K must" in lib.mmdeer_last_error()
    n1, n2 = lib.mmdeer_evidence_tail_scratch(64, 3, 64, 1), lib.mmdeer_evidence_tail_scratch(4097, 3, 64, 1)
    assert 0 < n1 < n2 and n1 % 4 == 0 and n2 % 4 == 0
    assert lib.mmdeer_evidence_tail_scratch(1 << 20, 3, 64, 1) - (1 << 20) * 12 == n2 - 4097 * 12     # the partials stop growing
    assert lib.mmdeer_evidence_tail_scratch(0, 1, 8, 1) >= 0
