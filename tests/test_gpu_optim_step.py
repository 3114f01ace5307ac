"""mmdeer_adamw_step and mmdeer_pack_weights on their own, through the C ABI, against tests/optim_ref.py (float64 on the device).

Operands are built from the public look-ups: fifty fp32 parameters, each inside a NaN-fenced arena, flat gradient and moment buffers
between NaN fences, the weights buffer pre-filled with a byte pattern.  Three launch plans -- compute_f32, bf16 with adam_fused = 1
(the tile path writes every image), bf16 with adam_fused = 0 (element-wise update + repack launch) -- each with pack_transposed 0 and
1.  Bounds: K * U * magnitude per element, K from tests/test_cpu_optim_ref.py; the worst ratios are printed
(pytest -s).
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from mmdeer import _lib

from . import optim_ref as R

pytestmark = pytest.mark.gpu

PLANS = (("fp32", 1, 1), ("bf16_fused", 0, 1), ("bf16_unfused", 0, 0))        # name, compute_f32, adam_fused
FENCE = 64                                                                    # floats of NaN around every operand
TAIL = 4096                                                                   # bytes behind the weights buffer that nobody may write


@functools.lru_cache(maxsize=1)
def H():
    """the harness: geometry, arena placement of the parameters, field offsets"""
    lib = _lib.load()
    G = R.Geometry(lib)
    dev = torch.device("cuda:0")
    pos, o = [], FENCE
    for i in range(G.n):
        pos.append(o)
        o += (G.numel[i] + 3) // 4 * 4 + FENCE + 4 * (i % 3)                  # 16-byte aligned, fences of varying length
    idx = np.full(G.flat, -1, dtype=np.int64)
    for i in range(G.n):
        idx[G.sl(i)] = pos[i] + np.arange(G.numel[i])
    inside = torch.from_numpy(G.mask).to(dev)
    h = dict(lib=lib, G=G, dev=dev, pos=pos, arena_elems=o, inside=inside, arena_idx=torch.from_numpy(idx[G.mask]).to(dev),
             W={f: G.weights_fields(lib, f) for f in (0, 1)}, lr=R.learning_rates(G))
    h["bg"] = {f: torch.from_numpy(R.background(h["W"][f]["bytes"] + TAIL)).to(dev) for f in (0, 1)}
    return type("Harness", (), h)


def fenced(x):
    """x between two NaN fences; returns the buffer and the view of x inside it (256-byte aligned)"""
    buf = torch.full((x.numel() + 2 * FENCE,), float("nan"), dtype=torch.float32, device=x.device)
    buf[FENCE:FENCE + x.numel()] = x
    return buf, buf[FENCE:FENCE + x.numel()]


def fences_intact(buf):
    return bool(torch.isnan(buf[:FENCE]).all()) and bool(torch.isnan(buf[-FENCE:]).all())


def to_arena(h, p_flat):
    arena = torch.full((h.arena_elems,), float("nan"), dtype=torch.float32, device=h.dev)
    arena[h.arena_idx] = p_flat[h.inside]
    return arena


def from_arena(h, arena, p_flat):
    """the updated parameters at their flat positions (the gaps keep p_flat's values); asserts every fence is intact"""
    out = p_flat.clone()
    out[h.inside] = arena[h.arena_idx]
    nan = torch.isnan(arena)
    nan[h.arena_idx] = False
    assert int(nan.sum()) == h.arena_elems - int(h.inside.sum()), "a fence around a parameter was written"
    return out


def param_pointers(h, arena):
    return (C.c_void_p * h.G.n)(*[arena.data_ptr() + 4 * q for q in h.pos])


def pack(h, arena, f32, w):
    _lib.check(h.lib.mmdeer_pack_weights(param_pointers(h, arena), w.data_ptr(), h.W[f32]["bytes"], f32, _lib.current_stream()))
    torch.cuda.synchronize()


def run_step(h, inputs, plan, pack_transposed=1, want_norm=True, lr=None):
    """one mmdeer_adamw_step on fresh copies of the inputs; returns flat p / exp_avg / exp_avg_sq, the norm, the weights buffer"""
    p, g, m, v, hyper = inputs
    _, f32, fused = plan
    arena = to_arena(h, p)
    gb, gv = fenced(g)
    mb, mv = fenced(m)
    vb, vv = fenced(v)
    w = h.bg[f32].clone()
    norm = torch.full((3,), float("nan"), dtype=torch.float32, device=h.dev)
    a = _lib.AdamWArgs()
    a.compute_f32, a.pack_transposed, a.step = f32, pack_transposed, hyper["step"]
    a.beta1, a.beta2, a.eps, a.weight_decay = hyper["beta1"], hyper["beta2"], hyper["eps"], hyper["wd"]
    a.max_grad_norm, a.grad_scale = hyper["max_norm"], hyper["grad_scale"]
    a.lr = (C.c_float * h.G.n)(*(h.lr if lr is None else lr))
    a.params = param_pointers(h, arena)
    a.grads, a.exp_avg, a.exp_avg_sq = gv.data_ptr(), mv.data_ptr(), vv.data_ptr()
    a.grad_norm = norm[1:].data_ptr() if want_norm else None
    a.weights, a.weights_bytes = w.data_ptr(), h.W[f32]["bytes"]
    a.stream = _lib.current_stream()
    with _lib.options(adam_fused=fused):
        _lib.check(h.lib.mmdeer_adamw_step(C.byref(a)))
    torch.cuda.synchronize()
    assert fences_intact(gb) and fences_intact(mb) and fences_intact(vb), "a fence around a flat buffer was written"
    assert torch.equal(gv, g), "the gradient buffer is an input"
    assert bool(torch.isnan(norm[0])) and bool(torch.isnan(norm[2])), "a neighbour of grad_norm was written"
    assert want_norm or bool(torch.isnan(norm[1]))
    return {"p": from_arena(h, arena, p), "exp_avg": mv.clone(), "exp_avg_sq": vv.clone(), "norm": float(norm[1]), "w": w, "arena": arena}


@functools.lru_cache(maxsize=1)
def device_inputs(name):
    h = H()
    p, g, m, v, hyper = R.case_inputs(h.G, name)
    return tuple(torch.from_numpy(t).to(h.dev) for t in (p, g, m, v)) + (hyper,)


def same_bits(a, b, fams=("p", "exp_avg", "exp_avg_sq")):
    return all(torch.equal(a[f].view(torch.int32), b[f].view(torch.int32)) for f in fams)


def weights_region(h, f32, w, skip=("wscratch",)):
    """the buffer with the named fields blanked (equal bytes in both operands of a comparison)"""
    W = h.W[f32]
    order = sorted(R.FIELDS, key=lambda f: (W[f], R.FIELDS.index(f)))
    out = w.clone()
    for k, f in enumerate(order):
        if f in skip:
            out[W[f]:(W[order[k + 1]] if k + 1 < len(order) else W["bytes"])] = 0
    return out


def field_span(h, f32, f):
    W = h.W[f32]
    order = sorted(R.FIELDS, key=lambda x: (W[x], R.FIELDS.index(x)))
    k = order.index(f)
    return W[f], (W[order[k + 1]] if k + 1 < len(order) else W["bytes"])


# =========================================================================== A. arithmetic against float64
@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_step_matches_float64_in_every_plan(name):
    """Every element of p, exp_avg, exp_avg_sq within K U magnitude of the float64 step teacher-forced with the kernel's own norm, the
    norm within its K of the float64 norm; fences intact, moment gaps untouched; the three plans, with pack_transposed 0 and 1, a
    second run and a run with grad_norm = NULL all give the same bits."""
    h = H()
    inputs = device_inputs(name)
    p, g, m, v, hyper = inputs
    runs = {(plan[0], pt): run_step(h, inputs, plan, pt) for plan in PLANS for pt in (1, 0)}
    first = runs[("fp32", 1)]
    worst = {}
    forced = {}
    for key, out in runs.items():
        if out["norm"] not in forced:
            forced[out["norm"]] = R.adamw_step_ref(h.G, p, g, m, v, h.lr, norm=out["norm"], **hyper)
        ref = forced[out["norm"]]
        r = R.ratios(out, ref)
        for fam, x in r.items():
            worst[fam] = max(worst.get(fam, 0.0), x)
        print(f"\n  {name} {key[0]} pack_transposed={key[1]}: " + "  ".join(f"{f} {x:.3f}" for f, x in r.items()), end="")
        for fam, x in r.items():
            assert x <= R.K[fam], (name, key, fam, x)
        gaps = ~h.inside
        assert bool((out["exp_avg"][gaps] == R.GAP_M).all()) and bool((out["exp_avg_sq"][gaps] == R.GAP_V).all()), key
        assert same_bits(out, first) and out["norm"] == first["norm"], (name, key)
    print(f"\n  worst of case {name}: " + "  ".join(f"{f} {x:.3f} (K {R.K[f]})" for f, x in worst.items()))
    for plan in PLANS:
        again = run_step(h, inputs, plan, 1)
        assert same_bits(again, first) and again["norm"] == first["norm"], plan
        assert torch.equal(again["w"], runs[(plan[0], 1)]["w"]), plan
        silent = run_step(h, inputs, plan, 1, want_norm=False)
        assert same_bits(silent, first), plan
        assert torch.equal(weights_region(h, plan[1], silent["w"]), weights_region(h, plan[1], again["w"])), plan
    if name == "zero":
        assert first["norm"] == 0.0
        assert all(bool(torch.isfinite(first[f][h.inside]).all()) for f in ("p", "exp_avg", "exp_avg_sq"))
        assert not first["exp_avg"][h.inside].any() and not first["exp_avg_sq"][h.inside].any()
        decay = 1.0 - torch.from_numpy(h.G.per_element(h.lr)).to(h.dev) * R.f32(hyper["wd"])
        assert R.ratio(first["p"], p.double() * decay, (p.double() * decay).abs()) <= R.K["p"]     # the parameters only decay


# =========================================================================== B. the gaps of the flat gradient buffer
@pytest.mark.parametrize("plan", PLANS, ids=[p[0] for p in PLANS])
def test_gradient_gaps_are_neither_read_nor_written(plan):
    """Every element of the flat gradient buffer outside the fifty parameters set to 3.0: the reported norm and all outputs equal
    the run with zero gaps bit for bit, and the gaps of the moment buffers keep their values."""
    h = H()
    p, g, m, v, hyper = device_inputs("s2b")
    clean = run_step(h, (p, g, m, v, hyper), plan)
    dirty_g = g.clone()
    dirty_g[~h.inside] = 3.0
    assert int((~h.inside).sum()) >= 180
    dirty = run_step(h, (p, dirty_g, m, v, hyper), plan)
    assert dirty["norm"] == clean["norm"], (dirty["norm"], clean["norm"])
    assert same_bits(dirty, clean)
    assert torch.equal(weights_region(h, plan[1], dirty["w"]), weights_region(h, plan[1], clean["w"]))
    gaps = ~h.inside
    assert bool((dirty["exp_avg"][gaps] == R.GAP_M).all()) and bool((dirty["exp_avg_sq"][gaps] == R.GAP_V).all())
    ref = R.adamw_step_ref(h.G, p, dirty_g, m, v, h.lr, **hyper)
    assert R.ratio(dirty["norm"], ref["norm"], ref["norm"]) <= R.K["norm"]


# =========================================================================== C. the weights buffer, decoded
@pytest.mark.parametrize("f32", [0, 1], ids=["bf16", "fp32"])
def test_pack_weights_writes_the_documented_images_and_nothing_else(f32):
    """After mmdeer_pack_weights on crafted parameters (random, bf16 ties under even and odd upper halves, +-0, fp32 denormals, the
    largest finite fp32) every image decodes, per the Python table, to the parameters rounded to nearest even, bit for bit; every
    other byte -- wscratch too -- keeps the pre-fill pattern."""
    h = H()
    W = h.W[f32]
    if f32:
        assert W["wfpack"] == W["wtfpack"] == W["wa_frag"] == W["bytes"]         # empty with compute_f32
    p_host = R.crafted_parameters(h.G)
    p = torch.from_numpy(p_host).to(h.dev)
    arena = to_arena(h, p)
    w = h.bg[f32].clone()
    pack(h, arena, f32, w)
    assert torch.equal(from_arena(h, arena, p).view(torch.int32), p.view(torch.int32))          # the parameters are inputs
    got = w.cpu().numpy()
    want = R.expected_images(h.G, p_host, f32)
    images = R.decode_weights(h.G, W, got, f32)
    assert images.keys() == want.keys()
    for k in want:
        assert np.array_equal(images[k], want[k]), (k, int((images[k] != want[k]).sum()))
    full = R.expected_weights(h.G, W, p_host, f32, h.bg[f32].cpu().numpy())
    diff = np.nonzero(got != full)[0]
    assert diff.size == 0, (diff.size, int(diff[0]), [f for f in R.FIELDS if field_span(h, f32, f)[0] <= diff[0] < field_span(h, f32, f)[1]])


@pytest.mark.parametrize("plan", PLANS, ids=[p[0] for p in PLANS])
@pytest.mark.parametrize("name", ["s2b", "s1000"])
def test_step_leaves_the_weights_a_pack_would(name, plan):
    """On the same pre-filled background the buffer after mmdeer_adamw_step equals, byte for byte, what mmdeer_pack_weights leaves
    when given the step's updated fp32 parameters (wscratch excluded); with pack_transposed = 0 the wtpack and wtfpack fields keep
    the pre-fill pattern entirely and everything else is equal.  And the numpy encoder agrees with both."""
    h = H()
    f32 = plan[1]
    inputs = device_inputs(name)
    for pt in (1, 0):
        out = run_step(h, inputs, plan, pt)
        packed = h.bg[f32].clone()
        pack(h, out["arena"], f32, packed)
        if pt == 0:
            for f in ("wtpack", "wtfpack"):
                lo, hi = field_span(h, f32, f)
                assert torch.equal(out["w"][lo:hi], h.bg[f32][lo:hi]), (f, "written with pack_transposed = 0")
                packed[lo:hi] = h.bg[f32][lo:hi]
        a, b = weights_region(h, f32, out["w"]), weights_region(h, f32, packed)
        assert torch.equal(a, b), (pt, int((a != b).sum()), int((a != b).nonzero()[0]))
        assert torch.equal(out["w"][h.W[f32]["bytes"]:], h.bg[f32][h.W[f32]["bytes"]:])
    full = R.expected_weights(h.G, h.W[f32], out["p"].cpu().numpy(), f32, h.bg[f32].cpu().numpy(), pack_transposed=False)
    assert np.array_equal(weights_region(h, f32, out["w"]).cpu().numpy(), weights_region(h, f32, torch.from_numpy(full)).numpy())


# =========================================================================== D. the host class
def test_fused_adamw_maps_every_group_to_its_parameter():
    """optim.FusedAdamW on a bf16 MultimodalDEER: every parameter in its own group with its own rate, the groups in shuffled order,
    grad_scale = 0.25 and clipping; a second step after two groups' rates changed.  Each step is adamw_step_ref of the parameters
    before it, the model's flat gradient and the optimiser's moments; the weights buffer is a pack of the new parameters."""
    from mmdeer import synth
    from mmdeer.model import ModelConfig, MultimodalDEER
    from mmdeer.optim import FusedAdamW

    h = H()
    m = MultimodalDEER(ModelConfig(compute_dtype="bf16", seed=11)).to(h.dev).train()
    b = synth.make_batch(64, seed=8)
    m.train_step(*(torch.from_numpy(b[k]).to(h.dev) for k in ("audio", "video", "text", "targets")))
    live = m.live_parameters()
    assert len(live) == h.G.n and [tuple(q.shape) for q in live] == [(r, c) if c > 1 else (r,) for r, c in zip(h.G.rows, h.G.cols)]
    rate = {id(q): R.f32(1e-3 * (1 + i / 64)) for i, q in enumerate(live)}
    others = [q for q in m.parameters() if id(q) not in rate]                   # parameters the fused backward never reaches
    order = np.random.default_rng(3).permutation(len(live))
    groups = [{"params": [live[i]], "lr": rate[id(live[i])]} for i in order]
    if others:
        groups.insert(7, {"params": others, "lr": 0.5})
    opt = FusedAdamW(m, groups, weight_decay=0.01, eps=1e-8)
    g = m._step_flat
    assert not g[~h.inside].any()
    gs = 0.25
    opt.max_grad_norm = R.f32(0.5 * gs * float(g.double().square().sum().sqrt()))

    def flat_params():
        out = torch.zeros(h.G.flat, dtype=torch.float32, device=h.dev)
        for i, q in enumerate(live):
            out[h.G.sl(i)] = q.detach().reshape(-1)
        return out

    for step in (1, 2):
        before = flat_params()
        mom = [t.clone() for t in opt._moments(h.dev)]
        lr = [rate[id(q)] for q in live]
        norm = opt.step(grad_scale=gs)
        torch.cuda.synchronize()
        hyper = dict(step=step, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.01, max_norm=opt.max_grad_norm, grad_scale=gs)
        ref = R.adamw_step_ref(h.G, before, g, mom[0], mom[1], lr, norm=float(norm), **hyper)
        got = {"p": flat_params(), "exp_avg": opt._exp_avg, "exp_avg_sq": opt._exp_avg_sq, "norm": float(norm)}
        r = R.ratios(got, ref)
        print(f"\n  FusedAdamW step {step}: " + "  ".join(f"{f} {x:.3f}" for f, x in r.items()), end="")
        for fam, x in r.items():
            assert x <= R.K[fam], (step, fam, x)
        w = m._weights(h.dev)
        packed = w.clone()
        ptrs = (C.c_void_p * h.G.n)(*[q.data_ptr() for q in live])
        _lib.check(h.lib.mmdeer_pack_weights(ptrs, packed.data_ptr(), packed.numel(), 0, _lib.current_stream()))
        torch.cuda.synchronize()
        assert torch.equal(weights_region(h, 0, w), weights_region(h, 0, packed)), step
        for i in (int(order[3]), int(order[40])):                             # a scheduler changes two groups' rates
            new = R.f32(rate[id(live[i])] * 0.37)
            rate[id(live[i])] = new
            next(gr for gr in opt.param_groups if gr["params"][0] is live[i])["lr"] = new
