"""The training step WITH DROPOUT LIVE of the audio, text and video encoders, of the stand-alone DEER heads (DEERLayer,
MultiDimensionalDEER) and of the fusion modules on the operator path (model.HierarchicalMultimodalFusion at a non-default geometry
through its wrapper, fusions.AdaptiveFusionGating, fusions.ConcatFusion) against float64 on the same masks.  The masks are drawn on
the CPU (tests/dropstep_ref.py: the uint32 restatement of the counter hash at the sites -- and, for the operator path's trimodal
attention, the seed offset -- the modules state), never by the library; the guard test ties that draw to mmdeer_dropout_mask per
(seed, site) and shape.  tests/test_cpu_dropstep_ref.py shows that the reference moves by >= 1500 x the bounds of test A under every
site mistake the modules could make (a neighbouring site, another step, a lost scale, batch-major rows, a second BatchNorm mask,
exchanged sites, global head columns; for the fusions also the trimodal mask under the plain seed or at site 83, the AV halves
exchanged, one AV mask per row or per column instead of per head, the adaptive encoder's mask on the wrong Linear), so a pass here is
a statement about the sites, the seeds, the scale and the backward's mask.

A. fp32 step: outputs, every parameter gradient, the input gradient (and the video encoder's running buffers) at the modules' own
   fp32 bounds of their golden tests.
B. the step counter: two forwards in a row are steps s and s + 1; the counter set back reproduces the step bit for bit; evaluation
   and dropout = 0 draw nothing.
C. bf16 step: relative l2 distance to float64 at most 2 x the distance of the bf16-emulating restatement (same masks) + 1e-6.
D. the seam: head.ComposedDEER(HierarchicalMultimodalFusion(40, 128, 300), MultiDimensionalDEER(512)) in fp32, both modules' dropout
   live and both step counters set: head outputs and the FUSION parameters' gradients -- which arrive through the head's backward --
   against fusion_forward followed by the head's reference, each on its own masks, at the bounds of test A.

Measured on an MI355X (every test prints its own figures: pytest -s), the largest fraction of a bound over a family's cases:
   A  outputs (rtol 1e-3 / atol 2e-5): audio 0.032, text by embeddings 0.145, text by ids 0.051, video 0.28, DEERLayer 0.0092,
      MultiDimensionalDEER 0.020; gradients (rtol 3e-3, 3e-3 of the largest element): audio 0.040, text 4.5e-4 / 4.1e-3, video 7.5e-4,
      heads 2.9e-4; the video encoder's running buffers (rtol 1e-5 / atol 1.2e-7): 0.43.
   B  second forward and dropout = 0: outputs <= 0.125, gradients <= 0.016, running buffers <= 0.29.
   C  distance to float64 / the emulation's own distance, 412 quantities: <= 1.04 (video 37 x 3, temporal_cnn.1.weight: 9.6e-2 against
      9.3e-2); 1.00 - 1.02 everywhere else.  Before the head emulation left the evidence tail's gradient in fp32, as
      csrc/nig_tail.hip keeps it, one 4-element bias gradient stood at 2.17 (1.7e-3 against 7.9e-4; now 1.7e-3 against 1.7e-3).
   The fusions on the operator path, measured the same way:
   A  outputs: HierarchicalMultimodalFusion 0.19 (40/128/300, B = 37), AdaptiveFusionGating 0.59 (B = 37: bilinear outputs up to 38),
      ConcatFusion 0.085; gradients: 5.7e-4, 2.3e-3, 2.2e-4.
   B  second forward and dropout = 0: outputs <= 0.15 / 0.26 / 0.059, gradients <= 4.8e-4 / 1.3e-3 / 2.0e-4.
   C  210 quantities: <= 1.03 (fusion B = 1, audio_visual_fusion.video_projection.bias: 2.8e-2 against 2.7e-2), 1.00 - 1.01 everywhere
      else.  The two reported 1-key weights are the head mean of the mask itself: the emulation returns them exactly, the module
      within 6e-8 (fp32), which the rule's + 1e-6 holds.
   D  head outputs 0.030, fusion and input gradients 4.5e-4.
Three breakages of the library were tried and each failed exactly the cases it touches: the inter-layer dropout's backward at scale 1
(audio A, B, C), a mask on the second BatchNorm layer too (video, T > 1), every head's layer 1 at head 0's site (MultiDimensionalDEER).
Two more for the operator path, each failing all four fusion cases of test A (the only ones run against them): the trimodal attention under the
module's plain seed (generic_fusion._TRI_SEED_OFFSET = 0), and drop_shift = 0 in _AVAttnFn.forward (one decision per column going
forward, one per head coming back)."""
import functools

import numpy as np
import pytest
import torch

from mmdeer import _lib, fusions

from . import dropstep_ref as D
from . import head_ref
from .rowkernel_ref import drop_keep
from .temporal_ref import seed_offset
from .test_oracle_golden import check_side_grads

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
AD = D.ADAPTERS
FIRST = [(n, a.cases[0]) for n, a in AD.items()]
FIRST_IDS = [f"{n}-{AD[n].case_id(c)}" for n, c in FIRST]


class _Golden(dict):
    """a dictionary read the way the gradient checkers read an .npz"""

    @property
    def files(self):
        return list(self)


def _has_drop(m):
    # the heads and the alternative fusions; the encoders count in ``_train_step``, and the HierarchicalMultimodalFusion wrapper reads
    # and writes the step of the fusion that runs through its own ``_train_step``
    return isinstance(getattr(m, "_drop", None), fusions._Drop)


def _set_step(m, step):
    if _has_drop(m):
        m._drop.step = step
    else:
        m._train_step = step


def _step_of(m):
    return m._drop.step if _has_drop(m) else m._train_step


@functools.lru_cache(None)
def _ref(name, case, step, emulate=False, mode="train"):
    """The reference step, computed once per (case, step): mode 'train' on the masks of ``step``; 'eval'; 'p0' = training, p = 0."""
    ad = AD[name]
    masks = ad.masks(case, step=step) if mode == "train" else ({} if mode == "p0" and name == "video" else None)
    return D.ref_step(ad, case, masks, emulate)


def _inputs(ad, case):
    X = {k: torch.from_numpy(v).to(DEV) for k, v in ad.inputs(case, ad.seed(case)).items()}
    return {k: v.requires_grad_(True) if k in ad.diff_inputs else v for k, v in X.items()}


def _run(ad, case, m, step=None, backward=True):
    if step is not None:
        _set_step(m, step)
    m.zero_grad(set_to_none=True)
    X = _inputs(ad, case)
    outs = ad.forward(m, X)
    if backward:
        W = ad.weights(case, outs)
        sum((outs[k] * W[k].float().to(DEV)).sum() for k in W).backward()
    grads = {n: p.grad for n, p in m.named_parameters() if not n.startswith(("spatial_backbone.", "bert."))}
    return dict(out={k: v.detach() for k, v in outs.items()}, grads=grads, dx={k: X[k].grad for k in ad.diff_inputs},
                buffers={k: v.detach().clone() for k, v in m.state_dict().items() if k.startswith("temporal_cnn.") and
                         ("running_" in k or k.endswith("num_batches_tracked"))})


def _check_fp32(ad, case, got, ref, what):
    """Test A's comparison; returns the largest fraction of each bound."""
    tag = "c"
    assert list(got["out"]) == list(ref["out"])
    worst = {"out": 0.0, "grad": 0.0, "buf": 0.0}
    for k, r in ref["out"].items():
        worst["out"] = max(worst["out"], D.out_fraction(got["out"][k], r))
    g = _Golden()
    zero, noise = D.rows_of(ad.zero_grads), D.rows_of(ad.noise_grads)          # {parameter: [row slices]}, slice(None) = all of it
    whole = lambda rows, k: any(sl == slice(None) for sl in rows.get(k, []))   # noqa: E731
    cmp = dict(got["grads"])       # what the gradient checker reads: the noise ROWS of a parameter are judged on their own below
    for k, r in ref["grads"].items():
        if whole(noise, k) and r is not None:
            continue
        if r is None:
            g[f"{tag}.gradnone.{k}"] = np.zeros(1)
        else:
            r = D.without_rows(r, zero.get(k, []) + noise.get(k, []))
            if k in noise:
                cmp[k] = D.without_rows(got["grads"][k], noise[k])
            g[f"{tag}.grad.{k}"] = r.numpy()
            if bool(r.any()):
                worst["grad"] = max(worst["grad"], D.grad_fraction(cmp[k], r))
    for k, r in ref["dx"].items():
        g[f"{tag}.dx.{k}"] = r.numpy()
        worst["grad"] = max(worst["grad"], D.grad_fraction(got["dx"][k], r))
    for k, r in ref["buffers"].items():
        if "running_" in k:
            worst["buf"] = max(worst["buf"], D.buffer_fraction(got["buffers"][k], r))
    print(f"{what}: largest fraction of the bound: outputs {worst['out']:.2e}, gradients {worst['grad']:.2e}" +
          (f", running buffers {worst['buf']:.2e}" if ref["buffers"] else ""))
    for k, r in ref["out"].items():
        np.testing.assert_allclose(got["out"][k].cpu().numpy(), r.numpy(), rtol=D.OUT_RTOL, atol=D.OUT_ATOL, err_msg=k)
    assert set(got["grads"]) == set(ref["grads"])
    if ad.name in ("deer_layer", "multi_dim"):
        assert all(f"{tag}.grad.{k}" in g for k in got["grads"])
        head_ref.check_grads(g, tag, got["grads"], got["dx"]["x"], rtol=D.G_RTOL, atol_frac=D.G_ATOL_FRAC)
    elif len(g) >= 10:
        check_side_grads(g, tag, cmp, got["dx"], rtol=D.G_RTOL, atol_frac=D.G_ATOL_FRAC)
    else:                                    # ConcatFusion: four parameters and one input, fewer than that checker asks to have seen
        assert len(g) == len(ref["grads"]) + len(ref["dx"]) and all(k.startswith((f"{tag}.grad.", f"{tag}.dx.")) for k in g)
        for k, r in g.items():
            kind, _, name = k[len(tag) + 1:].partition(".")
            have = cmp[name] if kind == "grad" else got["dx"][name]
            assert bool(np.abs(r).max()) and have is not None, k
            np.testing.assert_allclose(have.detach().cpu().numpy(), r, rtol=D.G_RTOL, atol=D.G_ATOL_FRAC * float(np.abs(r).max()), err_msg=k)
    for k, rows in zero.items():                                             # written as an exact zero
        if ref["grads"][k] is not None:
            assert got["grads"][k] is not None
            for sl in rows:
                assert float(got["grads"][k][sl].abs().max()) == 0.0, (k, sl)
    # analytically zero (under batch statistics, test_gpu_video_encoder.py; a shift the softmax does not see): rounding noise here as in
    # the reference
    for k, rows in noise.items():
        if ref["grads"][k] is not None:
            wmax = float(got["grads"][k.replace("bias", "weight")].abs().max())
            for sl in rows:
                assert float(ref["grads"][k][sl].abs().max()) <= 1e-4 * wmax and float(got["grads"][k][sl].abs().max()) <= 1e-4 * wmax, (k, sl)
    for k, r in ref["buffers"].items():
        if k.endswith("num_batches_tracked"):
            assert int(got["buffers"][k]) == int(r), k
        else:
            np.testing.assert_allclose(got["buffers"][k].cpu().numpy(), r.numpy(), rtol=D.BUF_RTOL, atol=D.BUF_ATOL, err_msg=k)
    return worst


# ------------------------------------------------------------------------------------------------------------------------ guard
def test_cpu_draw_is_the_library_draw_at_every_site_and_shape():
    """Guard: the references' masks are drawn on the CPU; per site and shape of every case, that draw is mmdeer_dropout_mask's."""
    lib, seen = _lib.load(), set()
    for name, case in D.ALL_CASES:
        for step in (D.STEP, D.STEP + 1):
            for rec in AD[name].sites(case):
                (_, site, rows, cols, p), seed = rec[:5], D.DROP_SEED + seed_offset(rec)
                if (seed, site, rows, cols, p, step) in seen:
                    continue
                seen.add((seed, site, rows, cols, p, step))
                got = torch.empty(rows, cols, dtype=torch.uint8, device=DEV)
                _lib.check(lib.mmdeer_dropout_mask(site, rows, cols, p, seed, step, got.data_ptr(), _lib.current_stream()))
                torch.cuda.synchronize()
                assert np.array_equal(got.cpu().numpy().astype(bool), drop_keep(site, rows, cols, p, seed, step)), (name, seed, site, rows, cols)
    assert len(seen) >= 40
    assert any(s != D.DROP_SEED for s, *_ in seen)              # the draw under a seed offset (the operator path's trimodal attention)


# ---------------------------------------------------------------------------------------------------------------------------- A
@pytest.mark.parametrize("name,case", D.ALL_CASES, ids=D.CASE_IDS)
def test_fp32_step_matches_float64_on_the_same_masks(name, case):
    ad = AD[name]
    m = ad.module(case, "fp32").to(DEV).train()
    got = _run(ad, case, m, D.STEP)
    assert _step_of(m) == D.STEP + 1
    _check_fp32(ad, case, got, _ref(name, case, D.STEP), f"A {name} {case}")
    if name == "video" and case[1] == 1:                                      # T = 1 skips the CNN: no gradient, no moved buffer
        assert all(v is None for k, v in got["grads"].items() if k.startswith(("temporal_cnn.", "temporal_attention.")))


# ---------------------------------------------------------------------------------------------------------------------------- B
@pytest.mark.parametrize("name,case", FIRST, ids=FIRST_IDS)
def test_step_counter(name, case):
    ad = AD[name]
    m = ad.module(case, "fp32").to(DEV).train()
    first = _run(ad, case, m, D.STEP)
    second = _run(ad, case, m)                                               # the counter ticked once: step s + 1
    assert _step_of(m) == D.STEP + 2
    if name == "video":      # the second forward starts from the buffers the first one moved: hand the reference that state
        state = dict(ad.state(case))
        state.update({k: v.cpu().numpy() for k, v in first["buffers"].items()})
        ref2 = D.ref_step(ad, case, ad.masks(case, step=D.STEP + 1), state=state)
    else:
        ref2 = _ref(name, case, D.STEP + 1)
    _check_fp32(ad, case, second, ref2, f"B {name} {case} second forward")
    assert not torch.equal(first["out"][next(iter(first["out"]))], second["out"][next(iter(second["out"]))])
    # the counter set back: the same step, bit for bit
    if name == "video":
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in ad.state(case).items()}, strict=False)
    again = _run(ad, case, m, D.STEP)
    for k in first["out"]:
        assert torch.equal(again["out"][k], first["out"][k]), k
    for k, g in first["grads"].items():
        assert (g is None and again["grads"][k] is None) or torch.equal(again["grads"][k], g), k
    for k in first["dx"]:
        assert torch.equal(again["dx"][k], first["dx"][k]), k
    # an evaluation forward draws nothing
    e = ad.module(case, "fp32").to(DEV).eval()
    _set_step(e, D.STEP)
    with torch.no_grad():
        ev = _run(ad, case, e, backward=False)
    assert _step_of(e) == D.STEP
    for k, r in _ref(name, case, D.STEP, mode="eval")["out"].items():
        np.testing.assert_allclose(ev["out"][k].cpu().numpy(), r.numpy(), rtol=D.OUT_RTOL, atol=D.OUT_ATOL, err_msg=k)
    # training with dropout = 0 is the unmasked step, and draws nothing
    z = ad.module(case, "fp32", p=0.0).to(DEV).train()
    got = _run(ad, case, z, D.STEP)
    assert _step_of(z) == D.STEP
    _check_fp32(ad, case, got, _ref(name, case, D.STEP, mode="p0"), f"B {name} {case} dropout 0")


# ---------------------------------------------------------------------------------------------------------------------------- C
@pytest.mark.parametrize("name,case", D.ALL_CASES, ids=D.CASE_IDS)
def test_bf16_step_within_twice_the_emulations_distance(name, case):
    ad = AD[name]
    m = ad.module(case, "bf16").to(DEV).train()
    got = _run(ad, case, m, D.STEP)
    f64, emu = _ref(name, case, D.STEP), _ref(name, case, D.STEP, True)
    rows, fails = [], []

    def hold(what, g, r, e):
        own, dist = D.rel(e, r), D.rel(g, r)
        rows.append((dist / max(own, 1e-300), what, dist, own))
        if not dist <= 2.0 * own + 1e-6:
            fails.append((what, dist, own))
    for k, r in f64["out"].items():
        if bool(torch.isfinite(r).all()):
            hold(f"output {k}", got["out"][k], r, emu["out"][k])
    for k, r in f64["grads"].items():
        if r is not None and not bool(r.any()) and k in ad.noise_grads:       # rounding noise that happens to be nothing in float64
            continue
        if r is None or not bool(r.any()):
            assert got["grads"][k] is None or not bool(got["grads"][k].any()), k
            continue
        exempt = D.rows_of(ad.bf16_exempt).get(k, [])
        if any(sl == slice(None) for sl in exempt):
            continue
        hold(k, D.without_rows(got["grads"][k], exempt), D.without_rows(r, exempt), D.without_rows(emu["grads"][k], exempt))
    for k, r in f64["dx"].items():
        hold(f"input {k}", got["dx"][k], r, emu["dx"][k])
    rows.sort(reverse=True)
    print(f"C {name} {case}: {len(rows)} quantities; largest distance / emulation's own distance: " +
          "; ".join(f"{w} {q:.2f} ({d:.1e} / {o:.1e})" for q, w, d, o in (rows if fails else rows[:3])))
    assert not fails, fails


# ---------------------------------------------------------------------------------------------------------------------------- D
def test_seam_fusion_gradients_through_the_heads_backward():
    from mmdeer import head
    fu = AD["fusion"]
    I, Dm, Hd = D.SEAM_HEAD
    hd = head.MultiDimensionalDEER(I, emotion_dims=Dm, hidden_dim=Hd, dropout=D.SEAM_CASE[4], seed=D.DROP_SEED)
    hd.load_state_dict({k: torch.from_numpy(v) for k, v in D._seam_head_state().items()}, strict=True)
    m = head.ComposedDEER(fu.module(D.SEAM_CASE, "fp32"), hd).to(DEV).train()
    _set_step(m.fusion, D.SEAM_STEPS[0])
    _set_step(m.head, D.SEAM_STEPS[1])
    X = {k: torch.from_numpy(v).to(DEV).requires_grad_(True) for k, v in fu.inputs(D.SEAM_CASE, D.SEAM_INPUT_SEED).items()}
    out = m(X["audio"], X["video"], X["text"])
    assert (_step_of(m.fusion), _step_of(m.head)) == (D.SEAM_STEPS[0] + 1, D.SEAM_STEPS[1] + 1)
    ref = D.seam_ref()
    W = D.seam_weights(ref["out"])
    sum((out[k] * W[k].float().to(DEV)).sum() for k in W).backward()
    worst = {"out": 0.0, "grad": 0.0}
    for k, r in ref["out"].items():
        worst["out"] = max(worst["out"], D.out_fraction(out[k], r))
    zero, noise = D.rows_of(fu.zero_grads), D.rows_of(fu.noise_grads)
    grads = {n: p.grad for n, p in m.fusion.named_parameters()}
    assert set(grads) == set(ref["grads"])
    cmp = {}
    for k, r in ref["grads"].items():
        if r is None:
            assert grads[k] is None, k
            continue
        cmp[k] = (D.without_rows(grads[k], noise.get(k, [])), D.without_rows(r, zero.get(k, []) + noise.get(k, [])))
        worst["grad"] = max(worst["grad"], D.grad_fraction(*cmp[k]))
    for k, r in ref["dx"].items():
        cmp["input " + k] = (X[k].grad, r)
        worst["grad"] = max(worst["grad"], D.grad_fraction(X[k].grad, r))
    print(f"D seam: largest fraction of the bound: head outputs {worst['out']:.2e}, fusion and input gradients {worst['grad']:.2e}")
    for k, r in ref["out"].items():
        np.testing.assert_allclose(out[k].detach().cpu().numpy(), r.numpy(), rtol=D.OUT_RTOL, atol=D.OUT_ATOL, err_msg=k)
    assert len(cmp) >= 24 + 3
    for k, (have, r) in cmp.items():
        np.testing.assert_allclose(have.detach().cpu().numpy(), r.numpy(), rtol=D.G_RTOL, atol=D.G_ATOL_FRAC * float(r.abs().max()), err_msg=k)
    for k, rows in zero.items():
        for sl in rows:
            assert float(grads[k][sl].abs().max()) == 0.0, (k, sl)
    for k, rows in noise.items():
        wmax = float(grads[k.replace("bias", "weight")].abs().max())
        for sl in rows:
            assert float(grads[k][sl].abs().max()) <= 1e-4 * wmax and float(ref["grads"][k][sl].abs().max()) <= 1e-4 * wmax, (k, sl)
