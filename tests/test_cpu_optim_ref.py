"""tests/optim_ref.py is right, and the comparison tests/test_gpu_optim_step.py makes with it has teeth.

 * adamw_step_ref equals clip_grad_norm_ + torch.optim.AdamW(foreach=False) in float64 with injected state, to float64 rounding;
 * the same operation order in numpy float32 (adamw_step_f32) gives the rounding constants: K of a family is twice its worst ratio
   over the GPU test's cases (printed: pytest -s), and eleven seeded errors exceed that bound;
 * the decoders of the weights buffer: frag is a bijection, the head-major permutation is the one test_fused_projection_attention
   asserts, the image table covers every matrix row once per image kind, the written bytes fit the fields, and a decoder with a wrong
   row offset does not survive the round trip.
"""
import functools

import numpy as np
import pytest
import torch

from mmdeer import _lib

from . import optim_ref as R

F64 = torch.float64


@functools.lru_cache(maxsize=1)
def geometry():
    return R.Geometry(_lib.load())


# =========================================================================== the reference against torch
class _TinyLib:
    """a parameter table of a few small tensors with alignment gaps, answered like the library's look-ups"""
    shapes = [(8, 12), (8, 1), (16, 4), (4, 1), (4, 1), (3, 20)]

    def __init__(self):
        self.offs, o = [], 0
        for r, c in self.shapes:
            self.offs.append(o)
            o += (r * c + 63) // 64 * 64
        self.flat = o

    def mmdeer_num_params(self): return len(self.shapes)
    def mmdeer_param_name(self, i): return f"p{i}".encode()
    def mmdeer_param_rows(self, i): return self.shapes[i][0]
    def mmdeer_param_cols(self, i): return self.shapes[i][1]
    def mmdeer_param_offset(self, i): return self.offs[i]
    def mmdeer_flat_elems(self): return self.flat


def _torch_adamw(G, p, g, m, v, lr, step, beta1, beta2, eps, wd, max_norm, grad_scale):
    ps = [torch.nn.Parameter(p[G.sl(i)].clone()) for i in range(G.n)]
    for i, t in enumerate(ps):
        t.grad = g[G.sl(i)].clone() * R.f32(grad_scale)
    norm = torch.linalg.vector_norm(torch.cat([t.grad for t in ps]))
    if max_norm > 0:
        torch.nn.utils.clip_grad_norm_(ps, R.f32(max_norm))
    opt = torch.optim.AdamW([{"params": [t], "lr": R.f32(l)} for t, l in zip(ps, lr)], betas=(R.f32(beta1), R.f32(beta2)), eps=R.f32(eps),
                            weight_decay=R.f32(wd), foreach=False)
    for i, t in enumerate(ps):
        opt.state[t] = {"step": torch.tensor(float(step - 1)), "exp_avg": m[G.sl(i)].clone(), "exp_avg_sq": v[G.sl(i)].clone()}
    opt.step()
    return ps, [opt.state[t] for t in ps], float(norm)


@pytest.mark.parametrize("step", [1, 2, 3, 1000, 100000])
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_reference_equals_torch_adamw_in_float64(step, wd):
    G = R.Geometry(_TinyLib())
    gen = torch.Generator().manual_seed(step)
    lr = [1e-3 * (1 + i / 4) for i in range(G.n)]
    p = torch.randn(G.flat, generator=gen, dtype=F64)
    g_wide = torch.randn(G.flat, generator=gen, dtype=F64) * 10.0 ** (torch.rand(G.flat, generator=gen, dtype=F64) * 12 - 10)
    m = torch.zeros(G.flat, dtype=F64) if step == 1 else torch.randn(G.flat, generator=gen, dtype=F64)
    v = torch.zeros(G.flat, dtype=F64) if step == 1 else torch.randn(G.flat, generator=gen, dtype=F64) ** 2
    outside = torch.from_numpy(~G.mask)
    assert int(outside.sum()) > 100
    for g in (g_wide, torch.zeros_like(g_wide)):
        g = torch.where(outside, torch.full_like(g, 3.0), g)              # values in the gaps do not enter
        for gs in (1.0, 0.25, -0.5):
            base = abs(gs) * float(g[~outside].square().sum().sqrt())
            for mx in (0.0, 0.5 * base, 4.0 * base) if base > 0 else (0.0, 1.0):
                ref = R.adamw_step_ref(G, p, g, m, v, lr, step, 0.9, 0.999, 1e-8, wd, mx, gs)
                ps, st, norm = _torch_adamw(G, p, g, m, v, lr, step, 0.9, 0.999, 1e-8, wd, mx, gs)
                assert ref["norm"] == pytest.approx(norm, rel=1e-14, abs=0)
                for i in range(G.n):
                    for fam, got in (("p", ps[i].detach()), ("exp_avg", st[i]["exp_avg"]), ("exp_avg_sq", st[i]["exp_avg_sq"])):
                        r = R.ratio(got, ref[fam][G.sl(i)], ref["mag_" + fam][G.sl(i)])
                        assert r * R.U < 1e-13, (fam, i, gs, mx, r * R.U)
                for fam, src in (("p", p), ("exp_avg", m), ("exp_avg_sq", v)):
                    assert torch.equal(ref[fam][outside], src[outside]) and not ref["mag_" + fam][outside].any()
                if base == 0:                                              # norm exactly 0: the parameters only decay
                    assert ref["norm"] == 0.0
                    decay = torch.from_numpy(1.0 - G.per_element([R.f32(x) for x in lr]) * R.f32(wd))
                    if step == 1:
                        assert torch.equal(ref["p"], p * decay)


def test_teacher_forcing_takes_the_clip_factor_from_the_given_norm():
    G = R.Geometry(_TinyLib())
    gen = torch.Generator().manual_seed(1)
    p, g = torch.randn(G.flat, generator=gen, dtype=F64), torch.randn(G.flat, generator=gen, dtype=F64)
    z = torch.zeros(G.flat, dtype=F64)
    lr = [1e-3] * G.n
    a = R.adamw_step_ref(G, p, g, z, z, lr, 1, 0.9, 0.999, 1e-8, 0.0, 1.0, 1.0)
    b = R.adamw_step_ref(G, p, g, z, z, lr, 1, 0.9, 0.999, 1e-8, 0.0, 1.0, 1.0, norm=2 * a["norm"])
    inside = torch.from_numpy(G.mask)
    assert b["norm"] == a["norm"]
    assert torch.allclose(b["exp_avg"][inside] * 2, a["exp_avg"][inside], rtol=1e-6, atol=0)


# =========================================================================== rounding constants
@functools.lru_cache(maxsize=1)
def _case(name):
    G = geometry()
    p, g, m, v, h = R.case_inputs(G, name)
    ref = R.adamw_step_ref(G, *(torch.from_numpy(t) for t in (p, g, m, v)), R.learning_rates(G), **h)
    return (p, g, m, v, h), ref


def _f32(name, variant=None):
    G = geometry()
    (p, g, m, v, h), ref = _case(name)
    got = R.adamw_step_f32(G, p, g, m, v, R.learning_rates(G), variant=variant, **h)
    forced = R.adamw_step_ref(G, *(torch.from_numpy(t) for t in (p, g, m, v)), R.learning_rates(G), norm=got["norm"], **h)
    forced["norm"] = ref["norm"]
    return {k: (torch.from_numpy(t) if k != "norm" else t) for k, t in got.items()}, forced


def test_float32_ratios_give_K():
    """the worst ratio of the float32 CPU evaluation per family over the GPU test's cases; K is twice that (rounded up)"""
    worst = {}
    for name in R.CASE_NAMES:
        got, ref = _f32(name)
        r = R.ratios(got, ref)
        print(f"\nfloat32 CPU ratios, case {name}: " + "  ".join(f"{f} {x:.3f}" for f, x in r.items()), end="")
        for fam, x in r.items():
            worst[fam] = max(worst.get(fam, 0.0), x)
            assert x <= R.K[fam] / 2, (name, fam, x)
        if name == "zero":
            assert got["norm"] == 0.0 and ref["norm"] == 0.0
            assert all(bool(torch.isfinite(got[f]).all()) for f in ("p", "exp_avg", "exp_avg_sq"))
    print("\nworst over the cases: " + "  ".join(f"{f} {x:.3f} (K {R.K[f]})" for f, x in worst.items()))
    for fam, x in worst.items():                           # K is tied to the measurement, not chosen
        assert R.K[fam] / 2 <= 1.1 * x + 0.01, (fam, x, R.K[fam])


def test_eps_matters_in_a_visible_share_of_the_elements():
    _, ref = _case("s1000")
    G = geometry()
    inside = torch.from_numpy(G.mask)
    root = (ref["exp_avg_sq"][inside]).sqrt()
    share = float(((root > 0.1 * R.EPS) & (root < 10 * R.EPS)).double().mean())
    assert share > 0.05, share


# =========================================================================== seeded errors
SEEDED = [("lr0_all", "s1"), ("lr_stack_first", "s1"), ("l2_decay", "s1"), ("eps_in_sqrt", "s1"),
          ("norm_no_scale", "s2b"), ("sign_lost", "s2b"), ("eps_not_bc2", "s2b"), ("bc_swapped", "s2b"), ("step_minus_1", "s2b"),
          ("m_unscaled", "s2b"), ("clip_no_1e6", "tiny")]


def test_every_seeded_error_has_a_case():
    assert sorted(v for v, _ in SEEDED) == sorted(R.VARIANTS)


@pytest.mark.parametrize("variant,name", SEEDED)
def test_seeded_errors_exceed_the_bound(variant, name):
    good, ref = _f32(name)
    assert not R.rejects(good, ref)
    bad, ref_bad = _f32(name, variant)
    r = R.ratios(bad, ref_bad)
    assert R.rejects(bad, ref_bad), r
    print(f"\nseeded {variant} on {name}: " + "  ".join(f"{f} {x:.3g}" for f, x in r.items()))


def test_stacked_head_rate_error_shows_only_in_the_other_two_heads():
    """the seeded error of the stacked image is confined to heads 1 and 2: the bound is per element, so it is found there"""
    G = geometry()
    bad, ref = _f32("s1", "lr_stack_first")
    for h, name in enumerate(R.STACKED_HEADS):
        s = G.sl(G.index(name))
        r = R.ratio(bad["p"][s], ref["p"][s], ref["mag_p"][s])
        assert (r > R.K["p"]) == (h > 0), (name, r)


# =========================================================================== decoders
def test_frag_is_a_bijection_and_the_fast_form_is_the_restatement():
    for rows, cols in ((16, 64), (48, 128), (128, 64), (32, 192)):
        M = np.arange(rows * cols, dtype=np.int32).reshape(rows, cols)
        f = R.frag(M)
        assert sorted(f.tolist()) == list(range(rows * cols))
        assert np.array_equal(f, R.frag_fast(M))
        assert np.array_equal(R.unfrag(f, rows, cols), M)
    # a 16-row block of the matrix is contiguous in the image (what lets a row range be a sub-image)
    M = np.arange(64 * 128, dtype=np.int32).reshape(64, 128)
    assert np.array_equal(R.frag(M)[16 * 128:], R.frag(M[16:]))


def test_head_major_rows_are_the_fused_attention_tests_permutation():
    src = R.head_major_rows()
    assert sorted(src.tolist()) == list(range(1536))
    w = torch.arange(1536 * 512, dtype=torch.int32).view(1536, 512)
    want = w.view(3, 8, 2, 32, 512).permute(1, 2, 0, 3, 4).reshape(1536, 512)
    assert torch.equal(torch.from_numpy(w.numpy()[src]), want)


def test_bf16_rne_is_torchs_rounding_on_the_crafted_values():
    G = geometry()
    p = R.crafted_parameters(G)
    want = torch.from_numpy(p).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(R.bf16_rne(p), want)
    bits = p.view(np.uint32)
    tie = (bits & 0xFFFF) == 0x8000
    assert tie.sum() > 1000 and (((bits[tie] >> 16) & 1) == 0).any() and (((bits[tie] >> 16) & 1) == 1).any()
    assert (R.bf16_rne(p)[tie] & 1 == 0).all()                                   # ties go to the even neighbour
    expo = (bits >> 23) & 0xFF
    assert ((expo == 0) & ((bits & 0x7FFFFF) != 0)).sum() > 1000                 # denormals
    assert (bits == 0x80000000).any() and (bits == 0).any() and (bits == 0x7F7FFFFF).any() and (bits == 0xFF7FFFFF).any()


def test_image_table_covers_every_matrix_row_once_per_kind():
    G = geometry()
    T = R.image_table()
    per_kind, images = {}, {}
    for e in T:
        i, row0, rows, cols, s_off, s_row, srows, w_off, ld, wt_col = R._resolve(G, e)
        assert G.is_matrix[i]
        for kind in e["kinds"]:
            per_kind[(kind, e["name"])] = True
            # the rows of the image the range lands in: S for the fragment images, the columns of W^T, else the matrix itself
            where, size, at = {"frag": (s_off, srows, s_row), "fragT": (s_off, srows, s_row), "wt": (w_off, ld, wt_col)}.get(kind, (G.off[i], G.rows[i], row0))
            cover = images.setdefault((kind, where), np.zeros(size, dtype=int))
            cover[at:at + rows] += 1
    for key, cover in images.items():
        assert (cover == 1).all(), key
    for i in range(G.n):                                     # the ranges of a parameter in the table cover all its rows once
        mine = [e["rows"] or (0, G.rows[i]) for e in T if e["name"] == G.names[i]]
        if mine:
            assert sorted(mine)[0][0] == 0 and sum(n for _, n in mine) == G.rows[i], G.names[i]
    has = lambda kind: {n for k, n in per_kind if k == kind}
    mats = {G.names[i] for i in range(G.n) if G.is_matrix[i]}
    last = {n for n in mats if "evidence_net.6" in n}
    inputs = {n for n in mats if n.endswith(("audio_projection.weight", "video_projection.weight", "text_projection.weight"))}
    assert len(last) == 3 and len(inputs) == 3
    assert has("wt") == mats - last - inputs                                     # every matrix with a dX has W^T
    assert has("fragT") == has("wt") - {"fusion.trimodal_fusion.modality_attention.in_proj_weight"}
    audio = {n for n in inputs if "audio_projection" in n}
    assert has("frag") == (has("fragT") | inputs) - audio                        # the padded audio weight has its own fragment image
    assert has("pad") == audio and has("hm") == {"fusion.trimodal_fusion.modality_attention.in_proj_weight"}
    # the AV in_proj: fragment images of the v third only
    frag_av = [e for e in T if e["name"] == R.AV_IN_PROJ and "frag" in e["kinds"]]
    assert len(frag_av) == 1 and frag_av[0]["rows"] == (512, 256) and frag_av[0]["S"] == (R.AV_IN_PROJ, 512, 256)


@pytest.mark.parametrize("f32", [0, 1])
def test_written_bytes_fit_the_fields_and_round_trip(f32):
    G = geometry()
    lib = _lib.load()
    W = G.weights_fields(lib, f32)
    order = sorted(R.FIELDS, key=lambda f: (W[f], R.FIELDS.index(f)))
    end = {f: (W[order[k + 1]] if k + 1 < len(order) else W["bytes"]) for k, f in enumerate(order)}
    if f32:
        assert W["wfpack"] == W["wtfpack"] == W["wa_frag"] == W["bytes"]          # empty with compute_f32
    p = R.crafted_parameters(G)
    tail = 4096
    bg = R.background(W["bytes"] + tail)
    buf = R.expected_weights(G, W, p, f32, bg)
    written = buf != bg                                       # the pattern is no byte pair of the data: (nearly) every written byte differs
    es = 2 if not f32 else 4
    nmat = sum(G.numel[i] for i in range(G.n) if G.is_matrix[i])
    for f in R.FIELDS:
        lo, hi = W[f], end[f]
        n = int(written[lo:hi].sum())
        cap = {"wpack": nmat * es, "vpack": (sum(G.numel) - nmat) * 4, "wa_pad": 256 * 128 * 2, "wa_frag": 256 * 128 * 2,
               "wqkv_hm": 1536 * 512 * 2, "wscratch": 0}.get(f)
        if f32 and f in ("wa_pad", "wqkv_hm", "wa_frag", "wfpack", "wtfpack"):
            cap = 0                                           # the bf16 images do not exist in fp32 mode
        if cap is not None:
            assert n <= cap and (cap == 0 or n > 0.98 * cap), (f, n, cap)
        assert n <= hi - lo
        if hi > lo and n:
            assert np.nonzero(written[lo:hi])[0].max() < G.flat * (4 if f == "vpack" else es), f
    assert not written[W["bytes"]:].any()
    # the round trip, and three decoders with a seeded wrong row offset
    want = R.expected_images(G, p, f32)
    got = R.decode_weights(G, W, buf, f32)
    assert got.keys() == want.keys()
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    for variant in ("v_at_row_0", "stack_reversed", "wt_col_dropped"):
        if f32 and variant == "v_at_row_0":
            continue                                          # the v third is a matrix of its own only in the fragment images
        bad = R.decode_weights(G, W, buf, f32, table=R.image_table(variant))
        assert bad.keys() != want.keys() or any(not np.array_equal(bad[k], want[k]) for k in want), variant
    # without the transposed copies: wtpack / wtfpack keep the background, everything else is the same
    nt = R.expected_weights(G, W, p, f32, bg, pack_transposed=False)
    for f in R.FIELDS:
        lo, hi = W[f], end[f]
        if f in ("wtpack", "wtfpack"):
            assert np.array_equal(nt[lo:hi], bg[lo:hi]), f
        else:
            assert np.array_equal(nt[lo:hi], buf[lo:hi]), f
