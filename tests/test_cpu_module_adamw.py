"""mmdeer_adamw_multi / optim.ModuleAdamW without a GPU: the eighth companion header (include/mmdeer_optim.h) through the strict parser,
its layout against the compiler, its symbols in the built library, every refusal of the entry (all decided on the host, before
anything is written), the float64 restatement (tests/optim_multi_ref.py) against clip_grad_norm_ + torch.optim.AdamW, the float32
restatement that gives the norm's K and carries the seeded errors, and the constructor and state_dict rules of ModuleAdamW."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from mmdeer import _header, _lib, build
from mmdeer.optim import ModuleAdamW

from . import optim_multi_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OPTIM_SYMBOLS = {"mmdeer_adamw_multi": 1, "mmdeer_adamw_multi_table_bytes": 2, "mmdeer_adamw_multi_uploads": 0}
OPTIM_STRUCTS = {"adamw_multi_tensor", "adamw_multi_class", "adamw_multi_args"}


# ------------------------------------------------------------------------------------------------ the C ABI additions
def test_new_symbols_are_declared_bound_and_exported():
    lib = _lib.load()
    assert {n: len(args) for n, _, args in _lib.OPTIM_SYMBOLS} == OPTIM_SYMBOLS
    for name, res, args in _lib.OPTIM_SYMBOLS:
        fn = getattr(lib, name)                                           # exported by the built library
        assert fn.restype is (C.c_int32 if name == "mmdeer_adamw_multi" else C.c_longlong) and fn.argtypes == args, name
    assert set(_lib.OPTIM_STRUCTS) == OPTIM_STRUCTS
    for name, cls in _lib.OPTIM_STRUCTS.items():                          # the ctypes mirrors against the library's own sizeof
        assert lib.mmdeer_sizeof(name.encode()) == C.sizeof(cls), name
    assert _lib.OPTIM_CONSTANTS == {"ADAMW_MULTI_MAX_CLASSES": 16, "ADAMW_MULTI_CHUNK": R.CHUNK, "ADAMW_MULTI_SCRATCH": R.NPART}
    new = {n for n, _, _ in _lib.OPTIM_SYMBOLS}
    for older in (_lib.SYMBOLS, _lib.VIDEO_SYMBOLS, _lib.FRAME_SYMBOLS, _lib.ROUTE_SYMBOLS, _lib.FRAME_BWD_SYMBOLS, _lib.BERT_SYMBOLS,
                  _lib.BERT_BWD_SYMBOLS, _lib.BERT_DROP_SYMBOLS):
        assert not new & {n for n, _, _ in older}
    assert not set(_lib.OPTIM_STRUCTS) & (set(_lib.STRUCTS) | set(_lib.VIDEO_STRUCTS) | set(_lib.FRAME_STRUCTS) | set(_lib.FRAME_BWD_STRUCTS) |
                                          set(_lib.BERT_STRUCTS) | set(_lib.BERT_BWD_STRUCTS) | set(_lib.BERT_DROP_STRUCTS))
    assert {"adamw_args", "adamw_flat_args"} <= set(_lib.STRUCTS)         # the two older entries are where they were
    assert "optim_multi.hip" in build.SOURCES and "optim.hip" in build.SOURCES
    assert _header.OPTIM_HEADER_PATH == build.OPTIM_HEADER_PATH
    assert os.path.samefile(build.OPTIM_HEADER_PATH, os.path.join(ROOT, "include", "mmdeer_optim.h"))
    assert lib.mmdeer_abi_version() == _lib.ABI_VERSION == 16            # additions only


def test_header_layout_matches_the_compiler(tmp_path):
    """Offsets and sizes of every field of the three new structs, as ctypes lays them out, asserted by the compiler on the header."""
    lines = ["#include <stddef.h>", '#include "mmdeer_optim.h"']
    for cname, cls in _lib._OPTIM_CLASSES.items():
        lines.append(f'static_assert(sizeof({cname}) == {C.sizeof(cls)}, "sizeof {cname}");')
        for field, _ in cls._fields_:
            d = getattr(cls, field)
            lines.append(f'static_assert(offsetof({cname}, {field}) == {d.offset}, "offsetof {cname}.{field}");')
            lines.append(f'static_assert(sizeof((({cname}*)0)->{field}) == {d.size}, "sizeof {cname}.{field}");')
    tu = tmp_path / "layout.cpp"
    tu.write_text("\n".join(lines) + "\n")
    r = subprocess.run([build._hipcc(), "-x", "c++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(tu)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    src = _header.read(_header.OPTIM_HEADER_PATH)
    for bad in (src.replace("int mmdeer_adamw_multi(", "int mmdeer_adamw_multi(uint16_t f, "),                  # the same strict parser
                src.replace("#define MMDEER_ADAMW_MULTI_CHUNK 1024", "#define MMDEER_ADAMW_MULTI_CHUNK 1024\n#if 0\n#endif"),
                src.replace("float* scratch;", "float* scratch; short s;")):
        assert bad != src
        with pytest.raises(_header.HeaderError):
            _header.parse(bad, _lib._OPTIM_NAMES, {})


# ------------------------------------------------------------------------------------------------ refusals (host side)
A = 1 << 20     # a plausible, aligned address: never dereferenced by the host checks


def _args(n=2, **kw):
    rec = (_lib.AdamWMultiTensor * max(n, 1))()
    for i in range(n):
        rec[i].param, rec[i].grad, rec[i].count, rec[i].moment_off, rec[i].cls = A + 4096 * i, 2 * A + 4096 * i, 100, 128 * i, i % 2
    a = _lib.AdamWMultiArgs()
    a.tensors, a.ntensors, a.nclasses = rec, n, 2
    for c in range(2):
        a.classes[c].lr, a.classes[c].weight_decay, a.classes[c].step = 1e-3, 0.01, 1
    a.exp_avg, a.exp_avg_sq, a.moment_elems = 3 * A, 4 * A, 256
    a.table, a.table_bytes, a.upload = 5 * A, 1 << 16, 1
    a.scratch, a.grad_norm = 6 * A, 7 * A
    a.beta1, a.beta2, a.eps, a.max_grad_norm, a.grad_scale = 0.9, 0.999, 1e-8, 1.0, 1.0
    a._keep = rec
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _tensor(field, value, i=1):
    a = _args()
    setattr(a._keep[i], field, value)
    return a


def _cls(field, value):
    a = _args()
    setattr(a.classes[1], field, value)
    return a


REFUSALS = {
    "null tensors": lambda: _args(tensors=None),
    "negative ntensors": lambda: _args(ntensors=-1),
    "null param": lambda: _tensor("param", None),
    "null grad": lambda: _tensor("grad", None),
    "misaligned param": lambda: _tensor("param", A + 2),
    "misaligned grad": lambda: _tensor("grad", A + 1),
    "misaligned fp32 mirror": lambda: (lambda a: (setattr(a._keep[0], "mirror_f32", 1), a)[1])(_tensor("mirror", A + 2, 0)),
    "misaligned bf16 mirror": lambda: _tensor("mirror", A + 1),
    "negative count": lambda: _tensor("count", -1),
    "class index above": lambda: _tensor("cls", 2),
    "class index below": lambda: _tensor("cls", -1),
    "step 0": lambda: _cls("step", 0),
    "lr 0": lambda: _cls("lr", 0.0),
    "lr negative": lambda: _cls("lr", -1e-3),
    "lr nan": lambda: _cls("lr", math.nan),
    "lr inf": lambda: _cls("lr", math.inf),
    "decay negative": lambda: _cls("weight_decay", -0.01),
    "eps 0": lambda: _args(eps=0.0),
    "eps nan": lambda: _args(eps=math.nan),
    "eps inf": lambda: _args(eps=math.inf),
    "beta1 1": lambda: _args(beta1=1.0),
    "beta2 negative": lambda: _args(beta2=-0.1),
    "moments overlap": lambda: _tensor("moment_off", 50),
    "moments pass the end": lambda: _tensor("moment_off", 200),
    "moment offset negative": lambda: _tensor("moment_off", -4),
    "too many classes": lambda: _args(nclasses=17),
    "no class": lambda: _args(nclasses=0),
    "null table": lambda: _args(table=None),
    "table too small": lambda: _args(table_bytes=64),
    "null moments": lambda: _args(exp_avg=None),
    "null scratch": lambda: _args(scratch=None),
}


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_refusals_set_last_error(what):
    """every refusal is decided before anything is launched or written: the addresses here are never dereferenced"""
    lib = _lib.load()
    a = REFUSALS[what]()
    before = lib.mmdeer_adamw_multi_uploads()
    assert lib.mmdeer_adamw_multi(C.byref(a)) == -1, what
    msg = lib.mmdeer_last_error().decode()
    assert msg and ("adamw_multi" in msg or "NULL" in msg), (what, msg)
    assert lib.mmdeer_adamw_multi_uploads() == before


def test_null_args_and_the_sizing_entry():
    lib = _lib.load()
    assert lib.mmdeer_adamw_multi(None) == -1 and lib.mmdeer_last_error()
    a = _args()
    # 2 tensors of 100 elements: one chunk each -> 2 records of 64 bytes + 2 chunk entries, rounded to 16
    assert lib.mmdeer_adamw_multi_table_bytes(a._keep, 2) == 144
    a._keep[1].count = R.CHUNK + 1
    assert lib.mmdeer_adamw_multi_table_bytes(a._keep, 2) == 144      # 128 + 3 * 4 = 140 -> 144
    a._keep[1].count, a._keep[1].param = R.CHUNK, A + 4               # one element past a 16-byte boundary: the body starts a group later
    assert lib.mmdeer_adamw_multi_table_bytes(a._keep, 2) == 144
    a._keep[0].count = 0                                              # skipped: no chunk
    assert lib.mmdeer_adamw_multi_table_bytes(a._keep, 2) == 144 - 0 and lib.mmdeer_adamw_multi_table_bytes(a._keep, 0) == 0
    a._keep[1].count = -5
    assert lib.mmdeer_adamw_multi_table_bytes(a._keep, 2) == -1 and lib.mmdeer_last_error()
    assert lib.mmdeer_adamw_multi_table_bytes(None, 1) == -1
    # nothing to do: no tensor with elements -> 0 without a launch (and without a look at the device)
    b = _args()
    b._keep[0].count = b._keep[1].count = 0
    assert lib.mmdeer_adamw_multi(C.byref(b)) == 0
    assert lib.mmdeer_adamw_multi(C.byref(_args(n=0))) == 0


# ------------------------------------------------------------------------------------------------ the restatement against torch
def test_reference_equals_torch_adamw_in_float64():
    """three steps of clip_grad_norm_ + torch.optim.AdamW in float64 on the CPU: two groups with differing lr and decay, a
    parameter whose grad is None on step 2 (torch leaves it, its moments and its step count alone), grad_scale folded into the
    gradients.  1e-12 of the largest element."""
    rng = np.random.default_rng(11)
    sizes, group = [7, 1, 33, 12, 5], [0, 1, 0, 1, 1]
    # the reference takes its scalars as the float32 values the library receives: give torch exactly those
    lr, wd, mx, gs = (R.f32(1e-2), R.f32(3e-3)), (R.f32(0.05), 0.0), 0.75, 0.5
    b1, b2, eps = R.f32(R.BETA1), R.f32(R.BETA2), R.f32(R.EPS)
    P = [torch.nn.Parameter(torch.from_numpy(rng.standard_normal(n))) for n in sizes]
    opt = torch.optim.AdamW([{"params": [p for p, g in zip(P, group) if g == c], "lr": lr[c], "weight_decay": wd[c]} for c in (0, 1)],
                            betas=(b1, b2), eps=eps)
    mine = [{"p": p.detach().numpy().copy(), "m": np.zeros(n), "v": np.zeros(n), "cls": 0, "skip": False} for p, n in zip(P, sizes)]
    steps = [0] * len(P)
    for it in range(3):
        G = [rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 1) for n in sizes]
        for i, p in enumerate(P):
            p.grad = None if (it == 1 and i == 2) else torch.from_numpy(G[i] * gs)
        torch.nn.utils.clip_grad_norm_(P, mx)
        opt.step()
        # classes: the distinct (group, step) pairs, as ModuleAdamW forms them
        keys = {}
        for i, t in enumerate(mine):
            t["g"], t["skip"] = G[i], it == 1 and i == 2
            if not t["skip"]:
                t["cls"] = keys.setdefault((group[i], steps[i]), len(keys))
                steps[i] += 1
        classes = [(lr[g], wd[g], s + 1) for (g, s) in keys]
        ref = R.adamw_multi_ref(mine, classes, b1, b2, eps, mx, gs)
        for t, r in zip(mine, ref["tensors"]):
            t["p"], t["m"], t["v"] = r["p"], r["exp_avg"], r["exp_avg_sq"]
        assert it != 1 or len(classes) == 2
        assert it != 2 or len(classes) == 3                     # the skipped parameter is a step behind its group
    for i, (p, t) in enumerate(zip(P, mine)):
        st = opt.state[p]
        assert int(st["step"]) == steps[i] == (2 if i == 2 else 3)
        for got, want in ((t["p"], p.detach().numpy()), (t["m"], st["exp_avg"].numpy()), (t["v"], st["exp_avg_sq"].numpy())):
            assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), i


def test_reference_rounds_its_scalars_to_float32_like_the_library():
    t = [{"p": np.ones(3), "g": np.ones(3), "m": np.zeros(3), "v": np.zeros(3), "cls": 0, "skip": False}]
    a = R.adamw_multi_ref(t, [(1e-2, 0.05, 1)], 0.9, 0.999, 1e-8, 0.0, 1.0)
    b = R.adamw_multi_ref(t, [(R.f32(1e-2), R.f32(0.05), 1)], R.f32(0.9), R.f32(0.999), R.f32(1e-8), 0.0, 1.0)
    assert np.array_equal(a["tensors"][0]["p"], b["tensors"][0]["p"])


def test_teacher_forcing_takes_the_clip_factor_from_the_given_norm():
    T, Cl, h, _ = R.case_inputs("m1")
    free = R.adamw_multi_ref(T, Cl, **h)
    forced = R.adamw_multi_ref(T, Cl, **h, norm=free["norm"] * 2)
    assert forced["norm"] == free["norm"]
    i = next(i for i, t in enumerate(T) if not t["skip"] and len(t["g"]) > 8)
    assert np.allclose(forced["tensors"][i]["exp_avg"], free["tensors"][i]["exp_avg"] / 2, rtol=1e-6)     # max_norm below the norm: clip halves


# ------------------------------------------------------------------------------------------------ the float32 restatement: K, seeded errors
@pytest.fixture(scope="module")
def evaluated():
    out = {}
    for name in R.CASE_NAMES:
        T, Cl, h, _ = R.case_inputs(name)
        got = R.adamw_multi_f32(T, Cl, **h)
        out[name] = (T, Cl, h, got, R.adamw_multi_ref(T, Cl, **h, norm=got["norm"]))
    return out


def test_float32_ratios_give_K(evaluated):
    """the worst ratio of the float32 CPU evaluation per family over the GPU test's cases: the update's stay below optim_ref.K / 2 (it is
    adamw_update4's order), and the norm's K is twice its worst (rounded up)"""
    worst = {}
    for name, (T, Cl, h, got, ref) in evaluated.items():
        for fam, x in R.ratios(got, ref).items():
            assert math.isfinite(x), (name, fam)
            worst[fam] = max(worst.get(fam, 0.0), x)
            assert x <= R.K[fam] / 2, (name, fam, x)
    print("\nworst over the cases: " + "  ".join(f"{f} {x:.3f} (K {R.K[f]})" for f, x in worst.items()))
    assert R.K["norm"] / 2 <= 1.1 * worst["norm"] + 0.01, worst             # tied to the measurement, not chosen
    from .optim_ref import K as K_UPDATE
    assert all(R.K[f] == K_UPDATE[f] for f in R.FAMILIES)


def test_the_cases_are_the_issues(evaluated):
    C_ = R.CHUNK
    sizes = [n for n, _, _, _ in R.EDGES]
    assert {1, 3, 4, 5, C_ - 1, C_, C_ + 1, 2 * C_ + 3, 300000} <= set(sizes)
    assert any(h == 1 and gh == 1 and n > C_ for n, h, gh, _ in R.EDGES) and any(s for _, _, _, s in R.EDGES)
    assert len(R.MANY) == 130 and all(1 <= n <= 70 for n, _, _, _ in R.MANY) and any(s for _, _, _, s in R.MANY)
    assert sum((n + h + C_ - 1) // C_ for n, h, _, _ in R.WRAP) > 2048
    steps = {s for c in R.CASES for s in c[2]}
    assert {1, 2, 1000} <= steps
    assert {c[3] > 1 for c in R.CASES} == {True, False} and any(0 < c[3] < 1 for c in R.CASES) and any(c[3] <= 0 for c in R.CASES)
    assert any(c[4] == 0.5 for c in R.CASES) and R.WD == (0.01, 0.0) and R.LR[0] != R.LR[1]
    for name, (T, Cl, h, got, ref) in evaluated.items():
        assert {t["cls"] for t in T if not t["skip"]} == {0, 1}, name


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_every_seeded_error_is_rejected_on_a_case(evaluated, variant):
    hit = []
    for name, (T, Cl, h, _, _) in evaluated.items():
        got = R.adamw_multi_f32(T, Cl, **h, variant=variant)
        if R.rejects(got, R.adamw_multi_ref(T, Cl, **h, norm=got["norm"])):
            hit.append(name)
    assert hit, variant
    if variant == "clip_no_1e6":
        assert hit == ["tiny"]


def test_bf16_rne_is_torchs_rounding():
    rng = np.random.default_rng(3)
    x = rng.standard_normal(4096).astype(np.float32)
    bits = x.view(np.uint32).copy()
    bits[:512] = (bits[:512] & 0xFFFF0000) | 0x8000              # ties, under even and odd upper halves
    x = bits.view(np.float32)
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(R.bf16_rne(x), want)


# ------------------------------------------------------------------------------------------------ ModuleAdamW: constructor, state_dict
def _params(*shapes):
    return [torch.nn.Parameter(torch.randn(*s)) for s in shapes]


def test_constructor_rules():
    P = _params((3, 4), (5,), (2, 2))
    for bad in (dict(lr=0.0), dict(lr=-1.0), dict(eps=0.0), dict(betas=(1.0, 0.999)), dict(betas=(0.9, -0.1)), dict(weight_decay=-1e-3)):
        with pytest.raises(ValueError):
            ModuleAdamW(P, **bad)
    ModuleAdamW([{"params": P[:1], "lr": 1e-4, "weight_decay": 0.0}, {"params": P[1:]}], lr=1e-3, weight_decay=0.01)      # allowed to differ
    with pytest.raises(NotImplementedError):
        ModuleAdamW([{"params": P[:1], "betas": (0.8, 0.999)}, {"params": P[1:]}])
    with pytest.raises(NotImplementedError):
        ModuleAdamW([{"params": P[:1], "eps": 1e-6}, {"params": P[1:]}])
    with pytest.raises(NotImplementedError):
        ModuleAdamW([{"params": P, "amsgrad": True}])
    # mirrors: the parameter's element count, contiguous, bf16 or fp32, on its device, and only for a parameter of the optimiser
    ModuleAdamW(P, mirrors={P[0]: torch.zeros(12, dtype=torch.bfloat16), P[1]: torch.zeros(5)})
    for bad in (torch.zeros(11, dtype=torch.bfloat16), torch.zeros(12, dtype=torch.float16), torch.zeros(24, dtype=torch.bfloat16)[::2],
                torch.zeros(12, dtype=torch.float64), "x"):
        with pytest.raises(ValueError):
            ModuleAdamW(P, mirrors={P[0]: bad})
    with pytest.raises(ValueError):
        ModuleAdamW(P[:2], mirrors={P[2]: torch.zeros(4)})
    opt = ModuleAdamW(P, lr=1e-3, max_grad_norm=1.0)
    assert isinstance(opt, torch.optim.Optimizer) and opt.max_grad_norm == 1.0 and opt.table_uploads == 0 and opt.last_grad_norm is None
    opt.step()                                                             # (no gradient anywhere: a no-op, and the scheduler sees a step before its own)
    torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.5).step()          # a scheduler drives it
    assert opt.param_groups[0]["lr"] == pytest.approx(5e-4)


def test_step_refuses_cpu_parameters_closures_and_takes_no_gradients():
    P = _params((3, 4), (5,))
    opt = ModuleAdamW(P, max_grad_norm=1.0)
    with pytest.raises(NotImplementedError):
        opt.step(closure=lambda: 0.0)
    assert float(opt.step()) == 0.0 and all(p._version == 0 for p in P) and not opt.state_dict()["state"]      # no gradient anywhere: torch's no-op
    before = [p.detach().clone() for p in P]
    P[0].grad = torch.ones_like(P[0])
    with pytest.raises(RuntimeError, match="CUDA"):
        opt.step()                                                         # no CPU path, and nothing moved
    assert all(torch.equal(p, b) for p, b in zip(P, before))
    opt.zero_grad()                                                        # torch's meaning: set_to_none
    assert P[0].grad is None


def test_state_dict_has_torch_adamws_format():
    P = _params((3, 4), (5,), (2,))
    groups = lambda: [{"params": P[:1], "lr": 1e-4, "weight_decay": 0.0}, {"params": P[1:]}]      # noqa: E731
    ref = torch.optim.AdamW(groups(), lr=1e-3, weight_decay=0.01)
    for p in P[:2]:
        p.grad = torch.randn_like(p)
    ref.step()
    want = ref.state_dict()
    opt = ModuleAdamW(groups(), lr=1e-3, weight_decay=0.01)
    empty = opt.state_dict()
    assert set(empty) == set(want) == {"state", "param_groups"} and empty["state"] == {}
    assert [set(g) for g in empty["param_groups"]] == [set(g) for g in want["param_groups"]]
    assert [g["params"] for g in empty["param_groups"]] == [g["params"] for g in want["param_groups"]]
    opt.load_state_dict(want)                                              # torch -> ModuleAdamW
    got = opt.state_dict()
    assert set(got["state"]) == set(want["state"]) == {0, 1}               # the parameter never stepped has no state, as in torch
    for i in got["state"]:
        assert set(got["state"][i]) == set(want["state"][i]) == {"step", "exp_avg", "exp_avg_sq"}
        assert float(got["state"][i]["step"]) == 1.0
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(got["state"][i][k], want["state"][i][k]) and got["state"][i][k].shape == P[i].shape
    back = torch.optim.AdamW(groups(), lr=5e-2)                            # ModuleAdamW -> torch
    back.load_state_dict(got)
    for p in P[:2]:
        p.grad = torch.randn_like(p)
    back.step()
    assert int(back.state[P[0]]["step"]) == 2 and back.param_groups[0]["lr"] == 1e-4 and back.param_groups[1]["weight_decay"] == 0.01


def test_trainer_config_field_is_off_by_default():
    from mmdeer.trainer import TrainingConfig
    assert TrainingConfig().module_optimizer is False
