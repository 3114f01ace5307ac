"""The HIP-graph replay of the BERT fine-tuning step without a GPU: the companion header include/mmdeer_graph.h through the strict
parser, its layout against the compiler, its symbols in the built library, the refusals of the new entries (all decided on the host,
before anything is launched), ModuleAdamW(capturable=True)'s host rules, capture_train_step's argument checks, and the bias
corrections of the capturable step against the float64 restatement's allowance (tests/optim_multi_ref.py)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from mmdeer import _header, _lib, bert, build, optim, text, train_graph
from mmdeer.optim import ModuleAdamW

from . import optim_multi_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DROP_DEV = {"mmdeer_bert_embed_drop_fwd_dev": "BertEmbedDropArgs", "mmdeer_bert_attn_drop_fwd_dev": "BertAttnDropArgs",
            "mmdeer_bert_drop_add_ln_fwd_dev": "BertDropAddLnArgs", "mmdeer_bert_attn_drop_bwd_dev": "BertAttnDropBwdArgs",
            "mmdeer_bert_drop_add_ln_bwd_dev": "BertDropAddLnBwdArgs"}
GRAPH_SYMBOLS = {**{n: 2 for n in DROP_DEV}, "mmdeer_adamw_multi_dev": 1, "mmdeer_adamw_multi_dev_uploads": 0, "mmdeer_adamw_multi_blocking_calls": 0}
GRAPH_STRUCTS = {"adamw_multi_class_dev", "adamw_multi_dev_args"}


# ------------------------------------------------------------------------------------------------ the C ABI additions
def test_new_symbols_are_declared_bound_and_exported():
    lib = _lib.load()
    assert {n: len(args) for n, _, args in _lib.GRAPH_SYMBOLS} == GRAPH_SYMBOLS
    for name, res, args in _lib.GRAPH_SYMBOLS:
        fn = getattr(lib, name)                                           # exported by the built library
        assert fn.restype is (C.c_longlong if not args else C.c_int32) and fn.argtypes == args, name
    assert set(_lib.GRAPH_STRUCTS) == GRAPH_STRUCTS and _lib.GRAPH_CONSTANTS == {}
    for name, cls in _lib.GRAPH_STRUCTS.items():                          # the ctypes mirrors against the library's own sizeof
        assert lib.mmdeer_sizeof(name.encode()) == C.sizeof(cls), name
    assert C.sizeof(_lib.AdamWMultiClassDev) == 16 == C.sizeof(_lib.AdamWMultiClass)
    new = {n for n, _, _ in _lib.GRAPH_SYMBOLS}
    for older in (_lib.SYMBOLS, _lib.VIDEO_SYMBOLS, _lib.FRAME_SYMBOLS, _lib.ROUTE_SYMBOLS, _lib.FRAME_BWD_SYMBOLS, _lib.BERT_SYMBOLS,
                  _lib.BERT_BWD_SYMBOLS, _lib.BERT_DROP_SYMBOLS, _lib.OPTIM_SYMBOLS):
        assert not new & {n for n, _, _ in older}
    assert _header.GRAPH_HEADER_PATH == build.GRAPH_HEADER_PATH
    assert os.path.samefile(build.GRAPH_HEADER_PATH, os.path.join(ROOT, "include", "mmdeer_graph.h"))
    assert lib.mmdeer_abi_version() == _lib.ABI_VERSION == 16            # additions only


def test_header_layout_matches_the_compiler(tmp_path):
    """Offsets and sizes of every field of the new structs, as ctypes lays them out, asserted by the compiler on the header -- read
    TOGETHER with the two headers whose structs it names as opaque types, in both orders."""
    body = []
    for cname, cls in _lib._GRAPH_CLASSES.items():
        body.append(f'static_assert(sizeof({cname}) == {C.sizeof(cls)}, "sizeof {cname}");')
        for field, _ in cls._fields_:
            d = getattr(cls, field)
            body.append(f'static_assert(offsetof({cname}, {field}) == {d.offset}, "offsetof {cname}.{field}");')
            body.append(f'static_assert(sizeof((({cname}*)0)->{field}) == {d.size}, "sizeof {cname}.{field}");')
    older = ['#include "mmdeer_bert_drop.h"', '#include "mmdeer_optim.h"']
    for k, includes in enumerate((older + ['#include "mmdeer_graph.h"'], ['#include "mmdeer_graph.h"'] + older, ['#include "mmdeer_graph.h"'])):
        tu = tmp_path / f"layout{k}.cpp"
        tu.write_text("\n".join(["#include <stddef.h>"] + includes + body) + "\n")
        r = subprocess.run([build._hipcc(), "-x", "c++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(tu)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
    src = _header.read(_header.GRAPH_HEADER_PATH)
    for bad in (src.replace("int mmdeer_adamw_multi_dev(", "int mmdeer_adamw_multi_dev(uint16_t f, "),                  # the same strict parser
                src.replace("#include <stdint.h>", "#include <stdint.h>\n#if 0\n#endif"),
                src.replace("float* scratch;", "float* scratch; short s;"),
                src.replace("typedef struct mmdeer_adamw_multi_tensor mmdeer_adamw_multi_tensor;", "")):
        assert bad != src
        with pytest.raises(_header.HeaderError):
            _header.parse(bad, _lib._GRAPH_NAMES, {})


# ------------------------------------------------------------------------------------------------ refusals (host side)
A = 1 << 20     # a plausible, aligned address: never dereferenced by the host checks


def refused(rc, match):
    assert rc == -1
    msg = _lib.load().mmdeer_last_error().decode()
    assert match in msg, msg


@pytest.mark.parametrize("name", sorted(DROP_DEV))
def test_dropout_counter_refusals(name):
    lib = _lib.load()
    fn = getattr(lib, name)

    def args(p=0.1, site=300):
        a = getattr(_lib, DROP_DEV[name])()
        a.dropout_p, a.site = p, site
        return a
    for off in (1, 2, 4, 7):
        refused(fn(C.byref(args()), A + off), "offset_dev must be 8-byte aligned")
    refused(fn(C.byref(args(p=0.0)), A + 4), "offset_dev must be 8-byte aligned")      # whatever p is
    # the plain entry's refusals come first and keep their text
    refused(fn(C.byref(args(p=1.0)), A), "dropout_p must be finite and in [0, 1)")
    refused(fn(C.byref(args(p=float("nan"))), A), "dropout_p must be finite and in [0, 1)")
    refused(fn(C.byref(args(site=-1)), A), "site must be >= 0")
    refused(fn(None, A), "NULL args")


def _dev_args(n=2, **kw):
    rec = (_lib.AdamWMultiTensor * max(n, 1))()
    for i in range(n):
        rec[i].param, rec[i].grad, rec[i].count, rec[i].moment_off, rec[i].cls = A + 4096 * i, 2 * A + 4096 * i, 100, 128 * i, i % 2
    a = _lib.AdamWMultiDevArgs()
    a.tensors, a.ntensors, a.nclasses, a.classes = C.cast(rec, C.c_void_p), n, 2, 8 * A
    a.exp_avg, a.exp_avg_sq, a.moment_elems = 3 * A, 4 * A, 256
    a.table, a.table_bytes, a.upload = 5 * A, 1 << 16, 1
    a.scratch, a.grad_norm = 6 * A, 7 * A
    a.beta1, a.beta2, a.eps, a.max_grad_norm, a.grad_scale = 0.9, 0.999, 1e-8, 1.0, 1.0
    a._keep = rec
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _dev_tensor(field, value, i=1):
    a = _dev_args()
    setattr(a._keep[i], field, value)
    return a


DEV_REFUSALS = {
    "null classes": (lambda: _dev_args(classes=None), "classes must be non-NULL"),
    "misaligned classes": (lambda: _dev_args(classes=8 * A + 8), "classes must be non-NULL device memory, 16-byte aligned"),
    "null tensors": (lambda: _dev_args(tensors=None), "tensors is NULL"),
    "negative ntensors": (lambda: _dev_args(ntensors=-1), "ntensors"),
    "no class": (lambda: _dev_args(nclasses=0), "classes (got 0)"),
    "17 classes": (lambda: _dev_args(nclasses=17), "classes (got 17)"),
    "beta1 of 1": (lambda: _dev_args(beta1=1.0), "betas"),
    "eps of 0": (lambda: _dev_args(eps=0.0), "eps"),
    "nan grad_scale": (lambda: _dev_args(grad_scale=float("nan")), "grad_scale"),
    "null exp_avg": (lambda: _dev_args(exp_avg=None), "exp_avg"),
    "null scratch": (lambda: _dev_args(scratch=None), "scratch"),
    "null table": (lambda: _dev_args(table=None), "table"),
    "misaligned table": (lambda: _dev_args(table=5 * A + 8), "table"),
    "small table": (lambda: _dev_args(table_bytes=64), "the table needs"),
    "null param": (lambda: _dev_tensor("param", None), "param / grad"),
    "misaligned grad": (lambda: _dev_tensor("grad", A + 1), "param / grad"),
    "misaligned bf16 mirror": (lambda: _dev_tensor("mirror", A + 1), "misaligned mirror"),
    "negative count": (lambda: _dev_tensor("count", -1), "count"),
    "class index above": (lambda: _dev_tensor("cls", 2), "class 2"),
    "moments past the buffers": (lambda: _dev_tensor("moment_off", 200), "pass the buffers"),
    "overlapping moments": (lambda: _dev_tensor("moment_off", 50), "overlap"),
}


@pytest.mark.parametrize("case", sorted(DEV_REFUSALS))
def test_adamw_multi_dev_refusals(case):
    lib = _lib.load()
    make, match = DEV_REFUSALS[case]
    before = lib.mmdeer_adamw_multi_dev_uploads(), lib.mmdeer_adamw_multi_uploads(), lib.mmdeer_adamw_multi_blocking_calls()
    refused(lib.mmdeer_adamw_multi_dev(C.byref(make())), match)
    assert before == (lib.mmdeer_adamw_multi_dev_uploads(), lib.mmdeer_adamw_multi_uploads(), lib.mmdeer_adamw_multi_blocking_calls())
    refused(lib.mmdeer_adamw_multi_dev(None), "args is NULL")


def test_adamw_multi_dev_without_elements_launches_nothing():
    a = _dev_args(n=2)
    for r in a._keep:
        r.count = 0
    assert _lib.load().mmdeer_adamw_multi_dev(C.byref(a)) == 0          # no chunk: no launch, no step, on a machine without a device too


# ------------------------------------------------------------------------------------------------ ModuleAdamW's host rules
def test_a_non_capturable_step_inside_a_capture_raises_before_the_library(monkeypatch):
    p = torch.nn.Parameter(torch.zeros(5))
    p.grad = torch.ones(5)
    opt = ModuleAdamW([p])
    assert opt.capturable is False

    def no_library(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    monkeypatch.setattr(optim._lib, "load", no_library)
    with pytest.raises(RuntimeError, match="capturable=True"):
        opt.step()
    assert opt._steps == [0] and not opt.state


def test_capturable_step_refuses_another_live_set_and_names_the_parameter():
    lin = torch.nn.Linear(4, 3)
    opt = ModuleAdamW.for_module(lin, capturable=True)
    assert opt.capturable and opt.class_buffer is None
    opt._live0 = (0, 1)                          # what the first step leaves behind (it needs a device): weight and bias took part
    lin.weight.grad = torch.zeros(3, 4)
    with pytest.raises(RuntimeError, match=r"parameter bias has no gradient, unlike at the first step"):
        opt.step()
    opt._live0 = (0,)
    lin.bias.grad = torch.zeros(3)
    with pytest.raises(RuntimeError, match=r"parameter bias has gradient, unlike at the first step"):
        opt.step()
    anon = ModuleAdamW([torch.nn.Parameter(torch.zeros(2, 3)), torch.nn.Parameter(torch.zeros(7))], capturable=True)
    anon._live0 = (0,)
    anon._params[1].grad = torch.zeros(7)
    with pytest.raises(RuntimeError, match=r"parameter #0 of shape \(2, 3\) has no gradient"):
        anon.step()
    # there is still no CPU path: the first step of CPU parameters raises as the non-capturable one does
    fresh = ModuleAdamW.for_module(torch.nn.Linear(4, 3), capturable=True)
    for q in fresh._params:
        q.grad = torch.zeros_like(q)
    with pytest.raises(RuntimeError, match="no CPU path"):
        fresh.step()


def test_capturable_state_dict_keeps_torchs_format_on_the_host():
    lin = torch.nn.Linear(4, 3)
    ref = torch.optim.AdamW(lin.parameters(), lr=1e-3)
    for q in lin.parameters():
        q.grad = torch.ones_like(q)
    ref.step()
    ref.step()
    opt = ModuleAdamW(lin.parameters(), lr=1e-3, capturable=True)
    opt.load_state_dict(ref.state_dict())
    assert opt._steps == [2, 2] and opt._live0 is None and opt.class_buffer is None
    sd = opt.state_dict()
    assert sd["param_groups"][0].keys() == ref.state_dict()["param_groups"][0].keys()
    for k, st in ref.state_dict()["state"].items():
        assert float(sd["state"][k]["step"]) == 2.0 and sd["state"][k]["step"].dtype == torch.float32
        assert torch.equal(sd["state"][k]["exp_avg"], st["exp_avg"]) and torch.equal(sd["state"][k]["exp_avg_sq"], st["exp_avg_sq"])
    back = torch.optim.AdamW(lin.parameters(), lr=1e-3)
    back.load_state_dict(sd)
    back.step()
    assert all(float(st["step"]) == 3.0 for st in back.state.values())


# ------------------------------------------------------------------------------------------------ capture_train_step's argument checks
def test_capture_train_step_argument_checks():
    lin = torch.nn.Linear(4, 3)
    good = ModuleAdamW.for_module(lin, capturable=True)
    x = torch.zeros(2, 4)
    fn = lambda t: lin(t).sum()      # noqa: E731
    with pytest.raises(TypeError, match="callable"):
        train_graph.capture_train_step(None, good, [x])
    for bad in (ModuleAdamW.for_module(lin), torch.optim.AdamW(lin.parameters())):
        with pytest.raises(TypeError, match="capturable=True"):
            train_graph.capture_train_step(fn, bad, [x])
    for w in (0, -1, True, 1.5):
        with pytest.raises(ValueError, match="warmup"):
            train_graph.capture_train_step(fn, good, [x], warmup=w)
    for static in ([], [x], [None]):                   # empty, a CPU tensor, not a tensor
        with pytest.raises(ValueError, match="static_inputs"):
            train_graph.capture_train_step(fn, good, static)


def test_module_counters_host_rules():
    tiny = dict(vocab_size=50, hidden_size=128, num_hidden_layers=3, num_attention_heads=2, intermediate_size=256, max_position_embeddings=40)
    enc = bert.BertEncoder(tiny, "fp32", finetune_layers=2, dropout=True).train()
    assert enc._drop() == (0, 0) and enc._drop() == (0, 1) and enc._train_step == 2       # the host counter, as before
    t = torch.zeros(1, dtype=torch.int64)
    enc.set_step_counter(t)
    d0, d1 = enc._drop(), enc._drop()
    assert d0[:2] == (0, 0) and d1[:2] == (0, 1) and d0[2] is t and d1[2] is t
    assert enc._train_step == 2 and enc.take_step_count() == 2 and enc.take_step_count() == 0
    assert enc._drop()[:2] == (0, 0)
    enc.set_step_counter(None)
    assert enc._drop() == (0, 2)
    for bad in (torch.zeros(1), torch.zeros(2, dtype=torch.int64), 3):
        with pytest.raises(ValueError, match="one-element int64 tensor"):
            enc.set_step_counter(bad)
    assert enc.eval()._drop() is None
    wide = bert.BertEncoder(dict(tiny, hidden_size=768, num_attention_heads=12, num_hidden_layers=1), "fp32", finetune_layers=1, dropout=True)
    te = text.TemporalTextEncoder({"hidden_dim": 512}, "fp32", bert=wide).train()
    assert te._drop() == (0.3, 0, 0)
    te.set_step_counter(t)
    assert wide._step_counter is t                      # the trunk gets the same call
    d = te._drop()
    assert d[:3] == (0.3, 0, 0) and d[3] is t and te._train_step == 1 and te.take_step_count() == 1
    te.set_step_counter(None)
    assert wide._step_counter is None and te._drop() == (0.3, 0, 1)
    assert "Not built: a captured graph" not in bert.__doc__


# ------------------------------------------------------------------------------------------------ the capturable step's bias corrections
def pow_int(beta, n):
    """csrc/optim_multi.hip: beta^n by repeated squaring in float64, rounded once to float32"""
    b, r = float(np.float32(beta)), 1.0
    while n > 0:
        if n & 1:
            r *= b
        b *= b
        n >>= 1
    return np.float32(r)


def test_device_bias_corrections_are_within_the_restatements_allowance():
    """tests/optim_multi_ref.py allows POW_ULPS ulps of beta^step for the host's powf; the device's power must not need more.  An ulp
    of a float32 value x is at most 2 U |x| (U = 2^-24, the restatement's unit)."""
    worst = 0.0
    for beta in (R.BETA1, R.BETA2, 0.5, 0.99999):
        b = float(np.float32(beta))
        for n in list(range(1, 2001)) + [10 ** 4, 10 ** 5, 10 ** 6, 2 ** 31 - 1]:
            exact = b ** n                                   # float64: relative error far below U
            got = float(pow_int(beta, n))
            if exact < 2.0 ** -126:                          # below float32's normal range the bias correction is 1 to the bit
                assert np.float32(1) - np.float32(got) == np.float32(1)
                continue
            worst = max(worst, abs(got - exact) / (2 * R.U * exact))
    assert worst <= R.POW_ULPS, worst
    assert worst <= 0.5 + 1e-6, worst                        # in fact one rounding
    # ... and the float32 restatement of the step, whose bias corrections are the correctly rounded powers, stays inside K
    tensors, classes, hyper, _ = R.case_inputs("m2")
    got = R.adamw_multi_f32(tensors, classes, **hyper)
    assert not R.rejects(got, R.adamw_multi_ref(tensors, classes, norm=got["norm"], **hyper))
    assert math.isfinite(got["norm"])
