#!/usr/bin/env python3
"""Do two builds of the library store the same bits in every operator of the BERT trunk?

    python tools/bert_ab_equal.py <library A> <library B> [--out listing.json]

One fresh child process per library, one after the other (the library is chosen as tools/bench_with_lib.py chooses it: both must
export every symbol of this tree's headers, so a build from before a header was added does not load); a child that ends abnormally
ends the tool before the next one starts.  The child runs the operator tests of tests/test_gpu_bert.py, tests/test_gpu_bert_backward.py
and tests/test_gpu_bert_dropout.py themselves, every parametrised case in fp32 and bf16, with a library
handle that after each ``mmdeer_bert_*`` call prints the sha256 of what the call stored -- so the shapes, masks, paddings and
inputs are the tests' own:
  mmdeer_bert_attn_fwd / _bwd      L in {1, 37, 64, 65, 129, 512}, 2 and 12 heads, the five masks (a dead sample among them), scores
                                   to +-80; ctx, dqkv and the log-sum-exp / delta workspace
  mmdeer_bert_embed_fwd            (B, L) in {(1, 1), (1, 5), (2, 67)} x H in {128, 768, 1024}, with and without type ids
  mmdeer_bert_add_ln_fwd / _bwd    the tests' M x N, with and without x / g2, in place, with and without the column sums
  mmdeer_bert_gelu_fwd / _bwd      the erf grids, out of place and in place
  the five dropout entries         (include/mmdeer_bert_drop.h) the dropout tests' attention, add-LN and embedding cases, p in {0, 0.1, 0.5}
  their five _dev twins at NULL    (include/mmdeer_graph.h) the same cases once more, every call of a dropout entry sent to its twin with
                                   a NULL counter, listed under "dev NULL: <case>"; within a listing each must equal its plain case
Then one forward + backward of the tiny and the 768-wide module with finetune_layers 1 and 2 (the tests' ``backward_once``):
last_hidden_state, every hidden state, every parameter gradient, and again every launch on the way.
The parent compares the two listings and exits 1 at the first difference, naming the case and the tensor."""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 900     # seconds

# what a call stores: field -> (rows, leading dimension, columns, "act" for the compute dtype or "f32"), from the argument struct
STORED = {
    "mmdeer_bert_embed_fwd": {"x": lambda a: (a.B * a.L, a.ld_x, a.H, "act")},
    "mmdeer_bert_attn_fwd": {"ctx": lambda a: (a.B * a.L, a.ld_ctx, a.H, "act")},
    "mmdeer_bert_add_ln_fwd": {"out": lambda a: (a.M, a.ld_out, a.N, "act")},
    "mmdeer_bert_gelu_fwd": {"out": lambda a: (a.M, a.ld_out, a.N, "act")},
    "mmdeer_bert_attn_bwd": {"dqkv": lambda a: (a.B * a.L, a.ld_dqkv, 3 * a.H, "act"),
                             "workspace": lambda a: (1, 0, a.workspace_bytes // 4, "f32")},
    "mmdeer_bert_add_ln_bwd": {"ds": lambda a: (a.M, a.ld_ds, a.N, "act"), "dgamma": lambda a: (1, 0, a.N, "f32"),
                               "dbeta": lambda a: (1, 0, a.N, "f32")},
    "mmdeer_bert_gelu_bwd": {"dx": lambda a: (a.M, a.ld_dx, a.N, "act")},
}
STORED.update({
    "mmdeer_bert_embed_drop_fwd": STORED["mmdeer_bert_embed_fwd"], "mmdeer_bert_attn_drop_fwd": STORED["mmdeer_bert_attn_fwd"],
    "mmdeer_bert_drop_add_ln_fwd": STORED["mmdeer_bert_add_ln_fwd"], "mmdeer_bert_attn_drop_bwd": STORED["mmdeer_bert_attn_bwd"],
    "mmdeer_bert_drop_add_ln_bwd": {**STORED["mmdeer_bert_add_ln_bwd"], "dy": lambda a: (a.M, a.ld_dy, a.N, "act")},
})
DROP = [n for n in STORED if "drop" in n]
STORED.update({n + "_dev": STORED[n] for n in DROP})
DEV_NULL = "dev NULL: "


def child(lib_path):
    sys.path.insert(0, ROOT)
    from mmdeer import build
    build.LIB_PATH = os.path.abspath(lib_path)
    build.needs_build = lambda: False
    import contextlib
    import gc
    import io
    import itertools

    import torch

    from mmdeer import _lib
    from tests import test_gpu_bert as TF
    from tests import test_gpu_bert_backward as TB
    from tests import test_gpu_bert_dropout as TD
    from tests.test_cpu_bert_backward import upstream

    real, where, out, to_dev = _lib.load(), ["", 0], sys.stdout, [False]

    def digest(t):
        return hashlib.sha256(t.detach().reshape(-1).contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()

    def emit(case, name, hexdigest):
        print(f"{case}\t{name}\t{hexdigest}", file=out, flush=True)

    def stored_bytes(ptr, nbytes):
        """the bytes at a device address, out of the live tensor whose storage holds them"""
        for t in gc.get_objects():
            if isinstance(t, torch.Tensor) and t.is_cuda:
                s = t.untyped_storage()
                if s.data_ptr() <= ptr and ptr + nbytes <= s.data_ptr() + s.nbytes():
                    flat = torch.empty(0, dtype=torch.uint8, device=t.device).set_(s)
                    return flat[ptr - s.data_ptr():ptr - s.data_ptr() + nbytes]
        raise RuntimeError("no live tensor holds an output of the call")

    class Recording:
        """the library, with the stores of every mmdeer_bert_* call listed"""

        def __getattr__(self, name):
            if name not in STORED:
                return getattr(real, name)
            if to_dev[0] and name in DROP:                # the second pass: the _dev twin with a NULL counter, listed under its name
                name += "_dev"
                fn = lambda ref: getattr(real, name)(ref, None)      # noqa: E731
            else:
                fn = getattr(real, name)

            def call(ref, *rest):
                rc = fn(ref, *rest)
                a = ref._obj
                for field, shape in STORED[name].items():
                    ptr = getattr(a, field)                   # a c_void_p field: an int, or None
                    rows, ld, cols, kind = shape(a)
                    if rc != 0 or not ptr or rows * cols == 0:
                        continue
                    size = 4 if kind == "f32" or a.act_f32 else 2
                    torch.cuda.synchronize()
                    emit(f"{where[0]} call {where[1]} {name}", field, digest(stored_bytes(ptr, ((rows - 1) * ld + cols) * size)))
                where[1] += 1
                return rc
            return call

    _lib.load = lambda build_if_missing=True: Recording()

    def cases(fn):
        """the parametrised cases of a test function as keyword dicts"""
        combos = [{}]
        for mark in getattr(fn, "pytestmark", []):
            if mark.name == "parametrize":
                names = [n.strip() for n in mark.args[0].split(",")]
                combos = [dict(c, **dict(zip(names, v if len(names) > 1 else (v,)))) for c, v in itertools.product(combos, mark.args[1])]
        return combos

    for fn in (TF.test_attention_against_float64, TF.test_attention_at_512_tokens, TF.test_attention_with_large_scores,
               TF.test_embed_ln_against_float64, TF.test_add_ln_against_float64, TF.test_gelu_is_the_erf_form,
               TB.test_attention_backward_against_float64, TB.test_attention_backward_at_512_tokens,
               TB.test_attention_backward_with_large_scores, TB.test_add_ln_backward_against_float64, TB.test_gelu_backward_is_the_erf_forms,
               TD.test_attention_dropout_against_float64, TD.test_attention_dropout_at_512_tokens, TD.test_drop_add_ln_against_float64,
               TD.test_embed_dropout_on_the_golden_tables):
        for kw in cases(fn):
            where[:] = [f"{fn.__name__}[{' '.join(f'{k}={v}' for k, v in sorted(kw.items()))}]", 0]
            with contextlib.redirect_stdout(io.StringIO()):
                fn(**kw)
            assert where[1] > 0, where
    to_dev[0] = True
    for fn in (TD.test_attention_dropout_against_float64, TD.test_attention_dropout_at_512_tokens, TD.test_drop_add_ln_against_float64,
               TD.test_embed_dropout_on_the_golden_tables):
        for kw in cases(fn):
            where[:] = [f"{DEV_NULL}{fn.__name__}[{' '.join(f'{k}={v}' for k, v in sorted(kw.items()))}]", 0]
            with contextlib.redirect_stdout(io.StringIO()):
                fn(**kw)
            assert where[1] > 0, where
    to_dev[0] = False
    for which, k, compute in itertools.product(("tiny", "big"), (1, 2), ("fp32", "bf16")):
        config, sd, ids, mask, typ, H, _, _ = TB.module_case(which, compute, k)
        where[:] = [f"module {which} finetune_layers={k} {compute}", 0]
        result, grads = TB.backward_once(TB.encoder(config, sd, compute, k), ids, mask, typ, upstream(mask, H))
        emit(where[0], "last_hidden_state", digest(result.last_hidden_state))
        for i, s in enumerate(result.hidden_states):
            emit(where[0], f"hidden_states[{i}]", digest(s))
        for n, g in grads.items():
            if g is not None:
                emit(where[0], f"grad {n}", digest(g))
    torch.cuda.synchronize()


def listing(lib):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", lib], capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    if r.returncode != 0:
        sys.exit(f"the child of {lib} ended with status {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
    return [tuple(line.split("\t")) for line in r.stdout.splitlines() if line.count("\t") == 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="+")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.child:
        return child(a.libs[0])
    if len(a.libs) != 2:
        ap.error("two libraries")
    la, lb = listing(a.libs[0]), listing(a.libs[1])
    diff = next(((x, y) for x, y in zip(la, lb) if x != y), None)
    if diff is None and len(la) != len(lb):
        diff = (("listing", "length", str(len(la))), ("listing", "length", str(len(lb))))
    if diff is None:                                      # a _dev twin at NULL stores its plain entry's bits
        plain = {(c, t): h for c, t, h in la}
        for c, t, h in la:
            if c.startswith(DEV_NULL):
                want = plain.get((c[len(DEV_NULL):].replace("_dev", ""), t))
                if want != h:
                    diff = ((c, t, h), (c, t, str(want)))
                    break
    res = {"libraries": [os.path.basename(l) for l in a.libs], "tensors": len(la), "equal": diff is None and len(la) > 0,
           "first_difference": None if diff is None else {"case": diff[0][0], "tensor": diff[0][1], "a": diff[0][2], "b": diff[1][2]},
           "sha256_of_a": [f"{c} | {t} | {h}" for c, t, h in la]}      # B's are these, up to first_difference
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    if not res["equal"]:
        print(f"DIFFERENT: {res['first_difference']}")
        sys.exit(1)
    print(f"equal: {len(la)} tensors of {len(set(c for c, _, _ in la))} cases")


if __name__ == "__main__":
    main()
