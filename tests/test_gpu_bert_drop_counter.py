"""The device step counter of the BERT trunk's five dropout entries (include/mmdeer_graph.h: mmdeer_bert_*_dev) on the GPU.

Everything here is bit for bit: the _dev entries run the plain entries' kernels and differ only in where the step comes from, so
  (offset = a, *counter = c)  ==  the plain entry at offset = a + c,   for (a, c) in (0, 0), (3, 4), (0, 2^32 + 1)
  a NULL counter              ==  the plain entry
  the counter                 is not written
  p = 0                       ==  the non-dropout entry (the counter is not read)
at the tiny model's shapes: hidden 128, 2 heads, B = 2 with the second sample's mask cut to 3 valid tokens, L = 5 and L = 33 (the
latter crosses the attention kernels' 32-key block), fp32 and bf16, p = 0.1 and 0.5.  What the masks ARE is held to float64 by
tests/test_gpu_bert_dropout.py through the plain entries."""
import ctypes as C
import functools

import pytest
import torch

from mmdeer import _lib, bert

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
H, HEADS, V, P, B = 128, 2, 50, 40, 2
SEED = 2 ** 40 + 7
PAIRS = [(0, 0), (3, 4), (0, 2 ** 32 + 1)]
ENTRIES = ("embed_drop_fwd", "attn_drop_fwd", "drop_add_ln_fwd", "attn_drop_bwd", "drop_add_ln_bwd")
ARGS = {"embed_drop_fwd": "BertEmbedDropArgs", "attn_drop_fwd": "BertAttnDropArgs", "drop_add_ln_fwd": "BertDropAddLnArgs",
        "attn_drop_bwd": "BertAttnDropBwdArgs", "drop_add_ln_bwd": "BertDropAddLnBwdArgs"}
# the non-dropout counterpart of each entry: (symbol, argument struct)
PLAIN = {"embed_drop_fwd": ("mmdeer_bert_embed_fwd", "BertEmbedArgs"), "attn_drop_fwd": ("mmdeer_bert_attn_fwd", "BertAttnArgs"),
         "drop_add_ln_fwd": ("mmdeer_bert_add_ln_fwd", "BertAddLnArgs"), "attn_drop_bwd": ("mmdeer_bert_attn_bwd", "BertAttnBwdArgs"),
         "drop_add_ln_bwd": ("mmdeer_bert_add_ln_bwd", "BertAddLnBwdArgs")}
SITES = {"embed_drop_fwd": bert.SITE_EMBED, "attn_drop_fwd": bert.site(1, 0), "drop_add_ln_fwd": bert.site(1, 1), "attn_drop_bwd": bert.site(1, 0),
         "drop_add_ln_bwd": bert.site(2, 2)}


@functools.lru_cache(maxsize=None)
def inputs(entry, L, compute):
    """the operands of one entry, drawn once per (entry, L, dtype) and never written"""
    g = torch.Generator().manual_seed(100 * ENTRIES.index(entry) + L)
    dt = torch.float32 if compute == "fp32" else torch.bfloat16
    M = B * L
    act = lambda *s: torch.randn(*s, generator=g).to(dt).to(DEV)                  # noqa: E731
    f32 = lambda *s: torch.randn(*s, generator=g).to(DEV)                          # noqa: E731
    mask = torch.ones(B, L)
    mask[1, 3:] = 0.0                                                              # one row cut to 3 valid tokens
    t = {"mask": mask.reshape(-1).to(DEV)}
    if entry == "embed_drop_fwd":
        t.update(ids=torch.randint(0, V, (M,), generator=g).to(DEV), word=f32(V, H), pos=f32(P, H), type=f32(2, H), gamma=f32(H), beta=f32(H))
    elif entry in ("attn_drop_fwd", "attn_drop_bwd"):
        t.update(qkv=act(M, 3 * H), dctx=act(M, H))
    else:
        t.update(y=act(M, H), x=act(M, H), g=act(M, H), gamma=f32(H), beta=f32(H))
    return t


def run(entry, L, compute, p, offset, counter=None, dev=True, plain=False):
    """One call -> the tensors it wrote.  ``dev``: the _dev entry with ``counter`` (a tensor, or None for NULL); else the plain dropout
    entry; ``plain``: the NON-dropout counterpart (p, offset and counter unused)."""
    lib, t, M = _lib.load(), inputs(entry, L, compute), B * L
    dt = torch.float32 if compute == "fp32" else torch.bfloat16
    a = getattr(_lib, ARGS[entry])()
    new = lambda *s, d=dt: torch.full(s, 7.0, dtype=d, device=DEV)                 # noqa: E731
    out = {}
    if entry == "embed_drop_fwd":
        out["x"] = new(M, H)
        a.ids, a.word, a.pos, a.type, a.gamma, a.beta = (t[k].data_ptr() for k in ("ids", "word", "pos", "type", "gamma", "beta"))
        a.x = out["x"].data_ptr()
        a.eps, a.B, a.L, a.H, a.V, a.P, a.T, a.ld_x = 1e-12, B, L, H, V, P, 2, H
    elif entry == "attn_drop_fwd":
        out["ctx"] = new(M, H)
        a.qkv, a.mask, a.ctx = t["qkv"].data_ptr(), t["mask"].data_ptr(), out["ctx"].data_ptr()
        a.B, a.L, a.H, a.ld_qkv, a.ld_ctx = B, L, H, 3 * H, H
    elif entry == "drop_add_ln_fwd":
        out["out"] = new(M, H)
        a.y, a.x, a.gamma, a.beta, a.out = t["y"].data_ptr(), t["x"].data_ptr(), t["gamma"].data_ptr(), t["beta"].data_ptr(), out["out"].data_ptr()
        a.eps, a.M, a.N, a.ld_y, a.ld_x, a.ld_out = 1e-12, M, H, H, H, H
    elif entry == "attn_drop_bwd":
        nbytes = lib.mmdeer_bert_attn_drop_bwd_workspace(B, L, H)
        out["dqkv"], ws = new(M, 3 * H), torch.zeros(nbytes // 4, device=DEV)
        a.qkv, a.mask, a.dctx, a.dqkv = t["qkv"].data_ptr(), t["mask"].data_ptr(), t["dctx"].data_ptr(), out["dqkv"].data_ptr()
        a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
        a.B, a.L, a.H, a.ld_qkv, a.ld_dctx, a.ld_dqkv = B, L, H, 3 * H, H, 3 * H
    else:
        n = lib.mmdeer_bert_drop_add_ln_bwd_scratch(M, H)
        out.update(ds=new(M, H), dgamma=new(H, d=torch.float32), dbeta=new(H, d=torch.float32))
        scratch = torch.zeros(n, device=DEV)
        a.y, a.x, a.g, a.gamma, a.ds = t["y"].data_ptr(), t["x"].data_ptr(), t["g"].data_ptr(), t["gamma"].data_ptr(), out["ds"].data_ptr()
        a.dgamma, a.dbeta, a.scratch, a.scratch_elems = out["dgamma"].data_ptr(), out["dbeta"].data_ptr(), scratch.data_ptr(), n
        a.eps, a.M, a.N, a.ld_y, a.ld_x, a.ld_g, a.ld_ds = 1e-12, M, H, H, H, H, H
        if not plain:
            out["dy"] = new(M, H)
            a.dy, a.ld_dy = out["dy"].data_ptr(), H
    a.act_f32, a.stream = int(compute == "fp32"), _lib.current_stream()
    if plain:
        sym, cls = PLAIN[entry]
        b = getattr(_lib, cls)()
        for name, _ in b._fields_:
            setattr(b, name, getattr(a, name))
        _lib.check(getattr(lib, sym)(C.byref(b)))
    else:
        a.site, a.dropout_p, a.seed, a.offset = SITES[entry], p, SEED, offset
        if dev:
            _lib.check(getattr(lib, f"mmdeer_bert_{entry}_dev")(C.byref(a), None if counter is None else counter.data_ptr()))
        else:
            _lib.check(getattr(lib, f"mmdeer_bert_{entry}")(C.byref(a)))
    torch.cuda.synchronize()
    return out


def same(got, want, what):
    assert set(got) == set(want), what
    for k in want:
        assert torch.equal(got[k], want[k]), f"{what}: {k} differs in {int((got[k] != want[k]).sum())} of {got[k].numel()} elements"


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("L", [5, 33])
@pytest.mark.parametrize("entry", ENTRIES)
def test_counter_plus_offset_is_the_plain_entry_at_the_sum(entry, L, p, compute):
    seen = []
    for a, c in PAIRS:
        counter = torch.tensor([c], dtype=torch.int64, device=DEV)
        assert counter.data_ptr() % 8 == 0
        got = run(entry, L, compute, p, a, counter)
        assert int(counter) == c, "the call wrote the counter"
        want = run(entry, L, compute, p, a + c, dev=False)
        same(got, want, f"{entry} at offset {a} + counter {c}")
        seen.append(want)
    first = next(iter(seen[0]))
    assert not torch.equal(seen[0][first], seen[1][first]) and not torch.equal(seen[1][first], seen[2][first]), "the step does not reach the masks"
    same(run(entry, L, compute, p, 5, None), run(entry, L, compute, p, 5, dev=False), f"{entry} with a NULL counter")


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
@pytest.mark.parametrize("L", [5, 33])
@pytest.mark.parametrize("entry", ENTRIES)
def test_p0_stores_the_non_dropout_entrys_bits(entry, L, compute):
    counter = torch.tensor([9], dtype=torch.int64, device=DEV)
    got = run(entry, L, compute, 0.0, 3, counter)
    want = run(entry, L, compute, 0.0, 0, plain=True)
    if entry == "drop_add_ln_bwd":
        assert torch.equal(got.pop("dy"), got["ds"]), "p = 0: dy is ds"
    same(got, want, f"{entry} at p = 0")
    assert int(counter) == 9
