"""The references tests/test_gpu_stackb_step.py holds Stack B's training step to, checked on their own (no GPU): the oracle's
training-mode forward (``stackb_forward(masks=...)``) and the masks ``tests/stackb_ref.py`` draws for it.

The sensitivity test is what makes the GPU test a test of the dropout SITES: every mistake of the kind the step could make in its
operand tables -- two site numbers swapped, the attention sites' ``>> 5`` lost, the estimator given the config's p, the heads'
column offset off by one head -- moves the float64 loss or a gradient by at least ten times what that test tolerates, so none of
them can hide inside its bounds."""
import copy
import json
import os

import numpy as np
import pytest
import torch

from mmdeer import stackb, synth
from mmdeer.stackb_layers import HID, SITE_ATTN_C, SITE_ATTN_S, SITE_AV, SITE_EST, SITE_H0, SITE_H3, SITE_RES, SITE_TRI, SITE_WN
from oracle import deer_oracle as O

from . import stackb_ref as R
from .rowkernel_ref import drop_keep
from .test_oracle_golden import stackb_oracle_gradients

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
B, STEP = 33, 5
# test A's bounds (tests/test_gpu_stackb_step.py)
LOSS_REL, G_RTOL, G_ATOL = 3e-4, 3e-3, 3e-3


def _model(**cfg):
    with open(os.path.join(GOLDEN, "stackb_state_dict_names.json")) as fh:
        shapes = json.load(fh)
    m = stackb.CompleteDEERModel(stackb.ModelConfig(**cfg))
    P = {k: torch.from_numpy(v) for k, v in synth.module_fill("stackb2", shapes).items()}
    m.load_state_dict(P)
    return m, P


@pytest.fixture(scope="module")
def base():
    m, P = _model()
    b = synth.make_batch(B, seed=12)
    ss = R.sites(m)
    masks, p = R.oracle_masks(ss, R.draw(ss, B, int(m.config.dropout_seed), STEP), B)
    loss, grads = stackb_oracle_gradients(O, P, b, masks, p, dtype=torch.float64)
    return m, P, b, ss, masks, p, loss, grads


def test_sites_are_the_layer_records_and_constants(base):
    m, _, _, ss, masks, p, _, _ = base
    by = {s.name: s for s in ss}
    assert len(ss) == 9 + 3 + 1 + 2 + 6 and len(by) == len(ss)
    assert [by[f"res.{e}.{l}"].site for l in range(3) for e in range(3)] == list(range(SITE_RES, SITE_RES + 9))
    assert (by["attn_self"].site, by["attn_cross"].site, by["est"].site, by["wn"].site) == (SITE_ATTN_S, SITE_ATTN_C, SITE_EST, SITE_WN)
    assert (by["av"].site, by["tri"].site) == (SITE_AV, SITE_TRI)
    assert [(by[f"h0.{d}"].site, by[f"h0.{d}"].dcol) for d in range(3)] == [(SITE_H0, d * HID) for d in range(3)]
    assert [(by[f"h3.{d}"].site, by[f"h3.{d}"].dcol) for d in range(3)] == [(SITE_H3 + d, 0) for d in range(3)]
    assert by["attn_self"].shift == by["attn_cross"].shift == 5 and by["attn_self"].rows == by["est"].rows == 3
    assert by["est"].p == 0.2 and all(s.p == m.config.dropout for s in ss if s.name != "est")
    assert all(s.dcol == 0 and s.shift == 0 for s in ss if s.name[:2] not in ("h0", "at"))
    assert masks["attn_self"].shape == (B, 3, 8) and masks["est"].shape == (B, 3, 128) and masks["wn"].shape == (B, 256)
    assert masks["av"].shape == masks["tri"].shape == (B, 512) and masks["h0.1"].shape == (B, 256) and masks["h3.2"].shape == (B, 128)
    # the heads' first layers are one draw of (B, 768) at site H0; the attention sites one decision per (row, head)
    h0 = drop_keep(SITE_H0, B, 3 * HID, m.config.dropout, int(m.config.dropout_seed), STEP)
    assert np.array_equal(np.concatenate([masks[f"h0.{d}"].numpy() for d in range(3)], 1), h0.astype(np.float64))
    at = drop_keep(SITE_ATTN_C, 3 * B, 8, m.config.dropout, int(m.config.dropout_seed), STEP)
    assert np.array_equal(masks["attn_cross"].reshape(3 * B, 8).numpy(), at.astype(np.float64))
    # keep_masks is the same thing in one call; another step draws other masks
    m2, p2 = R.keep_masks(m, B, STEP)
    assert p2 == p and all(torch.equal(m2[k], masks[k]) for k in masks)
    m3, _ = R.keep_masks(m, B, STEP + 1)
    assert not any(torch.equal(m3[k], masks[k]) for k in masks)
    for k, v in masks.items():
        assert set(v.unique().tolist()) <= {0.0, 1.0} and abs(float(v.mean()) - (1 - p[k])) < 0.12, k


def test_config_dropout_zero_leaves_the_estimator_live():
    m, _ = _model(dropout=0.0)
    masks, p = R.keep_masks(m, B, STEP)
    assert list(masks) == ["est"] and p == {"est": 0.2}


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_all_ones_masks_equal_the_unmasked_oracle_exactly(base, dtype):
    _, P, b, _, masks, p, _, _ = base
    ones = {k: torch.ones_like(v) for k, v in masks.items()}
    l0, g0, o0 = stackb_oracle_gradients(O, P, b, dtype=dtype, outputs=True)
    l1, g1, o1 = stackb_oracle_gradients(O, P, b, ones, {k: 0.0 for k in p}, dtype=dtype, outputs=True)
    assert l0.dtype == dtype and torch.equal(l0, l1)
    for k in o0:
        assert o0[k].dtype == dtype and torch.equal(o0[k], o1[k]), k
    for k in g0:
        assert (g0[k] is None and g1[k] is None) or torch.equal(g0[k], g1[k]), k
    # and the default call is the eval forward it was
    with torch.no_grad():
        xs = [torch.from_numpy(b[k]) for k in ("audio", "video", "text")]
        assert torch.equal(O.stackb_forward(P, *xs)["mu_all"], O.stackb_forward(P, *xs, masks={}, p=0.3)["mu_all"])


def test_masked_oracle_runs_in_float64_and_applies_every_site(base):
    _, P, b, ss, masks, p, loss, grads = base
    assert loss.dtype == torch.float64 and all(g is None or g.dtype == torch.float64 for g in grads.values())
    # closing ONE site's first element (or opening it) moves the loss: no site is ignored
    for s in ss:
        m2 = dict(masks)
        k = masks[s.name].clone()
        k.view(-1)[:k.shape[-1]] = 1.0 - k.view(-1)[:k.shape[-1]]
        m2[s.name] = k
        l2, _ = stackb_oracle_gradients(O, P, b, m2, p, dtype=torch.float64)
        assert float((l2 - loss).abs()) > 1e-9 * float(loss.abs()), s.name
    # one key per query: the query / key projections get exact zeros
    for blk in ("self_attention", "cross_attention"):
        for q in ("query_proj", "key_proj"):
            for t in ("weight", "bias"):
                g = grads[f"attention_module.{blk}.{q}.{t}"]
                assert g is not None and float(g.abs().max()) == 0.0


def test_relu_decisions_of_the_reference(base):
    """``masks["relu_seen"]`` names all 29 ReLUs; a decision tensor of -1 changes nothing, exactly; forcing one unit moves its row;
    ``disputed_relus`` lets a decision differ only within RELU_BAND of zero."""
    _, P, b, _, masks, p, loss, grads = base
    seen = {}
    l1, g1 = stackb_oracle_gradients(O, P, b, dict(masks, relu_seen=seen), p, dtype=torch.float64)
    assert len(seen) == 3 * 4 + 6 + 1 + 4 + 6 and torch.equal(l1, loss)
    own = {k: torch.full(z.shape, -1, dtype=torch.int8) for k, z in seen.items()}
    l2, g2 = stackb_oracle_gradients(O, P, b, dict(masks, relu=own), p, dtype=torch.float64)
    assert torch.equal(l2, loss) and all(g is None or torch.equal(g2[k], g) for k, g in grads.items())
    z = seen["tri.4"]
    i, j = divmod(int(torch.where(z > 0, z, torch.full_like(z, 9.0)).argmin()), z.shape[1])      # the active unit closest to zero
    dec = {k: (v > 0, None) for k, v in seen.items()}
    assert R.disputed_relus(seen, dec) == ({}, [])
    on = dec["tri.4"][0].clone()
    on[i, j] = False
    dec["tri.4"] = (on, None)
    if float(z[i, j]) > R.RELU_BAND * float(z.abs().max()):
        with pytest.raises(AssertionError):
            R.disputed_relus(seen, dec)
    decide, rows = R.disputed_relus(seen, dec, band=1.0)
    assert list(decide) == ["tri.4"] and int((decide["tri.4"] >= 0).sum()) == 1 and int(decide["tri.4"][i, j]) == 0 and len(rows) == 1
    _, g3 = stackb_oracle_gradients(O, P, b, dict(masks, relu=decide), p, dtype=torch.float64)
    d = (g3["fusion_module.trimodal_fusion.4.weight"] - grads["fusion_module.trimodal_fusion.4.weight"]).abs().sum(1)
    rest = d.clone()
    rest[j] = 0.0
    assert float(d[j]) > 10.0 * float(rest.max())          # (the other rows move through the forward value only: by the unit's tiny input)


def _swap(ss):
    by = {s.name: s for s in ss}
    by["av"].site, by["tri"].site = by["tri"].site, by["av"].site


def _no_shift(ss):
    for s in ss:
        if s.name in ("attn_self", "attn_cross"):
            s.shift = 0


def _est_config_p(ss, pc):
    for s in ss:
        if s.name == "est":
            s.p = pc


def _heads_dcol(ss):
    for s in ss:
        if s.name.startswith("h0."):
            s.dcol = (s.dcol + HID) % (3 * HID)


MUTATIONS = {"two sites swapped (av, tri)": _swap, "attention sites without >> 5": _no_shift,
             "estimator at the config's p": lambda ss: _est_config_p(ss, 0.3), "heads' dcol off by one head": _heads_dcol}


@pytest.mark.parametrize("name", list(MUTATIONS))
def test_step_test_is_sensitive_to_the_sites(base, name):
    """B = 33, default config, batch seed 12, dropout step 5 (the shapes of test A's B = 33 case): no seed had to be chosen."""
    m, P, b, ss, _, _, loss, grads = base
    mut = copy.deepcopy(ss)
    MUTATIONS[name](mut)
    masks, p = R.oracle_masks(mut, R.draw(mut, B, int(m.config.dropout_seed), STEP), B)
    l2, g2 = stackb_oracle_gradients(O, P, b, masks, p, dtype=torch.float64)
    moved = float((l2 - loss).abs() / loss.abs()) / LOSS_REL
    worst = ("loss", moved)
    for k, g in grads.items():
        if g is None or float(g.abs().max()) == 0.0:
            continue
        r = float(((g2[k] - g).abs() / (G_RTOL * g.abs() + G_ATOL * g.abs().max())).max())
        if r > worst[1]:
            worst = (k, r)
    print(f"{name}: loss moved by {moved:.1f} x its bound; most moved: {worst[0]} by {worst[1]:.1f} x its bound")
    assert worst[1] >= 10.0, (name, worst)
