"""One HIP graph for a training step that runs through autograd: forward, loss, backward and ``optim.ModuleAdamW(capturable=True)``.

``capture_train_step(step_fn, optimizer, static_inputs)`` records ``loss = step_fn(*static_inputs); loss.backward(); optimizer.step()``
once and returns ``replay``: each call of it copies a new batch into the static inputs and replays the several hundred launches of the
step without host work between them -- the BERT fine-tuning step (``BertEncoder(finetune_layers=k, dropout=True)`` under
``TemporalTextEncoder``) and the end-to-end step (``encoders.EndToEndDEER``: the three encoders, a fusion module, the DEER head and
the loss) are bound by the host's launch rate at small batches.  A replay repeats the kernel arguments of the capture, so
what must differ between steps lives on the device:

  dropout steps    every module under the optimiser's module (``ModuleAdamW.for_module``) or under ``modules`` that offers
                   ``set_step_counter`` gets a one-element int64 counter of its own, starting at the module's host step; at the end of
                   the captured region each counter takes the number of live forwards its module ran in the region (one small add
                   per module that drew, recorded with the step), so replay r draws the masks the r-th eager step would have drawn
                   (``stepcount.py`` states the protocol; ``bert.py`` and ``text.py`` state it for themselves)
  Adam's step      the optimiser's device records (``ModuleAdamW(capturable=True)``)
  lr, weight decay the same records; ``replay`` refreshes them when ``param_groups`` moved (an LR scheduler between replays)

Warm-up steps run first on a side stream (torch's rule for captures: allocator pools, the library, the optimiser's buffers and its
table exist before the capture).  They are not training steps: parameters, the modules' buffers and packed operands, moments, step
counts and dropout counters are then put back, in place, to what they were before the call, so a replay loop and an eager loop from
the same start can be compared bit for bit.  Gradients are set to None before the capture: autograd then assigns them from the
graph's pool, where the optimiser's captured table upload finds them at every replay.  The graph is one linear chain on one stream."""
from __future__ import annotations

from typing import Iterable, Optional, Sequence

import torch
from torch import nn

from .optim import ModuleAdamW


def _counted_modules(optimizer, modules) -> list:
    roots = list(modules) if modules is not None else []
    if optimizer._module is not None:
        roots.append(optimizer._module)
    roots += list(optimizer._owners)
    found, seen = [], set()
    for r in roots:
        if not isinstance(r, nn.Module):
            raise TypeError(f"capture_train_step: modules must be torch.nn.Modules (got {type(r).__name__})")
        for m in r.modules():            # a parent before its children: a child's own counter replaces the one its parent handed down
            if id(m) not in seen and hasattr(m, "set_step_counter") and hasattr(m, "take_step_count"):
                seen.add(id(m))
                found.append(m)
    return found


def capture_train_step(step_fn, optimizer, static_inputs: Sequence[torch.Tensor], modules: Optional[Iterable[nn.Module]] = None,
                       warmup: int = 2):
    """Capture ``loss = step_fn(*static_inputs)`` (a scalar tensor), ``loss.backward()`` and ``optimizer.step()`` as one HIP graph.

    ``optimizer``: an ``optim.ModuleAdamW`` built with ``capturable=True``.  ``static_inputs``: CUDA tensors; the graph reads THESE
    tensors, so ``replay`` copies into them.  ``modules``: where to look for modules with dropout step counters besides the optimiser's
    own module (``ModuleAdamW.for_module``).  ``warmup`` >= 1 eager steps precede the capture and are undone (the module docstring).

    Returns ``replay(*new_inputs) -> loss``: the static loss tensor of the graph (clone what must outlive the next replay).  A
    ``None`` among ``new_inputs`` keeps what the static input holds; another count, shape or dtype raises ``ValueError``.
    ``replay.graph``, ``replay.static_inputs``, ``replay.loss`` and ``replay.counters`` ([(module, counter tensor)]) are exposed."""
    if not callable(step_fn):
        raise TypeError("capture_train_step: step_fn must be callable")
    if not isinstance(optimizer, ModuleAdamW) or not optimizer.capturable:
        raise TypeError("capture_train_step: the optimiser must be an optim.ModuleAdamW built with capturable=True (its step count and "
                        "table upload are then device work that a capture records)")
    if isinstance(warmup, bool) or not isinstance(warmup, int) or warmup < 1:
        raise ValueError(f"capture_train_step: warmup must be an integer >= 1 (got {warmup!r}): the first step builds what a capture cannot")
    static = list(static_inputs)
    if not static or not all(isinstance(t, torch.Tensor) and t.is_cuda for t in static):
        raise ValueError("capture_train_step: static_inputs must be a non-empty sequence of CUDA tensors")
    counted = _counted_modules(optimizer, modules)
    dev = static[0].device

    # ---- what the warm-up may change, as it is now
    roots = [m for m in ([optimizer._module] if optimizer._module is not None else []) + list(modules or []) + list(optimizer._owners)]
    tensors, seen = [], set()
    for t in [p for r in roots for p in r.parameters()] + [b for r in roots for b in r.buffers()] + list(optimizer._params):
        if id(t) not in seen:
            seen.add(id(t))
            tensors.append(t)
    saved = [t.detach().clone() for t in tensors]
    opt_snap = optimizer.snapshot()
    host_steps = [(m, m._train_step) for m in counted]
    counters = [(m, torch.full((1,), int(m._train_step), dtype=torch.int64, device=dev)) for m in counted]
    for m, t in counters:
        m.set_step_counter(t)

    def region():
        loss = step_fn(*static)
        if not isinstance(loss, torch.Tensor) or loss.numel() != 1:
            raise ValueError("capture_train_step: step_fn must return a scalar tensor (the loss)")
        loss.backward()
        optimizer.step()
        for m, t in counters:
            k = m.take_step_count()              # the steps this region used: the next replay starts behind them
            if k:                                # (a module that drew nothing -- a DEER head run by its owner, eval() -- costs no launch)
                t.add_(k)
        return loss

    def drop_grads():
        for p in optimizer._params:
            p.grad = None

    try:
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(warmup):
                drop_grads()
                region()
        torch.cuda.current_stream(dev).wait_stream(side)
        # ---- undo the warm-up, in place
        with torch.no_grad():
            for t, was in zip(tensors, saved):
                t.copy_(was)
        optimizer.restore(opt_snap)
        for m in optimizer._owners:
            m._operands()                        # the packed operands of the restored parameters (the copies above moved the versions)
        optimizer._refresh_owner_mirrors()
        for (m, t), (_, step) in zip(counters, host_steps):
            t.fill_(int(step))
            m.take_step_count()
        drop_grads()
        torch.cuda.synchronize(dev)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            loss = region()
    except BaseException:
        for m, _ in counters:
            m.set_step_counter(None)
        raise

    def replay(*new_inputs):
        if len(new_inputs) != len(static):
            raise ValueError(f"replay: expected {len(static)} inputs (None keeps one), got {len(new_inputs)}")
        for i, (dst, src) in enumerate(zip(static, new_inputs)):
            if src is None:
                continue
            if not isinstance(src, torch.Tensor) or tuple(src.shape) != tuple(dst.shape) or src.dtype != dst.dtype:
                got = (tuple(src.shape), src.dtype) if isinstance(src, torch.Tensor) else type(src).__name__
                raise ValueError(f"replay: input {i} must have the captured shape and dtype {(tuple(dst.shape), dst.dtype)}, got {got}")
        for dst, src in zip(static, new_inputs):
            if src is not None:
                dst.copy_(src, non_blocking=True)
        optimizer.refresh_hyper()
        graph.replay()
        return loss

    replay.graph, replay.static_inputs, replay.loss, replay.counters = graph, static, loss, counters
    return replay
