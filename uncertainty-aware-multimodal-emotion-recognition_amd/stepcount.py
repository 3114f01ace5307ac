"""The dropout step-counter protocol of a module, stated once (``bert.py`` and ``text.py`` state the same rules for themselves).

A module with counter-hash dropout keeps a host step, ``_train_step``, that advances by one per forward in which dropout is live; its
launches get ``(p, seed, step)``.  A CAPTURED GRAPH replays the kernel arguments it recorded, so the host's step would freeze:

  set_step_counter(t)   ``t`` a one-element int64 tensor on the module's device: live forward number k = 0, 1, ... since
                        ``take_step_count()`` last returned draws at step k + *t, read on the device when the kernels run (the launches
                        get ``(p, seed, k, t)``: ``opseq.set_drop`` forwards the fourth element as ``offset_dev``, and the three
                        by-value entries go through their ``_dev`` twins, include/mmdeer_drop_dev.h).  ``None`` returns to the host
                        counter, which continues where it was.
  take_step_count()     live forwards since the last call (or since the counter was set); restarts at 0.  The owner of a captured graph
                        adds it to ``t`` at the end of the captured region (``mmdeer.train_graph.capture_train_step``).
  _train_step           the host step, readable.

With no counter set nothing changes: the same tuple, the same entries, the same bits.

``StepCounted`` is for modules that keep ``_train_step`` themselves (the audio and video encoders); ``DropOwner`` for modules that
keep it in a ``fusions._Drop`` (the DEER head, the fusion modules), where ``_train_step`` reads and writes ``_drop.step``."""
from __future__ import annotations

from typing import Optional

import torch


class StepCounted:
    """Mixin of an ``nn.Module`` with parameters and a ``_train_step`` attribute.  ``_drop_step(p, seed)`` is the module's one way to
    draw the dropout tuple of a live forward."""

    _step_counter: Optional[torch.Tensor] = None
    _counter_k = 0

    def _drop_step(self, p: float, seed: int):
        if self._step_counter is not None:           # the step on the device
            d = (p, int(seed), self._counter_k, self._step_counter)
            self._counter_k += 1
            return d
        d = (p, int(seed), self._train_step)
        self._train_step += 1
        return d

    def set_step_counter(self, t: Optional[torch.Tensor]) -> None:
        """Take the dropout step from the device (the module docstring), or with ``None`` from the host again."""
        if t is not None:
            dev = next(self.parameters()).device
            if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.numel() != 1 or t.device != dev:
                raise ValueError(f"set_step_counter: expected a one-element int64 tensor on {dev}, got "
                                 f"{(t.dtype, tuple(t.shape), t.device) if isinstance(t, torch.Tensor) else type(t).__name__}")
        self._step_counter, self._counter_k = t, 0

    def take_step_count(self) -> int:
        """live forwards since the last call (or since the counter was set); restarts at 0"""
        k, self._counter_k = self._counter_k, 0
        return k


class DropOwner(StepCounted):
    """Mixin of a module whose dropout state is ``self._drop``, a ``fusions._Drop``: its ``step`` IS the host step."""

    @property
    def _train_step(self) -> int:
        return self._drop.step

    @_train_step.setter
    def _train_step(self, v: int) -> None:
        self._drop.step = v


def counter_ptr(drop) -> Optional[int]:
    """the device counter's address of a dropout tuple ``(p, seed, step[, counter])``, or None"""
    return drop[3].data_ptr() if drop is not None and len(drop) > 3 and drop[3] is not None else None
