"""Optimiser step on the device: gradient clipping + AdamW fused with the weight pack (``FusedAdamW``, ``FlatAdamW``: one
model's flat gradient buffer each), and for any module that trains through autograd into ``.grad`` tensors (``ModuleAdamW``).

``FusedAdamW`` is a ``torch.optim.Optimizer`` (so the reference's LR schedulers drive it unchanged) whose
``step()`` is one call of ``mmdeer_adamw_step``: ``clip_grad_norm_`` + ``torch.optim.AdamW`` arithmetic on the flat
gradient buffer of ``MultimodalDEER.train_step``, in-place update of the fp32 parameters, and refresh of the packed
bf16 / transposed copies the GEMM kernels read -- the next ``train_step`` starts without a pack pass and nothing
synchronises with the host (reference semantics: src/training/training.py:121-150 optimiser and groups, :219-224
clip + step).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Iterable, Optional

import torch

from . import _lib


class FusedAdamW(torch.optim.Optimizer):
    def __init__(self, model, params: Optional[Iterable] = None, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 1e-2, max_grad_norm: float = 0.0):
        """``params``: parameters or torch-style groups (``{'params': [...], 'lr': ...}``); default all parameters of
        ``model``.  Parameters the fused backward never gives a gradient (the unreachable gating MLP) are accepted and
        left untouched, as torch's AdamW does for ``grad is None``."""
        if lr <= 0 or eps <= 0 or not (0 <= betas[0] < 1 and 0 <= betas[1] < 1) or weight_decay < 0:
            raise ValueError("FusedAdamW: bad hyper-parameters")
        groups = list(params) if params is not None else list(model.parameters())
        super().__init__(groups, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay))
        self.model = model
        self.max_grad_norm = float(max_grad_norm)
        self._live = model.live_parameters()
        hyper = {(g["betas"], g["eps"], g["weight_decay"]) for g in self.param_groups}
        if len(hyper) != 1:
            raise NotImplementedError("FusedAdamW: betas / eps / weight_decay must be the same in every group (lr may differ)")
        owner = {}
        for gi, g in enumerate(self.param_groups):
            for p in g["params"]:
                owner[id(p)] = gi
        missing = [i for i, p in enumerate(self._live) if id(p) not in owner]
        if missing:
            raise ValueError(f"FusedAdamW: {len(missing)} trainable parameter(s) of the model are in no parameter group")
        self._group_of = [owner[id(p)] for p in self._live]
        self._t = 0
        self._exp_avg: Optional[torch.Tensor] = None
        self._exp_avg_sq: Optional[torch.Tensor] = None
        self.last_grad_norm: Optional[torch.Tensor] = None

    def _moments(self, dev):
        if self._exp_avg is None or self._exp_avg.device != dev:
            n = self.model._flat_elems
            self._exp_avg = torch.zeros(n, dtype=torch.float32, device=dev)
            self._exp_avg_sq = torch.zeros(n, dtype=torch.float32, device=dev)
        return self._exp_avg, self._exp_avg_sq

    @torch.no_grad()
    def step(self, closure=None, grad_scale: float = 1.0):
        """One update from the gradients of the last ``train_step``.  Returns the pre-clip global gradient norm
        (device scalar, no sync)."""
        if closure is not None:
            raise NotImplementedError("FusedAdamW: closures are not supported")
        m = self.model
        flat = m._step_flat
        if flat is None:
            raise RuntimeError("FusedAdamW.step() needs the gradients of MultimodalDEER.train_step()")
        dev = flat.device
        wbuf = m._weights(dev)
        exp_avg, exp_avg_sq = self._moments(dev)
        self._t += 1
        g0 = self.param_groups[0]
        lib = _lib.load()
        a = _lib.AdamWArgs()
        a.compute_f32, a.pack_transposed, a.step = m.compute_f32, 1, self._t
        a.beta1, a.beta2 = float(g0["betas"][0]), float(g0["betas"][1])
        a.eps, a.weight_decay = float(g0["eps"]), float(g0["weight_decay"])
        a.max_grad_norm, a.grad_scale = self.max_grad_norm, float(grad_scale)
        lrs = (C.c_float * len(self._live))(*[float(self.param_groups[gi]["lr"]) for gi in self._group_of])
        a.lr = lrs
        a.params = (C.c_void_p * len(self._live))(*[p.data_ptr() for p in self._live])
        a.grads, a.exp_avg, a.exp_avg_sq = flat.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr()
        norm = torch.empty((), dtype=torch.float32, device=dev)
        a.grad_norm = norm.data_ptr()
        a.weights, a.weights_bytes = wbuf.data_ptr(), wbuf.numel()
        a.stream = _lib.current_stream()
        _lib.check(lib.mmdeer_adamw_step(C.byref(a)))
        # the parameters changed behind torch's version counters, and the model's packed copies are already current
        m._st.param_gen += 1
        m._st.packed_key = m._param_key(wbuf)
        self.last_grad_norm = norm
        return norm

    # ---- checkpointing (flat moments instead of torch's per-parameter state)
    def state_dict(self) -> Dict:
        groups = [{k: v for k, v in g.items() if k != "params"} for g in self.param_groups]
        return {"step": self._t, "param_groups": groups,
                "exp_avg": None if self._exp_avg is None else self._exp_avg.detach().cpu(),
                "exp_avg_sq": None if self._exp_avg_sq is None else self._exp_avg_sq.detach().cpu()}

    def load_state_dict(self, state: Dict) -> None:
        self._t = int(state["step"])
        for g, sg in zip(self.param_groups, state["param_groups"]):
            g.update(sg)
        if state.get("exp_avg") is not None:
            dev = self._live[0].device
            self._exp_avg = state["exp_avg"].to(dev).float().contiguous()
            self._exp_avg_sq = state["exp_avg_sq"].to(dev).float().contiguous()


class FlatAdamW(torch.optim.Optimizer):
    """clip_grad_norm_ + AdamW (training.py:121-150, 219-224) for a model whose parameters and gradients live in flat buffers
    (``stackb.CompleteDEERModel._flat``): ONE call of ``mmdeer_adamw_flat`` (two launches, plus one for the transposed copies)
    updates the fp32 parameters, the moments and the compute-dtype copies the GEMMs read.  A ``torch.optim.Optimizer``, so the
    reference's LR schedulers drive it unchanged; default parameter groups follow the reference trainer: parameters with
    'encoder' in their name at ``encoder_lr_scale`` x lr (training.py:125-140).  Parameters the backward never reaches (the
    calibration layer: ``grad is None`` under autograd, which torch's AdamW skips) are left untouched.

    The clipping norm is taken over the optimiser's own parameters (the segments of the flat gradient buffer it updates), as
    ``clip_grad_norm_`` over them would: with ``params=`` naming a subset (frozen encoders) the excluded parameters' gradients do not
    enter it.  betas / eps / weight_decay must be the same in every group; ``step()`` re-checks it (a scheduler or a caller editing
    ``param_groups`` later is not ignored silently)."""

    def __init__(self, model, params: Optional[Iterable] = None, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 1e-2, max_grad_norm: float = 0.0, encoder_lr_scale: float = 0.5, skip=("calibration_layer.",)):
        if lr <= 0 or eps <= 0 or not (0 <= betas[0] < 1 and 0 <= betas[1] < 1) or weight_decay < 0:
            raise ValueError("FlatAdamW: bad hyper-parameters")
        self.skip = tuple(skip)
        if params is None:
            named = [(n, p) for n, p in model.named_parameters() if not any(n.startswith(s) for s in self.skip)]
            groups = [g for g in ({"params": [p for n, p in named if "encoder" in n], "lr": lr * encoder_lr_scale},
                                  {"params": [p for n, p in named if "encoder" not in n], "lr": lr}) if g["params"]]
        else:
            groups = list(params)
        super().__init__(groups, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay))
        hyper = {(g["betas"], g["eps"], g["weight_decay"]) for g in self.param_groups}
        if len(hyper) != 1:
            raise NotImplementedError("FlatAdamW: betas / eps / weight_decay must be the same in every group (lr may differ)")
        self.model, self.max_grad_norm = model, float(max_grad_norm)
        self._t = 0
        self._m = self._v = self._scratch = None
        self.last_grad_norm: Optional[torch.Tensor] = None

    def _segments(self, st):
        """Maximal runs of consecutive parameters (flat order) with one learning rate; the alignment gaps inside a run hold
        zero parameters and zero gradients, which the update leaves at zero.  Parameters in no group are not touched."""
        lr_of = {id(p): float(g["lr"]) for g in self.param_groups for p in g["params"]}
        segs = []
        for name, p in self.model.named_parameters():
            if id(p) not in lr_of:
                continue
            lr = lr_of[id(p)]
            lo = st["offs"][name]
            hi = lo + (p.numel() + 63) // 64 * 64
            if segs and segs[-1][2] == lr and segs[-1][1] == lo:
                segs[-1][1] = hi
            else:
                segs.append([lo, hi, lr])
        return segs

    @torch.no_grad()
    def step(self, closure=None, grad_scale: float = 1.0):
        if closure is not None:
            raise NotImplementedError("FlatAdamW: closures are not supported")
        m = self.model
        dev = next(m.parameters()).device
        st = m._flat(dev)
        if self._m is None or self._m.device != dev or self._m.numel() != st["n"]:
            self._m = torch.zeros(st["n"], dtype=torch.float32, device=dev)
            self._v = torch.zeros_like(self._m)
            self._scratch = torch.empty(256, dtype=torch.float32, device=dev)
        segs = self._segments(st)
        if len({(tuple(g["betas"]), g["eps"], g["weight_decay"]) for g in self.param_groups}) != 1:
            raise NotImplementedError("FlatAdamW: betas / eps / weight_decay must be the same in every group (lr may differ)")
        self._t += 1
        g0 = self.param_groups[0]
        a = _lib.AdamWFlatArgs()
        a.params, a.grads, a.exp_avg, a.exp_avg_sq = st["p"].data_ptr(), st["g"].data_ptr(), self._m.data_ptr(), self._v.data_ptr()
        f32 = st["packed"] is st["p"]
        a.packed, a.packed_f32 = (None if f32 else st["packed"].data_ptr()), int(f32)
        a.flat_elems, a.nseg = st["n"], len(segs)
        self._keep = ((C.c_longlong * len(segs))(*[s[0] for s in segs]), (C.c_longlong * len(segs))(*[s[1] - s[0] for s in segs]),
                      (C.c_float * len(segs))(*[s[2] for s in segs]))
        a.seg_begin, a.seg_elems, a.seg_lr = self._keep
        norm = torch.empty((), dtype=torch.float32, device=dev)
        a.scratch, a.grad_norm, a.step = self._scratch.data_ptr(), norm.data_ptr(), self._t
        a.beta1, a.beta2, a.eps, a.weight_decay = float(g0["betas"][0]), float(g0["betas"][1]), float(g0["eps"]), float(g0["weight_decay"])
        a.max_grad_norm, a.grad_scale = self.max_grad_norm, float(grad_scale)
        a.stream = _lib.current_stream()
        _lib.check(_lib.load().mmdeer_adamw_flat(C.byref(a)))
        # the kernel wrote the parameters (and their compute-dtype copy) behind torch's version counters: the copy IS current
        m._flat_pack_t(st)                     # ... and the transposed copies of the matrices the dX GEMMs read (one launch)
        st["versions"] = tuple(p._version for p in m.parameters())
        m._packed = None                       # the inference operand image is rebuilt from the new parameters on demand
        self.last_grad_norm = norm
        return norm

    def zero_grad(self, set_to_none: bool = False):   # the fused backward overwrites every gradient it produces
        return None

    def state_dict(self) -> Dict:
        groups = [{k: v for k, v in g.items() if k != "params"} for g in self.param_groups]
        return {"step": self._t, "param_groups": groups, "exp_avg": None if self._m is None else self._m.detach().cpu(),
                "exp_avg_sq": None if self._v is None else self._v.detach().cpu()}

    def load_state_dict(self, state: Dict) -> None:
        self._t = int(state["step"])
        for g, sg in zip(self.param_groups, state["param_groups"]):
            g.update(sg)
        if state.get("exp_avg") is not None:
            dev = next(self.model.parameters()).device
            self._m = state["exp_avg"].to(dev).float().contiguous()
            self._v = state["exp_avg_sq"].to(dev).float().contiguous()
            self._scratch = torch.empty(256, dtype=torch.float32, device=dev)


_CHUNK = _lib.OPTIM_CONSTANTS["ADAMW_MULTI_CHUNK"]
_MAX_CLASSES = _lib.OPTIM_CONSTANTS["ADAMW_MULTI_MAX_CLASSES"]
_SCRATCH = _lib.OPTIM_CONSTANTS["ADAMW_MULTI_SCRATCH"]


class ModuleAdamW(torch.optim.Optimizer):
    """``clip_grad_norm_(params, max_grad_norm)`` + ``torch.optim.AdamW`` for ANY list of fp32 CUDA parameters that train through
    autograd into ordinary ``.grad`` tensors (the encoders, the DEER head modules, ``ComposedDEER``, the alternative fusions,
    ``BertEncoder(finetune_layers=k)``): ONE call of ``mmdeer_adamw_multi`` (include/mmdeer_optim.h), two launches on the current
    stream and no host synchronisation.  A ``torch.optim.Optimizer``, so the reference's LR schedulers drive it unchanged.

    ``params``: parameters or torch-style groups; ``lr`` and ``weight_decay`` may differ per group (decay 0 on LayerNorm and biases),
    ``betas`` / ``eps`` may not (``NotImplementedError``; re-checked at every step).  ``max_grad_norm <= 0``: no clipping.  The norm is
    taken over this optimiser's parameters that have a gradient.

    ``step(grad_scale=1.0)`` returns the norm of ``grad_scale * g`` before clipping as a device scalar (also ``last_grad_norm``).  A
    parameter whose ``grad is None`` is skipped exactly as torch skips it: neither it nor its moments are touched, its step count does
    not advance, and it is not in the norm.  CPU or non-fp32 parameters, non-contiguous parameters or gradients and closures raise:
    there is no fallback.  The update runs behind torch's version counters; every updated parameter's ``_version`` is then advanced
    (``torch.autograd.graph.increment_version``: no launch), so that caches keyed on it -- the encoders' packed operands -- rebuild as
    they do after torch's optimiser.

    ``mirrors``: a mapping parameter -> tensor of the same element count, contiguous, bf16 or fp32, on the parameter's device; after
    the update element i of the parameter is also stored at element i of its mirror (bf16: rounded to nearest even, what
    ``.to(torch.bfloat16)`` stores).  ``for_module`` collects them from the submodules that offer ``operand_mirrors()`` (``BertEncoder``),
    whose packed operands are then current after the step without a rebuild.

    ``state_dict()`` / ``load_state_dict()`` speak ``torch.optim.AdamW``'s format (per parameter ``step``, ``exp_avg``, ``exp_avg_sq``, and
    ``param_groups`` with its keys): a checkpoint moves between the two optimisers in both directions.  The moments live in two flat
    buffers; ``state[p]['exp_avg']`` is a view of one.  ``table_uploads`` counts the uploads of the device-side tensor table: one at
    the first step, one more whenever a gradient comes back at another address or another set of parameters has gradients."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
                 max_grad_norm: float = 0.0, mirrors=None):
        if not (lr > 0 and eps > 0 and 0 <= betas[0] < 1 and 0 <= betas[1] < 1 and weight_decay >= 0):
            raise ValueError("ModuleAdamW: bad hyper-parameters")
        # torch.optim.AdamW's own group keys (amsgrad, maximize, foreach, ...) with its defaults: a state_dict loads into either
        defaults = dict(torch.optim.AdamW([torch.zeros(1)], lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay).defaults)
        super().__init__(list(params), defaults)
        self.max_grad_norm = float(max_grad_norm)
        self._check_groups()
        self._params = [p for g in self.param_groups for p in g["params"]]
        self._group_of = [gi for gi, g in enumerate(self.param_groups) for _ in g["params"]]
        index = {id(p): i for i, p in enumerate(self._params)}
        self._mirrors = [None] * len(self._params)
        for p, t in (mirrors.items() if mirrors is not None else ()):
            if id(p) not in index:
                raise ValueError("ModuleAdamW: a mirror is given for a tensor that is not among the parameters")
            self._check_mirror(p, t)
            self._mirrors[index[id(p)]] = t
        self._steps = [0] * len(self._params)
        self._m = self._v = self._scratch = self._table = None
        self._offs = None
        self._sig = self._records = self._classes = None
        self._owners = []                   # for_module: the submodules whose operand_mirrors() the mirrors came from
        self._owner_packed = []
        self.table_uploads = 0
        self.last_grad_norm: Optional[torch.Tensor] = None

    @staticmethod
    def _check_mirror(p, t):
        if not isinstance(t, torch.Tensor) or t.dtype not in (torch.bfloat16, torch.float32):
            raise ValueError("ModuleAdamW: a mirror must be a bf16 or fp32 tensor")
        if t.numel() != p.numel() or not t.is_contiguous() or t.device != p.device:
            raise ValueError("ModuleAdamW: a mirror must be contiguous, on its parameter's device and of its element count "
                             f"(parameter {tuple(p.shape)} on {p.device}, mirror {tuple(t.shape)} on {t.device})")

    def _check_groups(self):
        g0 = self.param_groups[0]
        for g in self.param_groups:
            if tuple(g["betas"]) != tuple(g0["betas"]) or g["eps"] != g0["eps"]:
                raise NotImplementedError("ModuleAdamW: betas / eps must be the same in every group (lr and weight_decay may differ)")
            if g.get("amsgrad") or g.get("maximize"):
                raise NotImplementedError("ModuleAdamW: amsgrad / maximize are not built")

    @classmethod
    def for_module(cls, module, params=None, **kw):
        """The optimiser of ``module``'s trainable parameters (or of ``params``: parameters or groups) with the mirrors of every
        submodule that offers ``operand_mirrors()``; after each step those submodules' ``operands_current()`` is called, so their
        next forward reads the operands the step wrote instead of rebuilding them.  Submodules without mirrors rebuild their caches
        on the version bump, as after torch's optimiser.  As with any in-place optimiser, a backward through a tape recorded
        before a step is not supported: such a tape holds the operands this step overwrites."""
        groups = list(params) if params is not None else [p for p in module.parameters() if p.requires_grad]
        mine = {id(p) for g in groups for p in (g["params"] if isinstance(g, dict) else [g])}
        owners = [m for m in module.modules() if hasattr(m, "operand_mirrors") and hasattr(m, "operands_current")]
        mirrors = {}
        for m in owners:
            mirrors.update({p: t for p, t in m.operand_mirrors().items() if id(p) in mine})
        opt = cls(groups, mirrors=mirrors, **kw)
        opt._owners = owners
        opt._owner_packed = [m._operands() for m in owners]
        return opt

    def _refresh_owner_mirrors(self):
        """An owner rebuilt its operands since the mirrors were taken (a load_state_dict, a .to()): take the new ones."""
        index = {id(p): i for i, p in enumerate(self._params)}
        for k, m in enumerate(self._owners):
            packed = m._operands()
            if packed is self._owner_packed[k]:
                continue
            for p, t in m.operand_mirrors().items():
                if id(p) in index:
                    self._check_mirror(p, t)
                    self._mirrors[index[id(p)]] = t
            self._owner_packed[k] = m._operands()
            self._sig = None

    def _buffers(self, dev):
        if self._m is None or self._m.device != dev:
            offs, n = [], 0
            for p in self._params:            # moments at the parameter's offset modulo 4 elements: 16-byte accesses line up
                n = (n + 3) // 4 * 4 + (p.data_ptr() // 4) % 4
                offs.append(n)
                n += p.numel()
            self._offs = offs
            self._m = torch.zeros(max(n, 4), dtype=torch.float32, device=dev)
            self._v = torch.zeros_like(self._m)
            self._scratch = torch.empty(_SCRATCH, dtype=torch.float32, device=dev)
            self._sig = None
            for i, p in enumerate(self._params):
                st = self.state.get(p)
                if st and "exp_avg" in st:
                    self._adopt(i, st["exp_avg"], st["exp_avg_sq"])

    def _views(self, i):
        p, o = self._params[i], self._offs[i]
        return self._m[o:o + p.numel()].view(p.shape), self._v[o:o + p.numel()].view(p.shape)

    def _adopt(self, i, m, v):
        """the moments of parameter i into the flat buffers; its state entries become views of them"""
        p = self._params[i]
        vm, vv = self._views(i)
        if m.data_ptr() != vm.data_ptr():
            vm.copy_(m.to(vm.device, torch.float32).reshape(p.shape))
            vv.copy_(v.to(vv.device, torch.float32).reshape(p.shape))
        st = self.state[p]
        st["exp_avg"], st["exp_avg_sq"] = vm, vv

    @torch.no_grad()
    def step(self, closure=None, grad_scale: float = 1.0):
        if closure is not None:
            raise NotImplementedError("ModuleAdamW: closures are not supported")
        self._check_groups()
        # one pass over the parameters: who has a gradient, where it is, and the class (group, step count) of each, in order of first
        # appearance.  The full checks run only when something moved (below): an unchanged signature means the same tensors as before.
        live, gptr, pptr, cls_of, keys, ok = [], [], [], [], {}, True
        for i, p in enumerate(self._params):
            g = p.grad
            if g is None:
                continue
            live.append(i)
            gptr.append(g.data_ptr())
            pptr.append(p.data_ptr())
            ok = ok and g.is_contiguous() and g.dtype is torch.float32
            cls_of.append(keys.setdefault((self._group_of[i], self._steps[i]), len(keys)))
        if not live:
            dev = self._params[0].device if self._params else "cpu"
            self.last_grad_norm = torch.zeros((), dtype=torch.float32, device=dev)
            return self.last_grad_norm
        dev = self._params[live[0]].device
        sig = (tuple(live), tuple(cls_of), tuple(pptr), tuple(gptr))
        if not ok or sig != self._sig:
            for i in live:
                p = self._params[i]
                g = p.grad
                if not p.is_cuda or p.dtype != torch.float32 or g.dtype != torch.float32 or p.device != dev or g.device != dev:
                    raise RuntimeError("ModuleAdamW: parameters and gradients must be fp32 tensors on one CUDA device (there is no CPU path); "
                                       f"got {p.dtype} on {p.device}, gradient {g.dtype} on {g.device}")
                if not p.is_contiguous() or not g.is_contiguous() or g.numel() != p.numel():
                    raise RuntimeError(f"ModuleAdamW: parameters and gradients must be contiguous (parameter {tuple(p.shape)}, strides "
                                       f"{p.stride()}; gradient strides {g.stride()})")
        self._buffers(dev)
        for k, m in enumerate(self._owners):            # an owner that rebuilt its operands since the mirrors were taken
            if m._packed is not self._owner_packed[k]:
                self._refresh_owner_mirrors()
                break
        if len(keys) > _MAX_CLASSES:
            raise NotImplementedError(f"ModuleAdamW: {len(keys)} distinct (group, step count) pairs in one step; the kernel arguments "
                                      f"hold {_MAX_CLASSES}")
        lib = _lib.load()
        upload = sig != self._sig
        if upload:
            rec = (_lib.AdamWMultiTensor * len(live))()
            for r, i, c in zip(rec, live, cls_of):
                p, t = self._params[i], self._mirrors[i]
                r.param, r.grad, r.count, r.moment_off, r.cls = p.data_ptr(), p.grad.data_ptr(), p.numel(), self._offs[i], c
                if t is not None:
                    if t.device != dev:
                        raise RuntimeError("ModuleAdamW: a mirror is not on its parameter's device")
                    r.mirror, r.mirror_f32 = t.data_ptr(), int(t.dtype == torch.float32)
            need = lib.mmdeer_adamw_multi_table_bytes(rec, len(live))
            if need < 0:
                _lib.check(-1)
            if self._table is None or self._table.device != dev or self._table.numel() < need:
                self._table = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
            self._records = rec
        a = _lib.AdamWMultiArgs()
        a.tensors, a.ntensors, a.nclasses = self._records, len(live), len(keys)
        for (gi, t), c in keys.items():
            g = self.param_groups[gi]
            a.classes[c].lr, a.classes[c].weight_decay, a.classes[c].step = float(g["lr"]), float(g["weight_decay"]), t + 1
        g0 = self.param_groups[0]
        a.beta1, a.beta2, a.eps = float(g0["betas"][0]), float(g0["betas"][1]), float(g0["eps"])
        a.exp_avg, a.exp_avg_sq, a.moment_elems = self._m.data_ptr(), self._v.data_ptr(), self._m.numel()
        a.table, a.table_bytes, a.upload = self._table.data_ptr(), self._table.numel(), int(upload)
        norm = torch.empty((), dtype=torch.float32, device=dev)
        a.scratch, a.grad_norm = self._scratch.data_ptr(), norm.data_ptr()
        a.max_grad_norm, a.grad_scale, a.stream = self.max_grad_norm, float(grad_scale), _lib.current_stream()
        _lib.check(lib.mmdeer_adamw_multi(C.byref(a)))
        if upload:
            self._sig = sig
            self.table_uploads += 1
        for i in live:
            self._steps[i] += 1
            p = self._params[i]
            if "exp_avg" not in self.state[p]:
                self.state[p]["step"] = torch.tensor(0.0, dtype=torch.float32)
                self.state[p]["exp_avg"], self.state[p]["exp_avg_sq"] = self._views(i)
        # the kernel wrote behind torch's version counters
        torch.autograd.graph.increment_version([self._params[i] for i in live])
        for m in self._owners:
            m.operands_current()            # ... and straight into these modules' packed operands: they ARE current
        self.last_grad_norm = norm
        return norm

    def state_dict(self) -> Dict:
        for i, p in enumerate(self._params):
            st = self.state.get(p)
            if st and "step" in st:
                st["step"].fill_(float(self._steps[i]))
        return super().state_dict()

    def load_state_dict(self, state: Dict) -> None:
        super().load_state_dict(state)
        self._check_groups()
        self._sig = None
        for i, p in enumerate(self._params):
            st = self.state.get(p)
            if not st:
                self._steps[i] = 0
                continue
            step = st["step"]
            self._steps[i] = int(round(float(step)))
            st["step"] = torch.tensor(float(self._steps[i]), dtype=torch.float32)
            if self._m is not None:
                self._adopt(i, st["exp_avg"], st["exp_avg_sq"])
