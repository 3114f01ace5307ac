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


def _capturing() -> bool:
    """is the current stream being captured?  (without a device torch raises: nothing captures there)"""
    try:
        return bool(torch.cuda.is_current_stream_capturing())
    except Exception:       # noqa: BLE001
        return False


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
    the first step, one more whenever a gradient comes back at another address or another set of parameters has gradients.

    ``capturable=True`` makes ``step()`` one call of ``mmdeer_adamw_multi_dev``, which a stream capture can record (``torch.cuda.graph``,
    ``mmdeer.train_graph.capture_train_step``): what a replay must see change lives on the device.  The classes are the GROUPS; each
    has a 16-byte record (lr, weight_decay, steps done) in ``class_buffer``; the first launch adds 1 to the step counts and the second
    forms the bias corrections from them, so every replay is the next step.  ``state[p]['step']`` is a device scalar, a view of its
    group's count.  lr and weight_decay are read from the records: ``step()`` (and a replay, through ``refresh_hyper()``) rewrites them
    with one small copy when ``param_groups`` moved -- outside a capture; inside one a change raises.  The table upload is made of
    launches (no copy, no wait), so the first captured step, whose gradients sit at new addresses, uploads inside the graph.  Because
    the step count is device data there is one count per group: the parameters of a group that take part must all have done the same
    number of steps, and once the first step has run a step whose set of parameters with a gradient differs from the first step's
    raises ``RuntimeError`` naming the parameter.  ``state_dict()`` reads the counts back (one small copy to the host) and stays
    ``torch.optim.AdamW``'s format.  A NON-capturable ``step()`` inside a capture raises before any library call: its upload waits
    for the stream and its step is a host value."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
                 max_grad_norm: float = 0.0, mirrors=None, capturable: bool = False):
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
        self._module = None                 # for_module: the module itself (train_graph looks for step counters under it)
        self._names = {}                    # for_module: id(parameter) -> its name, for messages
        self.capturable = bool(capturable)
        self._cls = None                    # capturable: (classes, 4) int32 on the device: lr bits, weight_decay bits, steps done, 0
        self._cls_groups = None             # ... the group of each class
        self._cls_hyper = None              # ... the host shadow [(lr, weight_decay)] of what the records hold
        self._live0 = None                  # ... the parameters that had a gradient at the first step
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
        opt._owners, opt._module = owners, module
        opt._names = {id(p): n for n, p in module.named_parameters()}
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
        if self.capturable:
            return self._step_capturable(float(grad_scale))
        if _capturing():
            raise RuntimeError("ModuleAdamW.step() inside a stream capture: its step count is a host value and its table upload waits for "
                               "the stream.  Build the optimiser with capturable=True")
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

    # ---- capturable=True ------------------------------------------------------------------------------------------------
    def _name(self, i):
        p = self._params[i]
        return self._names.get(id(p), f"#{i} of shape {tuple(p.shape)}")

    @property
    def class_buffer(self) -> Optional[torch.Tensor]:
        """capturable: the device records (classes, 4) int32 -- lr and weight_decay as float32 bits, the steps done, 0"""
        return self._cls

    def _hyper(self):
        out = []
        for gi in self._cls_groups:
            g = self.param_groups[gi]
            lr, wd = float(g["lr"]), float(g["weight_decay"])
            if not (lr > 0 and lr != float("inf") and 0 <= wd != float("inf")):       # false for a NaN
                raise ValueError(f"ModuleAdamW: group {gi}: lr must be finite and positive and weight_decay finite and >= 0 (got {lr}, {wd})")
            out.append((lr, wd))
        return out

    def _sync_steps(self):
        """the device step counts into the host's per-parameter shadow (one small copy; not inside a capture)"""
        if self._cls is not None and self._live0 is not None:
            done = self._cls[:, 2].cpu().tolist()
            cls_of_group = {gi: c for c, gi in enumerate(self._cls_groups)}
            for i in self._live0:
                self._steps[i] = int(done[cls_of_group[self._group_of[i]]])

    def refresh_hyper(self) -> None:
        """capturable: rewrite the device records' lr and weight_decay if ``param_groups`` moved since they were written (an LR
        scheduler stepped).  One small copy on the current stream; inside a capture a change raises instead."""
        if self._cls is None:
            return
        hyper = self._hyper()
        if hyper != self._cls_hyper:
            if _capturing():
                raise RuntimeError("ModuleAdamW(capturable=True): lr / weight_decay changed inside a stream capture; change param_groups "
                                   "between replays")
            self._cls.view(torch.float32)[:, :2].copy_(torch.tensor(hyper, dtype=torch.float32))
            self._cls_hyper = hyper

    def snapshot(self) -> Dict:
        """capturable: the moments, the device step counts and which parameters have state, as they are now (``restore`` puts them
        back in place: warm-up steps before a capture are then no training steps)"""
        self._sync_steps()
        clone = lambda t: None if t is None else t.clone()       # noqa: E731
        return {"m": clone(self._m), "v": clone(self._v), "cls": clone(self._cls), "steps": list(self._steps),
                "stateful": {id(p) for p in self._params if self.state.get(p)}}

    def restore(self, snap: Dict) -> None:
        """Write a ``snapshot()`` back IN PLACE (addresses stay: a captured graph keeps reading these buffers).  Buffers and records
        that did not exist at the snapshot are zeroed (no moments, no steps done), and state entries made since are dropped."""
        for mine, was in ((self._m, snap["m"]), (self._v, snap["v"])):
            if mine is not None:
                mine.copy_(was) if was is not None and was.shape == mine.shape else mine.zero_()
        self._steps = list(snap["steps"])
        if self._cls is not None:
            if snap["cls"] is not None and snap["cls"].shape == self._cls.shape:
                self._cls[:, 2].copy_(snap["cls"][:, 2])
            else:
                cls_of_group = {gi: c for c, gi in enumerate(self._cls_groups)}
                done = [0] * len(self._cls_groups)
                for i in self._live0 or ():
                    done[cls_of_group[self._group_of[i]]] = self._steps[i]
                self._cls[:, 2].copy_(torch.tensor(done, dtype=torch.int32))
        for p in self._params:
            if id(p) not in snap["stateful"]:
                self.state.pop(p, None)

    def _step_capturable(self, grad_scale: float):
        self._check_groups()
        live = [i for i, p in enumerate(self._params) if p.grad is not None]
        if self._live0 is not None and tuple(live) != self._live0:
            odd = sorted(set(live) ^ set(self._live0))[0]
            raise RuntimeError(f"ModuleAdamW(capturable=True): parameter {self._name(odd)} "
                               f"{'has' if odd in live else 'has no'} gradient, unlike at the first step: the step counts are device data, "
                               "one per group, so the set of parameters that take part is fixed by the first step")
        if not live:
            dev = self._params[0].device if self._params else "cpu"
            self.last_grad_norm = torch.zeros((), dtype=torch.float32, device=dev)
            return self.last_grad_norm
        dev = self._params[live[0]].device
        pptr, gptr = tuple(self._params[i].data_ptr() for i in live), tuple(self._params[i].grad.data_ptr() for i in live)
        sig = (tuple(live), pptr, gptr)
        upload = sig != self._sig
        if upload:
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
        for k, m in enumerate(self._owners):
            if m._packed is not self._owner_packed[k]:
                self._refresh_owner_mirrors()
                upload = True
                break
        if self._live0 is None:
            # the first step (or the first after load_state_dict): classes = the groups that take part, in order of first appearance
            groups, done = [], []
            for i in live:
                gi = self._group_of[i]
                if gi not in groups:
                    groups.append(gi)
                    done.append(self._steps[i])
                elif self._steps[i] != done[groups.index(gi)]:
                    raise RuntimeError(f"ModuleAdamW(capturable=True): parameter {self._name(i)} has done {self._steps[i]} steps and another "
                                       f"of its group {done[groups.index(gi)]}: the step count is one device value per group")
            if len(groups) > _MAX_CLASSES:
                raise NotImplementedError(f"ModuleAdamW: {len(groups)} groups in one step; the kernels take {_MAX_CLASSES} classes")
            if _capturing():
                raise RuntimeError("ModuleAdamW(capturable=True): run one step before the capture (it builds the device records)")
            self._cls_groups = groups
            self._cls_hyper = self._hyper()
            rec = torch.zeros(len(groups), 4, dtype=torch.int32)
            rec.view(torch.float32)[:, :2] = torch.tensor(self._cls_hyper, dtype=torch.float32)
            rec[:, 2] = torch.tensor(done, dtype=torch.int32)
            self._cls = rec.to(dev)
        else:
            self.refresh_hyper()
        lib = _lib.load()
        if upload:
            cls_of_group = {gi: c for c, gi in enumerate(self._cls_groups)}
            rec = (_lib.AdamWMultiTensor * len(live))()
            for r, i in zip(rec, live):
                p, t = self._params[i], self._mirrors[i]
                r.param, r.grad, r.count, r.moment_off, r.cls = p.data_ptr(), p.grad.data_ptr(), p.numel(), self._offs[i], cls_of_group[self._group_of[i]]
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
        a = _lib.AdamWMultiDevArgs()
        a.tensors = C.cast(self._records, C.c_void_p)     # (an opaque type in mmdeer_graph.h; self._records keeps the array alive)
        a.ntensors, a.nclasses, a.classes = len(live), len(self._cls_groups), self._cls.data_ptr()
        g0 = self.param_groups[0]
        a.beta1, a.beta2, a.eps = float(g0["betas"][0]), float(g0["betas"][1]), float(g0["eps"])
        a.exp_avg, a.exp_avg_sq, a.moment_elems = self._m.data_ptr(), self._v.data_ptr(), self._m.numel()
        a.table, a.table_bytes, a.upload = self._table.data_ptr(), self._table.numel(), int(upload)
        norm = torch.empty((), dtype=torch.float32, device=dev)
        a.scratch, a.grad_norm = self._scratch.data_ptr(), norm.data_ptr()
        a.max_grad_norm, a.grad_scale, a.stream = self.max_grad_norm, grad_scale, _lib.current_stream()
        _lib.check(lib.mmdeer_adamw_multi_dev(C.byref(a)))
        if upload:
            self._sig = sig
            self.table_uploads += 1
        if self._live0 is None:
            self._live0 = tuple(live)
        cls_of_group = {gi: c for c, gi in enumerate(self._cls_groups)}
        for i in live:
            p = self._params[i]
            st = self.state[p]
            if "exp_avg" not in st:
                st["exp_avg"], st["exp_avg_sq"] = self._views(i)
            st["step"] = self._cls[cls_of_group[self._group_of[i]], 2]
        torch.autograd.graph.increment_version([self._params[i] for i in live])
        for m in self._owners:
            m.operands_current()
        self.last_grad_norm = norm
        return norm

    def state_dict(self) -> Dict:
        if self.capturable:
            self._sync_steps()
            sd = super().state_dict()
            index = {}
            for g in sd["param_groups"]:
                for k in g["params"]:
                    index[k] = len(index)
            # torch.optim.AdamW's format: a float32 scalar per parameter (the live entries are views of the device records)
            sd["state"] = {k: {**st, "step": torch.tensor(float(self._steps[index[k]]), dtype=torch.float32)} if "step" in st else st
                           for k, st in sd["state"].items()}
            return sd
        for i, p in enumerate(self._params):
            st = self.state.get(p)
            if st and "step" in st:
                st["step"].fill_(float(self._steps[i]))
        return super().state_dict()

    def load_state_dict(self, state: Dict) -> None:
        super().load_state_dict(state)
        self._check_groups()
        self._sig = None
        self._live0 = self._cls = self._cls_groups = self._cls_hyper = None      # capturable: the next step rebuilds the device records
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
