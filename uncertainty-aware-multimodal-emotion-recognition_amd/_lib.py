"""ctypes binding of libmmdeer_hip.so (include/mmdeer.h).

There is NO fallback: if the library cannot be loaded (or built from the in-tree
sources with hipcc) every entry point raises.  The product path never touches
``oracle/``.
"""
from __future__ import annotations

import ctypes as C
import os
import threading
from typing import Optional

# torch must be imported BEFORE libmmdeer_hip.so is dlopen'ed: the PyTorch-ROCm wheel ships its own
# libamdhip64.so, and the library has to bind to that already-loaded runtime (one HIP runtime per process,
# shared streams and device pointers) rather than pull in a second copy from /opt/rocm/lib.
# kernel arguments in device memory: a kernarg fetch from host memory costs a PCIe round trip per dependent
# scalar load (measured 8.7k vs 2.4k cycles of kernel setup, 0.69 vs 0.53 ms per train step).  Read at HIP init.
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")

import torch  # noqa: F401,E402

from . import _header, build as _build

_LIB: Optional[C.CDLL] = None
_LOCK = threading.Lock()

# C struct name (include/mmdeer.h) -> the class name the package and the tests use
_NAMES = {"mmdeer_" + c: n for c, n in (
    ("loss_cfg", "LossCfg"), ("forward_args", "ForwardArgs"), ("backward_args", "BackwardArgs"), ("gemm_args", "GemmArgs"),
    ("adamw_args", "AdamWArgs"), ("adamw_flat_args", "AdamWFlatArgs"), ("lstm_seq_args", "LstmSeqArgs"),
    ("temporal_pool_args", "TemporalPoolArgs"), ("token_embed_args", "TokenEmbedArgs"), ("token_pool_args", "TokenPoolArgs"),
    ("token_stats_args", "TokenStatsArgs"), ("evidence_tail_args", "EvidenceTailArgs"), ("stackb_attn_args", "StackBAttnArgs"),
    ("stackb_attn_train_args", "StackBAttnTrainArgs"), ("softmax_mix_args", "SoftmaxMixArgs"), ("stackb_weights", "StackBWeights"),
    ("stackb_forward_args", "StackBForwardArgs"), ("chain_seg", "ChainSeg"), ("chain_args", "ChainArgs"), ("repack_job", "RepackJob"))}
# pointer fields the host fills with ctypes arrays: typed, so that the assignment keeps the array alive (a c_void_p field takes none)
_TYPED_POINTERS = {
    ("mmdeer_adamw_args", "lr"): C.c_float, ("mmdeer_adamw_args", "params"): C.c_void_p,
    ("mmdeer_adamw_flat_args", "seg_begin"): C.c_longlong, ("mmdeer_adamw_flat_args", "seg_elems"): C.c_longlong,
    ("mmdeer_adamw_flat_args", "seg_lr"): C.c_float,
    ("mmdeer_forward_args", "params"): C.c_void_p,
}

# CONSTANTS: every MMDEER_<NAME> integer of the header; SYMBOLS: every function it declares as (name, restype, argtypes)
CONSTANTS, _CLASSES, SYMBOLS = _header.parse(_header.read(), _NAMES, _TYPED_POINTERS)
globals().update({cls.__name__: cls for cls in _CLASSES.values()})          # GemmArgs, ChainArgs, ...
# the ctypes mirror of every argument struct, by the name mmdeer_sizeof() knows it under (it does not know loss_cfg)
STRUCTS = {c.removeprefix("mmdeer_"): cls for c, cls in _CLASSES.items() if c != "mmdeer_loss_cfg"}
ABI_VERSION = CONSTANTS["ABI_VERSION"]
CHAIN_MAX_SEGS = CONSTANTS["CHAIN_MAX_SEGS"]
TEMPORAL_POOL_SCRATCH = CONSTANTS["TEMPORAL_POOL_SCRATCH"]
TOKEN_POOL_SCRATCH = CONSTANTS["TOKEN_POOL_SCRATCH"]
LOSS_OUT = CONSTANTS["LOSS_OUT"]
UNC_TABLE = CONSTANTS["UNC_TABLE"]
COMM_ID_BYTES = CONSTANTS["COMM_ID_BYTES"]
# include/mmdeer_video.h, the companion header of the temporal video encoder's operators: the same derivation, kept beside the
# tables of mmdeer.h
_VIDEO_NAMES = {"mmdeer_conv3_time_args": "Conv3TimeArgs", "mmdeer_bn_time_args": "BnTimeArgs"}
VIDEO_CONSTANTS, _VIDEO_CLASSES, VIDEO_SYMBOLS = _header.parse(_header.read(_header.VIDEO_HEADER_PATH), _VIDEO_NAMES, {})
globals().update({cls.__name__: cls for cls in _VIDEO_CLASSES.values()})    # Conv3TimeArgs, BnTimeArgs
VIDEO_STRUCTS = {c.removeprefix("mmdeer_"): cls for c, cls in _VIDEO_CLASSES.items()}
BN_TIME_SCRATCH = VIDEO_CONSTANTS["BN_TIME_SCRATCH"]
# include/mmdeer_frames.h, the companion header of the Conv2d backbone on frames: the same derivation again
_FRAME_NAMES = {"mmdeer_conv2d_args": "Conv2dArgs", "mmdeer_bn2d_args": "Bn2dArgs"}
FRAME_CONSTANTS, _FRAME_CLASSES, FRAME_SYMBOLS = _header.parse(_header.read(_header.FRAMES_HEADER_PATH), _FRAME_NAMES, {})
globals().update({cls.__name__: cls for cls in _FRAME_CLASSES.values()})    # Conv2dArgs, Bn2dArgs
FRAME_STRUCTS = {c.removeprefix("mmdeer_"): cls for c, cls in _FRAME_CLASSES.items()}
BN2D_SCRATCH = FRAME_CONSTANTS["BN2D_SCRATCH"]
# include/mmdeer_routes.h, the companion header of the layer chains' route queries (no struct of its own: mmdeer_chain_args is
# mmdeer.h's, passed by reference)
_, _, ROUTE_SYMBOLS = _header.parse(_header.read(_header.ROUTES_HEADER_PATH), {}, {})
# include/mmdeer_frames_bwd.h, the companion header of the Conv2d backbone's backward: tables of its own again
_FRAME_BWD_NAMES = {"mmdeer_bn2d_bwd_args": "Bn2dBwdArgs", "mmdeer_conv2d_wgrad_args": "Conv2dWgradArgs", "mmdeer_conv2d_dgrad_args": "Conv2dDgradArgs"}
FRAME_BWD_CONSTANTS, _FRAME_BWD_CLASSES, FRAME_BWD_SYMBOLS = _header.parse(_header.read(_header.FRAMES_BWD_HEADER_PATH), _FRAME_BWD_NAMES, {})
globals().update({cls.__name__: cls for cls in _FRAME_BWD_CLASSES.values()})    # Bn2dBwdArgs, Conv2dWgradArgs, Conv2dDgradArgs
FRAME_BWD_STRUCTS = {c.removeprefix("mmdeer_"): cls for c, cls in _FRAME_BWD_CLASSES.items()}
BN2D_BWD_SCRATCH = FRAME_BWD_CONSTANTS["BN2D_BWD_SCRATCH"]
# include/mmdeer_bert.h, the companion header of the BERT trunk's forward operators: tables of its own again
_BERT_NAMES = {"mmdeer_bert_embed_args": "BertEmbedArgs", "mmdeer_bert_attn_args": "BertAttnArgs", "mmdeer_bert_add_ln_args": "BertAddLnArgs",
               "mmdeer_bert_gelu_args": "BertGeluArgs"}
BERT_CONSTANTS, _BERT_CLASSES, BERT_SYMBOLS = _header.parse(_header.read(_header.BERT_HEADER_PATH), _BERT_NAMES, {})
globals().update({cls.__name__: cls for cls in _BERT_CLASSES.values()})    # BertEmbedArgs, BertAttnArgs, BertAddLnArgs, BertGeluArgs
BERT_STRUCTS = {c.removeprefix("mmdeer_"): cls for c, cls in _BERT_CLASSES.items()}
# include/mmdeer_bert_bwd.h, the companion header of the BERT trunk's backward operators: tables of its own again
_BERT_BWD_NAMES = {"mmdeer_bert_attn_bwd_args": "BertAttnBwdArgs", "mmdeer_bert_add_ln_bwd_args": "BertAddLnBwdArgs", "mmdeer_bert_gelu_bwd_args": "BertGeluBwdArgs"}
BERT_BWD_CONSTANTS, _BERT_BWD_CLASSES, BERT_BWD_SYMBOLS = _header.parse(_header.read(_header.BERT_BWD_HEADER_PATH), _BERT_BWD_NAMES, {})
globals().update({cls.__name__: cls for cls in _BERT_BWD_CLASSES.values()})    # BertAttnBwdArgs, BertAddLnBwdArgs, BertGeluBwdArgs
BERT_BWD_STRUCTS = {c.removeprefix("mmdeer_"): cls for c, cls in _BERT_BWD_CLASSES.items()}
# include/mmdeer_bert_drop.h, the companion header of the BERT trunk's operators with their dropout inside: tables of its own again
_BERT_DROP_NAMES = {"mmdeer_bert_embed_drop_args": "BertEmbedDropArgs", "mmdeer_bert_attn_drop_args": "BertAttnDropArgs",
                    "mmdeer_bert_drop_add_ln_args": "BertDropAddLnArgs", "mmdeer_bert_attn_drop_bwd_args": "BertAttnDropBwdArgs",
                    "mmdeer_bert_drop_add_ln_bwd_args": "BertDropAddLnBwdArgs"}
BERT_DROP_CONSTANTS, _BERT_DROP_CLASSES, BERT_DROP_SYMBOLS = _header.parse(_header.read(_header.BERT_DROP_HEADER_PATH), _BERT_DROP_NAMES, {})
globals().update({cls.__name__: cls for cls in _BERT_DROP_CLASSES.values()})    # BertEmbedDropArgs, BertAttnDropArgs, ...
BERT_DROP_STRUCTS = {c.removeprefix("mmdeer_"): cls for c, cls in _BERT_DROP_CLASSES.items()}
# include/mmdeer_optim.h, the companion header of the optimiser step over any list of tensors: tables of its own again
_OPTIM_NAMES = {"mmdeer_adamw_multi_tensor": "AdamWMultiTensor", "mmdeer_adamw_multi_class": "AdamWMultiClass", "mmdeer_adamw_multi_args": "AdamWMultiArgs"}
OPTIM_CONSTANTS, _OPTIM_CLASSES, OPTIM_SYMBOLS = _header.parse(_header.read(_header.OPTIM_HEADER_PATH), _OPTIM_NAMES, {})
globals().update({cls.__name__: cls for cls in _OPTIM_CLASSES.values()})    # AdamWMultiTensor, AdamWMultiClass, AdamWMultiArgs
OPTIM_STRUCTS = {c.removeprefix("mmdeer_"): cls for c, cls in _OPTIM_CLASSES.items()}
# include/mmdeer_graph.h, the companion header of the device step counters (the _dev twins of the dropout entries, the capturable
# optimiser step): tables of its own again; the older headers' structs it takes by reference are opaque there (c_void_p: pass byref)
_GRAPH_NAMES = {"mmdeer_adamw_multi_class_dev": "AdamWMultiClassDev", "mmdeer_adamw_multi_dev_args": "AdamWMultiDevArgs"}
GRAPH_CONSTANTS, _GRAPH_CLASSES, GRAPH_SYMBOLS = _header.parse(_header.read(_header.GRAPH_HEADER_PATH), _GRAPH_NAMES, {})
globals().update({cls.__name__: cls for cls in _GRAPH_CLASSES.values()})    # AdamWMultiClassDev, AdamWMultiDevArgs
GRAPH_STRUCTS = {c.removeprefix("mmdeer_"): cls for c, cls in _GRAPH_CLASSES.items()}
# include/mmdeer_drop_dev.h, the companion header of the same counter for mmdeer.h's three by-value dropout entries: symbols only
DROP_DEV_CONSTANTS, _DROP_DEV_CLASSES, DROP_DEV_SYMBOLS = _header.parse(_header.read(_header.DROP_DEV_HEADER_PATH), {}, {})
# include/mmdeer_seqlen.h, the companion header of the audio encoder's recurrence and pool with per-sample lengths: tables of its own again
_SEQLEN_NAMES = {"mmdeer_lstm_seq_len_args": "LstmSeqLenArgs", "mmdeer_temporal_pool_len_args": "TemporalPoolLenArgs"}
SEQLEN_CONSTANTS, _SEQLEN_CLASSES, SEQLEN_SYMBOLS = _header.parse(_header.read(_header.SEQLEN_HEADER_PATH), _SEQLEN_NAMES, {})
globals().update({cls.__name__: cls for cls in _SEQLEN_CLASSES.values()})    # LstmSeqLenArgs, TemporalPoolLenArgs
SEQLEN_STRUCTS = {c.removeprefix("mmdeer_"): cls for c, cls in _SEQLEN_CLASSES.items()}
GemmArgs = _CLASSES["mmdeer_gemm_args"]     # already a global by the update above; named here for gemm_args() below and for linters


def gemm_args(**fields):
    """An mmdeer_gemm_args with the neutral values (automatic tile, no dropout site, no mask scaling; all else zero) and ``fields``."""
    unknown = set(fields) - {name for name, _ in GemmArgs._fields_}
    if unknown:                        # ctypes itself would keep it as a plain attribute and pass the struct on without it
        raise TypeError(f"mmdeer_gemm_args has no field {sorted(unknown)}")
    return GemmArgs(**{"tile": -1, "drop_site": -1, "regen_site": -1, "mask_scale": 1.0, **fields})


def bind(lib: C.CDLL, require_all: bool = False) -> C.CDLL:
    """Set restype and argtypes of every symbol of include/mmdeer.h that ``lib`` exports (``require_all``: AttributeError for one
    it does not -- ABI drift between header and library)."""
    for name, res, args in SYMBOLS + VIDEO_SYMBOLS + FRAME_SYMBOLS + ROUTE_SYMBOLS + FRAME_BWD_SYMBOLS + BERT_SYMBOLS + BERT_BWD_SYMBOLS + BERT_DROP_SYMBOLS + OPTIM_SYMBOLS + GRAPH_SYMBOLS + DROP_DEV_SYMBOLS + SEQLEN_SYMBOLS:
        if require_all or hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    return lib


def lib_path() -> str:
    return _build.LIB_PATH


def load(build_if_missing: bool = True) -> C.CDLL:
    """Load (building first when the in-tree .so is missing or stale)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    with _LOCK:
        if _LIB is not None:
            return _LIB
        path = _build.LIB_PATH
        if build_if_missing and _build.needs_build():
            try:
                _build.build()
            except Exception as e:  # noqa: BLE001
                raise RuntimeError(
                    "libmmdeer_hip.so is missing or older than its sources and could not be (re)built with "
                    "hipcc --offload-arch=gfx950.  There is no CPU fallback for the mmdeer hot path and a stale "
                    f"library is never loaded.  Build error: {e}") from e
        if not os.path.exists(path):
            raise RuntimeError(f"libmmdeer_hip.so not found at {path}; run `python -m mmdeer.build`. "
                               "There is no CPU fallback for the mmdeer hot path.")
        lib = bind(C.CDLL(path), require_all=True)
        if lib.mmdeer_abi_version() != ABI_VERSION:
            raise RuntimeError("libmmdeer_hip.so ABI version mismatch")
        for cname, cls in {**STRUCTS, **VIDEO_STRUCTS, **FRAME_STRUCTS, **FRAME_BWD_STRUCTS, **BERT_STRUCTS, **BERT_BWD_STRUCTS, **BERT_DROP_STRUCTS, **OPTIM_STRUCTS, **GRAPH_STRUCTS, **SEQLEN_STRUCTS}.items():      # the ctypes mirrors against the library's own sizeof (a field added on one side only)
            if lib.mmdeer_sizeof(cname.encode()) != C.sizeof(cls):
                raise RuntimeError(f"mmdeer: ctypes layout of mmdeer_{cname} ({C.sizeof(cls)} bytes) differs from the library's "
                                   f"({lib.mmdeer_sizeof(cname.encode())})")
        # The library itself reads no environment variable (include/mmdeer.h).  For the A/B tools the host forwards
        # MMDEER_<OPTION> (e.g. MMDEER_FUSED_ATTN=0) to mmdeer_set_option once, here.
        i = 0
        while True:
            nm = lib.mmdeer_option_name(i)
            if nm is None:
                break
            env = os.environ.get("MMDEER_" + nm.decode().upper())
            if env is not None:
                if lib.mmdeer_set_option(nm, int(env)) != 0:
                    raise RuntimeError("mmdeer: " + lib.mmdeer_last_error().decode())
            i += 1
        _LIB = lib
    return _LIB


def set_option(name: str, value: int) -> None:
    """mmdeer_set_option: choose a launch plan (include/mmdeer.h lists the names); takes effect from the next call."""
    check(load().mmdeer_set_option(name.encode(), int(value)))


def get_option(name: str) -> int:
    v = C.c_int32(0)
    check(load().mmdeer_get_option(name.encode(), C.byref(v)))
    return v.value


class options:
    """``with _lib.options(fused_attn=0): ...`` -- set launch-plan options for a block and restore them afterwards."""

    def __init__(self, **kw):
        self.kw, self.old = kw, {}

    def __enter__(self):
        for k, v in self.kw.items():
            self.old[k] = get_option(k)
            set_option(k, v)
        return self

    def __exit__(self, *exc):
        for k, v in self.old.items():
            set_option(k, v)
        return False


def check(rc: int) -> None:
    if rc != 0:
        raise RuntimeError("mmdeer: " + load().mmdeer_last_error().decode())


def ptr(t) -> Optional[int]:
    """data_ptr of a tensor or None."""
    return None if t is None else t.data_ptr()


def set_bn_buffers(a, bn) -> None:
    """The running buffers of an nn BatchNorm module into the argument struct of a statistics call, which updates them on the device."""
    a.running_mean, a.running_var = bn.running_mean.data_ptr(), bn.running_var.data_ptr()
    a.num_batches_tracked, a.momentum = bn.num_batches_tracked.data_ptr(), bn.momentum


def current_stream() -> int:
    import torch
    return torch.cuda.current_stream().cuda_stream
