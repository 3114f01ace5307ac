#!/usr/bin/env python3
"""Do two builds of the library store the same bits in every BatchNorm operator?

    python tools/bn_ab_equal.py <library A> <library B> [--out listing.json]

One fresh child process per library, one after the other (the library is chosen as tools/bench_with_lib.py chooses it: the ABI is
the same in both).  The child runs a fixed, seeded list of cases -- the shapes and inputs of tests/test_gpu_video_encoder.py,
test_gpu_frame_encoder.py and test_gpu_frame_backward.py, in fp32 and bf16, with batch and with running statistics -- and prints
the sha256 of every output tensor:
  mmdeer_bn_time_stats / _apply / _bwd   R in {2, 390, 1221, 33001}: with and without `out`, mask_scale 1.25, and the dropout site into
                                         the interior of a padded buffer at B = 37, T = 7
  mmdeer_bn2d_stats / _apply             (N, H, W) in {(2, 1, 1), (6, 5, 13), (1, 61, 541)} x C in {64, 128, 256, 512}: PAD, POOL, AVG
  mmdeer_bn2d_bwd                        test_gpu_frame_backward.BN_CASES x the same C, the pool index bytes included
The parent compares the two listings and exits 1 at the first difference, naming the case and the tensor."""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 600     # seconds


def child(lib):
    sys.path.insert(0, ROOT)
    from mmdeer import build
    build.LIB_PATH = os.path.abspath(lib)
    build.needs_build = lambda: False
    import ctypes as C

    import torch

    from mmdeer import _lib, frames, video
    from tests import test_gpu_frame_backward as TB
    from tests import test_gpu_frame_encoder as TF
    from tests import test_gpu_video_encoder as TV

    def emit(case, **tensors):
        for name, t in tensors.items():
            digest = hashlib.sha256(t.detach().reshape(-1).contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()
            print(f"{case}\t{name}\t{digest}", flush=True)

    def module(kind, c):
        bn = kind(c)
        with torch.no_grad():
            bn.running_mean.copy_(torch.linspace(-1, 1, c)); bn.running_var.copy_(torch.linspace(0.5, 2, c)); bn.num_batches_tracked.fill_(41)
        return bn.to(TV.DEV)

    def buffers(bn):
        return {"running_mean": bn.running_mean, "running_var": bn.running_var, "num_batches_tracked": bn.num_batches_tracked}

    for compute in ("fp32", "bf16"):
        # ---- BatchNorm over time
        for Rn in (2, 390, 1221, 33001):
            case = f"bn_time R={Rn} {compute}"
            x, gamma, beta, dout = TV._bn_inputs(Rn, compute)
            bn = module(torch.nn.BatchNorm1d, TV.W)
            mean, rstd = video.bn_stats(x, compute, bn)
            emit(case + " stats", mean=mean, rstd=rstd, **buffers(bn))
            for running, (m, r) in ((False, (mean, rstd)), (True, (bn.running_mean, bn.running_var))):
                tag = f"{case} running={int(running)}"
                out = video.bn_apply(x, m, r, gamma, beta, torch.empty_like(x), compute, running=running)
                emit(tag + " apply", out=out)
                for with_out, scale in ((True, 1.0), (False, 1.0), (True, 1.25)):
                    dx, dg, db = video.bn_bwd(dout, out if with_out else None, x, m, r, gamma, torch.empty_like(x), compute,
                                              running=running, mask_scale=scale)
                    emit(f"{tag} bwd out={int(with_out)} mask_scale={scale}", dx=dx, dgamma=dg, dbeta=db)
        B, T = 37, 7
        x, gamma, beta, _ = TV._bn_inputs(B * T, compute, seed=2)
        mean, rstd = video.bn_stats(x, compute)
        buf = video.padded(T, B, TV._dt(compute), TV.DEV)
        video.bn_apply(x, mean, rstd, gamma, beta, video.interior(buf, B), compute, relu=False, drop=(0.3, 11, 5), site=145)
        emit(f"bn_time dropout B={B} T={T} {compute}", padded=buf)
        # ---- BatchNorm2d on channels-last rows, forward
        for N, H, W in TB.BN_SIZES:
            for c in (64, 128, 256, 512):
                case = f"bn2d N={N} H={H} W={W} C={c} {compute}"
                y, gamma, beta = TF._bn_inputs(N * H * W, c, compute)
                bn = module(torch.nn.BatchNorm2d, c)
                mean, rstd = frames.bn2d_stats(y, N, H, W, bn)
                emit(case + " stats", mean=mean, rstd=rstd, **buffers(bn))
                for running, (m, r) in ((False, (mean, rstd)), (True, (bn.running_mean, bn.running_var))):
                    for name, dest in (("pad", frames.PAD), ("pool", frames.POOL), ("avg", frames.AVG)):
                        emit(f"{case} running={int(running)} apply", **{name: frames.bn2d_apply(y, N, H, W, m, r, gamma, beta, dest, running=running)})
        # ---- BatchNorm2d backward, through the C ABI so that the pool index bytes are in hand
        for N, H, W, src in TB.BN_CASES:
            for c in (64, 128, 256, 512):
                y, gamma, beta, dout, rm, rv = TB.bn_bwd_inputs(N, H, W, c, compute, src)
                for running, (m, r) in ((False, frames.bn2d_stats(y, N, H, W)), (True, (rm, rv))):
                    dy, dg, db = torch.empty_like(y), torch.empty(c, device=TV.DEV), torch.empty(c, device=TV.DEV)
                    scratch = torch.empty(_lib.BN2D_BWD_SCRATCH, device=TV.DEV)
                    idx = torch.zeros(N * frames.conv_out(H, 3) * frames.conv_out(W, 3) * c, dtype=torch.uint8, device=TV.DEV)
                    a = _lib.Bn2dBwdArgs()
                    a.y, a.mean, a.rstd, a.gamma, a.beta = y.data_ptr(), m.data_ptr(), r.data_ptr(), gamma.data_ptr(), beta.data_ptr()
                    a.dout, a.dy, a.dgamma, a.dbeta, a.scratch, a.pool_idx = dout.data_ptr(), dy.data_ptr(), dg.data_ptr(), db.data_ptr(), scratch.data_ptr(), idx.data_ptr()
                    a.eps, a.src, a.running = 1e-5, TB.SRCS[src], int(running)
                    a.N, a.H, a.W, a.C, a.act_f32, a.stream = N, H, W, c, int(compute == "fp32"), _lib.current_stream()
                    _lib.check(_lib.load().mmdeer_bn2d_bwd(C.byref(a)))
                    out = {"dy": dy, "dgamma": dg, "dbeta": db}
                    if src == "pool":
                        out["pool_idx"] = idx
                    emit(f"bn2d_bwd N={N} H={H} W={W} C={c} {src} {compute} running={int(running)}", **out)
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
