#!/usr/bin/env python3
"""Time StatisticalValidator.compute_confidence_intervals (mmdeer/evaluation.py) at N in {20,000, 100,000, 1,000,000},
R = 1000 replicates, three dimensions, beside the float64 numpy restatement (tests/eval_ref.py) on the same machine's host.

Per N, after `--warmup` calls: `--runs` timed calls in one process.  `call_ms` is a host clock around the whole public call
(it ends in the copy of ci[D][2] to the host, i.e. in a synchronise); `moments_ms` is the two-event time of
mmdeer_bootstrap_moments alone (repack + gather + fold) and `gather_GBps` = R * N * 32 bytes over it: the bytes the draws
read from the repacked table, not a share of any peak.  The host figure times `--host-reps` replicates of the restatement
(index recipe, gather, masked float64 sums) and scales them to R; it is a yardstick, not a tuned baseline.
Prints one JSON object.

    python tools/eval_bootstrap_time.py [--runs 20] [--warmup 3] [--R 1000] [--N 20000,100000,1000000] [--host-reps 10]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mmdeer import evaluation as M, synth  # noqa: E402
from tests import eval_ref as E  # noqa: E402


def spread(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--R", type=int, default=1000)
    ap.add_argument("--N", default="20000,100000,1000000")
    ap.add_argument("--host-reps", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_bootstrap_time: needs a GPU (a timing taken without one says nothing)")
    dev = "cuda:0"
    res = {"device": torch.cuda.get_device_name(0), "R": a.R, "runs": a.runs, "warmup": a.warmup, "host_reps": a.host_reps, "rows": []}
    sv = M.StatisticalValidator(0.95)
    for N in [int(v) for v in a.N.split(",")]:
        p = (synth.normal(71, N * 3).reshape(N, 3) * 0.6).astype(np.float32)
        t = (0.9 * p + 0.3 * synth.normal(72, N * 3).reshape(N, 3)).astype(np.float32)
        P, T = torch.from_numpy(p).to(dev), torch.from_numpy(t).to(dev)
        for _ in range(a.warmup):
            ci = sv.compute_confidence_intervals(P, T, n_bootstrap=a.R, seed=1)
        call, mom_ms = [], []
        for _ in range(a.runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ci = sv.compute_confidence_intervals(P, T, n_bootstrap=a.R, seed=1)
            call.append((time.perf_counter() - t0) * 1e3)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            M.bootstrap_moments(P, T, a.R, 1)
            e1.record()
            torch.cuda.synchronize()
            mom_ms.append(e0.elapsed_time(e1))
        t0 = time.perf_counter()
        mom, flags = E.bootstrap_moments(p, t, a.host_reps, 1)
        host_s = (time.perf_counter() - t0) * a.R / a.host_reps
        row = {"N": N, "call": spread(call), "moments": spread(mom_ms),
               "gather_GBps": round(a.R * N * 32 / (statistics.median(mom_ms) * 1e-3) / 1e9, 1),
               "host_restatement_s_scaled_to_R": round(host_s, 2), "ci_valence": list(ci["valence"])}
        res["rows"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
