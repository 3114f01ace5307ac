#!/usr/bin/env python3
"""Time UncertaintyAnalyzer.analyze_uncertainty_quality (mmdeer/evaluation.py) at N in {20,000, 100,000}, three dimensions,
beside the float64 numpy restatement (tests/uncertainty_ref.py) on the same machine's host.

Per N, after `--warmup` calls: `--runs` timed calls in one process.  `call_ms` is a host clock around the whole public call
(it ends in the copies of the table and of the bin tables to the host, i.e. in a synchronise); `table_ms` is the two-event
time of mmdeer_uncertainty_table alone (two moment passes, the sort of the three columns, the prefix gather, the fold).
`host_ms` times the restatement INCLUDING the device-to-host copy of the three (N, 3) arrays it needs: what a user does
today.  It is the baseline, not the code under test, and it is plain numpy, not a tuned implementation.
Prints one JSON object.

    python tools/uncertainty_analysis_time.py [--runs 20] [--warmup 3] [--N 20000,100000]
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
from tests import uncertainty_ref as U  # noqa: E402


def spread(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--N", default="20000,100000")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("uncertainty_analysis_time: needs a GPU (a timing taken without one says nothing)")
    dev = "cuda:0"
    res = {"device": torch.cuda.get_device_name(0), "D": 3, "runs": a.runs, "warmup": a.warmup, "rows": []}
    an = M.UncertaintyAnalyzer()
    for N in [int(v) for v in a.N.split(",")]:
        p = (synth.normal(81, N * 3).reshape(N, 3) * 0.6).astype(np.float32)
        t = (0.9 * p + 0.3 * synth.normal(82, N * 3).reshape(N, 3)).astype(np.float32)
        u = (0.02 + 0.5 * synth.uniform01(83, N * 3).reshape(N, 3) + 0.3 * np.abs(p - t)).astype(np.float32)
        P, T, Uu = (torch.from_numpy(x).to(dev) for x in (p, t, u))
        keep = M.sparsification_cuts(N)
        for _ in range(a.warmup):
            out = an.analyze_uncertainty_quality(P, T, Uu)
        call, table, host = [], [], []
        for _ in range(a.runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = an.analyze_uncertainty_quality(P, T, Uu)
            call.append((time.perf_counter() - t0) * 1e3)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            M.uncertainty_table_device(P, T, Uu, keep)
            e1.record()
            torch.cuda.synchronize()
            table.append(e0.elapsed_time(e1))
            t0 = time.perf_counter()
            own = U.analyze(P.cpu().numpy(), T.cpu().numpy(), Uu.cpu().numpy())
            host.append((time.perf_counter() - t0) * 1e3)
        row = {"N": N, "call": spread(call), "table": spread(table), "host_restatement_with_copy": spread(host),
               "valence_ause": out["sparsification_analysis"]["valence_ause"],
               "valence_ause_host": own["sparsification_analysis"]["valence_ause"]}
        res["rows"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
