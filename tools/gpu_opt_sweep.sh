#!/bin/bash
# bench.py under a list of launch-plan options (each "NAME=VALUE[,NAME=VALUE]"), one line per setting: ms/step and the
# rocprofv3-free in-run roofline figure.  usage: gpu_opt_sweep.sh "" "SPLITK_MAX=4" "KSTEPS=24" ...
set -u
OUT=${OUT:-bench_out}; mkdir -p "$OUT"
for cfg in "$@"; do
  envs=""; for kv in ${cfg//,/ }; do envs="$envs MMDEER_$kv"; done
  env $envs timeout -k 10 300 python bench.py --full --steps 40 --warmup 10 --no-cpu-baseline ${BENCH_ARGS:-} > "$OUT/sweep.json" 2> "$OUT/sweep.err"
  python - "$cfg" "$OUT" <<'PY'
import json, os, sys
out = sys.argv[2]
try:
    d = json.loads([l for l in open(os.path.join(out, "sweep.json")) if l.startswith("{")][-1])
    print(f"{sys.argv[1] or 'default':28s} ms/step {d['ms_per_step']:.4f} (min {d['ms_per_step_min']:.4f} median {d['ms_per_step_median']:.4f})  roofline {d['roofline']['avg_launch_us']} us")
except Exception as e:
    print(sys.argv[1], "FAILED", e, open(os.path.join(out, "sweep.err")).read()[-400:])
PY
done
