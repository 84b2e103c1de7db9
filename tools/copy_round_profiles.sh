#!/bin/bash
# OUTDIR (scratch, written by tools/run_gpu_round.sh OUTDIR) -> profiles/<tag>_* (tracked): the files the judge reads
# usage: tools/copy_round_profiles.sh TAG OUTDIR
T=${1:-r06}
SRC=$(cd "${2:?usage: tools/copy_round_profiles.sh TAG OUTDIR}" && pwd) || exit 1
cd "$(dirname "$0")/.."
cp $SRC/bench.json profiles/${T}_bench.json
cp $SRC/bench_b1.json profiles/${T}_bench_b1.json
cp $SRC/bench_c5.json profiles/${T}_bench_mobilenetv3_b32.json
cp $SRC/bench_eval_c3.json profiles/${T}_bench_eval_target_bf16.json
cp $SRC/bench_eval_c2.json profiles/${T}_bench_eval_dyolov3_add_sl_fp32.json
cp $SRC/bench_eval_c3_fp32.json profiles/${T}_bench_eval_target_fp32.json
cp $SRC/ap_64pair.json profiles/${T}_ap_64pair.json 2>/dev/null
cp $SRC/serial_kernels.txt profiles/${T}_serial_kernels.txt 2>/dev/null; cp $SRC/serial_kernels.json profiles/${T}_serial_kernels.json 2>/dev/null
for c in c3 c5 b1 c3_full; do cp $SRC/cmd_roofline_$c.txt profiles/${T}_cmd_roofline_$c.txt; done
for f in pmc_summary.txt pmc_summary.json pmc_sq_summary.txt pmc_sq_summary.json step_kernels.txt step_kernels.json step_timeline.txt; do cp $SRC/$f profiles/${T}_$f; done
cp $SRC/prof/r3_kernel_stats.csv profiles/${T}_bench_kernel_stats.csv 2>/dev/null
python - <<PY
import json
for f in ("bench", "bench_mobilenetv3_b32", "bench_b1", "bench_eval_target_bf16"):
    d = json.loads(open("profiles/${T}_%s.json" % f).read().strip().splitlines()[-1])
    print(f, round(d["ms_per_step"], 2), "ms", round(d["value"], 1), d.get("roofline", {}).get("frac_is", "")[:60])
print(open("profiles/${T}_pmc_summary.txt").readline().strip())
print(open("profiles/${T}_step_kernels.txt").readline().strip())
print("code hash", json.load(open("profiles/${T}_step_kernels.json"))["code_sha"], json.load(open("profiles/${T}_pmc_summary.json"))["code_sha"])
PY
python tools/code_sha.py
