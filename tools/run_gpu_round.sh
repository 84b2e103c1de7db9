#!/bin/bash
# One GPU-box session: full GPU test suite, smoke, bench, rocprofv3 kernel-trace summary, PMC passes (HBM traffic).
# Outputs under OUTDIR, the one argument (copy what should be judged into profiles/ with tools/copy_round_profiles.sh).
OUT=$(mkdir -p "${1:?usage: bash tools/run_gpu_round.sh OUTDIR}" && cd "$1" && pwd) || exit 1
set -x
cd /tmp && export TMPDIR=/tmp && cd - >/dev/null
rm -f $OUT/ap_64pair.json
DYK_AP_JSON=$OUT/ap_64pair.json python -m pytest tests -m gpu -q 2>&1 | grep -vE "RCCL version|HIP version|ROCm version|Hostname|Librccl path|amdgpu.ids" | tail -60 > $OUT/pytest_gpu.log
python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1
python bench.py --full --steps 20 --warmup 5 --dump-cmds $OUT/cmds_c3.json > $OUT/bench.json 2> $OUT/bench.err
python tools/cmd_roofline.py $OUT/cmds_c3.json > $OUT/cmd_roofline_c3.txt 2>&1
DYK_ROOFLINE_TOP=1000 python tools/cmd_roofline.py $OUT/cmds_c3.json > $OUT/cmd_roofline_c3_full.txt 2>&1
tail -c 3000 $OUT/bench.json
# the other BASELINE configs (parity-test cases; kept beside the bench line for reference)
python bench.py --mode eval --cfg kaist_dyolov3_add_sl --dtype fp32 --steps 10 --warmup 3 > $OUT/bench_eval_c2.json 2>/dev/null
python bench.py --mode eval --steps 10 --warmup 3 > $OUT/bench_eval_c3.json 2>/dev/null
# the declared AP-parity path (fp32 evaluation of the target cfg) gets its throughput number too
python bench.py --mode eval --dtype fp32 --steps 10 --warmup 3 > $OUT/bench_eval_c3_fp32.json 2>/dev/null
python bench.py --cfg kaist_dyolov4_mobilenetv3_fshare_global_cse3 --batch 32 --steps 10 --warmup 3 --full --no-cpu-baseline --dump-cmds $OUT/cmds_c5.json > $OUT/bench_c5.json 2>/dev/null
python tools/cmd_roofline.py $OUT/cmds_c5.json > $OUT/cmd_roofline_c5.txt 2>&1
python bench.py --batch 1 --steps 30 --warmup 5 --full --no-cpu-baseline --dump-cmds $OUT/cmds_b1.json > $OUT/bench_b1.json 2>/dev/null
python tools/cmd_roofline.py $OUT/cmds_b1.json > $OUT/cmd_roofline_b1.txt 2>&1
rm -f $OUT/cmds_c3.json $OUT/cmds_c5.json $OUT/cmds_b1.json
rm -rf $OUT/prof $OUT/pmc_fetch $OUT/pmc_write && mkdir -p $OUT/prof
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof -o r3 -- python bench.py --steps 5 --warmup 2 --no-cpu-baseline --no-roofline > $OUT/prof/bench_under_prof.json 2> $OUT/prof/err.log
# the same plan on ONE stream: every kernel alone on the chip, the rocprofv3 counterpart of bench.py's live isolated figure
rm -rf $OUT/prof_serial && mkdir -p $OUT/prof_serial
DYK_STREAMS=1 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_serial -o s1 -- python bench.py --steps 3 --warmup 2 --no-cpu-baseline --no-roofline > $OUT/prof_serial/bench_under_prof.json 2> $OUT/prof_serial/err.log
python tools/step_kernel_summary.py $(ls $OUT/prof_serial/s1_kernel_trace.csv $OUT/prof_serial/*/s1_kernel_trace.csv 2>/dev/null | head -1) $OUT/serial_kernels.json > $OUT/serial_kernels.txt 2>&1
find $OUT/prof_serial -name "*kernel_trace.csv" -delete
# counters in their own runs, one pass per counter (TCC slots), kernel trace only
rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $OUT/pmc_fetch -o f -- python bench.py --steps 2 --warmup 1 --no-cpu-baseline --no-roofline > $OUT/pmc_fetch.log 2>&1
rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $OUT/pmc_write -o w -- python bench.py --steps 2 --warmup 1 --no-cpu-baseline --no-roofline > $OUT/pmc_write.log 2>&1
python tools/pmc_summary.py $OUT/pmc_fetch $OUT/pmc_write $OUT/pmc_summary.json > $OUT/pmc_summary.txt 2>&1
bash tools/run_pmc_sq.sh $OUT > $OUT/pmc_sq_run.log 2>&1
cat $OUT/pmc_summary.txt
# one step's kernels by family (durations as they ran in the step, autotune trials excluded) and per-stream occupancy
python tools/step_kernel_summary.py $OUT/prof/*/r3_kernel_trace.csv $OUT/step_kernels.json > $OUT/step_kernels.txt 2>&1 || python tools/step_kernel_summary.py $OUT/prof/r3_kernel_trace.csv $OUT/step_kernels.json > $OUT/step_kernels.txt 2>&1
head -20 $OUT/step_kernels.txt
python tools/trace_timeline.py $(ls $OUT/prof/r3_kernel_trace.csv $OUT/prof/*/r3_kernel_trace.csv 2>/dev/null | head -1) > $OUT/step_timeline.txt 2>&1
# keep the merge small: drop the per-dispatch traces
find $OUT/pmc_fetch $OUT/pmc_write -name "*kernel_trace.csv" -delete
find $OUT/pmc_fetch $OUT/pmc_write -name "*counter_collection.csv" -size +20M -delete
ls -R $OUT/prof | head -30
