#!/bin/bash
# Quick GPU-box session: GPU test suite, smoke, the bench line, and the same step through the RCCL exchange path on one rank.
# Outputs under OUTDIR, the one argument.
OUT=${1:?usage: bash tools/run_gpu_check.sh OUTDIR}
cd /tmp && export TMPDIR=/tmp && cd - >/dev/null
mkdir -p $OUT
python -m pytest tests -m gpu -q -x 2>&1 | tail -25 > $OUT/pytest_gpu.log
cat $OUT/pytest_gpu.log | tail -12
python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1; tail -2 $OUT/smoke.log
python bench.py --full --steps 20 --warmup 5 > $OUT/bench.json 2> $OUT/bench.err; tail -c 1500 $OUT/bench.json; tail -3 $OUT/bench.err
DYK_FORCE_DDP=1 MASTER_ADDR=127.0.0.1 MASTER_PORT=29533 RANK=0 WORLD_SIZE=1 LOCAL_RANK=0 python bench.py --steps 12 --warmup 3 --no-cpu-baseline --no-roofline > $OUT/bench_ddp1.json 2> $OUT/bench_ddp1.err; tail -c 600 $OUT/bench_ddp1.json; tail -3 $OUT/bench_ddp1.err
python bench.py --gpus 2 --steps 2 --warmup 1 > $OUT/bench_gpus2.log 2>&1; tail -2 $OUT/bench_gpus2.log
