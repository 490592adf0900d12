#!/bin/bash
# steady-state kernel trace of one bench workload (single lane, graph replay).  Usage: bash tools/gpu_trace_workload.sh <tag> <workload> [bench args]
set -u
ROOT=$PWD; OUT=${OUT:-$ROOT/out}; export OUT; mkdir -p "$OUT"; export TMPDIR=/tmp PYTHONUNBUFFERED=1
R=$1; W=$2; shift 2
rm -rf $OUT/prof_w
(cd /tmp && timeout 400 rocprofv3 --kernel-trace --stats -d $OUT/prof_w -o $R -- python $ROOT/bench.py --full --workload $W --steps 5 --warmup 2 --no-cpu-baseline --no-alt-precision --no-sequence-leg --lanes 1 "$@") > $OUT/prof_w.log 2>&1; echo "prof exit $?"
db=$(find $OUT/prof_w -name "*.db" | head -1); python tools/prof_steady.py $db 2 > $OUT/${R}_kernel_trace_${W}.txt 2>&1; head -45 $OUT/${R}_kernel_trace_${W}.txt | cut -c1-160
rm -rf $OUT/prof_w gpucore.*
