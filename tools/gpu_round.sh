#!/bin/bash
# Runs ON THE GPU BOX (via gpurun): parity tests, smoke, a short bench and a rocprofv3 kernel trace of it.
# Everything lands in $OUT (an absolute path; default out/ in the repository).  Usage: tools/gpu_round.sh [tests|bench|prof|all]
set -u
what=${1:-all}
ROOT=$PWD; OUT=${OUT:-$ROOT/out}; export OUT; mkdir -p "$OUT"
export TMPDIR=/tmp
export PYTHONUNBUFFERED=1
rocminfo 2>/dev/null | grep -E "Marketing Name|Compute Unit|Max Clock" | head -6 > $OUT/device.txt
nproc >> $OUT/device.txt; lscpu | grep -E "Model name|^CPU\(s\)" >> $OUT/device.txt
if [[ $what == all || $what == tests ]]; then
  timeout 1500 python -m pytest tests -m gpu -q -s --timeout 600 -p no:cacheprovider > $OUT/tests.log 2>&1
  echo "pytest exit $?" >> $OUT/tests.log
  tail -5 $OUT/tests.log
fi
if [[ $what == all || $what == smoke ]]; then
  timeout 600 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1; echo "smoke exit $?" >> $OUT/smoke.log; tail -3 $OUT/smoke.log
fi
if [[ $what == all || $what == bench ]]; then
  timeout 900 python bench.py --full --steps ${STEPS:-10} --warmup 3 > $OUT/bench.log 2>&1; echo "bench exit $?" >> $OUT/bench.log; tail -4 $OUT/bench.log
fi
if [[ $what == all || $what == prof ]]; then
  rm -rf $OUT/prof
  (cd /tmp && timeout 900 rocprofv3 --kernel-trace --stats -d $OUT/prof -o r01 -- python $ROOT/bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --lanes 1) > $OUT/prof.log 2>&1
  echo "prof exit $?" >> $OUT/prof.log
  db=$(find $OUT/prof -name "*.db" | head -1); python tools/prof_steady.py $db 2 > $OUT/prof_steady.txt 2>&1; head -12 $OUT/prof_steady.txt; tail -3 $OUT/prof.log
fi
if [[ $what == pmc ]]; then
  # PMC passes on the dominant kernel only, counters in their own runs (no trace domains besides kernel-trace)
  for c in FETCH_SIZE WRITE_SIZE "SQ_WAVES SQ_BUSY_CYCLES SQ_VALU_MFMA_BUSY_CYCLES SQ_INSTS_MFMA GRBM_GUI_ACTIVE" "SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_WAIT_INST_ANY SQ_WAIT_ANY SQ_ACTIVE_INST_ANY SQ_WAVE_CYCLES"; do
    tag=$(echo $c | tr ' ' '_' | cut -c1-40)
    (cd /tmp && timeout 300 rocprofv3 --pmc $c --kernel-trace -d $OUT/pmc_$tag -o pmc -- python $ROOT/tools/pmc_conv.py 3 ${PMC_CFG:-0}) > $OUT/pmc_$tag.log 2>&1
    echo "pmc $tag exit $?"; tail -2 $OUT/pmc_$tag.log
  done
  python tools/pmc_summary.py ${ROUND:-r02} 3 | tail -12
  rm -rf $OUT/pmc_*/ gpucore.*
fi
