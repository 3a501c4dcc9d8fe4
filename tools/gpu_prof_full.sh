#!/bin/bash
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/bench_out}
mkdir -p "$OUT"
export TMPDIR=/tmp
cd $R
{ timeout 600 rocprofv3 --kernel-trace --stats -d $OUT/prof_full -- \
    python bench.py --full --steps 3 --warmup 1 --skip-cpu-baseline;
  echo "TRACE_RC=$?"; } > $OUT/prof_full.log 2>&1
{ timeout 300 rocprofv3 --kernel-trace -d $OUT/prof_sort -- \
    python -m pytest tests/test_gpu_sort.py -m gpu -q;
  echo "SORT_RC=$?"; } >> $OUT/prof_full.log 2>&1
grep -E "RC=" $OUT/prof_full.log
