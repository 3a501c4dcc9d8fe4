#!/bin/bash
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/bench_out}
mkdir -p "$OUT"
export TMPDIR=/tmp
cd $R
{ timeout 500 rocprofv3 --kernel-trace --stats -d $OUT/p2_trace -- python bench.py --full --steps 3 --warmup 1 --skip-cpu-baseline;
  echo TRACE_RC=$?;
  timeout 300 rocprofv3 --pmc FETCH_SIZE -d $OUT/p2_fetch -- python bench.py --steps 3 --warmup 1 --skip-q3 --skip-cpu-baseline;
  echo FETCH_RC=$?;
  timeout 300 rocprofv3 --pmc WRITE_SIZE -d $OUT/p2_write -- python bench.py --steps 3 --warmup 1 --skip-q3 --skip-cpu-baseline;
  echo WRITE_RC=$?; } > $OUT/prof2.log 2>&1
grep -E "RC=" $OUT/prof2.log
