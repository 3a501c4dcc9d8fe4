#!/bin/bash
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/bench_out}
mkdir -p "$OUT"
export TMPDIR=/tmp
cd $R
{ timeout 500 rocprofv3 --kernel-trace -d $OUT/q3prof -- python bench.py --full --steps 3 --warmup 1 --skip-cpu-baseline; echo RC=$?; } > $OUT/q3prof.log 2>&1
grep RC= $OUT/q3prof.log
