#!/bin/bash
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/bench_out}
mkdir -p "$OUT"
{ timeout 900 python bench.py --full --sf 300 --steps 3 --warmup 1;
  echo "SF300_RC=$?"; } > $OUT/sf300.log 2>&1
grep -E "SF300_RC" $OUT/sf300.log
