#!/bin/bash
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/bench_out}
mkdir -p "$OUT"
# runs on the GPU box: full gpu pytest + bench (no cpu baseline)
{ timeout 500 python -m pytest tests -m gpu -q; echo "PYTEST_RC=$?";
  timeout 400 python bench.py --full --steps 5 --warmup 2 --skip-cpu-baseline;
  echo "BENCH_RC=$?"; } > $OUT/gpu_check.log 2>&1
grep -E "passed|failed|RC=" $OUT/gpu_check.log
