#!/bin/bash
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/bench_out}
mkdir -p "$OUT"
# round-2 call A: full GPU suite (incl. new multiproc/sparse tests) +
# bench with the v2 probe/topk kernels + kernel trace
{ timeout 1100 python -m pytest tests -m gpu -q; echo "PYTEST_RC=$?"; } \
  > $OUT/r02b_pytest.log 2>&1
{ timeout 400 python bench.py --full --steps 10 --warmup 3; echo "BENCH_RC=$?"; } \
  > $OUT/r02b_bench.log 2>&1
cd /tmp && export TMPDIR=/tmp
rm -rf /tmp/proff && mkdir -p /tmp/proff
{ timeout 400 rocprofv3 --kernel-trace --stats -d /tmp/proff -o tr -- \
    python $R/bench.py --full --steps 3 --warmup 1 --skip-cpu-baseline \
    > /tmp/bench_prof.json 2>/tmp/bench_prof.err; echo "PROF_RC=$?"; } \
  > $OUT/r02b_prof.log 2>&1
DB=$(find /tmp/proff -name '*.db' | head -1)
python $R/tools/rocpd_summary.py "$DB" \
  > $OUT/r02b_kernel_trace.txt 2>&1
cd $R
grep -E "passed|failed|RC=" $OUT/r02b_pytest.log $OUT/r02b_prof.log
tail -c 1500 $OUT/r02b_bench.log
