#!/bin/bash
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/bench_out}
mkdir -p "$OUT"
# full validation + fresh profiles + SF300 evidence
cd $R
{ timeout 600 python -m pytest tests -m gpu -q; echo "PYTEST_RC=$?"; } > $OUT/full2.log 2>&1
{ timeout 300 python bench.py --full --steps 5 --warmup 2 --skip-cpu-baseline; echo "BENCH_RC=$?"; } >> $OUT/full2.log 2>&1
cd /tmp && export TMPDIR=/tmp
{ timeout 600 rocprofv3 --kernel-trace --stats -d /tmp/prof -o trace -- python $R/bench.py --full --steps 3 --warmup 1 --skip-cpu-baseline > /dev/null 2>&1; echo "PROF_RC=$?"; } >> $OUT/full2.log 2>&1
cp /tmp/prof/*trace*stats* $OUT/ 2>/dev/null || find /tmp/prof -name '*stats*' -exec cp {} $OUT/ \; 2>/dev/null
ls /tmp/prof >> $OUT/full2.log 2>&1
cd $R
{ GG_BIG=300 timeout 500 python bench.py --full --steps 3 --warmup 1 --skip-cpu-baseline > $OUT/sf300.json 2>$OUT/sf300.err; echo "SF300_RC=$?"; } >> $OUT/full2.log 2>&1
grep -E "passed|failed|RC=" $OUT/full2.log
