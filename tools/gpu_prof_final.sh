#!/bin/bash
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/bench_out}
mkdir -p "$OUT"
# fresh kernel-trace profile of the full bench (Q1+Q3+Q5) + SF300 evidence
cd /tmp && export TMPDIR=/tmp
rm -rf /tmp/proff && mkdir -p /tmp/proff
{ timeout 600 rocprofv3 --kernel-trace --stats -d /tmp/proff -o tr -- python $R/bench.py --full --steps 3 --warmup 1 --skip-cpu-baseline > /tmp/bench_prof.json 2>/tmp/bench_prof.err; echo "PROF_RC=$?"; } > $OUT/proffinal.log 2>&1
DB=$(find /tmp/proff -name '*.db' | head -1)
{ python $R/tools/rocpd_summary.py "$DB"; } > $OUT/kernel_trace_final.txt 2>&1
cp /tmp/bench_prof.json $OUT/ 2>/dev/null
cd $R
{ timeout 600 python bench.py --full --sf 300 --steps 3 --warmup 1 --skip-cpu-baseline > $OUT/sf300_final.json 2>$OUT/sf300_final.err; echo "SF300_RC=$?"; } >> $OUT/proffinal.log 2>&1
{ timeout 300 python -m pytest tests/test_gpu_engine.py tests/test_gpu_fullsize.py -q; echo "PYTEST_RC=$?"; } >> $OUT/proffinal.log 2>&1
grep -E "RC=|passed|failed" $OUT/proffinal.log
