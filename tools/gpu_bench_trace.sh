#!/bin/bash
# Kernel timeline of the default bench step (pipelined): rocprofv3 --kernel-trace over the plain bench run, then
# tools/train_step_timeline.py on its last complete step.  Output in $OUT/bench_trace (OUT default run_logs/).
cd "$(dirname "$0")/.." || exit 1
OUT=${OUT:-run_logs}/bench_trace
rm -rf "$OUT"; mkdir -p "$OUT"
export TMPDIR=${TMPDIR:-/tmp}
timeout -k 10 900 python -c "import __graft_entry__ as g; g.build()" > "$OUT/build.log" 2>&1 || { tail -n 20 "$OUT/build.log"; exit 1; }
timeout -k 10 300 rocprofv3 --kernel-trace --output-format csv -d "$OUT" -o trace -- \
  python bench.py --steps 20 --warmup 5 --gemm-mode 6 > "$OUT/log.txt" 2>&1
rc=$?
echo "trace: exit $rc"
if [ $rc -ne 0 ]; then tail -n 20 "$OUT/log.txt"; exit $rc; fi
f=$(find "$OUT" -name "*kernel_trace.csv" | head -1)
python tools/train_step_timeline.py "$f" k_colsum_final > "$OUT/timeline.txt" 2>&1 || { tail -n 20 "$OUT/timeline.txt"; exit 1; }
head -n 120 "$OUT/timeline.txt"
