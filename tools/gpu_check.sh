#!/bin/bash
# The whole check on a GPU machine: build, the full bench (bench.py --full, with its tables), the GPU tests, smoke().
#   tools/gpu_check.sh [TAG] [extra pytest args]
# Logs and the bench line go to $OUT (default run_logs/).  The script stops at the first step that fails or times out.
TAG=${1:-check}; [ $# -gt 0 ] && shift
cd "$(dirname "$0")/.." || exit 1
OUT=${OUT:-run_logs}
mkdir -p "$OUT"
export TMPDIR=${TMPDIR:-/tmp}

step() {      # step NAME SECONDS COMMAND...: output to $OUT/NAME.log; the script ends at the first failure
  local name=$1 secs=$2; shift 2
  timeout -k 10 "$secs" "$@" > "$OUT/$name.log" 2>&1
  local rc=$?
  echo "$name: exit $rc"
  if [ $rc -ne 0 ]; then tail -n 40 "$OUT/$name.log"; exit $rc; fi
}

step build_$TAG 900 python -c "import __graft_entry__ as g; g.build()"
rocminfo 2>/dev/null | grep -m1 -oE "gfx[0-9a-f]+"
step bench_$TAG 900 python bench.py --full --steps 20 --warmup 5
grep '^{' "$OUT/bench_$TAG.log" | tail -n 1 > "$OUT/bench_$TAG.json"
cp bench_details.json "$OUT/bench_details_$TAG.json"
python tools/bench_table.py "$OUT/bench_$TAG.json" || exit 1
step pytest_gpu_$TAG 2400 python -m pytest tests -m gpu -q --timeout 1200 -p no:cacheprovider --durations=8 "$@"
tail -n 12 "$OUT/pytest_gpu_$TAG.log"
step smoke_$TAG 300 python -c "import __graft_entry__ as g; g.smoke()"
tail -n 1 "$OUT/smoke_$TAG.log"
