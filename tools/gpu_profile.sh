#!/bin/bash
# rocprofv3 passes over the plain bench run of one workload: kernel trace + stats, then FETCH_SIZE and WRITE_SIZE in
# SEPARATE --pmc runs (they do not fit one pass on gfx950 -- MI355X_MICROARCH.md, and a counter run carries no tracing).
#   tools/gpu_profile.sh TAG WORKLOAD [serial]     serial: exclusive kernel durations (no side streams, no pipelined prep)
# The summary goes to $OUT/<tag>_rocprof_<workload>[_serial].md (+ _traffic.json; OUT default run_logs/): copy the ones
# to keep into profiles/.  The script stops at the first pass that fails or times out.
TAG=${1:-prof}; WL=${2:-fb237_block}; MODE=$3
cd "$(dirname "$0")/.." || exit 1
OUT=${OUT:-run_logs}
export TMPDIR=${TMPDIR:-/tmp}
SUF=""; ENVS=""
if [ "$MODE" = "serial" ]; then export RGCN_STREAMS=0 RGCN_BENCH_PREFETCH=0; SUF="_serial"; ENVS="RGCN_STREAMS=0 RGCN_BENCH_PREFETCH=0 "; fi
CMD="python bench.py --workload $WL --steps 20 --warmup 5"
P=$OUT/prof_${TAG}_${WL}${SUF}
rm -rf "$P"; mkdir -p "$P"

profile() {      # profile NAME ROCPROF-ARGS...: one rocprofv3 run over $CMD; the script ends at the first failure
  local name=$1; shift
  # shellcheck disable=SC2086
  timeout -k 10 300 rocprofv3 "$@" -- $CMD > "$P/$name.log" 2>&1
  local rc=$?
  echo "$name: exit $rc"
  if [ $rc -ne 0 ]; then tail -n 20 "$P/$name.log"; exit $rc; fi
}

timeout -k 10 900 python -c "import __graft_entry__ as g; g.build()" > "$P/build.log" 2>&1 || { tail -n 20 "$P/build.log"; exit 1; }
profile trace --kernel-trace --stats -d "$P/trace" -o trace
profile fetch --pmc FETCH_SIZE -d "$P/pmc_fetch" -o fetch
profile write --pmc WRITE_SIZE -d "$P/pmc_write" -o write
python tools/rocprof_summary.py "$P" "$OUT/${TAG}_rocprof_${WL}${SUF}.md" "$ENVS$CMD" | head -40
rm -rf "$P/trace" "$P/pmc_fetch" "$P/pmc_write"      # the per-dispatch databases: the summaries are what is kept
