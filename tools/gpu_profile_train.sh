#!/bin/bash
# rocprofv3 passes over the device train step (tools/train_step_trace.py: rgcn_train_step_device on resident inputs,
# N = 330,000 decoder triples, every kernel on the main stream): kernel trace + stats, then FETCH_SIZE and WRITE_SIZE in
# separate --pmc runs.
#   tools/gpu_profile_train.sh TAG [fb15k]
# The summary goes to $OUT/<tag>_rocprof_train_step[_fb15k].md (OUT default run_logs/).  The script stops at the first pass
# that fails or times out.
TAG=${1:-prof}; WL=$2
cd "$(dirname "$0")/.." || exit 1
OUT=${OUT:-run_logs}
export TMPDIR=${TMPDIR:-/tmp}
export RGCN_STREAMS=0
CMD="python tools/train_step_trace.py 12 $WL"
SUF=""; [ -n "$WL" ] && SUF="_$WL"
P=$OUT/prof_${TAG}_train_step${SUF}
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
python tools/rocprof_summary.py "$P" "$OUT/${TAG}_rocprof_train_step${SUF}.md" "RGCN_STREAMS=0 $CMD" | head -45
rm -rf "$P/trace" "$P/pmc_fetch" "$P/pmc_write"
