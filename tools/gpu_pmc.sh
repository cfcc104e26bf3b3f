#!/bin/bash
# PMC counters of the kernels whose names contain KERNEL_SUBSTRING, on one stream (exclusive kernel durations).  Every
# counter pass is a rocprofv3 --pmc run of its own, with no tracing in the same run (the counters of one pass must fit
# the hardware's counter slots; MI355X_MICROARCH.md).
#   tools/gpu_pmc.sh WORKLOAD KERNEL_SUBSTRING [SET]
# WORKLOAD: a bench.py workload (fb237_block, fb237_block_traingraph, ...); train_step or train_step_fb15k: the device train
# step of tools/train_step_trace.py; gemm: the GEMM kernels on their own (tools/gemm_pmc.py, librgcn_devtools.so).
# SET, the named counter sets (default: rows):
#   rows  where a layer kernel's cycles go: waves, instruction mix, LDS, L1 / L2 requests, bytes (k_block_rows)
#   msg   the same without the LDS and bytes passes: the HBM-bound kernels (k_block_msg_fwd / _bwd, k_combine; on
#         fb237_block_traingraph the full-graph scale)
#   dec   the decoder's entity-gradient kernels in the train step (k_dec_ent): L2 hit rate, fabric bytes, occupancy
#   gemm  MFMA busy, LDS bank conflicts, L2 / L1 passes of the GEMM kernels (k_gemm)
# e.g. tools/gpu_pmc.sh fb237_block k_block_rows; tools/gpu_pmc.sh train_step k_dec_ent dec; tools/gpu_pmc.sh gemm k_gemm gemm
# Summaries go to $OUT/pmc_<workload>_<set>/summary.txt (OUT default run_logs/).  The script stops at the first pass that
# fails or times out.
WL=${1:?usage: tools/gpu_pmc.sh WORKLOAD KERNEL_SUBSTRING [SET]}
KSUB=${2:?usage: tools/gpu_pmc.sh WORKLOAD KERNEL_SUBSTRING [SET]}
SET=${3:-rows}
cd "$(dirname "$0")/.." || exit 1
OUT=${OUT:-run_logs}/pmc_${WL}_${SET}
rm -rf "$OUT"; mkdir -p "$OUT"
export TMPDIR=${TMPDIR:-/tmp}
export RGCN_STREAMS=0 RGCN_BENCH_PREFETCH=0      # read by bench.py and tools/train_step_trace.py

case "$WL" in
  train_step) CMD="python tools/train_step_trace.py 6" ;;
  train_step_fb15k) CMD="python tools/train_step_trace.py 6 fb15k" ;;
  gemm) CMD="python tools/gemm_pmc.py" ;;
  *) CMD="python bench.py --workload $WL --steps 6 --warmup 2" ;;
esac

SQ_CYCLES="SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_INST_ANY SQ_WAIT_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VMEM SQ_INST_CYCLES_VMEM GRBM_GUI_ACTIVE"
SQ_INSTS="SQ_INSTS_VALU SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_INSTS_SALU SQ_INSTS_SMEM SQ_INST_LEVEL_VMEM SQ_LEVEL_WAVES SQ_WAVES"
SQ_LDS="SQ_INSTS_LDS SQ_ACTIVE_INST_LDS SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_WAIT_INST_LDS SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_SCA SQ_INST_LEVEL_LDS"
TCP="TCP_PENDING_STALL_CYCLES_sum TCP_TCC_READ_REQ_sum TCP_TCC_WRITE_REQ_sum TCP_TCC_READ_REQ_LATENCY_sum"
TCC="TCC_HIT_sum TCC_MISS_sum TCC_REQ_sum TCC_EA0_WRREQ_sum"
BYTES="FETCH_SIZE WRITE_SIZE TCP_TOTAL_CACHE_ACCESSES_sum TCP_TCC_READ_REQ_sum"
case "$SET" in
  rows) PASSES=("$SQ_CYCLES" "$SQ_INSTS" "$SQ_LDS" "$TCP" "$TCC" "$BYTES") ;;
  msg) PASSES=("$SQ_CYCLES" "$SQ_INSTS" "$TCP" "$TCC") ;;
  dec) PASSES=("SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VMEM SQ_INST_CYCLES_VMEM GRBM_GUI_ACTIVE SQ_WAVES"
               "SQ_INSTS_VALU SQ_INSTS_VMEM_RD SQ_INSTS_LDS SQ_INST_LEVEL_VMEM SQ_LEVEL_WAVES SQ_ACTIVE_INST_LDS SQ_LDS_BANK_CONFLICT SQ_WAIT_INST_LDS"
               "TCP_PENDING_STALL_CYCLES_sum TCP_TCC_READ_REQ_sum TCP_TCC_READ_REQ_LATENCY_sum TCP_TOTAL_CACHE_ACCESSES_sum"
               "TCC_HIT_sum TCC_MISS_sum TCC_REQ_sum"
               "FETCH_SIZE") ;;
  gemm) PASSES=("SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_VALU_MFMA_BUSY_CYCLES SQ_WAIT_INST_ANY SQ_WAIT_ANY SQ_ACTIVE_INST_ANY SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE"
                "SQ_INSTS_VALU SQ_INSTS_MFMA SQ_INSTS_LDS SQ_INSTS_SALU SQ_WAIT_INST_LDS SQ_INST_CYCLES_VMEM GRBM_GUI_ACTIVE SQ_WAVES"
                "SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_ACTIVE_INST_VMEM SQ_ACTIVE_INST_MISC SQ_ACTIVE_INST_SCA SQ_INST_LEVEL_LDS SQ_INST_LEVEL_VMEM SQ_LEVEL_WAVES"
                "TCC_HIT_sum TCC_MISS_sum TCC_REQ_sum"
                "TCP_TCC_READ_REQ_sum TCP_PENDING_STALL_CYCLES_sum TCP_TCC_READ_REQ_LATENCY_sum") ;;
  *) echo "unknown counter set: $SET (rows, msg, dec, gemm)"; exit 2 ;;
esac

timeout -k 10 900 python -c "import __graft_entry__ as g; g.build()" > "$OUT/build.log" 2>&1 || { tail -n 20 "$OUT/build.log"; exit 1; }
n=0
for counters in "${PASSES[@]}"; do
  n=$((n + 1))
  # shellcheck disable=SC2086  # (the counter list and the command are word lists)
  timeout -k 10 300 rocprofv3 --pmc $counters -d "$OUT/p$n" -o "p$n" -- $CMD > "$OUT/p$n.log" 2>&1
  rc=$?
  if [ $rc -ne 0 ]; then echo "pass p$n ($counters): exit $rc"; tail -n 20 "$OUT/p$n.log"; exit $rc; fi
  python tools/pmc_summary.py "$OUT/p$n/p${n}_results.db" "$KSUB" | tee -a "$OUT/summary.txt"
  rm -rf "$OUT/p$n"      # the per-dispatch database: the summary is what is kept
done
