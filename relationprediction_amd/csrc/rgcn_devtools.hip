// Entry points that exist in librgcn_devtools.so only (include/rgcn_devtools.h): the dense contractions on their own, the
// XCD placement probe, the device-memory count.  The product library compiles this file to nothing.
#include "rgcn_api_internal.h"

using namespace rgcn;

extern "C" {

#ifdef RGCN_DEVTOOLS
namespace {
// the XCD every workgroup of a plain 1-D launch lands on (HW_REG_XCC_ID, bits 3:0)
__global__ void k_xcd_of_block(int32_t* out) {
  uint32_t id;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(id));
  if (threadIdx.x == 0) out[blockIdx.x] = (int32_t)(id & 0xf);
}
}  // namespace

rgcn_status rgcn_debug_xcd_map(rgcn_ctx* c, int32_t n_blocks, int32_t* out_host) {
  RGCN_NEED(c);
  if (n_blocks <= 0 || !out_host) RGCN_FAIL(c, RGCN_ERR_INVALID, "bad arguments");
  DevPool pool;      // the operands of the entry points below live for the call: a local pool frees them on every return
  int32_t* dev = nullptr;
  RGCN_TRY(dmalloc(c, pool, &dev, (size_t)n_blocks, true));
  hipLaunchKernelGGL(k_xcd_of_block, dim3((unsigned)n_blocks), dim3(256), 0, c->stream, dev);
  RGCN_HIP(c, hipGetLastError());
  return to_host(c, out_host, dev, sizeof(int32_t) * (size_t)n_blocks);
}

rgcn_status rgcn_debug_device_memory(rgcn_ctx* c, int64_t* blocks, int64_t* bytes) {
  RGCN_NEED(c);
  if (!blocks || !bytes) RGCN_FAIL(c, RGCN_ERR_INVALID, "bad arguments");
  *blocks = *bytes = 0;
  for (const DevPool* p : {&c->pool, &c->g.pool, &c->g_alt.pool, &c->dec.pool, &c->nbr.pool, &c->opt.pool,
                           &c->opt.part_pool, &c->ranking.pool}) {
    *blocks += p->blocks();
    *bytes += p->bytes();
  }
  return RGCN_OK;
}

rgcn_status rgcn_debug_gemm(rgcn_ctx* c, int32_t ta, int32_t tb, int32_t M, int32_t N, int32_t K,
                            int32_t split_k, const float* a_host, const float* b_host, float* c_host) {
  RGCN_NEED(c);
  if (M <= 0 || N <= 0 || K <= 0 || !a_host || !b_host || !c_host) RGCN_FAIL(c, RGCN_ERR_INVALID, "bad arguments");
  if (ta && tb) RGCN_FAIL(c, RGCN_ERR_UNSUPPORTED, "TT form not instantiated");
  DevPool pool;
  float *A = nullptr, *B = nullptr, *C = nullptr;
  RGCN_TRY(dmalloc(c, pool, &A, (size_t)M * K, false));
  RGCN_TRY(dmalloc(c, pool, &B, (size_t)K * N, false));
  RGCN_TRY(dmalloc(c, pool, &C, (size_t)M * N, true));
  RGCN_TRY(to_dev(c, A, a_host, sizeof(float) * (size_t)M * K));
  RGCN_TRY(to_dev(c, B, b_host, sizeof(float) * (size_t)K * N));
  int sk = split_k > 0 ? split_k : auto_split_k(M, N, K);
  if ((size_t)sk * M * N > c->slab_floats) sk = 1;
  // trans_a: A given as [K,M] (row-contiguous operand); trans_b: B given as [N,K] (k-contiguous)
  RGCN_TRY(gemm_f32(c, "debug_gemm", ta == 0, tb != 0, M, N, K, A, ta ? M : K, B, tb ? K : N, C, N, sk));
  return to_host(c, c_host, C, sizeof(float) * (size_t)M * N);
}

rgcn_status rgcn_debug_gemm_presplit(rgcn_ctx* c, int32_t tb, int32_t M, int32_t N, int32_t K, int32_t iters,
                                     const float* a_host, const float* b_host, float* c_host, float* avg_ms) {
  RGCN_NEED(c);
  if (M <= 0 || N <= 0 || K <= 0 || !a_host || !b_host || !c_host) RGCN_FAIL(c, RGCN_ERR_INVALID, "bad arguments");
  DevPool pool;
  float *A = nullptr, *B = nullptr, *C = nullptr;
  void* F = nullptr;
  RGCN_TRY(dmalloc(c, pool, &A, (size_t)M * K, false));
  RGCN_TRY(dmalloc(c, pool, &B, (size_t)K * N, false));
  RGCN_TRY(dmalloc(c, pool, &C, (size_t)M * N, true));
  RGCN_TRY(dmalloc(c, pool, &F, 16 * gemm_bfrag_words(K, N), false));
  RGCN_TRY(to_dev(c, A, a_host, sizeof(float) * (size_t)M * K));
  RGCN_TRY(to_dev(c, B, b_host, sizeof(float) * (size_t)K * N));
  const PresplitJob pj{B, F, tb ? K : N, K, N, tb ? 1 : 0};
  RGCN_TRY(gemm_presplit_b(c, &pj, 1));
  GemmBatch gb;
  gb.bfrag = F;
  gb.wide = 1;
  RGCN_TRY(gemm_f32(c, "debug_gemm", true, tb != 0, M, N, K, A, K, B, tb ? K : N, C, N, 1, &gb));
  RGCN_TRY(to_host(c, c_host, C, sizeof(float) * (size_t)M * N));
  if (iters > 0 && avg_ms) {
    RGCN_TRY(rgcn_timer_start(c));
    for (int it = 0; it < iters; ++it)
      RGCN_TRY(gemm_f32(c, "debug_gemm", true, tb != 0, M, N, K, A, K, B, tb ? K : N, C, N, 1, &gb));
    float ms = 0.f;
    RGCN_TRY(rgcn_timer_stop(c, &ms));
    *avg_ms = ms / iters;
  }
  return RGCN_OK;
}

rgcn_status rgcn_debug_gemm_prologue(rgcn_ctx* c, int32_t wide, int32_t prologue, int32_t M, int32_t N, int32_t K,
                                     int32_t lda, int32_t row_limit, const float* a_host, const float* bias_host,
                                     const float* b_host, float* a_out_host, float* c_host) {
  RGCN_NEED(c);
  if (M <= 0 || N <= 0 || K <= 0 || lda < K || row_limit > M || !a_host || !bias_host || !b_host || !a_out_host || !c_host)
    RGCN_FAIL(c, RGCN_ERR_INVALID, "bad arguments");
  DevPool pool;
  float *A = nullptr, *B = nullptr, *C = nullptr, *bias = nullptr, *Aout = nullptr;
  int32_t* lim = nullptr;
  void* F = nullptr;
  RGCN_TRY(dmalloc(c, pool, &A, (size_t)M * lda, false));
  RGCN_TRY(dmalloc(c, pool, &Aout, (size_t)M * lda, false));
  RGCN_TRY(dmalloc(c, pool, &B, (size_t)K * N, false));
  RGCN_TRY(dmalloc(c, pool, &bias, (size_t)K, false));
  RGCN_TRY(dmalloc(c, pool, &C, (size_t)M * N, true));
  RGCN_TRY(dmalloc(c, pool, &lim, 1, true));
  RGCN_TRY(dmalloc(c, pool, &F, 16 * gemm_bfrag_words(K, N), false));
  RGCN_TRY(to_dev(c, A, a_host, sizeof(float) * (size_t)M * lda));
  RGCN_TRY(to_dev(c, Aout, a_out_host, sizeof(float) * (size_t)M * lda));
  RGCN_TRY(to_dev(c, B, b_host, sizeof(float) * (size_t)K * N));
  RGCN_TRY(to_dev(c, bias, bias_host, sizeof(float) * (size_t)K));
  if (row_limit >= 0) RGCN_TRY(to_dev(c, lim, &row_limit, sizeof(int32_t)));
  const PresplitJob pj{B, F, N, K, N, 0};
  RGCN_TRY(gemm_presplit_b(c, &pj, 1));
  GemmCall q{true, false, M, N, K, A, lda, B, N, C, N, 1, c->slab, GemmBatch()};
  q.batch.bfrag = F;
  q.batch.wide = wide ? 1 : 0;
  if (row_limit >= 0) q.batch.limit = lim;
  if (prologue) {
    q.batch.a_bias = bias;
    q.batch.a_out = Aout;
  }
  // the kernel under test is chosen here, not by the tile-count heuristic (gemm_plan's knob: 3 = wide everywhere, 0 = never)
  const GemmPlan plan = gemm_plan(q, c->gemm_mode, wide ? 3 : 0);
  if (prologue && !plan.prologue) RGCN_FAIL(c, RGCN_ERR_UNSUPPORTED, "no prologue kernel takes this product");
  RGCN_TRY(gemm_run(c, "debug_gemm", q, plan));
  RGCN_TRY(to_host(c, c_host, C, sizeof(float) * (size_t)M * N));
  return to_host(c, a_out_host, Aout, sizeof(float) * (size_t)M * lda);
}

rgcn_status rgcn_debug_gemm_time(rgcn_ctx* c, int32_t ta, int32_t tb, int32_t M, int32_t N, int32_t K,
                                 int32_t split_k, int32_t iters, const float* a_host,
                                 const float* b_host, float* avg_ms) {
  RGCN_NEED(c);
  if (M <= 0 || N <= 0 || K <= 0 || iters <= 0 || !a_host || !b_host || !avg_ms)
    RGCN_FAIL(c, RGCN_ERR_INVALID, "bad arguments");
  if (ta && tb) RGCN_FAIL(c, RGCN_ERR_UNSUPPORTED, "TT form not instantiated");
  DevPool pool;
  float *A = nullptr, *B = nullptr, *C = nullptr;
  RGCN_TRY(dmalloc(c, pool, &A, (size_t)M * K, false));
  RGCN_TRY(dmalloc(c, pool, &B, (size_t)K * N, false));
  RGCN_TRY(dmalloc(c, pool, &C, (size_t)M * N, true));
  RGCN_TRY(to_dev(c, A, a_host, sizeof(float) * (size_t)M * K));
  RGCN_TRY(to_dev(c, B, b_host, sizeof(float) * (size_t)K * N));
  int sk = split_k > 0 ? split_k : auto_split_k(M, N, K);
  if ((size_t)sk * M * N > c->slab_floats) sk = 1;
  for (int it = 0; it < 3; ++it)
    RGCN_TRY(gemm_f32(c, "debug_gemm", ta == 0, tb != 0, M, N, K, A, ta ? M : K, B, tb ? K : N, C, N, sk));
  RGCN_TRY(rgcn_timer_start(c));
  for (int it = 0; it < iters; ++it)
    RGCN_TRY(gemm_f32(c, "debug_gemm", ta == 0, tb != 0, M, N, K, A, ta ? M : K, B, tb ? K : N, C, N, sk));
  float ms = 0.f;
  RGCN_TRY(rgcn_timer_stop(c, &ms));
  *avg_ms = ms / iters;
  return RGCN_OK;
}

#endif  // RGCN_DEVTOOLS

}  // extern "C"
