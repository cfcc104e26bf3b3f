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
  for (const DevPool* p : {&c->pool, &c->g.pool, &c->g_alt.pool, &c->dec.pool, &c->nbr.pool, &c->known.pool, &c->types.pool, &c->opt.pool,
                           &c->opt.part_pool, &c->ranking.pool}) {
    *blocks += p->blocks();
    *bytes += p->bytes();
  }
  return RGCN_OK;
}

// the split of rgcn_debug_gemm / rgcn_debug_gemm_time: the caller's own count must fit the context's slab (an explicit
// split is never lowered); only the automatic choice falls back to no split
static rgcn_status debug_split(rgcn_ctx* c, int32_t split_k, int32_t M, int32_t N, int32_t K, int* sk) {
  if (split_k > 1) {
    GemmCall q;      // (the slices that exist: gemm_plan's arithmetic on K alone)
    q.M = M; q.N = N; q.K = K; q.split_k = split_k;
    const int splits = gemm_plan(q, c->gemm_mode, 1).splits;
    const size_t need = (size_t)splits * M * N;
    if (splits > 1 && need > c->slab_floats)
      RGCN_FAIL(c, RGCN_ERR_INVALID, "split_k " + std::to_string(split_k) + " needs " + std::to_string(need) +
                                         " slab floats, the context has " + std::to_string(c->slab_floats));
  }
  *sk = split_k > 0 ? split_k : auto_split_k(M, N, K);
  if (split_k <= 0 && (size_t)*sk * M * N > c->slab_floats) *sk = 1;
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
  int sk = 1;
  RGCN_TRY(debug_split(c, split_k, M, N, K, &sk));
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
  int sk = 1;
  RGCN_TRY(debug_split(c, split_k, M, N, K, &sk));
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

rgcn_status rgcn_debug_gemm_call(rgcn_ctx* c, const rgcn_debug_gemm_desc* d, const float* a_host, const float* b_host,
                                 float* c_host, rgcn_debug_gemm_plan* out) {
  RGCN_NEED(c);
  if (!d || !a_host || !b_host || !c_host || !out) RGCN_FAIL(c, RGCN_ERR_INVALID, "bad arguments");
  *out = rgcn_debug_gemm_plan{};
  const int M = d->M, N = d->N, K = d->K, groups = d->groups;
  // everything the kernels index with is checked against the buffers here: a descriptor that would reach past them never launches
  if (M <= 0 || N <= 0 || K <= 0 || groups < 1 || groups > 64 || d->strideA < 0 || d->strideB < 0 || d->strideC < 0)
    RGCN_FAIL(c, RGCN_ERR_INVALID, "bad shape, group count or stride");
  for (int32_t off : {d->a_offset, d->b_offset, d->c_offset})
    if (off < 0 || off > 3) RGCN_FAIL(c, RGCN_ERR_INVALID, "a base offset is 0 .. 3 floats");
  const bool a_kc = d->a_kc != 0, b_kc = d->b_kc != 0;
  const int rowsA = a_kc ? M : K, colsA = a_kc ? K : M, rowsB = b_kc ? N : K, colsB = b_kc ? K : N;
  if (d->lda < colsA || d->ldb < colsB || d->ldc < N) RGCN_FAIL(c, RGCN_ERR_INVALID, "a leading dimension is below the extent");
  const size_t needA = (size_t)(groups - 1) * d->strideA + (size_t)rowsA * d->lda;
  const size_t needB = (size_t)(groups - 1) * d->strideB + (size_t)rowsB * d->ldb;
  const size_t needC = (size_t)(groups - 1) * d->strideC + (size_t)M * d->ldc;
  if (d->a_floats < 0 || d->b_floats < 0 || d->c_floats < 0 || (size_t)d->a_floats < needA || (size_t)d->b_floats < needB ||
      (size_t)d->c_floats < needC)
    RGCN_FAIL(c, RGCN_ERR_INVALID, "a host buffer is smaller than the strided extent of its operand");
  if (groups > 1 && (size_t)d->strideC < (size_t)M * d->ldc) RGCN_FAIL(c, RGCN_ERR_INVALID, "the groups' products overlap");
  if (d->limit != nullptr) {
    if (d->limit_stride < 1) RGCN_FAIL(c, RGCN_ERR_INVALID, "limit_stride < 1");
    for (int g = 0; g < groups; ++g) {
      const int32_t n = d->limit[(size_t)g * d->limit_stride];
      if (n < 0 || n > (d->limit_on_k ? K : M)) RGCN_FAIL(c, RGCN_ERR_INVALID, "a group's extent is outside 0 .. M resp. K");
    }
  }
  DevPool pool;
  float *A = nullptr, *B = nullptr, *C = nullptr;
  int32_t* lim = nullptr;
  char* F = nullptr;
  RGCN_TRY(dmalloc(c, pool, &A, (size_t)d->a_floats + 4, true));
  RGCN_TRY(dmalloc(c, pool, &B, (size_t)d->b_floats + 4, true));
  RGCN_TRY(dmalloc(c, pool, &C, (size_t)d->c_floats + 4, true));
  A += d->a_offset; B += d->b_offset; C += d->c_offset;
  RGCN_TRY(to_dev(c, A, a_host, sizeof(float) * (size_t)d->a_floats));
  RGCN_TRY(to_dev(c, B, b_host, sizeof(float) * (size_t)d->b_floats));
  RGCN_TRY(to_dev(c, C, c_host, sizeof(float) * (size_t)d->c_floats));
  GemmCall q{a_kc, b_kc, M, N, K, A, d->lda, B, d->ldb, C, d->ldc, d->split_k, c->slab, GemmBatch()};
  q.batch.groups = groups;
  q.batch.strideA = (size_t)d->strideA; q.batch.strideB = (size_t)d->strideB; q.batch.strideC = (size_t)d->strideC;
  q.batch.wide = d->wide;
  if (d->limit != nullptr) {
    const size_t n = (size_t)(groups - 1) * d->limit_stride + 1;
    RGCN_TRY(dmalloc(c, pool, &lim, n, true));
    RGCN_TRY(to_dev(c, lim, d->limit, sizeof(int32_t) * n));
    q.batch.limit = lim;
    q.batch.limit_stride = d->limit_stride;
    q.batch.limit_on_k = d->limit_on_k ? 1 : 0;
  }
  if (d->presplit_b) {
    const size_t words = gemm_bfrag_words(K, N);
    RGCN_TRY(dmalloc(c, pool, &F, 16 * words * groups, false));
    std::vector<PresplitJob> jobs;
    for (int g = 0; g < groups; ++g)
      jobs.push_back(PresplitJob{B + (size_t)g * d->strideB, F + 16 * words * g, d->ldb, K, N, b_kc ? 1 : 0});
    RGCN_TRY(gemm_presplit_b(c, jobs.data(), groups));
    q.batch.bfrag = F;
    q.batch.strideBfrag = words;
  }
  const GemmPlan p = gemm_plan(q, c->gemm_mode, d->w8_knob);
  out->kernel = (int32_t)p.kernel; out->terms = p.terms; out->vec = p.vec; out->vecC = p.vecC; out->table = p.table;
  out->prologue = p.prologue; out->swizzle = p.swizzle; out->splits = p.splits; out->k_per_split = p.k_per_split;
  out->slabs = p.slabs; out->ldc = p.ldc; out->tiles_m = p.tiles_m; out->tiles_n = p.tiles_n; out->grid_x = p.grid_x;
  out->grid_y = groups;
  if (!p.refused && p.slabs && (size_t)groups * p.splits * M * N > c->slab_floats)
    RGCN_FAIL(c, RGCN_ERR_INVALID, "the split needs " + std::to_string((size_t)groups * p.splits * M * N) +
                                       " slab floats (groups x splits x M x N), the context has " + std::to_string(c->slab_floats));
  if (!p.refused && p.vec && d->limit != nullptr && d->limit_on_k && (a_kc || b_kc))
    for (int g = 0; g < groups; ++g)
      if (d->limit[(size_t)g * d->limit_stride] % 4 != 0)
        RGCN_FAIL(c, RGCN_ERR_INVALID, "an extent on K that is no multiple of 4 with 16-byte loads of a k-contiguous operand");
  RGCN_TRY(gemm_run(c, "debug_gemm", q, p));
  return to_host(c, c_host, C, sizeof(float) * (size_t)d->c_floats);
}

#endif  // RGCN_DEVTOOLS

}  // extern "C"
