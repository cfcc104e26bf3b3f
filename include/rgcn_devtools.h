/*
 * rgcn_devtools.h -- entry points that exist ONLY in librgcn_devtools.so, the -DRGCN_DEVTOOLS build of the same
 * sources that tools/ and the dense-contraction tests load.  The product library (librgcn.so, include/rgcn.h) does
 * not export them and carries no experiment hooks.
 */
#ifndef RGCN_DEVTOOLS_H_
#define RGCN_DEVTOOLS_H_

#include "rgcn.h"

#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden: these declarations are its whole dynamic symbol table */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

/* ---- the dense contractions on their own (GPU parity tests of the GEMM kernels, tools/gemm_*.py) ---- */
/* C[M,N] = op(A) . op(B) through the library's fp32-MFMA GEMM.  trans_a == 0: A is [M,K] row-major,
 * else A is [K,M] row-major (used transposed); trans_b == 0: B is [K,N], else [N,K].
 * split_k == 0 picks the split the encoder would use (and falls back to none when its slabs do not fit the context's
 * slab); > 1 forces that many K slabs (as many as K has k-tiles for), and is RGCN_ERR_INVALID when slabs * M * N floats
 * do not fit: an explicit split is never lowered. */
rgcn_status rgcn_debug_gemm(rgcn_ctx* ctx, int32_t trans_a, int32_t trans_b, int32_t M, int32_t N,
                            int32_t K, int32_t split_k, const float* a_host, const float* b_host,
                            float* c_host);

/* Same contraction on device copies of the operands, `iters` back-to-back launches timed with HIP
 * events on the context's stream; *avg_ms = mean time of one product (incl. the split-K reduce). */
rgcn_status rgcn_debug_gemm_time(rgcn_ctx* ctx, int32_t trans_a, int32_t trans_b, int32_t M, int32_t N,
                                 int32_t K, int32_t split_k, int32_t iters, const float* a_host,
                                 const float* b_host, float* avg_ms);

/* C[M,N] = A . op(B) with B handed to the kernel PRE-SPLIT into bf16 planes in MFMA fragment order -- the way the encoder
 * passes its weights (W_self, the basis tensors) since round 5, csrc/gemm_bf16x3.hip B_PRE.  A is [M,K]; trans_b == 0: B
 * is [K,N], else [N,K].  Bitwise the result of rgcn_debug_gemm on the same operands (split arithmetic, modes 6 / 9;
 * mode 0 ignores the table).  iters > 0: also the mean time of one product over that many launches. */
rgcn_status rgcn_debug_gemm_presplit(rgcn_ctx* ctx, int32_t trans_b, int32_t M, int32_t N, int32_t K, int32_t iters,
                                     const float* a_host, const float* b_host, float* c_host, float* avg_ms);

/* One product C[M,N] = relu(A + bias) . B through the A-operand prologue of the pre-split-weight NN kernels (GemmBatch::
 * a_bias / a_out; csrc/gemm_bf16x3_w8.hip, csrc/gemm_bf16x3.hip APRO; modes 6 / 9), or -- prologue == 0 -- the plain product
 * A . B on the same kernel.  A is [M,K] with leading dimension lda >= K, B is [K,N], bias is [K].  a_out_host ([M,lda], in
 * and out) is copied to the device before the launch and back after it: what the kernel leaves untouched keeps the caller's
 * values.  wide != 0: the 128 x 256 / eight-wavefront kernel, else the 128 x 128 one (whatever RGCN_GEMM_W8 says:
 * the choice goes straight into the call's plan).  row_limit >= 0: the row extent is read on the device (GemmBatch::limit, the round-robin XCD swizzle) and
 * rows >= row_limit do not exist; < 0: no limit (the contiguous XCD swizzle). */
rgcn_status rgcn_debug_gemm_prologue(rgcn_ctx* ctx, int32_t wide, int32_t prologue, int32_t M, int32_t N, int32_t K,
                                     int32_t lda, int32_t row_limit, const float* a_host, const float* bias_host,
                                     const float* b_host, float* a_out_host, float* c_host);

/* Any call the dense contractions take (csrc/gemm_plan.h GemmCall / GemmBatch), one launch, and the plan it obeyed.
 * tests/test_gpu_gemm_launch_grid.py runs every launch form through it and asserts which cell of the plan it reached. */
typedef struct rgcn_debug_gemm_desc {
  int32_t a_kc, b_kc;                 /* A stored [m][k] (else [k][m]); B stored [n][k] (else [k][n]) */
  int32_t M, N, K;
  int32_t lda, ldb, ldc;              /* >= the contiguous extent of the operand */
  int32_t split_k;                    /* as GemmCall::split_k: <= 1 no split, > 1 that many slices of K (never lowered) */
  int32_t groups;                     /* >= 1 */
  int64_t strideA, strideB, strideC;  /* floats between consecutive groups' operands */
  const int32_t* limit;               /* host, (groups - 1) * limit_stride + 1 entries, or NULL: extent of group g at
                                       * limit[g * limit_stride], 0 .. M (rows) resp. 0 .. K (limit_on_k) */
  int32_t limit_stride, limit_on_k;
  int32_t presplit_b;                 /* != 0: B also comes pre-split, one fragment table per group (GemmBatch::bfrag) */
  int32_t wide, w8_knob;              /* GemmBatch::wide and gemm_plan's knob argument, as given */
  int32_t a_offset, b_offset, c_offset;   /* 0 .. 3 floats added to the 16-byte-aligned device base of A, B, C */
  int64_t a_floats, b_floats, c_floats;   /* sizes of the host buffers: at least (groups - 1) * stride + rows * ld */
} rgcn_debug_gemm_desc;

typedef struct rgcn_debug_gemm_plan {
  int32_t kernel;                     /* GemmKernel: 0 none, 1 f32, 2 staged, 3 presplit, 4 w8 */
  int32_t terms, vec, vecC, table, prologue, swizzle;
  int32_t splits, k_per_split, slabs, ldc;
  int32_t tiles_m, tiles_n, grid_x, grid_y;
} rgcn_debug_gemm_plan;

/* a_host, b_host: the whole strided extent of the operands.  c_host (in and out) is copied to the device before the
 * launch and back after it: what the launch leaves untouched keeps the caller's values.  *plan: what gemm_plan answered
 * (filled before anything is launched, also when the call fails).  A split whose slabs (groups * splits * M * N floats) do
 * not fit the context's slab is RGCN_ERR_INVALID, the message naming both numbers; an extent on K that is no multiple of
 * 4 together with 16-byte loads of a k-contiguous operand likewise; what gemm_plan refuses is RGCN_ERR_UNSUPPORTED. */
rgcn_status rgcn_debug_gemm_call(rgcn_ctx* ctx, const rgcn_debug_gemm_desc* desc, const float* a_host,
                                 const float* b_host, float* c_host, rgcn_debug_gemm_plan* plan);

/* ---- placement self-check ---- */
/* out_host[b] = the XCD (HW_REG_XCC_ID) workgroup b of a plain 1-D launch of n_blocks workgroups ran on.  The
 * destination-major block layer (csrc/block_rows.hip) and the decoder's line kernel give column band x to the workgroups
 * with blockIdx % 8 == x and count on them sharing one L2: a performance assumption HIP does not promise
 * (MI355X_MICROARCH.md: "observed, for speed only: block b runs on XCD b % 8").  tests/test_gpu_parity.py::
 * test_workgroups_of_a_band_share_an_xcd re-checks it on the box the suite runs on. */
rgcn_status rgcn_debug_xcd_map(rgcn_ctx* ctx, int32_t n_blocks, int32_t* out_host);

/* ---- device-memory ownership ---- */
/* The device allocations the context owns right now, summed over all its owners (the context itself, both graph sets, the
 * decoder batch, the sampler, the optimizer, the ranking scratch): live blocks and their bytes as allocated.  Caller-owned
 * memory (rgcn_device_alloc) and the pinned host buffers are not counted.  tests/test_gpu_memory_ownership.py. */
rgcn_status rgcn_debug_device_memory(rgcn_ctx* ctx, int64_t* blocks, int64_t* bytes);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* RGCN_DEVTOOLS_H_ */
