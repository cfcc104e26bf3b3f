// Which kernel takes a dense contraction, and with which launch parameters: decided HERE, once per call, by a pure host
// function of the call's shapes, strides and pointer alignment.  gemm_f32() obeys the plan (gemm_run, gemm_f32.hip), the
// schedule asks it whether layer 1's self-loop product can form H0 (rgcn_schedule.hip), tests/test_gemm_plan.py pins its
// table without a GPU.  Host only: nothing from HIP, no context, no environment.
#ifndef RGCN_GEMM_PLAN_H_
#define RGCN_GEMM_PLAN_H_

#include <cstddef>
#include <cstdint>

namespace rgcn {

// Several contractions of one shape in ONE launch (blockIdx.y = group), each with its own operands and -- read on the
// device, so that nothing about the graph has to come back to the host -- its own extent along M (rows of A and C that
// exist; workgroups of tiles beyond it leave at once and write nothing) or along K (the depth of the contraction; the
// split-K slices divide the ACTUAL depth evenly).  The row-compacted basis contraction (basis.hip) is two groups, one
// per message direction, whose row counts the graph preparation leaves in GraphBufs::unit_ptr.
struct GemmBatch {
  int groups = 1;
  size_t strideA = 0, strideB = 0, strideC = 0;   // floats between consecutive groups' operands
  const int32_t* limit = nullptr;                 // device, limit[g * limit_stride]: extent of group g (<= M resp. K)
  int limit_stride = 1;
  int limit_on_k = 0;                             // 0: rows of A / C (never with split_k > 1: gemm_plan refuses); 1: depth K
  // (an extent on K that is no multiple of 4 needs operands that are NOT k-contiguous, or dword loads: the plan cannot see
  // the extent, and a 16-byte load of a k-contiguous operand takes its four k all or nothing.  The one call site,
  // units_product_dw, is the TN form.)
  // optional: B already split into bf16 planes in MFMA fragment order (gemm_presplit_b; a weight, split once per weight
  // update instead of once per tile and step).  Used by the split-arithmetic kernel when A is k-contiguous and there is no
  // split over K; ignored otherwise (B itself must still be passed).  strideBfrag: 16-byte words between groups.
  const void* bfrag = nullptr;
  size_t strideBfrag = 0;
  // with bfrag: ask for the 128 x 256 / eight-wavefront kernel (gemm_bf16x3_w8.hip; one workgroup holds a whole CU) instead
  // of the 128 x 128 / four-wavefront one (two per CU, room for another kernel's workgroups beside them).  Same result bit
  // for bit; which is faster in the step depends on what runs beside the product: the forward
  // products run alone on the main stream (wide), the backward ones beside dW_self and the relation-weight kernels (not
  // wide).  gemm_plan() below decides what becomes of the request.
  int wide = 0;
  // optional A-operand prologue with write-back (the pre-split-weight NN kernels only: GemmPlan::prologue): every A element
  // enters the product as fmaxf(a + a_bias[k], 0.f), and -- a_out != nullptr -- the transformed operand is also written to
  // a_out, which has A's leading dimension and group stride.  Layer 1's self-loop product forms H0 = relu(W_emb + b_emb)
  // this way, in k_input_fwd's arithmetic, from the operand it has in registers anyway.
  const float* a_bias = nullptr;    // [K]
  float* a_out = nullptr;
};

// One call: C[M,N] (ldc) = A(m,k) . B(k,n).  a_kc: A stored [m][k] (k contiguous, lda) else [k][m]; b_kc: B stored [n][k]
// (k contiguous, ldb) else [k][n].  split_k > 1 writes partial slabs to `slab` ([group][split_k][M][N]) and reduces them
// into C deterministically.
struct GemmCall {
  bool a_kc = true, b_kc = false;
  int M = 0, N = 0, K = 0;
  const float* A = nullptr;
  int lda = 0;
  const float* B = nullptr;
  int ldb = 0;
  float* C = nullptr;
  int ldc = 0;
  int split_k = 1;
  float* slab = nullptr;      // the context's split-K slabs: their alignment decides vecC where slabs are used
  GemmBatch batch;
  size_t slab_floats = 0;     // capacity of `slab` in floats where it is the caller's own; 0: the context's slabs
};

enum GemmKernel {
  GEMM_NONE = 0,          // nothing is launched: an empty product, or a refused call (GemmPlan::refused)
  GEMM_F32 = 1,           // k_gemm_f32: the fp32 MFMA (gemm mode 0)
  GEMM_STAGED = 2,        // k_gemm_bf16x3<a_kc, b_kc, vec, terms>: both operands staged and split per tile
  GEMM_PRESPLIT = 3,      // k_gemm_bf16x3<.., B_PRE>: 128 x 128 tiles, B from its fragment table
  GEMM_W8 = 4             // k_gemm_w8: 128 x 256 tiles, eight wavefronts, B from its fragment table
};

struct GemmPlan {
  GemmKernel kernel = GEMM_NONE;
  const char* refused = nullptr;      // why no kernel takes the call (RGCN_ERR_UNSUPPORTED); nullptr: not refused
  bool a_kc = true, b_kc = false;     // the call's storage forms (the staged kernels' template arguments)
  int terms = 0;                      // partial products of the split arithmetic: 3, 6 or 9 (0: fp32 MFMA)
  bool vec = false;                   // 16-byte operand loads
  bool table = false;                 // B comes from GemmBatch::bfrag
  bool prologue = false;              // the A-operand prologue runs (GemmBatch::a_bias / a_out)
  int swizzle = 1;                    // workgroup remap: 1 a contiguous range of tiles per XCD, 2 row panels round-robin
  int splits = 1, k_per_split = 0;    // slices of K (k_per_split: a multiple of the k-tile)
  bool slabs = false;                 // the kernel writes split-K slabs (GemmCall::slab, ldc = N), a reduce follows
  int ldc = 0;                        // leading dimension of what the kernel writes
  int vecC = 0;                       // 16-byte stores of the product
  int tiles_m = 0, tiles_n = 0, grid_x = 0;      // of the chosen kernel's tile
};

constexpr int kGemmBK = 16, kGemmBM = 128, kGemmBN = 128, kGemmWideBN = 256;
constexpr int kGemmPrologueMaxKT = 127;      // k-tiles of the prologue kernels' LDS copy of the bias vector

// 16-byte loads legal and float4 validity all-or-nothing: aligned base, ld % 4 == 0, and the contiguous extent (K for a
// k-contiguous operand, the row count for a row-contiguous one) % 4 == 0.
inline bool gemm_vec_ok(const float* p, int ld, int contiguous_extent) {
  return (reinterpret_cast<uintptr_t>(p) & 15u) == 0 && (ld % 4) == 0 && (contiguous_extent % 4) == 0 &&
         contiguous_extent >= 4;
}

// gemm_mode: rgcn_ctx::gemm_mode (0, 3, 6, 9).  w8_knob (devtools knob RGCN_GEMM_W8; the product library passes 1): which
// table products go to the eight-wavefront kernel -- 0 none, 1 those the call site marks wide, 2 / 3 all it can take.
inline GemmPlan gemm_plan(const GemmCall& q, int gemm_mode, int w8_knob) {
  GemmPlan p;
  const GemmBatch& b = q.batch;
  auto refuse = [&p](const char* why) { p.kernel = GEMM_NONE; p.refused = why; return p; };
  if (q.M <= 0 || q.N <= 0) return p;
  if (!q.a_kc && q.b_kc) return refuse("gemm TT form not instantiated");
  const char* const no_prologue = "gemm: the A-operand prologue exists in the pre-split-weight NN kernels only";
  const bool nn = q.a_kc && !q.b_kc;
  if (b.a_bias != nullptr && (gemm_mode == 0 || !nn || q.split_k > 1)) return refuse(no_prologue);
  // (tiles beyond a row extent leave without writing their slab, and the reduce sums whole slabs: rows beyond the extent
  // would receive what an earlier call left there)
  if (b.limit != nullptr && !b.limit_on_k && q.split_k > 1)
    return refuse("gemm: a row limit cannot be combined with a split over K");
  p.a_kc = q.a_kc; p.b_kc = q.b_kc;
  p.terms = gemm_mode == 0 ? 0 : gemm_mode == 9 ? 9 : gemm_mode == 3 ? 3 : 6;
  // (the NN product with a pre-split weight fetches B from its fragment table and never loads B itself: B's own alignment
  // and width do not matter there -- a weight of any width reaches the pre-split kernels, with or without the prologue)
  const bool b_unread = b.bfrag != nullptr && nn && gemm_mode != 0 && q.split_k <= 1;
  p.vec = gemm_vec_ok(q.A, q.lda, q.a_kc ? q.K : q.M) && (b_unread || gemm_vec_ok(q.B, q.ldb, q.b_kc ? q.K : q.N)) &&
          b.strideA % 4 == 0 && (b_unread || b.strideB % 4 == 0);
  p.swizzle = (b.limit != nullptr && !b.limit_on_k && q.split_k <= 1) ? 2 : 1;
  const int want = q.split_k < 1 ? 1 : q.split_k;
  int kps = (q.K + want - 1) / want;
  kps = ((kps + kGemmBK - 1) / kGemmBK) * kGemmBK;
  if (kps < kGemmBK) kps = kGemmBK;
  p.k_per_split = kps;
  p.splits = q.K > 0 ? (q.K + kps - 1) / kps : 1;
  p.slabs = p.splits > 1;
  p.ldc = p.slabs ? q.N : q.ldc;
  // (every group's product starts 16-byte aligned: slabs lie splits * M * N floats apart, a multiple of 4 with N)
  p.vecC = ((reinterpret_cast<uintptr_t>(p.slabs ? q.slab : q.C) & 15u) == 0 && p.ldc % 4 == 0 && q.N % 4 == 0 &&
            (p.slabs || b.groups <= 1 || b.strideC % 4 == 0)) ? 1 : 0;
  p.kernel = GEMM_F32;
  int bn = kGemmBN;
  if (gemm_mode != 0) {
    p.table = b.bfrag != nullptr && p.splits == 1 && q.a_kc && p.vec;
    const bool six_or_nine = p.terms != 3;
    if (b.a_bias != nullptr && !(p.table && !q.b_kc && !b.limit_on_k && six_or_nine &&
                                 (q.K + kGemmBK - 1) / kGemmBK <= kGemmPrologueMaxKT))
      return refuse(no_prologue);
    p.prologue = b.a_bias != nullptr;
    bool wide = b.wide != 0;
    if (wide && b.limit == nullptr) {
      // one workgroup per CU and nothing to hide a tile's fill and its stores behind: the wide kernel wins when the launch is ONE
      // round of tiles that fills most of the chip (FB15k-237: 228 tiles, 45.8 against 48.8 us), and loses to the two-per-CU
      // kernel over several rounds (WN18, 640 tiles: 125 against 114 us) -- profiles/r06_gemm_w8.md
      const long t = (long)((q.M + kGemmBM - 1) / kGemmBM) * ((q.N + kGemmWideBN - 1) / kGemmWideBN) * b.groups;
      wide = t <= 256 && t >= 160;
    }
    // (the eight-wavefront kernel reads batch.limit as a row limit only)
    const bool w8 = p.table && !b.limit_on_k && six_or_nine && (w8_knob >= 2 || (w8_knob == 1 && wide));
    p.kernel = w8 ? GEMM_W8 : p.table ? GEMM_PRESPLIT : GEMM_STAGED;
    if (w8) bn = kGemmWideBN;
  }
  p.tiles_m = (q.M + kGemmBM - 1) / kGemmBM;
  p.tiles_n = (q.N + bn - 1) / bn;
  p.grid_x = p.swizzle == 2 ? ((p.tiles_m + 7) / 8) * 8 * p.tiles_n : p.tiles_m * p.tiles_n * p.splits;
  return p;
}

}  // namespace rgcn
#endif  // RGCN_GEMM_PLAN_H_
