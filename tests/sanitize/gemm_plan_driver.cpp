// Driver of the GEMM decision table (csrc/gemm_plan.h: pure host C++, nothing from HIP) for tests/test_gemm_plan.py, built
// with AddressSanitizer / UndefinedBehaviorSanitizer like sampler_driver.cpp.  One line per case: what gemm_plan() answers
// for a call; the test holds the expected lines as literals.  No pointer is ever dereferenced: only alignment matters.
#include <cstdint>
#include <cstdio>

#include "../../relationprediction_amd/csrc/gemm_plan.h"

using namespace rgcn;

alignas(16) static float bufA[8], bufB[8], bufC[8], bufS[8], bufBias[8];
alignas(16) static char bufF[16];
static int32_t lim[2];

static void show(const char* name, const GemmCall& q, int mode = 6, int knob = 1) {
  const GemmPlan p = gemm_plan(q, mode, knob);
  static const char* const kname[] = {"none", "f32", "staged", "presplit", "w8"};
  if (p.refused) { std::printf("%s: refused: %s\n", name, p.refused); return; }
  if (p.kernel == GEMM_NONE) { std::printf("%s: none\n", name); return; }
  std::printf("%s: %s<%d,%d> terms=%d vec=%d table=%d pro=%d swz=%d splits=%d kps=%d slabs=%d ldc=%d vecC=%d tiles=%dx%d grid=%d\n",
              name, kname[p.kernel], (int)p.a_kc, (int)p.b_kc, p.terms, (int)p.vec, (int)p.table, (int)p.prologue, p.swizzle,
              p.splits, p.k_per_split, (int)p.slabs, p.ldc, p.vecC, p.tiles_m, p.tiles_n, p.grid_x);
}

// leading dimensions = the contiguous extent, 16-byte-aligned pointers, one group
static GemmCall call(bool a_kc, bool b_kc, int M, int N, int K, int split_k = 1) {
  GemmCall q;
  q.a_kc = a_kc; q.b_kc = b_kc; q.M = M; q.N = N; q.K = K;
  q.A = bufA; q.lda = a_kc ? K : M;
  q.B = bufB; q.ldb = b_kc ? K : N;
  q.C = bufC; q.ldc = N;
  q.split_k = split_k;
  q.slab = bufS;
  return q;
}
static GemmCall table(GemmCall q, int wide) {
  q.batch.bfrag = bufF;
  q.batch.wide = wide;
  return q;
}
static GemmCall bias(GemmCall q) {
  q.batch.a_bias = bufBias;
  q.batch.a_out = bufC;
  return q;
}

int main() {
  // the headline forward product and its neighbours
  show("fwd_14541", table(call(true, false, 14541, 500, 500), 1));
  show("fwd_14541_bias", bias(table(call(true, false, 14541, 500, 500), 1)));
  show("fwd_14951", table(call(true, false, 14951, 500, 500), 1));
  show("fwd_40943", table(call(true, false, 40943, 500, 500), 1));
  show("fwd_40943_bias", bias(table(call(true, false, 40943, 500, 500), 1)));
  // the wide heuristic's boundaries: N 256, M = 128 t
  const int wide_t[4] = {159, 160, 256, 257};
  for (int t : wide_t) {
    char name[32];
    std::snprintf(name, sizeof name, "wide_t%d", t);
    show(name, table(call(true, false, 128 * t, 256, 64), 1));
  }
  // NT (dH), TN (dW), TT
  show("nt", table(call(true, true, 14541, 500, 500), 0));
  show("nt_knob3", table(call(true, true, 14541, 500, 500), 0), 6, 3);
  show("nt_knob0", table(call(true, true, 14541, 500, 500), 0), 6, 0);
  show("nt_wide_knob0", table(call(true, true, 14541, 500, 500), 1), 6, 0);
  show("fwd_14541_knob0", table(call(true, false, 14541, 500, 500), 1), 6, 0);
  show("tn_split8", call(false, false, 500, 500, 14541, 8));
  show("tt", call(false, true, 500, 500, 500));
  // empty shapes
  show("empty_m0", call(true, false, 0, 500, 500));
  show("empty_n0", call(true, false, 500, 0, 500));
  show("empty_m_negative", bias(call(false, true, -1, 500, 500)));
  // the arithmetic modes
  show("mode0", table(call(true, false, 14541, 500, 500), 1), 0, 3);
  show("mode0_tn_split8", call(false, false, 500, 500, 14541, 8), 0);
  show("mode0_bias", bias(table(call(true, false, 14541, 500, 500), 1)), 0);
  show("mode9", table(call(true, false, 14541, 500, 500), 1), 9);
  show("mode9_bias", bias(table(call(true, false, 14541, 500, 500), 1)), 9);
  show("mode3_knob3", table(call(true, false, 14541, 500, 500), 1), 3, 3);
  show("mode3_bias", bias(table(call(true, false, 14541, 500, 500), 1)), 3, 3);
  // the prologue's bounds
  show("pro_k2032", bias(table(call(true, false, 256, 128, 2032), 0)));
  show("pro_k2036", bias(table(call(true, false, 256, 128, 2036), 0)));
  show("pro_nt", bias(table(call(true, true, 256, 128, 500), 0)));
  show("pro_split2", bias(table(call(true, false, 256, 128, 500, 2), 0)));
  {
    GemmCall q = bias(table(call(true, false, 256, 128, 500), 0));
    q.batch.limit = lim;
    q.batch.limit_on_k = 1;
    show("pro_limit_on_k", q);
  }
  show("pro_no_table", bias(call(true, false, 256, 128, 500)));
  // alignment
  {
    GemmCall q = table(call(true, false, 256, 128, 500), 0);
    q.A = bufA + 1;
    show("a_off4", q);
    show("a_off4_bias", bias(q));
    q = table(call(true, false, 256, 128, 500), 0);
    q.lda = 502;
    show("lda502", q);
    show("k502", table(call(true, false, 256, 128, 502), 0));
    q = table(call(true, false, 256, 5, 500), 0);
    q.B = bufB + 1;
    show("n5_b_off4", q);
    q = table(call(true, false, 256, 5, 16, 4), 0);
    q.B = bufB + 1;
    show("n5_b_off4_split4_k16", q);
  }
  // two groups whose row extent is read on the device
  {
    GemmCall q = table(call(true, false, 1100, 500, 500), 1);
    q.batch.groups = 2;
    q.batch.strideA = 1100 * 500; q.batch.strideB = 500 * 500; q.batch.strideC = 1100 * 500;
    q.batch.limit = lim;
    show("groups_row_limit", q);
    q.batch.strideA += 1;
    show("groups_row_limit_strideA_odd", q);
    q.batch.strideA -= 1;
    q.batch.strideC += 1;      // the second group's product is not 16-byte aligned
    show("groups_row_limit_strideC_odd", q);
  }
  // a row limit and a split over K: refused (the reduce sums whole slabs); an extent on K splits as before
  {
    GemmCall q = call(false, false, 500, 500, 14541, 8);
    q.batch.limit = lim;
    show("row_limit_split8", q);
    q.batch.limit_on_k = 1;
    show("limit_on_k_split8", q);
  }
  {
    GemmCall q = table(call(true, false, 256, 128, 500), 1);
    q.batch.limit = lim;
    q.batch.limit_on_k = 1;
    show("limit_on_k_knob3", q, 6, 3);
  }
  std::printf("gemm_plan_driver: ok\n");
  return 0;
}
