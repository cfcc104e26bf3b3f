// What the row kernels of the basis family share (basis.hip, basis_onehot.hip, basis_tdiag.hip, basis_pdiag.hip): the
// float4 / scalar column primitives, the launch geometry, the walk over the rows of an incidence CSR in its two forms, and
// the (VEC, TPR) dispatch.  decoder.hip, elementwise.hip and block_msgs.hip take the primitives and the dispatch only.
//
// The walk: workgroups [0, n_long_blocks) take one LONG row (more than kLongRow slots) of the long-row list at a time,
// 8 slot lanes x 128 column lanes, the eight partial sums added through LDS in lane order.  The others give TPR lanes to
// a row, kRowThreads / TPR rows per workgroup, and leave the long rows to the workgroups above.  No atomics: every sum
// has a fixed order.
#pragma once

#include "rgcn_internal.h"

namespace rgcn {

constexpr int BT = 8;   // basis functions per launch of a banked row kernel (register budget); B > 8 loops on the host
constexpr int kRowThreads = 1024;

template <int VEC>
__device__ __forceinline__ void vload(const float* p, float (&v)[VEC]) {
  if constexpr (VEC == 4) {
    float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
    v[0] = *p;
  }
}
template <int VEC>
__device__ __forceinline__ void vstore(float* p, const float (&v)[VEC]) {
  if constexpr (VEC == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  else *p = v[0];
}

// the segment of x in a CSR-style pointer list: the last i with ptr[i] <= x
__device__ __forceinline__ int find_segment(const int32_t* __restrict__ ptr, int n_seg, int x) {
  int lo = 0, hi = n_seg;
  while (hi - lo > 1) {
    int mid = (lo + hi) >> 1;
    if (ptr[mid] <= x) lo = mid; else hi = mid;
  }
  return lo;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
// leading workgroups of a row launch that walk the long-row list: 64 at minibatch scale, 512 at full-graph scale (the
// 272,115-edge training graph has 5,000+ long rows and a 2,397-slot hub)
inline int long_blocks(const rgcn_ctx* c) { return 2 * c->g.E > 65536 ? 512 : 64; }
// lanes per row of a row kernel: 64, 128 or 256 by the number of column vectors
inline int row_lanes(int nvec) { return nvec <= 64 ? 64 : (nvec <= 128 ? 128 : 256); }
// nlb long-row workgroups, then kRowThreads / tpr rows per workgroup
inline dim3 row_grid(int nlb, int V, int tpr) {
  const int rpb = kRowThreads / tpr;
  return dim3(nlb + (V + rpb - 1) / rpb);
}

// entry i of the eight slot lanes' partial sums, added in lane order
template <int VEC>
__device__ __forceinline__ float lds_sum8(const float (&red)[8][128 * VEC], int i) {
  float u = red[0][i];
#pragma unroll
  for (int w = 1; w < 8; ++w) u += red[w][i];
  return u;
}

// Single accumulator.  range(s0, s1, step, cidx, acc) adds the slots s0, s0 + step, ... < s1 of a row at column vector
// cidx; epilogue(v, cidx, acc) finishes and stores row v there.  OPTIONAL_ROWS: row_ptr may be nullptr (with
// n_long_blocks == 0), every row is then empty and only the epilogue runs.
template <int VEC, int TPR, bool OPTIONAL_ROWS = false, class Range, class Epilogue>
__device__ __forceinline__ void row_walk(const int32_t* row_ptr, const int32_t* long_rows, const int32_t* nlong, int V,
                                         int nvec, int n_long_blocks, Range range, Epilogue epilogue) {
  if ((int)blockIdx.x < n_long_blocks) {
    __shared__ float red[8][128 * VEC];
    const int cl = threadIdx.x & 127, sl = threadIdx.x >> 7;
    const int n = *nlong;
    for (int lb = blockIdx.x; lb < n; lb += n_long_blocks) {
      const int v = long_rows[lb];
      const int beg = row_ptr[v], end = row_ptr[v + 1];
      for (int c0 = 0; c0 < nvec; c0 += 128) {
        const int cidx = c0 + cl;
        float acc[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
        if (cidx < nvec) range(beg + sl, end, 8, cidx, acc);
#pragma unroll
        for (int k = 0; k < VEC; ++k) red[sl][cl * VEC + k] = acc[k];
        __syncthreads();
        if (sl == 0 && cidx < nvec) {
#pragma unroll
          for (int k = 0; k < VEC; ++k) acc[k] = lds_sum8<VEC>(red, cl * VEC + k);
          epilogue(v, cidx, acc);
        }
        __syncthreads();
      }
    }
    return;
  }
  const int v = ((int)blockIdx.x - n_long_blocks) * (kRowThreads / TPR) + threadIdx.x / TPR;
  if (v >= V) return;
  const int lane = threadIdx.x % TPR;
  int beg = 0, end = 0;
  if (!OPTIONAL_ROWS || row_ptr != nullptr) {
    beg = row_ptr[v];
    end = row_ptr[v + 1];
    if (end - beg > kLongRow) return;      // a long-row workgroup of this launch owns it
  }
  for (int cidx = lane; cidx < nvec; cidx += TPR) {
    float acc[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
    range(beg, end, 1, cidx, acc);
    epilogue(v, cidx, acc);
  }
}

// Banked: BT accumulators per direction, of which the first nbt are live.  range(s0, s1, step, cidx, accf, accb) adds
// the slots of a row into the forward- and backward-direction banks; row(v, beg, end, ctx) runs once per row, outside the
// column loop, fills what the stores of that row need (base pointers, unit indices) and returns false for a short row
// that stores nothing; store(ctx, dir, b, cidx, t) writes basis row b of direction dir.
template <int VEC, int TPR, class Ctx, class Row, class Range, class Store>
__device__ __forceinline__ void row_walk_banked(const int32_t* row_ptr, const int32_t* long_rows, const int32_t* nlong,
                                                int V, int nvec, int nbt, int n_long_blocks, Row row, Range range,
                                                Store store) {
  if ((int)blockIdx.x < n_long_blocks) {
    __shared__ float red[8][128 * VEC];
    const int cl = threadIdx.x & 127, sl = threadIdx.x >> 7;
    const int n = *nlong;
    for (int lb = blockIdx.x; lb < n; lb += n_long_blocks) {
      const int v = long_rows[lb];
      const int beg = row_ptr[v], end = row_ptr[v + 1];
      Ctx ctx;
      (void)row(v, beg, end, ctx);
      for (int c0 = 0; c0 < nvec; c0 += 128) {
        const int cidx = c0 + cl;
        float accf[BT][VEC], accb[BT][VEC];
#pragma unroll
        for (int b = 0; b < BT; ++b)
#pragma unroll
          for (int k = 0; k < VEC; ++k) { accf[b][k] = 0.f; accb[b][k] = 0.f; }
        if (cidx < nvec) range(beg + sl, end, 8, cidx, accf, accb);
#pragma unroll
        for (int q = 0; q < 2 * BT; ++q) {
          const int b = q % BT;
          if (b < nbt) {
#pragma unroll
            for (int k = 0; k < VEC; ++k) red[sl][cl * VEC + k] = q < BT ? accf[b][k] : accb[b][k];
            __syncthreads();
            if (sl == 0 && cidx < nvec) {
              float t[VEC];
#pragma unroll
              for (int k = 0; k < VEC; ++k) t[k] = lds_sum8<VEC>(red, cl * VEC + k);
              store(ctx, q < BT ? 0 : 1, b, cidx, t);
            }
            __syncthreads();
          }
        }
      }
    }
    return;
  }
  const int v = ((int)blockIdx.x - n_long_blocks) * (kRowThreads / TPR) + threadIdx.x / TPR;
  if (v >= V) return;
  const int lane = threadIdx.x % TPR;
  const int beg = row_ptr[v], end = row_ptr[v + 1];
  if (end - beg > kLongRow) return;      // a long-row workgroup of this launch owns it
  Ctx ctx;
  if (!row(v, beg, end, ctx)) return;
  for (int cidx = lane; cidx < nvec; cidx += TPR) {
    float accf[BT][VEC], accb[BT][VEC];
#pragma unroll
    for (int b = 0; b < BT; ++b)
#pragma unroll
      for (int k = 0; k < VEC; ++k) { accf[b][k] = 0.f; accb[b][k] = 0.f; }
    range(beg, end, 1, cidx, accf, accb);
#pragma unroll
    for (int b = 0; b < BT; ++b)
      if (b < nbt) {
        store(ctx, 0, b, cidx, accf[b]);
        store(ctx, 1, b, cidx, accb[b]);
      }
  }
}

// kernel<VEC, TPR> for VEC in {4, 1} and TPR in {64, 128, 256}: every compiled variant of a row kernel
#define RGCN_LAUNCH_ROWS(kernel, vec4, tpr, grid, block, stream, ...)                                      \
  do {                                                                                                     \
    if (vec4) {                                                                                            \
      if ((tpr) == 64) hipLaunchKernelGGL((kernel<4, 64>), grid, block, 0, stream, __VA_ARGS__);           \
      else if ((tpr) == 128) hipLaunchKernelGGL((kernel<4, 128>), grid, block, 0, stream, __VA_ARGS__);    \
      else hipLaunchKernelGGL((kernel<4, 256>), grid, block, 0, stream, __VA_ARGS__);                      \
    } else {                                                                                               \
      if ((tpr) == 64) hipLaunchKernelGGL((kernel<1, 64>), grid, block, 0, stream, __VA_ARGS__);           \
      else if ((tpr) == 128) hipLaunchKernelGGL((kernel<1, 128>), grid, block, 0, stream, __VA_ARGS__);    \
      else hipLaunchKernelGGL((kernel<1, 256>), grid, block, 0, stream, __VA_ARGS__);                      \
    }                                                                                                      \
  } while (0)

}  // namespace rgcn
