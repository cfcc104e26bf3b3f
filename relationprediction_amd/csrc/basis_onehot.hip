// Featureless first layer of the basis encoder: BasisGcn with onehot_input=True (UseInputTransform=No;
// code/common/model_builder.py:140-165,277-283, code/encoders/message_gcns/gcn_basis.py:16-24,60-71,
// code/encoders/message_gcns/message_gcn.py:28-79, code/common/shared_functions.py:5-9).
//
// The layer's input is the entity id, so dot_or_lookup takes its lookup branch: the "weights" are per-entity tables
// W_forward, W_backward [V,B,d] and W_self [V,d], and a message is a row of a table instead of a row of a GEMM:
//     pre1[v] = dropout(W_self)[v] + sum_{m -> v} n_m sum_b C_dir(m)[rel_m,b] W_dir(m)[src_m,b,:]
// There is no dense contraction, no [units, B.d] intermediate and nothing below the layer (no dH).  Three kernels:
//   k_onehot_fwd     destination-major over the incidence CSR: every slot gathers the B.d floats of its sender's table row
//                    (10 KB at B = 5, d = 500: the traffic of the layer), the combine (W_self row, dropout, relu) is the
//                    epilogue, H_1 is written once;
//   k_onehot_tables  source-major over the same CSR: dW_dir[u,b,:] = sum_{m: src_m = u, dir} n_m C[rel_m,b] D[dst_m,:], one
//                    gather of a D row per slot, coefficients applied in registers, every (u, dir, b) row written exactly
//                    once -- zeros for a vertex that sends nothing, in the same pass (the tables are dense parameters:
//                    Adam reads every row of their gradient);
//   k_onehot_dcoef   per relation chunk, as k_basis_dcoef: dC[r,b] = sum_{m: rel_m = r} n_m <W_dir[src_m,b,:], D[dst_m,:]>,
//                    chunk partials to the slab, summed by basis_dcoef_reduce in chunk order.
// dW_self = dropout-scaled D is a copy (rgcn_schedule.hip).  Conventions are basis.hip's: float4 columns with a scalar
// form for d % 4 != 0, rows above kLongRow slots by a whole workgroup from the long-row list (the basis kind never cuts
// giant rows: a workgroup walks a hub of any length, eight slots at a time), no atomics, fixed summation order.
#include "rgcn_internal.h"
#include "row_walk.h"

namespace rgcn {

namespace {

// ---------------------------------------------------------------- forward
struct OnehotFwdArgs {
  const float* W;            // [2][V][B][d]: W_forward, W_backward
  const float* wself;        // [V][d]
  float* out;                // H_1 [V][d]
  const int32_t* row_ptr;    // incidence CSR (rows = destinations)
  const int32_t* d_src;      // per slot: sender, directed relation, normalisation
  const int32_t* d_rel;
  const float* d_norm;
  const float* coef;         // [2R][B]
  const int32_t* long_rows;
  const int32_t* nlong;
  int32_t V, d, B, R, relu;
  DropSpec drop;             // applied to the W_self row
};

// acc += sum over slots [s0, s1) step `step` of  n * sum_b C[rel,b] * W_dir[src,b,:]   (two slots in flight)
template <int VEC>
__device__ __forceinline__ void lookup_range(const OnehotFwdArgs& a, int s0, int s1, int step, int cidx, float (&acc)[VEC]) {
  const size_t tstride = (size_t)a.B * a.d, dstride = (size_t)a.V * tstride;
  for (int s = s0; s < s1; s += 2 * step) {
    const bool two = s + step < s1;
    const int src0 = a.d_src[s], rel0 = a.d_rel[s];
    const float n0 = a.d_norm[s];
    const int src1 = two ? a.d_src[s + step] : src0, rel1 = two ? a.d_rel[s + step] : rel0;
    const float n1 = two ? a.d_norm[s + step] : 0.f;
    const float* w0 = a.W + (rel0 < a.R ? 0 : dstride) + (size_t)src0 * tstride + (size_t)cidx * VEC;
    const float* w1 = a.W + (rel1 < a.R ? 0 : dstride) + (size_t)src1 * tstride + (size_t)cidx * VEC;
    const float* c0 = a.coef + (size_t)rel0 * a.B;
    const float* c1 = a.coef + (size_t)rel1 * a.B;
    for (int b = 0; b < a.B; ++b) {
      float v0[VEC], v1[VEC];
      vload<VEC>(w0 + (size_t)b * a.d, v0);
      vload<VEC>(w1 + (size_t)b * a.d, v1);
      const float x0 = n0 * c0[b], x1 = n1 * c1[b];
#pragma unroll
      for (int k = 0; k < VEC; ++k) acc[k] = fmaf(x1, v1[k], fmaf(x0, v0[k], acc[k]));
    }
  }
}

// H_1[v] = act(dropout(W_self)[v] + gathered)
template <int VEC>
__device__ __forceinline__ void lookup_epilogue(const OnehotFwdArgs& a, const DropKey& key, size_t off, float (&acc)[VEC]) {
  float ws[VEC];
  vload<VEC>(a.wself + off, ws);
#pragma unroll
  for (int k = 0; k < VEC; ++k) {
    acc[k] = fmaf(ws[k], drop_factor(a.drop, key, off + k), acc[k]);
    if (a.relu) acc[k] = fmaxf(acc[k], 0.f);
  }
  vstore<VEC>(a.out + off, acc);
}

// the single-accumulator row walk (row_walk.h) over the destination rows
template <int VEC, int TPR>
__global__ void __launch_bounds__(kRowThreads) k_onehot_fwd(OnehotFwdArgs a, int n_long_blocks) {
  const DropKey key = drop_key(a.drop);
  row_walk<VEC, TPR>(
      a.row_ptr, a.long_rows, a.nlong, a.V, a.d / VEC, n_long_blocks,
      [&a](int s0, int s1, int step, int cidx, float (&acc)[VEC]) { lookup_range<VEC>(a, s0, s1, step, cidx, acc); },
      [&a, &key](int v, int cidx, float (&acc)[VEC]) { lookup_epilogue<VEC>(a, key, (size_t)v * a.d + (size_t)cidx * VEC, acc); });
}

// ---------------------------------------------------------------- table gradients
struct OnehotTablesArgs {
  const float* D;            // dL/dpre1 [V][d]
  float* G;                  // [2][V][B][d]: dW_forward, dW_backward
  const int32_t* row_ptr;    // incidence CSR (rows = sources)
  const int32_t* s_dst;      // per source-order slot: receiver, directed relation, normalisation
  const int32_t* s_rel;
  const float* s_norm;
  const float* coef;         // [2R][B]
  const int32_t* long_rows;
  const int32_t* nlong;
  int32_t V, d, B, R, b0, nbt;
};

// one slot into the accumulators of the table its message reads (wave-uniform branch)
template <int VEC>
__device__ __forceinline__ void tables_entry(const OnehotTablesArgs& a, int rel, float nrm, const float (&x)[VEC],
                                             float (&accf)[BT][VEC], float (&accb)[BT][VEC]) {
  const float* cf = a.coef + (size_t)rel * a.B + a.b0;
  if (rel < a.R) {
#pragma unroll
    for (int b = 0; b < BT; ++b)
      if (b < a.nbt) {
        const float w = nrm * cf[b];
#pragma unroll
        for (int k = 0; k < VEC; ++k) accf[b][k] = fmaf(w, x[k], accf[b][k]);
      }
  } else {
#pragma unroll
    for (int b = 0; b < BT; ++b)
      if (b < a.nbt) {
        const float w = nrm * cf[b];
#pragma unroll
        for (int k = 0; k < VEC; ++k) accb[b][k] = fmaf(w, x[k], accb[b][k]);
      }
  }
}

// slots [s0, s1) with stride `step` of one source row, for one vector column: 4 gathers of D rows in flight
template <int VEC>
__device__ __forceinline__ void tables_range(const OnehotTablesArgs& a, int s0, int s1, int step, int cidx,
                                             float (&accf)[BT][VEC], float (&accb)[BT][VEC]) {
  int s = s0;
  for (; s + 3 * step < s1; s += 4 * step) {
    int dst[4], rel[4];
    float nrm[4], x[4][VEC];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      dst[u] = a.s_dst[s + u * step]; rel[u] = a.s_rel[s + u * step]; nrm[u] = a.s_norm[s + u * step];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) vload<VEC>(a.D + (size_t)dst[u] * a.d + (size_t)cidx * VEC, x[u]);
#pragma unroll
    for (int u = 0; u < 4; ++u) tables_entry<VEC>(a, rel[u], nrm[u], x[u], accf, accb);
  }
  for (; s < s1; s += step) {
    float x[VEC];
    vload<VEC>(a.D + (size_t)a.s_dst[s] * a.d + (size_t)cidx * VEC, x);
    tables_entry<VEC>(a, a.s_rel[s], a.s_norm[s], x, accf, accb);
  }
}

// Every row u writes its nbt basis rows of BOTH tables (zeros where it sends nothing in that direction).  The walk is
// row_walk.h's banked form written out: through the template the float4 variants take 105 VGPRs, not 103, which at 1024
// threads is 112 per wave, not 104, and leaves no room on a SIMD for a wave of k_onehot_dcoef (67 VGPRs), which runs
// beside this kernel on side stream 0 -- measured as 6 % on this kernel and 0.8 % on the one-hot train step.
template <int VEC, int TPR>
__global__ void __launch_bounds__(kRowThreads) k_onehot_tables(OnehotTablesArgs a, int n_long_blocks) {
  const int nvec = a.d / VEC;
  const size_t tstride = (size_t)a.B * a.d, dstride = (size_t)a.V * tstride;
  if ((int)blockIdx.x < n_long_blocks) {
    __shared__ float red[8][128 * VEC];
    const int cl = threadIdx.x & 127, sl = threadIdx.x >> 7;
    const int n = *a.nlong;
    for (int lb = blockIdx.x; lb < n; lb += n_long_blocks) {
      const int u = a.long_rows[lb];
      const int beg = a.row_ptr[u], end = a.row_ptr[u + 1];
      for (int c0 = 0; c0 < nvec; c0 += 128) {
        const int cidx = c0 + cl;
        float accf[BT][VEC], accb[BT][VEC];
#pragma unroll
        for (int b = 0; b < BT; ++b)
#pragma unroll
          for (int k = 0; k < VEC; ++k) { accf[b][k] = 0.f; accb[b][k] = 0.f; }
        if (cidx < nvec) tables_range<VEC>(a, beg + sl, end, 8, cidx, accf, accb);
#pragma unroll
        for (int q = 0; q < 2 * BT; ++q) {
          const int b = q % BT;
          if (b < a.nbt) {
#pragma unroll
            for (int k = 0; k < VEC; ++k) red[sl][cl * VEC + k] = q < BT ? accf[b][k] : accb[b][k];
            __syncthreads();
            if (sl == 0 && cidx < nvec) {
              float t[VEC];
#pragma unroll
              for (int k = 0; k < VEC; ++k) t[k] = lds_sum8<VEC>(red, cl * VEC + k);
              vstore<VEC>(a.G + (q < BT ? 0 : dstride) + (size_t)u * tstride + (size_t)(a.b0 + b) * a.d + (size_t)cidx * VEC, t);
            }
            __syncthreads();
          }
        }
      }
    }
    return;
  }
  const int u = ((int)blockIdx.x - n_long_blocks) * (kRowThreads / TPR) + threadIdx.x / TPR;
  if (u >= a.V) return;
  const int lane = threadIdx.x % TPR;
  const int beg = a.row_ptr[u], end = a.row_ptr[u + 1];
  if (end - beg > kLongRow) return;      // a long-row workgroup of this launch owns it
  float* gf = a.G + (size_t)u * tstride + (size_t)a.b0 * a.d;
  float* gb = gf + dstride;
  for (int cidx = lane; cidx < nvec; cidx += TPR) {
    float accf[BT][VEC], accb[BT][VEC];
#pragma unroll
    for (int b = 0; b < BT; ++b)
#pragma unroll
      for (int k = 0; k < VEC; ++k) { accf[b][k] = 0.f; accb[b][k] = 0.f; }
    tables_range<VEC>(a, beg, end, 1, cidx, accf, accb);
#pragma unroll
    for (int b = 0; b < BT; ++b)
      if (b < a.nbt) {
        vstore<VEC>(gf + (size_t)b * a.d + (size_t)cidx * VEC, accf[b]);
        vstore<VEC>(gb + (size_t)b * a.d + (size_t)cidx * VEC, accb[b]);
      }
  }
}

// ---------------------------------------------------------------- coefficient gradients
struct OnehotDcoefArgs {
  const float* D;            // [V][d]
  const float* W;            // [2][V][B][d]
  const int32_t* m_src;      // relation-sorted message list
  const int32_t* m_dst;
  const float* m_norm;
  const int32_t* rel_ptr;
  const int32_t* chunk_ptr;
  float* slab;               // [chunks][B]
  int32_t V, R, B, d, chunk;
};

// One workgroup (4 waves) per relation chunk; wave w takes messages beg+w, beg+w+4, ...; the wave's lanes split the d
// features, reduce the B dot products by shuffles, partial sums meet in LDS.
template <int VEC>
__global__ void __launch_bounds__(256) k_onehot_dcoef(OnehotDcoefArgs a) {
  __shared__ float red[4][64];
  const int bid = blockIdx.x;
  const int R2 = 2 * a.R;
  if (bid >= a.chunk_ptr[R2]) return;
  const int rel = find_segment(a.chunk_ptr, R2, bid);
  const int beg = a.rel_ptr[rel] + (bid - a.chunk_ptr[rel]) * a.chunk;
  const int end = min(beg + a.chunk, a.rel_ptr[rel + 1]);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t tstride = (size_t)a.B * a.d;
  const float* table = a.W + (rel < a.R ? 0 : (size_t)a.V * tstride);
  const int nvec = a.d / VEC;
  for (int b0 = 0; b0 < a.B; b0 += BT) {
    float part[BT];
#pragma unroll
    for (int b = 0; b < BT; ++b) part[b] = 0.f;
    for (int j = beg + wave; j < end; j += 4) {
      const float nrm = a.m_norm[j];
      const float* xp = a.D + (size_t)a.m_dst[j] * a.d;
      const float* wp = table + (size_t)a.m_src[j] * tstride + (size_t)b0 * a.d;
      for (int cidx = lane; cidx < nvec; cidx += 64) {
        float x[VEC];
        vload<VEC>(xp + (size_t)cidx * VEC, x);
#pragma unroll
        for (int b = 0; b < BT; ++b)
          if (b0 + b < a.B) {
            float w[VEC];
            vload<VEC>(wp + (size_t)b * a.d + (size_t)cidx * VEC, w);
            float t = 0.f;
#pragma unroll
            for (int k = 0; k < VEC; ++k) t = fmaf(x[k], w[k], t);
            part[b] = fmaf(nrm, t, part[b]);
          }
      }
    }
#pragma unroll
    for (int b = 0; b < BT; ++b) {
      float t = part[b];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) t += __shfl_down(t, off, 64);
      if (lane == 0) red[wave][b] = t;
    }
    __syncthreads();
    if (threadIdx.x < BT && b0 + (int)threadIdx.x < a.B)
      a.slab[(size_t)bid * a.B + b0 + threadIdx.x] =
          ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
    __syncthreads();
  }
}

}  // namespace

rgcn_status onehot_forward(rgcn_ctx* c, float* out) {
  const LayerBufs& lb = c->layers[1];
  OnehotFwdArgs a;
  a.W = lb.wrel; a.wself = lb.wself; a.out = out;
  a.row_ptr = c->g.row_ptr; a.d_src = c->g.d_src; a.d_rel = c->g.d_rel; a.d_norm = c->g.d_norm;
  a.coef = lb.coef; a.long_rows = c->g.long_rows; a.nlong = c->g.nlong;
  a.V = c->V; a.d = c->d; a.B = c->B; a.R = c->R; a.relu = c->L > 1 ? 1 : 0;
  a.drop = make_drop(c, 1, true);
  const bool vec4 = (c->d % 4 == 0) && aligned16(a.W) && aligned16(a.wself) && aligned16(out);
  const int nvec = vec4 ? c->d / 4 : c->d;
  const int tpr = row_lanes(nvec);
  const int nlb = long_blocks(c);
  dim3 grid = row_grid(nlb, c->V, tpr), block(kRowThreads);
  const double M = 2.0 * c->g.E, V = c->V, Bd = (double)c->B * c->d;
  const double senders = M < 2.0 * V ? M : 2.0 * V;      // compulsory: each (sender, direction) table row once
  ProfScope ps(c, "onehot_fwd", 4.0 * Bd * M + 12.0 * M + 8.0 * V * c->d, 2.0 * M * Bd,
               4.0 * Bd * senders + 12.0 * M + 8.0 * V * c->d);
  RGCN_LAUNCH_ROWS(k_onehot_fwd, vec4, tpr, grid, block, c->stream, a, nlb);
  RGCN_HIP(c, hipGetLastError());
  return RGCN_OK;
}

rgcn_status onehot_backward_tables(rgcn_ctx* c, const float* D) {
  const LayerBufs& lb = c->layers[1];
  OnehotTablesArgs a;
  a.D = D; a.G = lb.grel;
  a.row_ptr = c->g.row_ptr; a.s_dst = c->g.s_dst; a.s_rel = c->g.s_rel; a.s_norm = c->g.s_norm;
  a.coef = lb.coef; a.long_rows = c->g.long_rows; a.nlong = c->g.nlong;
  a.V = c->V; a.d = c->d; a.B = c->B; a.R = c->R;
  const bool vec4 = (c->d % 4 == 0) && aligned16(D) && aligned16(a.G);
  const int nvec = vec4 ? c->d / 4 : c->d;
  const int tpr = row_lanes(nvec);
  const int nlb = long_blocks(c);
  dim3 grid = row_grid(nlb, c->V, tpr), block(kRowThreads);
  const double M = 2.0 * c->g.E, V = c->V;
  const double rows = M < V ? M : V;                     // compulsory: each gathered row of D once
  for (int b0 = 0; b0 < c->B; b0 += BT) {
    a.b0 = b0;
    a.nbt = c->B - b0 < BT ? c->B - b0 : BT;
    // the write of both tables' gradient -- 2 V nbt d floats, zeros included -- is the kernel's traffic
    ProfScope ps(c, "onehot_tables_bwd", 4.0 * c->d * (M + 2.0 * V * a.nbt) + 12.0 * M, 2.0 * M * a.nbt * c->d,
                 4.0 * c->d * (rows + 2.0 * V * a.nbt) + 12.0 * M);
    RGCN_LAUNCH_ROWS(k_onehot_tables, vec4, tpr, grid, block, c->stream, a, nlb);
    RGCN_HIP(c, hipGetLastError());
  }
  return RGCN_OK;
}

rgcn_status onehot_dcoef(rgcn_ctx* c, const float* D) {
  const LayerBufs& lb = c->layers[1];
  if (c->g.E > 0) {
    const int nchunks = (int)((2 * c->g.E + c->g.chunk - 1) / c->g.chunk) + 2 * c->R;
    if ((size_t)nchunks * c->B > c->slab_dw_floats) RGCN_FAIL(c, RGCN_ERR_STATE, "internal: dC slab too small");
    OnehotDcoefArgs a;
    a.D = D; a.W = lb.wrel; a.m_src = c->g.m_src; a.m_dst = c->g.m_dst; a.m_norm = c->g.m_norm;
    a.rel_ptr = c->g.rel_ptr; a.chunk_ptr = c->g.chunk_ptr; a.slab = c->slab_dw;
    a.V = c->V; a.R = c->R; a.B = c->B; a.d = c->d; a.chunk = c->g.chunk;
    const double M = 2.0 * c->g.E, V = c->V;
    const double rows = M < V ? M : V, senders = M < 2.0 * V ? M : 2.0 * V;
    ProfScope ps(c, "onehot_dcoef", 4.0 * c->d * M * (1.0 + c->B) + 16.0 * M, 2.0 * M * c->B * c->d,
                 4.0 * c->d * (rows + c->B * senders) + 16.0 * M);
    if (c->d % 4 == 0 && aligned16(D) && aligned16(a.W))
      hipLaunchKernelGGL((k_onehot_dcoef<4>), dim3(nchunks), dim3(256), 0, c->stream, a);
    else
      hipLaunchKernelGGL((k_onehot_dcoef<1>), dim3(nchunks), dim3(256), 0, c->stream, a);
    RGCN_HIP(c, hipGetLastError());
  }
  return basis_dcoef_reduce(c, 1);
}

}  // namespace rgcn
