// Basis layer with per-feature coefficients (BasisGcnTimesDiag, code/encoders/message_gcns/gcn_basis_times_diag.py;
// RGCN_KIND_BASIS_TDIAG): the coefficient of a message is a VECTOR per (relation, basis) over the output channels,
//     W_r = sum_b W_b . diag(sigmoid(C[r,b,:])).
// In BasisGcn the coefficient is a scalar, which is why basis.hip can aggregate first and contract afterwards.  Here it
// multiplies the OUTPUT channel of the contraction, so aggregation does not commute with it: the layer transforms first,
//     G      = sigmoid(C)                                               [2R][B][d]   (k_tdiag_sigmoid, once per weight update)
//     P_dir  = H . W_dir.reshape(d, B.d)                                 [2][V][B.d]  (one batched GEMM, rgcn_schedule.hip)
//     pre[v] = dropout(H . W_self)[v] + sum_{m -> v} n_m sum_b G[rel_m,b,:] * P_dir(m)[src_m,b,:] + b
// the last line destination-major over the incidence CSR (k_tdiag_rows: per slot the B.d contiguous floats of P_dir[src] and
// of G[rel]), with the self-loop term, dropout, the bias and relu as its epilogue.
// Backward, D = dL/dpre:
//     dP_dir[u,b,:] = sum_{m: src_m = u, dir} n_m G[rel_m,b,:] * D[dst_m,:]        source-major (k_tdiag_dp), every row written:
//                     dW_dir = H^T . dP_dir reads all of them
//     dG[rel,b,:]   = sum_{m: rel_m = rel} n_m P_dir[src_m,b,:] * D[dst_m,:]        per relation chunk into slabs (k_tdiag_dcoef),
//     dC            = dG * G * (1 - G)                                             the slabs added in chunk order (k_tdiag_dcoef_reduce)
//     dH            = dS . W_self^T + dP_f . W_f^T + dP_b . W_b^T                   GEMMs; k_tdiag_dh_join adds, gates, copies
// No float atomics: every sum has a fixed order, two passes over the same inputs give the same bits.
#include "rgcn_internal.h"
#include "row_walk.h"

namespace rgcn {

namespace {

// sigmoid without special cases: z = +inf -> 1 / (1 + 0) = 1, z = -inf -> 1 / (1 + inf) = 0
__global__ void k_tdiag_sigmoid(const float* __restrict__ C, float* __restrict__ G, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) G[i] = 1.0f / (1.0f + __expf(-C[i]));
}

// ---------------------------------------------------------------- forward: destination-major rows
struct RowArgs {
  const float* P;            // [2][V][B*d]
  const float* G;            // [2R][B][d]
  const float* bias;         // [d]
  const int32_t* row_ptr;    // incidence CSR (rows = destinations)
  const int32_t* d_src;      // per slot: source vertex, directed relation, normalisation
  const int32_t* d_rel;
  const float* d_norm;
  const int32_t* long_rows;
  const int32_t* nlong;
  int32_t B, R;
  CombineArgs c;             // out, base (the self-loop product, dropout `drop`), relu, V, d
};

// acc += sum over slots s0, s0 + step, ... < s1 of  n * sum_b G[rel,b,:] * P[dir,src,b,:]   at column vector cidx
template <int VEC>
__device__ __forceinline__ void row_range(const RowArgs& a, int s0, int s1, int step, int cidx, float (&acc)[VEC]) {
  const int d = a.c.d;
  const size_t Bd = (size_t)a.B * d;
  for (int s = s0; s < s1; s += step) {
    const int src = a.d_src[s], rel = a.d_rel[s];
    const float nrm = a.d_norm[s];
    const int dir = rel < a.R ? 0 : 1;
    const float* p = a.P + ((size_t)dir * a.c.V + src) * Bd + (size_t)cidx * VEC;
    const float* g = a.G + (size_t)rel * Bd + (size_t)cidx * VEC;
    float t[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) t[k] = 0.f;
    for (int b = 0; b < a.B; ++b) {
      float pv[VEC], gv[VEC];
      vload<VEC>(p + (size_t)b * d, pv);
      vload<VEC>(g + (size_t)b * d, gv);
#pragma unroll
      for (int k = 0; k < VEC; ++k) t[k] = fmaf(gv[k], pv[k], t[k]);
    }
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = fmaf(nrm, t[k], acc[k]);
  }
}

// (dropout(self-loop) + messages) + b, relu, store
template <int VEC>
__device__ __forceinline__ void row_epilogue(const RowArgs& a, const DropKey& key, int v, int cidx, const float (&acc)[VEC]) {
#pragma clang fp contract(off)
  const size_t off = (size_t)v * a.c.d + (size_t)cidx * VEC;
  float s[VEC], bb[VEC], o[VEC];
  vload<VEC>(a.c.base + off, s);
  vload<VEC>(a.bias + (size_t)cidx * VEC, bb);
#pragma unroll
  for (int k = 0; k < VEC; ++k) {
    const float pre = (s[k] * drop_factor(a.c.drop, key, off + k) + acc[k]) + bb[k];
    o[k] = a.c.relu ? fmaxf(pre, 0.f) : pre;
  }
  vstore<VEC>(a.c.out + off, o);
}

// the single-accumulator row walk (row_walk.h) over the destination rows
template <int VEC, int TPR>
__global__ void __launch_bounds__(kRowThreads) k_tdiag_rows(RowArgs a, int n_long_blocks) {
  const DropKey key = drop_key(a.c.drop);
  row_walk<VEC, TPR>(
      a.row_ptr, a.long_rows, a.nlong, a.c.V, a.c.d / VEC, n_long_blocks,
      [&a](int s0, int s1, int step, int cidx, float (&acc)[VEC]) { row_range<VEC>(a, s0, s1, step, cidx, acc); },
      [&a, &key](int v, int cidx, const float (&acc)[VEC]) { row_epilogue<VEC>(a, key, v, cidx, acc); });
}

// ---------------------------------------------------------------- backward: source-major dP
struct DpArgs {
  const float* D;            // [V,d]
  const float* G;            // [2R][B][d]
  float* dP;                 // [2][V][B*d]
  const int32_t* row_ptr;    // incidence CSR (rows = sources)
  const int32_t* s_dst;      // per source-order slot: destination vertex, directed relation, normalisation
  const int32_t* s_rel;
  const float* s_norm;
  const int32_t* long_rows;
  const int32_t* nlong;
  int32_t V, d, B, R, b0, nbt;
};

template <int VEC>
__device__ __forceinline__ void dp_range(const DpArgs& a, int s0, int s1, int step, int cidx, float (&accf)[BT][VEC],
                                         float (&accb)[BT][VEC]) {
  const size_t Bd = (size_t)a.B * a.d;
  for (int s = s0; s < s1; s += step) {
    const int dst = a.s_dst[s], rel = a.s_rel[s];
    const float nrm = a.s_norm[s];
    float x[VEC];
    vload<VEC>(a.D + (size_t)dst * a.d + (size_t)cidx * VEC, x);
#pragma unroll
    for (int k = 0; k < VEC; ++k) x[k] *= nrm;
    const float* g = a.G + (size_t)rel * Bd + (size_t)a.b0 * a.d + (size_t)cidx * VEC;
    if (rel < a.R) {      // (wave-uniform in the long-row workgroups, per row group otherwise)
#pragma unroll
      for (int b = 0; b < BT; ++b)
        if (b < a.nbt) {
          float gv[VEC];
          vload<VEC>(g + (size_t)b * a.d, gv);
#pragma unroll
          for (int k = 0; k < VEC; ++k) accf[b][k] = fmaf(gv[k], x[k], accf[b][k]);
        }
    } else {
#pragma unroll
      for (int b = 0; b < BT; ++b)
        if (b < a.nbt) {
          float gv[VEC];
          vload<VEC>(g + (size_t)b * a.d, gv);
#pragma unroll
          for (int k = 0; k < VEC; ++k) accb[b][k] = fmaf(gv[k], x[k], accb[b][k]);
        }
    }
  }
}

struct DpRow {
  float* p[2];               // the row's dP rows of the two directions, at basis b0
};

// The banked row walk (row_walk.h) over the source rows.  A row that sends nothing writes its zeros: dW = H^T . dP reads
// every row.
template <int VEC, int TPR>
__global__ void __launch_bounds__(kRowThreads) k_tdiag_dp(DpArgs a, int n_long_blocks) {
  const size_t Bd = (size_t)a.B * a.d;
  row_walk_banked<VEC, TPR, DpRow>(
      a.row_ptr, a.long_rows, a.nlong, a.V, a.d / VEC, a.nbt, n_long_blocks,
      [&a, Bd](int v, int, int, DpRow& r) {
        r.p[0] = a.dP + (size_t)v * Bd + (size_t)a.b0 * a.d;
        r.p[1] = a.dP + ((size_t)a.V + v) * Bd + (size_t)a.b0 * a.d;
        return true;
      },
      [&a](int s0, int s1, int step, int cidx, float (&accf)[BT][VEC], float (&accb)[BT][VEC]) {
        dp_range<VEC>(a, s0, s1, step, cidx, accf, accb);
      },
      [&a](const DpRow& r, int dir, int b, int cidx, const float (&t)[VEC]) {
        vstore<VEC>(r.p[dir] + (size_t)b * a.d + (size_t)cidx * VEC, t);
      });
}

// ---------------------------------------------------------------- backward: coefficient gradient
struct DcoefArgs {
  const float* P;            // [2][V][B*d]
  const float* D;            // [V,d]
  const int32_t* m_src;      // relation-sorted message list
  const int32_t* m_dst;
  const float* m_norm;
  const int32_t* rel_ptr;
  const int32_t* chunk_ptr;
  float* slab;               // [chunks][B*d]
  int32_t V, R, B, d, chunk;
};

// One workgroup per relation chunk; every thread owns VEC of the B.d entries of the chunk's slab row and adds the chunk's
// messages in list order.
template <int VEC>
__global__ void __launch_bounds__(256) k_tdiag_dcoef(DcoefArgs a) {
  const int bid = blockIdx.x;
  const int R2 = 2 * a.R;
  if (bid >= a.chunk_ptr[R2]) return;
  const int rel = find_segment(a.chunk_ptr, R2, bid);
  const int beg = a.rel_ptr[rel] + (bid - a.chunk_ptr[rel]) * a.chunk;
  const int end = min(beg + a.chunk, a.rel_ptr[rel + 1]);
  const int dir = rel < a.R ? 0 : 1;
  const int Bd = a.B * a.d;
  const float* Pd = a.P + (size_t)dir * a.V * Bd;
  for (int e = threadIdx.x * VEC; e < Bd; e += 256 * VEC) {
    const int col = e % a.d;      // (d % VEC == 0: the VEC entries share a basis function)
    float acc[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
    for (int j = beg; j < end; ++j) {
      const float nrm = a.m_norm[j];
      float p[VEC], x[VEC];
      vload<VEC>(Pd + (size_t)a.m_src[j] * Bd + e, p);
      vload<VEC>(a.D + (size_t)a.m_dst[j] * a.d + col, x);
#pragma unroll
      for (int k = 0; k < VEC; ++k) acc[k] = fmaf(nrm, p[k] * x[k], acc[k]);
    }
    vstore<VEC>(a.slab + (size_t)bid * Bd + e, acc);
  }
}

// gcoef[rel,b,:] = G (1 - G) * (the relation's chunk partials in chunk order, compensated like k_basis_dcoef_reduce)
__global__ void k_tdiag_dcoef_reduce(const float* __restrict__ slab, const int32_t* __restrict__ chunk_ptr,
                                     const float* __restrict__ G, float* __restrict__ gcoef, int R2, int Bd) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)R2 * Bd) return;
  const int rel = (int)(i / Bd), e = (int)(i - (int64_t)rel * Bd);
  float acc = 0.f, comp = 0.f;
  {
#pragma clang fp contract(off)
    for (int c = chunk_ptr[rel]; c < chunk_ptr[rel + 1]; ++c) {
      const float y = slab[(size_t)c * Bd + e] - comp;
      const float t = acc + y;
      comp = (t - acc) - y;
      acc = t;
    }
  }
  const float g = G[i];
  gcoef[i] = acc * (g * (1.0f - g));
}

// ---------------------------------------------------------------- backward: dH epilogue
template <int VEC>
__global__ void __launch_bounds__(256) k_tdiag_dh_join(CombineArgs a, const float* __restrict__ dh, int64_t nvec) {
  const DropKey key = drop_key(a.drop2);
  const size_t Vd = (size_t)a.V * a.d;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * blockDim.x) {
    const size_t off = (size_t)i * VEC;
    float s[VEC], f[VEC], b[VEC];
    vload<VEC>(a.base + off, s);
    vload<VEC>(dh + off, f);
    vload<VEC>(dh + Vd + off, b);
#pragma unroll
    for (int k = 0; k < VEC; ++k) s[k] = (s[k] + f[k]) + b[k];
    if (a.gate != nullptr) {
      float gt[VEC];
      vload<VEC>(a.gate + off, gt);
#pragma unroll
      for (int k = 0; k < VEC; ++k) s[k] = gt[k] > 0.f ? s[k] : 0.f;
    }
    vstore<VEC>(a.out + off, s);
    if (a.out2 != nullptr) {
      float o2[VEC];
#pragma unroll
      for (int k = 0; k < VEC; ++k) o2[k] = s[k] * drop_factor(a.drop2, key, off + k);
      vstore<VEC>(a.out2 + off, o2);
    }
  }
}

}  // namespace

rgcn_status tdiag_refresh_gates(rgcn_ctx* c, int layer) {
  LayerBufs& lb = c->layers[layer];
  if (lb.tdiag_g_version == c->weights_version) return RGCN_OK;
  const int64_t n = (int64_t)2 * c->R * c->B * c->d;
  ProfScope ps(c, "tdiag_sigmoid", 8.0 * n, 4.0 * n);
  hipLaunchKernelGGL(k_tdiag_sigmoid, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, lb.coef, lb.tdiag_g, n);
  RGCN_HIP(c, hipGetLastError());
  lb.tdiag_g_version = c->weights_version;
  return RGCN_OK;
}

rgcn_status tdiag_rows_forward(rgcn_ctx* c, int layer, const float* P, const CombineArgs& ca) {
  const LayerBufs& lb = c->layers[layer];
  RowArgs a;
  a.P = P; a.G = lb.tdiag_g; a.bias = lb.bias;
  a.row_ptr = c->g.row_ptr; a.d_src = c->g.d_src; a.d_rel = c->g.d_rel; a.d_norm = c->g.d_norm;
  a.long_rows = c->g.long_rows; a.nlong = c->g.nlong;
  a.B = c->B; a.R = c->R; a.c = ca;
  if (ca.base == nullptr || ca.out == nullptr) RGCN_FAIL(c, RGCN_ERR_STATE, "internal: tdiag_rows_forward needs base and out");
  const bool vec4 = (c->d % 4 == 0) && aligned16(P) && aligned16(a.G) && aligned16(a.bias) && aligned16(ca.base) &&
                    aligned16(ca.out);
  const int nvec = vec4 ? c->d / 4 : c->d;
  const int tpr = row_lanes(nvec);
  const int nlb = long_blocks(c);
  dim3 grid = row_grid(nlb, c->V, tpr), block(kRowThreads);
  const double M = 2.0 * c->g.E, Bd = (double)c->B * c->d;
  const double rows = M < 2.0 * c->V ? M : 2.0 * c->V;      // compulsory: each gathered row of P once, G once
  ProfScope ps(c, "tdiag_rows_fwd", 4.0 * (2.0 * M * Bd + 2.0 * c->V * c->d) + 12.0 * M, 2.0 * M * Bd + 2.0 * M * c->d,
               4.0 * (rows * Bd + 2.0 * c->R * Bd + 2.0 * c->V * c->d) + 12.0 * M);
  RGCN_LAUNCH_ROWS(k_tdiag_rows, vec4, tpr, grid, block, c->stream, a, nlb);
  RGCN_HIP(c, hipGetLastError());
  return RGCN_OK;
}

rgcn_status tdiag_dp(rgcn_ctx* c, int layer, const float* D, float* dP) {
  DpArgs a;
  a.D = D; a.G = c->layers[layer].tdiag_g; a.dP = dP;
  a.row_ptr = c->g.row_ptr; a.s_dst = c->g.s_dst; a.s_rel = c->g.s_rel; a.s_norm = c->g.s_norm;
  a.long_rows = c->g.long_rows; a.nlong = c->g.nlong;
  a.V = c->V; a.d = c->d; a.B = c->B; a.R = c->R;
  const bool vec4 = (c->d % 4 == 0) && aligned16(D) && aligned16(a.G) && aligned16(dP);
  const int nvec = vec4 ? c->d / 4 : c->d;
  const int tpr = row_lanes(nvec);
  const int nlb = long_blocks(c);
  dim3 grid = row_grid(nlb, c->V, tpr), block(kRowThreads);
  const double M = 2.0 * c->g.E;
  for (int b0 = 0; b0 < c->B; b0 += BT) {
    a.b0 = b0;
    a.nbt = c->B - b0 < BT ? c->B - b0 : BT;
    const double rows = M < c->V ? M : (double)c->V;
    ProfScope ps(c, "tdiag_dp", 4.0 * c->d * (M * (1.0 + a.nbt) + 2.0 * c->V * a.nbt) + 12.0 * M, 2.0 * M * a.nbt * c->d,
                 4.0 * c->d * (rows + 2.0 * c->R * a.nbt + 2.0 * c->V * a.nbt) + 12.0 * M);
    RGCN_LAUNCH_ROWS(k_tdiag_dp, vec4, tpr, grid, block, c->stream, a, nlb);
    RGCN_HIP(c, hipGetLastError());
  }
  return RGCN_OK;
}

rgcn_status tdiag_dcoef(rgcn_ctx* c, int layer, const float* P, const float* D) {
  const int R2 = 2 * c->R, Bd = c->B * c->d;
  const LayerBufs& lb = c->layers[layer];
  if (c->g.E > 0) {
    const int nchunks = (int)((2 * c->g.E + c->g.chunk - 1) / c->g.chunk) + R2;
    if ((size_t)nchunks * Bd > c->slab_dw_floats) RGCN_FAIL(c, RGCN_ERR_STATE, "internal: dC slab too small");
    DcoefArgs a;
    a.P = P; a.D = D; a.m_src = c->g.m_src; a.m_dst = c->g.m_dst; a.m_norm = c->g.m_norm;
    a.rel_ptr = c->g.rel_ptr; a.chunk_ptr = c->g.chunk_ptr; a.slab = c->slab_dw;
    a.V = c->V; a.R = c->R; a.B = c->B; a.d = c->d; a.chunk = c->g.chunk;
    const double M = 2.0 * c->g.E;
    const double rows = M < c->V ? M : (double)c->V;
    ProfScope ps(c, "tdiag_dcoef", 4.0 * (M * (Bd + (double)c->B * c->d) + (double)nchunks * Bd) + 12.0 * M, 3.0 * M * Bd,
                 4.0 * (rows * (Bd + c->d) + (double)nchunks * Bd) + 12.0 * M);
    if (c->d % 4 == 0 && aligned16(P) && aligned16(D) && aligned16(c->slab_dw))
      hipLaunchKernelGGL((k_tdiag_dcoef<4>), dim3(nchunks), dim3(256), 0, c->stream, a);
    else
      hipLaunchKernelGGL((k_tdiag_dcoef<1>), dim3(nchunks), dim3(256), 0, c->stream, a);
    RGCN_HIP(c, hipGetLastError());
  }
  const int64_t n = (int64_t)R2 * Bd;
  ProfScope ps(c, "tdiag_dcoef_reduce", 4.0 * (2.0 * n + 2.0 * c->g.E / c->g.chunk * Bd + (double)n), 4.0 * n);
  hipLaunchKernelGGL(k_tdiag_dcoef_reduce, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, c->slab_dw,
                     c->g.chunk_ptr, lb.tdiag_g, lb.gcoef, R2, Bd);
  RGCN_HIP(c, hipGetLastError());
  return RGCN_OK;
}

rgcn_status tdiag_dh_join(rgcn_ctx* c, const float* dh, const CombineArgs& ca) {
  if (ca.base == nullptr || ca.out == nullptr) RGCN_FAIL(c, RGCN_ERR_STATE, "internal: tdiag_dh_join needs base and out");
  const int64_t n = (int64_t)c->V * c->d;
  const bool vec4 = (c->d % 4 == 0) && aligned16(dh) && aligned16(ca.base) && aligned16(ca.out) && aligned16(ca.gate) &&
                    aligned16(ca.out2);
  const int64_t nvec = vec4 ? n / 4 : n;
  int64_t blocks = (nvec + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  if (blocks < 1) blocks = 1;
  ProfScope ps(c, "tdiag_dh_join", 4.0 * n * (5.0 + (ca.out2 ? 1.0 : 0.0)), 2.0 * n);
  if (vec4) hipLaunchKernelGGL((k_tdiag_dh_join<4>), dim3((unsigned)blocks), dim3(256), 0, c->stream, ca, dh, nvec);
  else hipLaunchKernelGGL((k_tdiag_dh_join<1>), dim3((unsigned)blocks), dim3(256), 0, c->stream, ca, dh, nvec);
  RGCN_HIP(c, hipGetLastError());
  return RGCN_OK;
}

}  // namespace rgcn
