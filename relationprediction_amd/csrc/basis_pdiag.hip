// Basis layer with a per-relation diagonal (BasisGcnWithDiag, code/encoders/message_gcns/gcn_basis_plus_diag.py;
// RGCN_KIND_BASIS_PDIAG): the basis layer plus a DistMult-like term per message, H[src] * D[rho], D a trained vector per
// directed relation, and a bias that is added and trained.  AS EXECUTED by the reference the two basis
// products are swapped on their way into the messages: the basis term of a message to v is formed from v's OWN features
// under the OTHER direction's basis tensor.  It therefore does not depend on the source, and a row's messages of one
// direction collapse into B mixing scalars:
//     a_dir[v,b] = sum_{m -> v, dir(m) = dir} n_m C_dir[r_m,b]                                           [2][V][B]
//     pre[v]     = dropout(H . W_self)[v] + sum_dir sum_b a_dir[v,b] (H[v] . W_other(dir)[:,b,:])
//                  + sum_{m -> v} n_m D[rho_m,:] * H[src_m,:] + b
// The dense work is the basis kind's (basis.hip, rgcn_schedule.hip): Zc[(v,dir),b,:] = a_dir[v,b] H[v,:] over the compacted
// (row, direction) units, Zc . W' as two groups of one batched GEMM -- with the two weight groups stored SWAPPED
// (LayerBufs::wrel: group 0 = W_backward), so the forward-direction units contract with W_backward and dW_backward comes
// from them.  This file holds what is new:
//     k_pdiag_rows      destination-major, ONE walk over a row's slots: the 2B mixing scalars, the diagonal aggregate
//                       (d floats of H[src] and one row of D per slot), and the row's own Zc rows
//     k_pdiag_epilogue  ((dropout(S) + the two unit products) + aggregate) + b, relu
// Backward, G = dL/dpre (db = its column sums, dZc = G[units] . W'^T and dW' = Zc^T . G[units] by the basis GEMMs):
//     k_pdiag_row_bwd   row-local: da_dir[v,b] = <H[v], dZc[(v,dir),b,:]>, dh[v] = sum_dir sum_b a_dir[v,b] dZc[(v,dir),b,:]
//     k_pdiag_dcoef     dC[rho,b] = sum_{m: rho_m = rho} n_m da_dir[dst_m,b]      per relation chunk, B scalars per message
//     k_pdiag_ddiag     dD[rho,:] = sum_{m: rho_m = rho} n_m H[src_m,:] * G[dst_m,:]  per relation chunk into slabs,
//     k_pdiag_ddiag_reduce  the slabs added in chunk order (compensated)
//     k_pdiag_dh_join   source-major: dH[v] = ((dS . W_self^T + dh)[v] + sum_{m: src_m = v} n_m D[rho_m,:] * G[dst_m,:])
//                       * relu'(H), and the dropout-scaled copy
// No float atomics: every sum has a fixed order, two passes over the same inputs give the same bits.
#include "rgcn_internal.h"
#include "row_walk.h"

namespace rgcn {

namespace {

constexpr int kMixLanes = 128;      // 2 B <= 128 mixing scalars per row (B <= 64: rgcn_create)

// ---------------------------------------------------------------- forward: destination-major rows
struct RowArgs {
  const float* Hin;          // [V,d]
  const float* coef;         // [2R][B]
  const float* dtab;         // [2R][d]
  float* Z;                  // compacted [2][V][B*d]
  float* a;                  // [2][V][B]
  float* agg;                // [V,d]
  const int32_t* unit_ptr;   // [2][V+1]
  const int32_t* row_ptr;    // incidence CSR (rows = destinations)
  const int32_t* d_src;      // per slot: source vertex, directed relation, normalisation
  const int32_t* d_rel;
  const float* d_norm;
  const int32_t* long_rows;
  const int32_t* nlong;
  int32_t V, d, B, R;
};

// mixing scalar j = dir * B + b of one row over the slots s0, s0 + step, ... < s1: sum of n C[rel,b] over the slots of dir
__device__ __forceinline__ float mix_range(const RowArgs& a, int s0, int s1, int step, int j) {
  const int dir = j / a.B, b = j - dir * a.B;
  float acc = 0.f;
  for (int s = s0; s < s1; s += step) {
    const int rel = a.d_rel[s];
    if ((rel < a.R ? 0 : 1) == dir) acc = fmaf(a.d_norm[s], a.coef[(size_t)rel * a.B + b], acc);
  }
  return acc;
}

// acc += sum over slots s0, s0 + step, ... < s1 of  n * D[rel,:] * Hin[src,:]   at column vector cidx
template <int VEC>
__device__ __forceinline__ void diag_range(const RowArgs& a, int s0, int s1, int step, int cidx, float (&acc)[VEC]) {
  const size_t col = (size_t)cidx * VEC;
  for (int s = s0; s < s1; s += step) {
    const int src = a.d_src[s], rel = a.d_rel[s];
    const float nrm = a.d_norm[s];
    float x[VEC], t[VEC];
    vload<VEC>(a.Hin + (size_t)src * a.d + col, x);
    vload<VEC>(a.dtab + (size_t)rel * a.d + col, t);
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = fmaf(nrm * t[k], x[k], acc[k]);
  }
}

// the aggregate of row v at column vector cidx, and the row's own unit rows a[dir][b] * Hin[v] where the unit exists
template <int VEC>
__device__ __forceinline__ void row_store(const RowArgs& a, int v, int cidx, const float (&acc)[VEC], const float* mix) {
  const size_t col = (size_t)cidx * VEC;
  vstore<VEC>(a.agg + (size_t)v * a.d + col, acc);
  float h[VEC];
  vload<VEC>(a.Hin + (size_t)v * a.d + col, h);
  for (int dir = 0; dir < 2; ++dir) {
    const int32_t* up = a.unit_ptr + (size_t)dir * (a.V + 1) + v;
    const int u = up[0];
    if (up[1] > u) {
      float* z = a.Z + ((size_t)dir * a.V + u) * a.B * a.d + col;
      for (int b = 0; b < a.B; ++b) {
        const float w = mix[dir * a.B + b];
        float o[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) o[k] = w * h[k];
        vstore<VEC>(z + (size_t)b * a.d, o);
      }
    }
  }
}

// Workgroups [0, n_long_blocks): one LONG row (more than kLongRow slots) at a time, 8 slot lanes x 128 column lanes, the
// eight partial sums added through LDS in lane order -- first for the 2B mixing scalars (column lane = scalar), then per
// 128 column vectors of the aggregate.  The others: TPR lanes per destination row, 1024 / TPR rows each; lane j < 2B forms
// mixing scalar j, the row's lanes meet at a barrier, then every lane takes its column vectors.
template <int VEC, int TPR>
__global__ void __launch_bounds__(kRowThreads) k_pdiag_rows(RowArgs a, int n_long_blocks) {
  const int nvec = a.d / VEC;
  const int nmix = 2 * a.B;
  if ((int)blockIdx.x < n_long_blocks) {
    __shared__ float red[8][128 * VEC];
    __shared__ float mix[kMixLanes];
    const int cl = threadIdx.x & 127, sl = threadIdx.x >> 7;
    const int n = *a.nlong;
    for (int lb = blockIdx.x; lb < n; lb += n_long_blocks) {
      const int v = a.long_rows[lb];
      const int beg = a.row_ptr[v], end = a.row_ptr[v + 1];
      red[sl][cl] = cl < nmix ? mix_range(a, beg + sl, end, 8, cl) : 0.f;
      __syncthreads();
      if (sl == 0 && cl < nmix) {
        const float u = lds_sum8<VEC>(red, cl);
        mix[cl] = u;
        a.a[((size_t)(cl / a.B) * a.V + v) * a.B + cl % a.B] = u;
      }
      __syncthreads();
      for (int c0 = 0; c0 < nvec; c0 += 128) {
        const int cidx = c0 + cl;
        float acc[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
        if (cidx < nvec) diag_range<VEC>(a, beg + sl, end, 8, cidx, acc);
#pragma unroll
        for (int k = 0; k < VEC; ++k) red[sl][cl * VEC + k] = acc[k];
        __syncthreads();
        if (sl == 0 && cidx < nvec) {
#pragma unroll
          for (int k = 0; k < VEC; ++k) acc[k] = lds_sum8<VEC>(red, cl * VEC + k);
          row_store<VEC>(a, v, cidx, acc, mix);
        }
        __syncthreads();
      }
    }
    return;
  }
  __shared__ float mixs[kRowThreads / 64][kMixLanes];
  const int r = threadIdx.x / TPR, lane = threadIdx.x % TPR;
  const int v = ((int)blockIdx.x - n_long_blocks) * (kRowThreads / TPR) + r;
  int beg = 0, end = 0;
  bool active = v < a.V;
  if (active) {
    beg = a.row_ptr[v];
    end = a.row_ptr[v + 1];
    active = end - beg <= kLongRow;      // otherwise a long-row workgroup of this launch owns it
  }
  if (active)
    for (int j = lane; j < nmix; j += TPR) {      // a row without messages writes its zeros: the table is read back whole
      const float u = mix_range(a, beg, end, 1, j);
      mixs[r][j] = u;
      a.a[((size_t)(j / a.B) * a.V + v) * a.B + j % a.B] = u;
    }
  __syncthreads();
  if (!active) return;
  for (int cidx = lane; cidx < nvec; cidx += TPR) {
    float acc[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
    diag_range<VEC>(a, beg, end, 1, cidx, acc);
    row_store<VEC>(a, v, cidx, acc, mixs[r]);
  }
}

// ---------------------------------------------------------------- forward: epilogue
struct EpiArgs {
  const float* prod;         // compacted unit products [2][V][d]
  const float* agg;          // [V,d]
  const float* bias;         // [d]
  const int32_t* unit_ptr;   // [2][V+1]
  CombineArgs c;             // out, base (the self-loop product, dropout `drop`), relu, V, d
};

// one 64-lane group per row, four rows per workgroup
template <int VEC>
__global__ void __launch_bounds__(256) k_pdiag_epilogue(EpiArgs a) {
#pragma clang fp contract(off)
  const int v = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (v >= a.c.V) return;
  const DropKey key = drop_key(a.c.drop);
  const int d = a.c.d, nvec = d / VEC;
  const int uf = a.unit_ptr[v], ub = a.unit_ptr[(size_t)a.c.V + 1 + v];
  const bool has_f = a.unit_ptr[v + 1] > uf, has_b = a.unit_ptr[(size_t)a.c.V + 2 + v] > ub;
  for (int cidx = lane; cidx < nvec; cidx += 64) {
    const size_t col = (size_t)cidx * VEC, off = (size_t)v * d + col;
    float s[VEC], g[VEC], bb[VEC], o[VEC];
    vload<VEC>(a.c.base + off, s);
#pragma unroll
    for (int k = 0; k < VEC; ++k) s[k] *= drop_factor(a.c.drop, key, off + k);
    if (has_f) {      // forward direction first, then backward: a fixed order
      float p[VEC];
      vload<VEC>(a.prod + (size_t)uf * d + col, p);
#pragma unroll
      for (int k = 0; k < VEC; ++k) s[k] += p[k];
    }
    if (has_b) {
      float p[VEC];
      vload<VEC>(a.prod + ((size_t)a.c.V + ub) * d + col, p);
#pragma unroll
      for (int k = 0; k < VEC; ++k) s[k] += p[k];
    }
    vload<VEC>(a.agg + off, g);
    vload<VEC>(a.bias + col, bb);
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      const float pre = (s[k] + g[k]) + bb[k];
      o[k] = a.c.relu ? fmaxf(pre, 0.f) : pre;
    }
    vstore<VEC>(a.c.out + off, o);
  }
}

// ---------------------------------------------------------------- backward: row-local part
struct RowBwdArgs {
  const float* Hin;          // [V,d]
  const float* dZ;           // compacted [2][V][B*d]
  const float* a;            // [2][V][B]
  float* da;                 // [2][V][B]
  float* dh;                 // [V,d]
  const int32_t* unit_ptr;   // [2][V+1]
  int32_t V, d, B;
};

// one wave per row, four rows per workgroup: the B dot products of a direction reduced by shuffles (every lane ends with the
// total: the same tree whatever the lane), then the row's columns
template <int VEC>
__global__ void __launch_bounds__(256) k_pdiag_row_bwd(RowBwdArgs a) {
  const int v = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (v >= a.V) return;      // (whole waves leave: the shuffles below stay inside a wave)
  const int nvec = a.d / VEC;
  const float* h = a.Hin + (size_t)v * a.d;
  const float* z[2];
  bool has[2];
#pragma unroll
  for (int dir = 0; dir < 2; ++dir) {
    const int32_t* up = a.unit_ptr + (size_t)dir * (a.V + 1) + v;
    const int u = up[0];
    has[dir] = up[1] > u;
    z[dir] = a.dZ + ((size_t)dir * a.V + u) * a.B * a.d;
  }
#pragma unroll
  for (int dir = 0; dir < 2; ++dir) {
    float* out = a.da + ((size_t)dir * a.V + v) * a.B;
    if (!has[dir]) {      // the table is read back whole by nobody, but dC's kernel never has to ask whether a unit exists
      for (int b = lane; b < a.B; b += 64) out[b] = 0.f;
      continue;
    }
    for (int b = 0; b < a.B; ++b) {
      float t = 0.f;
      for (int cidx = lane; cidx < nvec; cidx += 64) {
        float x[VEC], y[VEC];
        vload<VEC>(h + (size_t)cidx * VEC, x);
        vload<VEC>(z[dir] + (size_t)b * a.d + (size_t)cidx * VEC, y);
#pragma unroll
        for (int k = 0; k < VEC; ++k) t = fmaf(x[k], y[k], t);
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off, 64);
      if (lane == 0) out[b] = t;
    }
  }
  for (int cidx = lane; cidx < nvec; cidx += 64) {
    float acc[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
#pragma unroll
    for (int dir = 0; dir < 2; ++dir)
      if (has[dir]) {
        const float* w = a.a + ((size_t)dir * a.V + v) * a.B;
        for (int b = 0; b < a.B; ++b) {
          float y[VEC];
          vload<VEC>(z[dir] + (size_t)b * a.d + (size_t)cidx * VEC, y);
          const float wb = w[b];
#pragma unroll
          for (int k = 0; k < VEC; ++k) acc[k] = fmaf(wb, y[k], acc[k]);
        }
      }
    vstore<VEC>(a.dh + (size_t)v * a.d + (size_t)cidx * VEC, acc);
  }
}

// ---------------------------------------------------------------- backward: coefficient and diagonal gradients
struct RelArgs {
  const float* da;           // [2][V][B]            (dcoef)
  const float* Hin;          // [V,d]                (ddiag)
  const float* D;            // [V,d]                (ddiag)
  const int32_t* m_src;      // relation-sorted message list
  const int32_t* m_dst;
  const float* m_norm;
  const int32_t* rel_ptr;
  const int32_t* chunk_ptr;
  float* slab;               // [chunks][B] (dcoef) or [chunks][d] (ddiag)
  int32_t V, R, B, d, chunk;
};

// One workgroup (one wave) per relation chunk; lane b adds the chunk's messages in list order.
__global__ void __launch_bounds__(64) k_pdiag_dcoef(RelArgs a) {
  const int bid = blockIdx.x;
  const int R2 = 2 * a.R;
  if (bid >= a.chunk_ptr[R2]) return;
  const int rel = find_segment(a.chunk_ptr, R2, bid);
  const int beg = a.rel_ptr[rel] + (bid - a.chunk_ptr[rel]) * a.chunk;
  const int end = min(beg + a.chunk, a.rel_ptr[rel + 1]);
  const float* da = a.da + (size_t)(rel < a.R ? 0 : 1) * a.V * a.B;
  const int b = threadIdx.x;      // (B <= 64)
  if (b >= a.B) return;
  float acc = 0.f;
  for (int j = beg; j < end; ++j) acc = fmaf(a.m_norm[j], da[(size_t)a.m_dst[j] * a.B + b], acc);
  a.slab[(size_t)bid * a.B + b] = acc;
}

// One workgroup per relation chunk; every thread owns VEC of the d entries of the chunk's slab row and adds the chunk's
// messages in list order.
template <int VEC>
__global__ void __launch_bounds__(256) k_pdiag_ddiag(RelArgs a) {
  const int bid = blockIdx.x;
  const int R2 = 2 * a.R;
  if (bid >= a.chunk_ptr[R2]) return;
  const int rel = find_segment(a.chunk_ptr, R2, bid);
  const int beg = a.rel_ptr[rel] + (bid - a.chunk_ptr[rel]) * a.chunk;
  const int end = min(beg + a.chunk, a.rel_ptr[rel + 1]);
  for (int e = threadIdx.x * VEC; e < a.d; e += 256 * VEC) {
    float acc[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
    for (int j = beg; j < end; ++j) {
      const float nrm = a.m_norm[j];
      float x[VEC], g[VEC];
      vload<VEC>(a.Hin + (size_t)a.m_src[j] * a.d + e, x);
      vload<VEC>(a.D + (size_t)a.m_dst[j] * a.d + e, g);
#pragma unroll
      for (int k = 0; k < VEC; ++k) acc[k] = fmaf(nrm, x[k] * g[k], acc[k]);
    }
    vstore<VEC>(a.slab + (size_t)bid * a.d + e, acc);
  }
}

// gdtab[rel,:] = the relation's chunk partials in chunk order, compensated like k_basis_dcoef_reduce
__global__ void k_pdiag_ddiag_reduce(const float* __restrict__ slab, const int32_t* __restrict__ chunk_ptr,
                                     float* __restrict__ gdtab, int R2, int d) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)R2 * d) return;
  const int rel = (int)(i / d), e = (int)(i - (int64_t)rel * d);
  float acc = 0.f, comp = 0.f;
  {
#pragma clang fp contract(off)
    for (int c = chunk_ptr[rel]; c < chunk_ptr[rel + 1]; ++c) {
      const float y = slab[(size_t)c * d + e] - comp;
      const float t = acc + y;
      comp = (t - acc) - y;
      acc = t;
    }
  }
  gdtab[i] = acc;
}

// ---------------------------------------------------------------- backward: source-major dH gather + join
struct JoinArgs {
  const float* D;            // [V,d] G = dL/dpre
  const float* dtab;         // [2R][d]
  const float* dh;           // [V,d] the row-local part
  const int32_t* row_ptr;    // incidence CSR (rows = sources)
  const int32_t* s_dst;      // per source-order slot: destination vertex, directed relation, normalisation
  const int32_t* s_rel;
  const float* s_norm;
  const int32_t* long_rows;
  const int32_t* nlong;
  CombineArgs c;             // out = ((base + dh) + gathered) * (gate > 0) ; out2 = out * dropout(drop2)
};

// acc += sum over slots s0, s0 + step, ... < s1 of  n * D[rel,:] * G[dst,:]   at column vector cidx
template <int VEC>
__device__ __forceinline__ void join_range(const JoinArgs& a, int s0, int s1, int step, int cidx, float (&acc)[VEC]) {
  const int d = a.c.d;
  const size_t col = (size_t)cidx * VEC;
  for (int s = s0; s < s1; s += step) {
    const int dst = a.s_dst[s], rel = a.s_rel[s];
    const float nrm = a.s_norm[s];
    float x[VEC], t[VEC];
    vload<VEC>(a.D + (size_t)dst * d + col, x);
    vload<VEC>(a.dtab + (size_t)rel * d + col, t);
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = fmaf(nrm * t[k], x[k], acc[k]);
  }
}

template <int VEC>
__device__ __forceinline__ void join_epilogue(const JoinArgs& a, const DropKey& key, size_t off, const float (&acc)[VEC]) {
#pragma clang fp contract(off)
  float s[VEC], r[VEC];
  vload<VEC>(a.c.base + off, s);
  vload<VEC>(a.dh + off, r);
#pragma unroll
  for (int k = 0; k < VEC; ++k) s[k] = (s[k] + r[k]) + acc[k];
  if (a.c.gate != nullptr) {
    float gt[VEC];
    vload<VEC>(a.c.gate + off, gt);
#pragma unroll
    for (int k = 0; k < VEC; ++k) s[k] = gt[k] > 0.f ? s[k] : 0.f;
  }
  vstore<VEC>(a.c.out + off, s);
  if (a.c.out2 != nullptr) {
    float o2[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) o2[k] = s[k] * drop_factor(a.c.drop2, key, off + k);
    vstore<VEC>(a.c.out2 + off, o2);
  }
}

// the single-accumulator row walk (row_walk.h) over the source rows
template <int VEC, int TPR>
__global__ void __launch_bounds__(kRowThreads) k_pdiag_dh_join(JoinArgs a, int n_long_blocks) {
  const int d = a.c.d;
  const DropKey key = drop_key(a.c.drop2);
  row_walk<VEC, TPR>(
      a.row_ptr, a.long_rows, a.nlong, a.c.V, d / VEC, n_long_blocks,
      [&a](int s0, int s1, int step, int cidx, float (&acc)[VEC]) { join_range<VEC>(a, s0, s1, step, cidx, acc); },
      [&a, &key, d](int v, int cidx, const float (&acc)[VEC]) { join_epilogue<VEC>(a, key, (size_t)v * d + (size_t)cidx * VEC, acc); });
}

}  // namespace

rgcn_status pdiag_rows_forward(rgcn_ctx* c, int layer, const float* Hin, float* Zc, float* amix, float* agg) {
  const LayerBufs& lb = c->layers[layer];
  RowArgs a;
  a.Hin = Hin; a.coef = lb.coef; a.dtab = lb.dtab; a.Z = Zc; a.a = amix; a.agg = agg;
  a.unit_ptr = c->g.unit_ptr; a.row_ptr = c->g.row_ptr; a.d_src = c->g.d_src; a.d_rel = c->g.d_rel; a.d_norm = c->g.d_norm;
  a.long_rows = c->g.long_rows; a.nlong = c->g.nlong;
  a.V = c->V; a.d = c->d; a.B = c->B; a.R = c->R;
  if (2 * c->B > kMixLanes) RGCN_FAIL(c, RGCN_ERR_STATE, "internal: pdiag_rows_forward needs 2 B <= 128");
  const bool vec4 = (c->d % 4 == 0) && aligned16(Hin) && aligned16(a.dtab) && aligned16(Zc) && aligned16(agg);
  const int nvec = vec4 ? c->d / 4 : c->d;
  const int tpr = row_lanes(nvec);
  const int nlb = long_blocks(c);
  dim3 grid = row_grid(nlb, c->V, tpr), block(kRowThreads);
  const double M = 2.0 * c->g.E, units = basis_units(c);
  const double rows = M < c->V ? M : (double)c->V;      // compulsory: each gathered row of H once
  ProfScope ps(c, "pdiag_rows_fwd", 4.0 * c->d * (2.0 * M + c->V + c->B * units) + 12.0 * M + 8.0 * c->V * c->B,
               2.0 * M * (c->d + c->B) + c->B * units * c->d,
               4.0 * c->d * (rows + 2.0 * c->R + c->V + c->B * units) + 12.0 * M + 8.0 * c->V * c->B);
  RGCN_LAUNCH_ROWS(k_pdiag_rows, vec4, tpr, grid, block, c->stream, a, nlb);
  RGCN_HIP(c, hipGetLastError());
  return RGCN_OK;
}

rgcn_status pdiag_epilogue(rgcn_ctx* c, int layer, const float* prod, const float* agg, const CombineArgs& ca) {
  if (ca.base == nullptr || ca.out == nullptr) RGCN_FAIL(c, RGCN_ERR_STATE, "internal: pdiag_epilogue needs base and out");
  EpiArgs a;
  a.prod = prod; a.agg = agg; a.bias = c->layers[layer].bias; a.unit_ptr = c->g.unit_ptr; a.c = ca;
  const bool vec4 = (c->d % 4 == 0) && aligned16(prod) && aligned16(agg) && aligned16(a.bias) && aligned16(ca.base) &&
                    aligned16(ca.out);
  const double Vd = (double)c->V * c->d;
  ProfScope ps(c, "pdiag_epilogue", 4.0 * (3.0 * Vd + basis_units(c) * c->d) + 16.0 * c->V, 4.0 * Vd);
  dim3 grid((unsigned)((c->V + 3) / 4)), block(256);
  if (vec4) hipLaunchKernelGGL((k_pdiag_epilogue<4>), grid, block, 0, c->stream, a);
  else hipLaunchKernelGGL((k_pdiag_epilogue<1>), grid, block, 0, c->stream, a);
  RGCN_HIP(c, hipGetLastError());
  return RGCN_OK;
}

rgcn_status pdiag_row_backward(rgcn_ctx* c, const float* Hin, const float* dZc, const float* amix, float* da, float* dh) {
  RowBwdArgs a;
  a.Hin = Hin; a.dZ = dZc; a.a = amix; a.da = da; a.dh = dh; a.unit_ptr = c->g.unit_ptr;
  a.V = c->V; a.d = c->d; a.B = c->B;
  const bool vec4 = (c->d % 4 == 0) && aligned16(Hin) && aligned16(dZc) && aligned16(dh);
  const double units = basis_units(c);
  ProfScope ps(c, "pdiag_row_bwd", 4.0 * c->d * (2.0 * c->B * units + 2.0 * c->V) + 16.0 * c->V * c->B, 4.0 * units * c->B * c->d,
               4.0 * c->d * (c->B * units + 2.0 * c->V) + 16.0 * c->V * c->B);
  dim3 grid((unsigned)((c->V + 3) / 4)), block(256);
  if (vec4) hipLaunchKernelGGL((k_pdiag_row_bwd<4>), grid, block, 0, c->stream, a);
  else hipLaunchKernelGGL((k_pdiag_row_bwd<1>), grid, block, 0, c->stream, a);
  RGCN_HIP(c, hipGetLastError());
  return RGCN_OK;
}

static RelArgs rel_args(const rgcn_ctx* c) {
  RelArgs a;
  a.da = nullptr; a.Hin = nullptr; a.D = nullptr; a.slab = nullptr;
  a.m_src = c->g.m_src; a.m_dst = c->g.m_dst; a.m_norm = c->g.m_norm;
  a.rel_ptr = c->g.rel_ptr; a.chunk_ptr = c->g.chunk_ptr;
  a.V = c->V; a.R = c->R; a.B = c->B; a.d = c->d; a.chunk = c->g.chunk;
  return a;
}

rgcn_status pdiag_dcoef(rgcn_ctx* c, int layer, const float* da) {
  if (c->g.E > 0) {
    const int nchunks = (int)((2 * c->g.E + c->g.chunk - 1) / c->g.chunk) + 2 * c->R;
    if ((size_t)nchunks > c->pdiag_slab_chunks) RGCN_FAIL(c, RGCN_ERR_STATE, "internal: dC slab too small");
    RelArgs a = rel_args(c);
    a.da = da; a.slab = c->slab_dw;
    const double M = 2.0 * c->g.E;
    ProfScope ps(c, "pdiag_dcoef", 4.0 * c->B * (M + nchunks) + 8.0 * M, 2.0 * M * c->B);
    hipLaunchKernelGGL(k_pdiag_dcoef, dim3(nchunks), dim3(64), 0, c->stream, a);
    RGCN_HIP(c, hipGetLastError());
  }
  return basis_dcoef_reduce(c, layer);      // (an empty graph has no chunks: zeros)
}

rgcn_status pdiag_ddiag(rgcn_ctx* c, int layer, const float* Hin, const float* D) {
  const int R2 = 2 * c->R, d = c->d;
  if (c->g.E > 0) {
    const int nchunks = (int)((2 * c->g.E + c->g.chunk - 1) / c->g.chunk) + R2;
    if ((size_t)nchunks > c->pdiag_slab_chunks) RGCN_FAIL(c, RGCN_ERR_STATE, "internal: dD slab too small");
    RelArgs a = rel_args(c);
    a.Hin = Hin; a.D = D; a.slab = c->pdiag_slab_dd;
    const double M = 2.0 * c->g.E;
    const double rows = M < c->V ? M : (double)c->V;
    ProfScope ps(c, "pdiag_ddiag", 4.0 * d * (2.0 * M + nchunks) + 12.0 * M, 3.0 * M * d,
                 4.0 * d * (2.0 * rows + nchunks) + 12.0 * M);
    if (d % 4 == 0 && aligned16(Hin) && aligned16(D) && aligned16(a.slab))
      hipLaunchKernelGGL((k_pdiag_ddiag<4>), dim3(nchunks), dim3(256), 0, c->stream, a);
    else
      hipLaunchKernelGGL((k_pdiag_ddiag<1>), dim3(nchunks), dim3(256), 0, c->stream, a);
    RGCN_HIP(c, hipGetLastError());
  }
  const int64_t n = (int64_t)R2 * d;
  ProfScope ps(c, "pdiag_ddiag_reduce", 4.0 * (n + 2.0 * c->g.E / c->g.chunk * d + (double)n), 4.0 * n);
  hipLaunchKernelGGL(k_pdiag_ddiag_reduce, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, c->pdiag_slab_dd,
                     c->g.chunk_ptr, c->layers[layer].gdtab, R2, d);
  RGCN_HIP(c, hipGetLastError());
  return RGCN_OK;
}

rgcn_status pdiag_dh_join(rgcn_ctx* c, int layer, const float* D, const float* dh, const CombineArgs& ca) {
  if (ca.base == nullptr || ca.out == nullptr) RGCN_FAIL(c, RGCN_ERR_STATE, "internal: pdiag_dh_join needs base and out");
  JoinArgs a;
  a.D = D; a.dtab = c->layers[layer].dtab; a.dh = dh;
  a.row_ptr = c->g.row_ptr; a.s_dst = c->g.s_dst; a.s_rel = c->g.s_rel; a.s_norm = c->g.s_norm;
  a.long_rows = c->g.long_rows; a.nlong = c->g.nlong; a.c = ca;
  const bool vec4 = (c->d % 4 == 0) && aligned16(D) && aligned16(a.dtab) && aligned16(dh) && aligned16(ca.base) &&
                    aligned16(ca.out) && aligned16(ca.gate) && aligned16(ca.out2);
  const int nvec = vec4 ? c->d / 4 : c->d;
  const int tpr = row_lanes(nvec);
  const int nlb = long_blocks(c);
  dim3 grid = row_grid(nlb, c->V, tpr), block(kRowThreads);
  const double M = 2.0 * c->g.E;
  const double rows = M < c->V ? M : (double)c->V;
  ProfScope ps(c, "pdiag_dh_join", 4.0 * c->d * (2.0 * M + (ca.out2 ? 5.0 : 4.0) * c->V) + 12.0 * M, 3.0 * M * c->d,
               4.0 * c->d * (rows + 2.0 * c->R + (ca.out2 ? 5.0 : 4.0) * c->V) + 12.0 * M);
  RGCN_LAUNCH_ROWS(k_pdiag_dh_join, vec4, tpr, grid, block, c->stream, a, nlb);
  RGCN_HIP(c, hipGetLastError());
  return RGCN_OK;
}

}  // namespace rgcn
