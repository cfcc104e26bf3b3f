// The softmax-over-relations loss term ([Decoder] RelationSoftmaxWeight; rgcn_relation_softmax_device): for every positive
// (s, r, o) of a step the gold relation against all the others at once -- the objective the relation queries
// (rgcn_rank_relation_device) evaluate.  Not in the reference; off unless asked for.
//
//   q_n      = codes[s_n] * codes[o_n]                      (pair_query.h: k_rank_pair's arithmetic)
//   E[n,r']  = q_n . W_relation[r']                         (the NT GEMM of the relation queries)
//   ell_n    = log sum_{r' in C_n} exp(E[n,r']) - E[n,r_n]  (row maximum over C_n subtracted)
//   term     = weight / P * sum_n ell_n
//   G[n,r']  = weight / P * (softmax over C_n at r' - [r' = r_n]),  0 outside C_n
//   dW_relation[r'] += sum_n G[n,r'] q_n                    (TN GEMM, split over the positives)
//   dq_n = sum_r' G[n,r'] W_relation[r']                    (NN GEMM, K = padded R)
//   dcodes[s_n] += dq_n * codes[o_n],  dcodes[o_n] += dq_n * codes[s_n]
// C_n is every relation, or (exclusive) the gold one and those r' for which (s_n, r', o_n) is no known positive.
//
// Nothing [P, R] larger than a chunk is ever held: the positives are walked in chunks of RelsmPlan::chunk rows, every
// chunk adds to the loss and to both gradients in chunk order.  No atomics on floats: the entity side is a segmented
// reduction over a by-entity CSR of the chunk's 2n incidences (rows above kRelsmLongRow in pieces, finished in piece
// order), every other sum is a GEMM's or one thread's.  Two calls return the same bytes.
#include <algorithm>
#include <cmath>

#include "pair_query.h"
#include "rgcn_internal.h"
#include "row_walk.h"

namespace rgcn {

namespace {

__global__ void k_relsm_pair(const float* __restrict__ codes, const int32_t* __restrict__ X, int n, int d,
                             float* __restrict__ Q, int V) {
  const int row = blockIdx.x;
  if (row >= n) return;
  pair_query_row(codes, X, row, d, Q, V);
}

__device__ __forceinline__ float wave_max(float x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x = fmaxf(x, __shfl_xor(x, off, 64));
  return x;
}
// (a butterfly: every lane ends with the same sum, added in the same order)
__device__ __forceinline__ float wave_sum(float x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
  return x;
}

// One wavefront per positive, four per workgroup.  The row's energies are read from E (left as they are) and its
// gradients written to G; lane l owns the relations l, l + 64, ... in every pass, so what the first pass leaves in G (the
// energy, or -inf for a relation outside C_n) is read back by the lane that wrote it.  Under the mask every lane searches
// the index of known positives for its own relations: the searches of a row are independent of each other.
// A positive with an id out of range raises flag 2, one whose label is not 1 raises flag 64; their G rows are zero and
// nothing is dereferenced through a bad id.
__global__ void __launch_bounds__(256) k_relsm_rows(const float* __restrict__ E, float* __restrict__ G,
                                                    const int32_t* __restrict__ X, const float* __restrict__ Y, int n,
                                                    int V, int R, int ld, KnownIndex known, int masked, float scale,
                                                    float* __restrict__ part, int32_t* errflag) {
  __shared__ float red[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row = blockIdx.x * 4 + wave;
  float ell = 0.f;
  if (row < n) {
    const int s = X[3 * row], r = X[3 * row + 1], o = X[3 * row + 2];
    const bool ok = (unsigned)s < (unsigned)V && (unsigned)o < (unsigned)V && (unsigned)r < (unsigned)R;
    const bool positive = Y == nullptr || Y[row] == 1.0f;
    if (lane == 0 && !ok) atomicOr(errflag, 2);
    if (lane == 0 && !positive) atomicOr(errflag, 64);
    const float* e = E + (size_t)row * ld;
    float* g = G + (size_t)row * ld;
    if (!ok || !positive) {
      for (int j = lane; j < R; j += 64) g[j] = 0.f;
    } else {
      float m = -INFINITY;
      for (int j = lane; j < R; j += 64) {
        float x = e[j];
        if (masked && j != r && known_has(known, known_key(s, j, o, V))) x = -INFINITY;
        g[j] = x;
        m = fmaxf(m, x);
      }
      m = wave_max(m);            // finite: the gold relation is always a candidate
      float sum = 0.f;
      for (int j = lane; j < R; j += 64) sum += expf(g[j] - m);
      sum = wave_sum(sum);
      const float inv = 1.0f / sum;
      for (int j = lane; j < R; j += 64) {
        const float p = expf(g[j] - m) * inv;      // 0 outside C_n
        g[j] = scale * (p - (j == r ? 1.0f : 0.0f));
      }
      // C_n = {r_n}: sum = exp(0) = 1 and m = E[n, r_n], so ell_n = 0 and the row of G is 0, exactly
      ell = (logf(sum) + m) - e[r];
    }
  }
  if (lane == 0) red[wave] = ell;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// loss += scale * sum of the row pass's partials (double accumulation, one workgroup, fixed order: k_dec_loss's style)
__global__ void __launch_bounds__(256) k_relsm_loss(const float* __restrict__ part, int nparts, double scale,
                                                    double* __restrict__ loss) {
  __shared__ double red[256];
  double a = 0.0;
  for (int i = threadIdx.x; i < nparts; i += 256) a += part[i];
  red[threadIdx.x] = a;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] += scale * red[0];
}

__global__ void k_relsm_add(const float* __restrict__ dW, float* __restrict__ gWr, int count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) gWr[i] += dW[i];
}

// ---- by-entity CSR of the chunk's 2n incidences: i < n the subject side of positive i, i >= n the object side of i - n
__global__ void k_relsm_keys(const int32_t* __restrict__ X, int n, int V, int R, uint32_t* __restrict__ key) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 2 * n) return;
  const bool subj = i < n;
  const int t = subj ? i : i - n;
  const int s = X[3 * t], r = X[3 * t + 1], o = X[3 * t + 2];
  const bool ok = (unsigned)s < (unsigned)V && (unsigned)o < (unsigned)V && (unsigned)r < (unsigned)R;
  key[i] = ok ? (uint32_t)(subj ? s : o) : (uint32_t)V;      // (a bad row sorts behind the last entity)
}

__device__ __forceinline__ int relsm_lower_bound(const uint32_t* a, int n, uint32_t x) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// row offsets + the long rows and their pieces; the pieces of one row get consecutive ids, so the finishing pass adds
// them in a fixed order whatever order the rows were registered in (k_dec_ptrs' scheme)
__global__ void k_relsm_ptrs(const uint32_t* __restrict__ key_s, int n2, int V, int32_t* __restrict__ row_ptr,
                             int32_t* long_rows, int32_t* long_first, int32_t* long_cnt, int32_t* nlong, int cap,
                             int32_t* piece_row, int32_t* piece_k, int piece_cap) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v > V) return;
  const int beg = relsm_lower_bound(key_s, n2, (uint32_t)v);
  row_ptr[v] = beg;
  if (v == V) return;
  const int end = relsm_lower_bound(key_s, n2, (uint32_t)(v + 1));
  if (end - beg > kRelsmLongRow) {
    const int np = (end - beg + kRelsmPiece - 1) / kRelsmPiece;
    const int i = atomicAdd(nlong, 1);
    const int base = atomicAdd(nlong + 1, np);
    if (i < cap) { long_rows[i] = v; long_first[i] = base; long_cnt[i] = np; }
    for (int k = 0; k < np; ++k)
      if (base + k < piece_cap) { piece_row[base + k] = v; piece_k[base + k] = k; }
  }
}

// slot-ordered incidence arrays: the positive of the slot and the OTHER entity of that positive
__global__ void k_relsm_slots(const int32_t* __restrict__ X, int n, const int32_t* __restrict__ perm,
                              const int32_t* __restrict__ row_ptr, int V, int32_t* __restrict__ e_other,
                              int32_t* __restrict__ e_trip) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= row_ptr[V]) return;            // bad rows sort behind the last entity
  const int i = perm[s];
  const int t = i < n ? i : i - n;
  e_other[s] = i < n ? X[3 * t + 2] : X[3 * t];
  e_trip[s] = t;
}

struct RelsmEntArgs {
  const float* codes;
  const float* dQ;
  const int32_t* row_ptr;
  const int32_t* e_other;
  const int32_t* e_trip;
  const int32_t* long_rows;
  const int32_t* long_first;
  const int32_t* long_cnt;
  const int32_t* nlong;
  const int32_t* piece_row;
  const int32_t* piece_k;
  float* piece_slab;
  float* dcodes;
  int32_t V, d, long_cap, piece_cap;
};

// the slots [s0, s1) of a row at column vector cidx, in slot order: acc += dq[positive] * codes[other]
template <int VEC>
__device__ __forceinline__ void relsm_range(const RelsmEntArgs& a, int s0, int s1, int cidx, float (&acc)[VEC]) {
  int s = s0;
  // four incidences' rows in flight together; the sums keep slot order
  for (; s + 3 < s1; s += 4) {
    float u[4][VEC], g[4][VEC];
    int tr[4], ot[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) { tr[t] = a.e_trip[s + t]; ot[t] = a.e_other[s + t]; }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      vload<VEC>(a.dQ + (size_t)tr[t] * a.d + (size_t)cidx * VEC, g[t]);
      vload<VEC>(a.codes + (size_t)ot[t] * a.d + (size_t)cidx * VEC, u[t]);
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int k = 0; k < VEC; ++k) acc[k] = fmaf(g[t][k], u[t][k], acc[k]);
  }
  for (; s < s1; ++s) {
    float u[VEC], g[VEC];
    vload<VEC>(a.dQ + (size_t)a.e_trip[s] * a.d + (size_t)cidx * VEC, g);
    vload<VEC>(a.codes + (size_t)a.e_other[s] * a.d + (size_t)cidx * VEC, u);
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = fmaf(g[k], u[k], acc[k]);
  }
}

// short rows: one wavefront per entity, four per workgroup; an entity no positive of the chunk touches leaves at once
template <int VEC>
__global__ void __launch_bounds__(256) k_relsm_entity_rows(RelsmEntArgs a) {
  const int lane = threadIdx.x & 63;
  const int v = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (v >= a.V) return;
  const int beg = a.row_ptr[v], end = a.row_ptr[v + 1];
  if (end == beg || end - beg > kRelsmLongRow) return;
  const int nvec = a.d / VEC;
  for (int cidx = lane; cidx < nvec; cidx += 64) {
    float acc[VEC], cur[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
    relsm_range<VEC>(a, beg, end, cidx, acc);
    float* dst = a.dcodes + (size_t)v * a.d + (size_t)cidx * VEC;
    vload<VEC>(dst, cur);
#pragma unroll
    for (int k = 0; k < VEC; ++k) cur[k] += acc[k];
    vstore<VEC>(dst, cur);
  }
}

// one piece (kRelsmPiece slots) of a long row per wavefront, four per workgroup: its partial sum to the piece slab
template <int VEC>
__global__ void __launch_bounds__(256) k_relsm_entity_pieces(RelsmEntArgs a) {
  const int lb = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (lb >= min(a.nlong[1], a.piece_cap)) return;
  const int v = a.piece_row[lb];
  const int beg = a.row_ptr[v] + a.piece_k[lb] * kRelsmPiece;
  const int end = min(a.row_ptr[v + 1], beg + kRelsmPiece);
  const int nvec = a.d / VEC;
  for (int cidx = threadIdx.x & 63; cidx < nvec; cidx += 64) {
    float acc[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
    relsm_range<VEC>(a, beg, end, cidx, acc);
    vstore<VEC>(a.piece_slab + (size_t)lb * a.d + (size_t)cidx * VEC, acc);
  }
}

// long rows: the pieces of every row added in piece order, then added to the row of dL/dcodes
template <int VEC>
__global__ void __launch_bounds__(256) k_relsm_entity_finish(RelsmEntArgs a) {
  const int nvec = a.d / VEC;
  const int n = min(a.nlong[0], a.long_cap);
  for (int i = blockIdx.x; i < n; i += gridDim.x) {
    const int v = a.long_rows[i], first = a.long_first[i], cnt = a.long_cnt[i];
    if (first + cnt > a.piece_cap) continue;      // (cannot happen: the caps are sums of what 2n incidences can form)
    for (int cidx = threadIdx.x; cidx < nvec; cidx += 256) {
      float acc[VEC], part[VEC], cur[VEC];
#pragma unroll
      for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
      for (int p = 0; p < cnt; ++p) {
        vload<VEC>(a.piece_slab + (size_t)(first + p) * a.d + (size_t)cidx * VEC, part);
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[k] += part[k];
      }
      float* dst = a.dcodes + (size_t)v * a.d + (size_t)cidx * VEC;
      vload<VEC>(dst, cur);
#pragma unroll
      for (int k = 0; k < VEC; ++k) cur[k] += acc[k];
      vstore<VEC>(dst, cur);
    }
  }
}

}  // namespace

void relation_softmax_free(rgcn_ctx* c) {
  RelsmBufs& q = c->relsm;
  q.pool.release();
  const float weight = q.weight;
  const int64_t step_positives = q.step_positives;
  const bool exclusive = q.exclusive;
  q = RelsmBufs();
  q.weight = weight; q.step_positives = step_positives; q.exclusive = exclusive;      // (the setting is not the buffers')
}

rgcn_status relation_softmax_reserve(rgcn_ctx* c, int64_t max_positives) {
  RelsmBufs& q = c->relsm;
  if (q.maxP >= max_positives && q.maxP > 0) return RGCN_OK;
  relation_softmax_free(c);
  const RelsmPlan plan = relsm_plan(max_positives, c->R, c->dc, kRelsmSlabFloats);
  const size_t n = (size_t)plan.chunk, Rp = (size_t)plan.padded_r, d = (size_t)c->dc, V = (size_t)c->V;
  RGCN_TRY(dmalloc(c, q.pool, &q.Q, n * d, false));
  RGCN_TRY(dmalloc(c, q.pool, &q.dQ, n * d, false));
  // (zeroed: the pad columns of E and G and the pad rows of Wp are never written and must read as zero)
  RGCN_TRY(dmalloc(c, q.pool, &q.E, n * Rp, true));
  RGCN_TRY(dmalloc(c, q.pool, &q.G, n * Rp, true));
  RGCN_TRY(dmalloc(c, q.pool, &q.Wp, Rp * d, true));
  RGCN_TRY(dmalloc(c, q.pool, &q.dW, Rp * d, false));
  RGCN_TRY(dmalloc(c, q.pool, &q.loss_part, (n + 3) / 4, false));
  // the split-K slabs of dW are the term's own (an embedding context's scratch is one tile; and nothing else shares them)
  q.slab_floats = (size_t)std::max(plan.split_k, 1) * Rp * d;
  RGCN_TRY(dmalloc(c, q.pool, &q.slab, q.slab_floats, false));
  RGCN_TRY(dmalloc(c, q.pool, &q.key, 2 * n, false));
  RGCN_TRY(dmalloc(c, q.pool, &q.key_s, 2 * n, false));
  RGCN_TRY(dmalloc(c, q.pool, &q.key_t, 2 * n, false));
  RGCN_TRY(dmalloc(c, q.pool, &q.perm, 2 * n, false));
  RGCN_TRY(dmalloc(c, q.pool, &q.val_t, 2 * n, false));
  RGCN_TRY(dmalloc(c, q.pool, &q.table, sort_table_elems(2 * n), false));
  RGCN_TRY(dmalloc(c, q.pool, &q.row_ptr, V + 1, false));
  RGCN_TRY(dmalloc(c, q.pool, &q.e_other, 2 * n, false));
  RGCN_TRY(dmalloc(c, q.pool, &q.e_trip, 2 * n, false));
  q.long_cap = (int32_t)(2 * n / kRelsmLongRow + 1);
  q.piece_cap = (int32_t)(2 * n / kRelsmPiece + q.long_cap + 1);      // sum of ceil(len / piece) over the long rows
  RGCN_TRY(dmalloc(c, q.pool, &q.long_rows, (size_t)q.long_cap, false));
  RGCN_TRY(dmalloc(c, q.pool, &q.long_first, (size_t)q.long_cap, false));
  RGCN_TRY(dmalloc(c, q.pool, &q.long_cnt, (size_t)q.long_cap, false));
  RGCN_TRY(dmalloc(c, q.pool, &q.nlong, 2, false));
  RGCN_TRY(dmalloc(c, q.pool, &q.piece_row, (size_t)q.piece_cap, false));
  RGCN_TRY(dmalloc(c, q.pool, &q.piece_k, (size_t)q.piece_cap, false));
  RGCN_TRY(dmalloc(c, q.pool, &q.piece_slab, (size_t)q.piece_cap * d, false));
  q.plan = plan;
  q.maxP = max_positives;
  return RGCN_OK;
}

// The by-entity CSR of n positives (row offsets, long rows and their pieces, slot arrays): it depends on X only.  On the
// current stream.
static rgcn_status relsm_build_csr(rgcn_ctx* c, const int32_t* X, int n) {
  RelsmBufs& q = c->relsm;
  const int V = c->V, R = c->R, T = 256;
  {
    ProfScope ps(c, "relsm_counters_clear", 8.0, 0);
    RGCN_HIP(c, hipMemsetAsync(q.nlong, 0, 2 * sizeof(int32_t), c->stream));
  }
  {
    ProfScope ps(c, "relsm_keys", 20.0 * n, 0);
    hipLaunchKernelGGL(k_relsm_keys, dim3((unsigned)((2 * n + T - 1) / T)), dim3(T), 0, c->stream, X, n, V, R, q.key);
  }
  SortSpec sp{q.key, q.key_s, q.perm, q.key_t, q.val_t, nullptr, q.table, (int64_t)2 * n, (uint32_t)V};
  RGCN_TRY(sort_pairs(c, "relsm_sort", 1, &sp));
  {
    ProfScope ps(c, "relsm_ptrs", 8.0 * V, 0);
    hipLaunchKernelGGL(k_relsm_ptrs, dim3((unsigned)((V + 1 + T - 1) / T)), dim3(T), 0, c->stream, q.key_s, 2 * n, V,
                       q.row_ptr, q.long_rows, q.long_first, q.long_cnt, q.nlong, q.long_cap, q.piece_row, q.piece_k,
                       q.piece_cap);
  }
  {
    ProfScope ps(c, "relsm_slots", 36.0 * n, 0);
    hipLaunchKernelGGL(k_relsm_slots, dim3((unsigned)((2 * n + T - 1) / T)), dim3(T), 0, c->stream, X, n, q.perm, q.row_ptr,
                       V, q.e_other, q.e_trip);
  }
  RGCN_HIP(c, hipGetLastError());
  return RGCN_OK;
}

// The first chunk's CSR ahead of time: a fused step calls this beside decoder_prepare, on the side stream that builds the
// decoder batch's CSRs while the encoder's forward pass runs.  relation_softmax_compute takes it if it is handed the same
// positives, and builds its own otherwise (and for every later chunk).
rgcn_status relation_softmax_prepare(rgcn_ctx* c, const int32_t* pos_dev, int64_t P) {
  RelsmBufs& q = c->relsm;
  q.csr_X = nullptr;
  if (q.maxP <= 0 || P <= 0 || !pos_dev) return RGCN_OK;      // (relation_softmax_compute names what is missing)
  const int n = (int)std::min<int64_t>(q.plan.chunk, P);
  RGCN_TRY(relsm_build_csr(c, pos_dev, n));
  q.csr_X = pos_dev;
  q.csr_n = n;
  return RGCN_OK;
}

rgcn_status relation_softmax_compute(rgcn_ctx* c, const float* codes, const int32_t* pos_dev, const float* Y_dev, int64_t P,
                                     float weight, bool exclusive) {
  RelsmBufs& q = c->relsm;
  const int V = c->V, R = c->R, d = c->dc, Rp = q.plan.padded_r;
  if (q.maxP <= 0) RGCN_FAIL(c, RGCN_ERR_STATE, "call rgcn_relation_softmax_reserve first");
  if (exclusive && c->known.count <= 0) RGCN_FAIL(c, RGCN_ERR_STATE, "call rgcn_known_positives_reserve first");
  const KnownIndex index{exclusive ? c->known.keys : nullptr, exclusive ? c->known.count : 0, V, R};
  const float scale = (float)((double)weight / (double)P);
  const bool vec4 = (d % 4 == 0) && aligned16(codes) && aligned16(q.dQ) && aligned16(c->dcodes_own) && aligned16(q.piece_slab);
  // ProfScope's third argument is the design bytes, its fifth the compulsory bytes; where a pass streams every operand
  // once (everything here but the two gathers) the two are the same figure and the fifth is left to default to the third
  {
    ProfScope ps(c, "relsm_wp_copy", 8.0 * R * d, 0);
    RGCN_HIP(c, hipMemcpyAsync(q.Wp, c->w_rel, sizeof(float) * (size_t)R * d, hipMemcpyDeviceToDevice, c->stream));
  }
  const int T = 256;
  for (int64_t b = 0; b < P; b += q.plan.chunk) {
    const int n = (int)std::min<int64_t>(q.plan.chunk, P - b);
    const int32_t* X = pos_dev + 3 * b;
    const float* Y = Y_dev ? Y_dev + b : nullptr;
    {
      // design: two gathered code rows per positive and the query row written; compulsory: every code row the chunk
      // touches once (at most 2n, at most V) and the query rows
      ProfScope ps(c, "relsm_pair", 4.0 * 3 * n * d, 1.0 * n * d, 4.0 * d * std::min<double>(2.0 * n, V) + 4.0 * n * d + 12.0 * n);
      hipLaunchKernelGGL(k_relsm_pair, dim3((unsigned)n), dim3(128), 0, c->stream, codes, X, n, d, q.Q, V);
    }
    RGCN_TRY(gemm_f32(c, "relsm_energies", true, true, n, R, d, q.Q, d, q.Wp, d, q.E, Rp, 1));
    const int nblocks = (n + 3) / 4;
    {
      // design: the row read once and written once, 12 bytes of the positive (under the mask also R searches of the
      // index per row, 8 bytes a probe, from L2: not in the figure, as for the exclusive samplers)
      ProfScope ps(c, exclusive ? "relsm_rows_masked" : "relsm_rows", 8.0 * n * R + 16.0 * n, 0);
      hipLaunchKernelGGL(k_relsm_rows, dim3((unsigned)nblocks), dim3(256), 0, c->stream, q.E, q.G, X, Y, n, V, R, Rp, index,
                         exclusive ? 1 : 0, scale, q.loss_part, c->g.errflag);
    }
    {
      ProfScope ps(c, "relsm_loss", 4.0 * nblocks + 16.0, 0);
      hipLaunchKernelGGL(k_relsm_loss, dim3(1), dim3(256), 0, c->stream, q.loss_part, nblocks, (double)weight / (double)P,
                         c->dec.loss);
    }
    RGCN_TRY(gemm_f32(c, "relsm_dq", true, false, n, d, Rp, q.G, Rp, q.Wp, d, q.dQ, d, 1));
    {
      // dL/dW_relation is not needed before the optimizer: the LAST chunk's product and its add go to side stream 2, behind
      // the decoder's k_dec_rel_reduce there, and run beside the entity side and the encoder's backward pass (the caller
      // joins it: stream_join(c, 2)).  Earlier chunks stay on the main stream: the next chunk overwrites the G and Q they
      // read.  The slabs are the term's own, so nothing is shared with the backward pass's GEMMs.
      StreamScope side(c, b + q.plan.chunk >= P ? 2 : -1);
      GemmCall dw{false, false, Rp, d, n, q.G, Rp, q.Q, d, q.dW, d, relsm_split(n, Rp, d, q.slab_floats), q.slab, GemmBatch()};
      dw.slab_floats = q.slab_floats;
      RGCN_TRY(gemm_f32(c, "relsm_dw", dw));
      ProfScope ps(c, "relsm_dw_add", 12.0 * R * d, 0);
      hipLaunchKernelGGL(k_relsm_add, dim3((unsigned)((R * d + T - 1) / T)), dim3(T), 0, c->stream, q.dW, c->g_rel, R * d);
    }
    // entity side: the chunk's by-entity CSR, unless relation_softmax_prepare built it beside the encoder's forward pass
    const bool prepared = b == 0 && q.csr_X == X && q.csr_n == n;
    q.csr_X = nullptr;
    if (!prepared) RGCN_TRY(relsm_build_csr(c, X, n));
    RelsmEntArgs a;
    a.codes = codes; a.dQ = q.dQ; a.row_ptr = q.row_ptr; a.e_other = q.e_other; a.e_trip = q.e_trip;
    a.long_rows = q.long_rows; a.long_first = q.long_first; a.long_cnt = q.long_cnt; a.nlong = q.nlong;
    a.piece_row = q.piece_row; a.piece_k = q.piece_k; a.piece_slab = q.piece_slab; a.dcodes = c->dcodes_own;
    a.V = V; a.d = d; a.long_cap = q.long_cap; a.piece_cap = q.piece_cap;
    {
      // design: two row gathers per incidence (2n incidences) + the touched rows read and written; compulsory: the
      // chunk's dQ and the touched code rows once, the touched rows of dL/dcodes read and written
      ProfScope ps(c, "relsm_entity_grad", 16.0 * n * d + 16.0 * n + 16.0 * n * d, 4.0 * n * d,
                   4.0 * n * d + 12.0 * d * std::min<double>(2.0 * n, V) + 16.0 * n);
      const dim3 grid_p((unsigned)((q.piece_cap + 3) / 4)), grid_r((unsigned)((V + 3) / 4)), grid_f(128), block(256);
      if (vec4) {
        hipLaunchKernelGGL((k_relsm_entity_pieces<4>), grid_p, block, 0, c->stream, a);
        hipLaunchKernelGGL((k_relsm_entity_rows<4>), grid_r, block, 0, c->stream, a);
        hipLaunchKernelGGL((k_relsm_entity_finish<4>), grid_f, block, 0, c->stream, a);
      } else {
        hipLaunchKernelGGL((k_relsm_entity_pieces<1>), grid_p, block, 0, c->stream, a);
        hipLaunchKernelGGL((k_relsm_entity_rows<1>), grid_r, block, 0, c->stream, a);
        hipLaunchKernelGGL((k_relsm_entity_finish<1>), grid_f, block, 0, c->stream, a);
      }
    }
    RGCN_HIP(c, hipGetLastError());
    q.last_n = n;
  }
  return RGCN_OK;
}

}  // namespace rgcn
