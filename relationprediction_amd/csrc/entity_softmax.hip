// The softmax-over-entities loss term ([Decoder] EntitySoftmaxWeight; rgcn_entity_softmax_device): for every positive
// (s, r, o) of a step the gold object of (s, r, ?) and the gold subject of (?, r, o) against ALL entities at once -- the
// objective the entity rank queries (rgcn_rank_device) evaluate.  Not in the reference; off unless asked for.
//
// Every positive n < P gives two rows: the object row m = n (query entity a = s_n, gold g = o_n) and the subject row
// m = P + n (a = o_n, g = s_n).  With c the codes and W = W_relation:
//   q_m      = c[a_m] * W[r_m]                              (pair_query.h: k_rank_query's arithmetic)
//   E[m,e]   = q_m . c[e]                                   (the NT GEMM of the entity queries)
//   ell_m    = log sum_{e in C_m} exp(E[m,e]) - E[m,g_m]    (row maximum over C_m subtracted)
//   term     = weight / (2 P) * sum_m ell_m
//   G[m,e]   = weight / (2 P) * (softmax over C_m at e - [e = g_m]),  0 outside C_m
//   dcodes[e]   += sum_m G[m,e] q_m                         (TN GEMM, split over the chunk's rows; one dense add)
//   dq_m = sum_e G[m,e] c[e]                                (NN GEMM, K = V or padded V: entity_softmax_plan.h)
//   dcodes[a_m] += dq_m * W[r_m],   dW_relation[r_m] += dq_m * c[a_m]
// C_m is every entity, or (exclusive) the gold one and those e for which the row's completed triple is no known positive.
//
// Nothing [2P, V] larger than a chunk is ever held, and G overwrites E in place (a row is 58 KB at FB15k-237): the rows
// are walked in chunks of EntsmPlan::chunk, every chunk adds to the loss and to the gradients in chunk order.  No atomics
// on floats: the query side is two segmented reductions over CSRs of the chunk's rows (by query entity, by relation; rows
// above kEntsmLongRow in pieces, finished in piece order), every other sum is a GEMM's or one thread's.  Two calls
// return the same bytes.
//
// The mask SCATTERS: the known entities of a row's pair are one contiguous range of a sorted key array
// (entity_softmax_range.h: two lower-bound searches per row, none per candidate), and the lanes of the row's wavefront
// write -inf over the energies the range names.  A __syncthreads() -- a barrier with workgroup-scope release and acquire
// fences -- stands between those writes and the passes that read the row, so that no lane reads a column another lane
// masked on the strength of wavefront lockstep alone.  Behind it every lane touches its own columns only.
#include <algorithm>
#include <cmath>

#include "entity_softmax_range.h"
#include "pair_query.h"
#include "rgcn_internal.h"
#include "row_walk.h"

namespace rgcn {

namespace {

// Row i of the chunk is row m = m0 + i of the call: (query entity, relation, gold, side) to `rows`, its query to Q.
// A positive with an id out of range raises flag 2, one whose label is not 1 raises flag 64; their gold is recorded as -1
// (the row pass zeroes the row, the reductions skip it) and nothing is dereferenced through a bad id.
__global__ void k_entsm_rows(const float* __restrict__ codes, const float* __restrict__ wrel,
                             const int32_t* __restrict__ X, const float* __restrict__ Y, int64_t P, int64_t m0, int n,
                             int d, int V, int R, float* __restrict__ Q, int32_t* __restrict__ rows, int32_t* errflag) {
  const int i = blockIdx.x;
  if (i >= n) return;
  const int64_t m = m0 + i;
  const int side = m >= P ? 1 : 0;
  const int64_t t = side ? m - P : m;
  const int s = X[3 * t], r = X[3 * t + 1], o = X[3 * t + 2];
  const int a = side ? o : s, g = side ? s : o;
  if (threadIdx.x == 0) {
    const bool ok = (unsigned)s < (unsigned)V && (unsigned)o < (unsigned)V && (unsigned)r < (unsigned)R;
    const bool positive = Y == nullptr || Y[t] == 1.0f;
    if (!ok) atomicOr(errflag, 2);
    if (!positive) atomicOr(errflag, 64);
    rows[4 * i] = a; rows[4 * i + 1] = r; rows[4 * i + 2] = (ok && positive) ? g : -1; rows[4 * i + 3] = side;
  }
  entity_query_row(codes, wrel, a, r, i, d, Q, V, R);
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

// One wavefront per row, four per workgroup; the row's energies become its gradients in place.  ld = padded V, so a row
// is ld / 4 aligned float4; behind the barrier lane l owns the vectors l, l + 64, ... in every pass.  Columns >= V are
// pad: never candidates, written as zero.  Every wavefront reaches the barrier, whatever its row is.
__global__ void __launch_bounds__(256) k_entsm_row_pass(float* __restrict__ E, const int32_t* __restrict__ rows, int n, int V,
                                                        int ld, const uint64_t* __restrict__ keys_by_subject,
                                                        const uint64_t* __restrict__ keys_by_object, int64_t count,
                                                        int masked, float scale, float* __restrict__ part) {
  __shared__ float red[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row = blockIdx.x * 4 + wave;
  const bool active = row < n;
  int a = 0, r = 0, g = -1, side = 0;
  if (active) { a = rows[4 * row]; r = rows[4 * row + 1]; g = rows[4 * row + 2]; side = rows[4 * row + 3]; }
  const bool valid = g >= 0;      // (ids in range, label 1)
  float* e = E + (size_t)(active ? row : 0) * ld;
  if (valid && masked) {
    const uint64_t* keys = side ? keys_by_object : keys_by_subject;
    const uint64_t base = entsm_base(a, r, V);
    const EntsmRange range = entsm_range(keys, count, base, (uint64_t)V);
    for (int64_t i = range.lo + lane; i < range.hi; i += 64) {
      const int j = (int)(keys[i] - base);      // in [0, V): the range holds keys of [base, base + V) only
      if (j != g) e[j] = -INFINITY;             // (the gold entity stays a candidate although it is known)
    }
  }
  __syncthreads();
  float ell = 0.f;
  const int nvec = ld >> 2;
  if (active && !valid) {
    for (int v = lane; v < nvec; v += 64) reinterpret_cast<float4*>(e)[v] = make_float4(0.f, 0.f, 0.f, 0.f);
  } else if (valid) {
    float m = -INFINITY, eg = -INFINITY;
    for (int v = lane; v < nvec; v += 64) {
      const float4 x4 = reinterpret_cast<const float4*>(e)[v];
      const float x[4] = {x4.x, x4.y, x4.z, x4.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int j = 4 * v + k;
        if (j < V) m = fmaxf(m, x[k]);
        if (j == g) eg = x[k];
      }
    }
    m = wave_max(m);              // finite: the gold entity is always a candidate
    eg = wave_max(eg);            // (one lane holds it, the others -inf)
    float sum = 0.f;
    for (int v = lane; v < nvec; v += 64) {
      const float4 x4 = reinterpret_cast<const float4*>(e)[v];
      const float x[4] = {x4.x, x4.y, x4.z, x4.w};
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (4 * v + k < V) sum += expf(x[k] - m);
    }
    sum = wave_sum(sum);
    const float inv = 1.0f / sum;
    for (int v = lane; v < nvec; v += 64) {
      const float4 x4 = reinterpret_cast<const float4*>(e)[v];
      const float x[4] = {x4.x, x4.y, x4.z, x4.w};
      float y[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int j = 4 * v + k;
        const float p = expf(x[k] - m) * inv;      // 0 outside C_m
        y[k] = j < V ? scale * (p - (j == g ? 1.0f : 0.0f)) : 0.f;
      }
      reinterpret_cast<float4*>(e)[v] = make_float4(y[0], y[1], y[2], y[3]);
    }
    // C_m = {g_m}: sum = exp(0) = 1 and m = E[m, g_m], so ell_m = 0 and the row of G is 0, exactly
    ell = (logf(sum) + m) - eg;
  }
  if (lane == 0) red[wave] = ell;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// loss += scale * sum of the row pass's partials (double accumulation, one workgroup, fixed order: k_dec_loss's style)
__global__ void __launch_bounds__(256) k_entsm_loss(const float* __restrict__ part, int nparts, double scale,
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

// the candidate side's dense pass: dcodes[V, d] += dC[V, d]
__global__ void k_entsm_add(const float* __restrict__ dC, float* __restrict__ dcodes, size_t count) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) dcodes[i] += dC[i];
}

// ---- the query side: a CSR of the chunk's n rows by segment (col 0: the query entity, nseg = V; col 1: the relation,
// nseg = R), relation_softmax.hip's by-entity pattern with one incidence per row
__global__ void k_entsm_keys(const int32_t* __restrict__ rows, int n, int col, int nseg, uint32_t* __restrict__ key) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  key[i] = rows[4 * i + 2] >= 0 ? (uint32_t)rows[4 * i + col] : (uint32_t)nseg;      // (a bad row sorts behind the last segment)
}

__device__ __forceinline__ int entsm_lower_bound_u32(const uint32_t* a, int n, uint32_t x) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// segment offsets + the long segments and their pieces; the pieces of one segment get consecutive ids, so the finishing
// pass adds them in a fixed order whatever order the segments were registered in (k_dec_ptrs' scheme)
__global__ void k_entsm_ptrs(const uint32_t* __restrict__ key_s, int n, int nseg, int32_t* __restrict__ row_ptr,
                             int32_t* long_rows, int32_t* long_first, int32_t* long_cnt, int32_t* nlong, int cap,
                             int32_t* piece_row, int32_t* piece_k, int piece_cap) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v > nseg) return;
  const int beg = entsm_lower_bound_u32(key_s, n, (uint32_t)v);
  row_ptr[v] = beg;
  if (v == nseg) return;
  const int end = entsm_lower_bound_u32(key_s, n, (uint32_t)(v + 1));
  if (end - beg > kEntsmLongRow) {
    const int np = (end - beg + kEntsmPiece - 1) / kEntsmPiece;
    const int i = atomicAdd(nlong, 1);
    const int base = atomicAdd(nlong + 1, np);
    if (i < cap) { long_rows[i] = v; long_first[i] = base; long_cnt[i] = np; }
    for (int k = 0; k < np; ++k)
      if (base + k < piece_cap) { piece_row[base + k] = v; piece_k[base + k] = k; }
  }
}

// slot-ordered: the row of the OTHER factor of the slot's chunk row (by entity: its relation; by relation: its entity)
__global__ void k_entsm_slots(const int32_t* __restrict__ rows, const int32_t* __restrict__ perm,
                              const int32_t* __restrict__ row_ptr, int nseg, int other_col, int32_t* __restrict__ e_other) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= row_ptr[nseg]) return;            // bad rows sort behind the last segment
  e_other[s] = rows[4 * perm[s] + other_col];
}

struct EntsmSegArgs {
  const float* other;      // [*, d] the factor table: W_relation (by entity) or the codes (by relation)
  const float* dQ;
  const int32_t* row_ptr;
  const int32_t* e_other;
  const int32_t* e_row;    // the chunk row of every slot (the sort's permutation)
  const int32_t* long_rows;
  const int32_t* long_first;
  const int32_t* long_cnt;
  const int32_t* nlong;
  const int32_t* piece_row;
  const int32_t* piece_k;
  float* piece_slab;
  float* dst;              // [nseg, d] what the sums are added to
  int32_t nseg, d, long_cap, piece_cap;
};

// the slots [s0, s1) of a segment at column vector cidx, in slot order: acc += dq[row] * other[row's factor]
template <int VEC>
__device__ __forceinline__ void entsm_seg_range(const EntsmSegArgs& a, int s0, int s1, int cidx, float (&acc)[VEC]) {
  int s = s0;
  // four slots' rows in flight together; the sums keep slot order
  for (; s + 3 < s1; s += 4) {
    float u[4][VEC], g[4][VEC];
    int tr[4], ot[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) { tr[t] = a.e_row[s + t]; ot[t] = a.e_other[s + t]; }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      vload<VEC>(a.dQ + (size_t)tr[t] * a.d + (size_t)cidx * VEC, g[t]);
      vload<VEC>(a.other + (size_t)ot[t] * a.d + (size_t)cidx * VEC, u[t]);
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int k = 0; k < VEC; ++k) acc[k] = fmaf(g[t][k], u[t][k], acc[k]);
  }
  for (; s < s1; ++s) {
    float u[VEC], g[VEC];
    vload<VEC>(a.dQ + (size_t)a.e_row[s] * a.d + (size_t)cidx * VEC, g);
    vload<VEC>(a.other + (size_t)a.e_other[s] * a.d + (size_t)cidx * VEC, u);
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = fmaf(g[k], u[k], acc[k]);
  }
}

// short segments: one wavefront each, four per workgroup; a segment no row of the chunk touches leaves at once
template <int VEC>
__global__ void __launch_bounds__(256) k_entsm_seg_rows(EntsmSegArgs a) {
  const int lane = threadIdx.x & 63;
  const int v = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (v >= a.nseg) return;
  const int beg = a.row_ptr[v], end = a.row_ptr[v + 1];
  if (end == beg || end - beg > kEntsmLongRow) return;
  const int nvec = a.d / VEC;
  for (int cidx = lane; cidx < nvec; cidx += 64) {
    float acc[VEC], cur[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
    entsm_seg_range<VEC>(a, beg, end, cidx, acc);
    float* dst = a.dst + (size_t)v * a.d + (size_t)cidx * VEC;
    vload<VEC>(dst, cur);
#pragma unroll
    for (int k = 0; k < VEC; ++k) cur[k] += acc[k];
    vstore<VEC>(dst, cur);
  }
}

// one piece (kEntsmPiece slots) of a long segment per wavefront, four per workgroup: its partial sum to the piece slab
template <int VEC>
__global__ void __launch_bounds__(256) k_entsm_seg_pieces(EntsmSegArgs a) {
  const int lb = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (lb >= min(a.nlong[1], a.piece_cap)) return;
  const int v = a.piece_row[lb];
  const int beg = a.row_ptr[v] + a.piece_k[lb] * kEntsmPiece;
  const int end = min(a.row_ptr[v + 1], beg + kEntsmPiece);
  const int nvec = a.d / VEC;
  for (int cidx = threadIdx.x & 63; cidx < nvec; cidx += 64) {
    float acc[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
    entsm_seg_range<VEC>(a, beg, end, cidx, acc);
    vstore<VEC>(a.piece_slab + (size_t)lb * a.d + (size_t)cidx * VEC, acc);
  }
}

// long segments: the pieces of every segment added in piece order, then added to the segment's row of dst
template <int VEC>
__global__ void __launch_bounds__(256) k_entsm_seg_finish(EntsmSegArgs a) {
  const int nvec = a.d / VEC;
  const int n = min(a.nlong[0], a.long_cap);
  for (int i = blockIdx.x; i < n; i += gridDim.x) {
    const int v = a.long_rows[i], first = a.long_first[i], cnt = a.long_cnt[i];
    if (first + cnt > a.piece_cap) continue;      // (cannot happen: the caps are sums of what n rows can form)
    for (int cidx = threadIdx.x; cidx < nvec; cidx += 256) {
      float acc[VEC], part[VEC], cur[VEC];
#pragma unroll
      for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
      for (int p = 0; p < cnt; ++p) {
        vload<VEC>(a.piece_slab + (size_t)(first + p) * a.d + (size_t)cidx * VEC, part);
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[k] += part[k];
      }
      float* dst = a.dst + (size_t)v * a.d + (size_t)cidx * VEC;
      vload<VEC>(dst, cur);
#pragma unroll
      for (int k = 0; k < VEC; ++k) cur[k] += acc[k];
      vstore<VEC>(dst, cur);
    }
  }
}

}  // namespace

void entity_softmax_free(rgcn_ctx* c) {
  EntsmBufs& q = c->entsm;
  q.pool.release();
  const float weight = q.weight;
  const int64_t step_positives = q.step_positives;
  const bool exclusive = q.exclusive;
  q = EntsmBufs();
  q.weight = weight; q.step_positives = step_positives; q.exclusive = exclusive;      // (the setting is not the buffers')
}

rgcn_status entity_softmax_reserve(rgcn_ctx* c, int64_t max_positives) {
  EntsmBufs& q = c->entsm;
  if (q.maxP >= max_positives && q.maxP > 0) return RGCN_OK;
  entity_softmax_free(c);
  const EntsmPlan plan = entsm_plan(max_positives, c->V, c->dc, kEntsmSlabFloats);
  const size_t n = (size_t)plan.chunk, Vp = (size_t)plan.padded_v, d = (size_t)c->dc;
  const size_t nseg = (size_t)std::max(c->V, c->R);
  RGCN_TRY(dmalloc(c, q.pool, &q.Q, n * d, false));
  RGCN_TRY(dmalloc(c, q.pool, &q.dQ, n * d, false));
  // (zeroed: the pad columns of E / G and the pad rows of Cp are never written by a product and must read as zero)
  RGCN_TRY(dmalloc(c, q.pool, &q.E, n * Vp, true));
  if (plan.nn_padded) RGCN_TRY(dmalloc(c, q.pool, &q.Cp, Vp * d, true));
  RGCN_TRY(dmalloc(c, q.pool, &q.dC, Vp * d, false));
  RGCN_TRY(dmalloc(c, q.pool, &q.loss_part, (n + 3) / 4, false));
  // the split-K slabs of dC are the term's own (an embedding context's scratch is one tile; and nothing else shares them)
  q.slab_floats = plan.split_k > 1 ? (size_t)plan.split_k * Vp * d : 4;
  RGCN_TRY(dmalloc(c, q.pool, &q.slab, q.slab_floats, false));
  RGCN_TRY(dmalloc(c, q.pool, &q.rows, 4 * n, false));
  RGCN_TRY(dmalloc(c, q.pool, &q.key, n, false));
  RGCN_TRY(dmalloc(c, q.pool, &q.key_s, n, false));
  RGCN_TRY(dmalloc(c, q.pool, &q.key_t, n, false));
  RGCN_TRY(dmalloc(c, q.pool, &q.perm, n, false));
  RGCN_TRY(dmalloc(c, q.pool, &q.val_t, n, false));
  RGCN_TRY(dmalloc(c, q.pool, &q.table, sort_table_elems(n), false));
  RGCN_TRY(dmalloc(c, q.pool, &q.row_ptr, nseg + 1, false));
  RGCN_TRY(dmalloc(c, q.pool, &q.e_other, n, false));
  q.long_cap = (int32_t)(n / kEntsmLongRow + 1);
  q.piece_cap = (int32_t)(n / kEntsmPiece + q.long_cap + 1);      // sum of ceil(len / piece) over the long segments
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

// One segmented reduction of the chunk's n rows, on the current stream: dst[seg] += sum over the segment's rows, in row
// order, of dq[row] * other[the row's other factor].  col: the column of `rows` that names the segment (0 the query
// entity, 1 the relation); the other factor is the other column.
static rgcn_status entsm_reduce(rgcn_ctx* c, const char* tag, int n, int col, int nseg, const float* other, float* dst) {
  EntsmBufs& q = c->entsm;
  const int d = c->dc, T = 256;
  {
    ProfScope ps(c, "entsm_counters_clear", 8.0, 0);
    RGCN_HIP(c, hipMemsetAsync(q.nlong, 0, 2 * sizeof(int32_t), c->stream));
  }
  {
    ProfScope ps(c, "entsm_keys", 20.0 * n, 0);
    hipLaunchKernelGGL(k_entsm_keys, dim3((unsigned)((n + T - 1) / T)), dim3(T), 0, c->stream, q.rows, n, col, nseg, q.key);
  }
  SortSpec sp{q.key, q.key_s, q.perm, q.key_t, q.val_t, nullptr, q.table, (int64_t)n, (uint32_t)nseg};
  RGCN_TRY(sort_pairs(c, "entsm_sort", 1, &sp));
  {
    ProfScope ps(c, "entsm_ptrs", 8.0 * nseg, 0);
    hipLaunchKernelGGL(k_entsm_ptrs, dim3((unsigned)((nseg + 1 + T - 1) / T)), dim3(T), 0, c->stream, q.key_s, n, nseg,
                       q.row_ptr, q.long_rows, q.long_first, q.long_cnt, q.nlong, q.long_cap, q.piece_row, q.piece_k,
                       q.piece_cap);
  }
  {
    ProfScope ps(c, "entsm_slots", 12.0 * n, 0);
    hipLaunchKernelGGL(k_entsm_slots, dim3((unsigned)((n + T - 1) / T)), dim3(T), 0, c->stream, q.rows, q.perm, q.row_ptr,
                       nseg, 1 - col, q.e_other);
  }
  EntsmSegArgs a;
  a.other = other; a.dQ = q.dQ; a.row_ptr = q.row_ptr; a.e_other = q.e_other; a.e_row = q.perm;
  a.long_rows = q.long_rows; a.long_first = q.long_first; a.long_cnt = q.long_cnt; a.nlong = q.nlong;
  a.piece_row = q.piece_row; a.piece_k = q.piece_k; a.piece_slab = q.piece_slab; a.dst = dst;
  a.nseg = nseg; a.d = d; a.long_cap = q.long_cap; a.piece_cap = q.piece_cap;
  const bool vec4 = (d % 4 == 0) && aligned16(other) && aligned16(q.dQ) && aligned16(dst) && aligned16(q.piece_slab);
  {
    // design: two row gathers per chunk row + the touched rows of dst read and written
    ProfScope ps(c, tag, 8.0 * n * d + 8.0 * n + 8.0 * d * std::min<double>(n, nseg), 2.0 * n * d);
    const dim3 grid_p((unsigned)((q.piece_cap + 3) / 4)), grid_r((unsigned)((nseg + 3) / 4)), grid_f(128), block(256);
    if (vec4) {
      hipLaunchKernelGGL((k_entsm_seg_pieces<4>), grid_p, block, 0, c->stream, a);
      hipLaunchKernelGGL((k_entsm_seg_rows<4>), grid_r, block, 0, c->stream, a);
      hipLaunchKernelGGL((k_entsm_seg_finish<4>), grid_f, block, 0, c->stream, a);
    } else {
      hipLaunchKernelGGL((k_entsm_seg_pieces<1>), grid_p, block, 0, c->stream, a);
      hipLaunchKernelGGL((k_entsm_seg_rows<1>), grid_r, block, 0, c->stream, a);
      hipLaunchKernelGGL((k_entsm_seg_finish<1>), grid_f, block, 0, c->stream, a);
    }
  }
  RGCN_HIP(c, hipGetLastError());
  return RGCN_OK;
}

rgcn_status entity_softmax_compute(rgcn_ctx* c, const float* codes, const int32_t* pos_dev, const float* Y_dev, int64_t P,
                                   float weight, bool exclusive) {
  EntsmBufs& q = c->entsm;
  const int V = c->V, R = c->R, d = c->dc, Vp = q.plan.padded_v;
  if (q.maxP <= 0) RGCN_FAIL(c, RGCN_ERR_STATE, "call rgcn_entity_softmax_reserve first");
  if (exclusive && c->known.count <= 0) RGCN_FAIL(c, RGCN_ERR_STATE, "call rgcn_known_positives_reserve first");
  const int64_t total = 2 * P;
  const float scale = (float)((double)weight / (double)total);
  const float* nn_b = codes;      // B of the NN product, [K, d]
  int nn_k = V;
  if (q.plan.nn_padded) {
    ProfScope ps(c, "entsm_codes_copy", 8.0 * V * d, 0);
    RGCN_HIP(c, hipMemcpyAsync(q.Cp, codes, sizeof(float) * (size_t)V * d, hipMemcpyDeviceToDevice, c->stream));
    nn_b = q.Cp;
    nn_k = Vp;
  }
  const int T = 256;
  for (int64_t b = 0; b < total; b += q.plan.chunk) {
    const int n = (int)std::min<int64_t>(q.plan.chunk, total - b);
    {
      // design: two gathered rows per chunk row and the query row written
      ProfScope ps(c, "entsm_rows", 4.0 * 3 * n * d + 28.0 * n, 1.0 * n * d);
      hipLaunchKernelGGL(k_entsm_rows, dim3((unsigned)n), dim3(128), 0, c->stream, codes, c->w_rel, pos_dev, Y_dev, P, b, n, d, V,
                         R, q.Q, q.rows, c->g.errflag);
    }
    RGCN_TRY(gemm_f32(c, "entsm_energies", true, true, n, V, d, q.Q, d, codes, d, q.E, Vp, 1));
    const int nblocks = (n + 3) / 4;
    {
      // design: the row read three times and written once (the later reads from L2: a row is 4 V bytes), 16 bytes of the
      // row's record; under the mask two searches of the index per row and one store per known entity of its pair
      ProfScope ps(c, exclusive ? "entsm_row_pass_masked" : "entsm_row_pass", 16.0 * n * Vp + 16.0 * n, 0, 8.0 * n * Vp + 16.0 * n);
      hipLaunchKernelGGL(k_entsm_row_pass, dim3((unsigned)nblocks), dim3(256), 0, c->stream, q.E, q.rows, n, V, Vp,
                         exclusive ? c->known.keys : nullptr, exclusive ? c->known.keys_by_object : nullptr,
                         exclusive ? c->known.count : (int64_t)0, exclusive ? 1 : 0, scale, q.loss_part);
    }
    {
      ProfScope ps(c, "entsm_loss", 4.0 * nblocks + 16.0, 0);
      hipLaunchKernelGGL(k_entsm_loss, dim3(1), dim3(256), 0, c->stream, q.loss_part, nblocks, (double)weight / (double)total,
                         c->dec.loss);
    }
    RGCN_TRY(gemm_f32(c, "entsm_dq", true, false, n, d, nn_k, q.E, Vp, nn_b, d, q.dQ, d, 1));
    {
      // the candidate side: dC = G^T Q over the chunk's rows (pad rows of dC come out zero: G's pad columns are), then
      // one dense add.  The slabs are the term's own.
      GemmCall dc{false, false, Vp, d, n, q.E, Vp, q.Q, d, q.dC, d, entsm_split(n, Vp, d, q.slab_floats), q.slab, GemmBatch()};
      dc.slab_floats = q.slab_floats;
      RGCN_TRY(gemm_f32(c, "entsm_dc", dc));
      const size_t count = (size_t)V * d;
      ProfScope ps(c, "entsm_dc_add", 12.0 * V * d, 0);
      hipLaunchKernelGGL(k_entsm_add, dim3((unsigned)((count + T - 1) / T)), dim3(T), 0, c->stream, q.dC, c->dcodes_own, count);
    }
    // the query side: by query entity into dL/dcodes, by relation into dL/dW_relation
    RGCN_TRY(entsm_reduce(c, "entsm_entity_grad", n, 0, V, c->w_rel, c->dcodes_own));
    RGCN_TRY(entsm_reduce(c, "entsm_relation_grad", n, 1, R, codes, c->g_rel));
    RGCN_HIP(c, hipGetLastError());
    q.last_n = n;
  }
  return RGCN_OK;
}

}  // namespace rgcn
