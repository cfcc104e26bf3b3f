// Link-prediction ranking on the device: the evaluation half of the reference's scoring path.
//
// Reference: BilinearDiag.predict_all_subject_scores / predict_all_object_scores
// (code/decoders/bilinear_diag.py:51-61) give, for every query triple, sigmoid(energy) against EVERY entity;
// Scorer.evaluate_mrr + MrrScore.append_line (code/common/evaluation.py:148-153, 349-389) turn each row into
//     raw rank      = #{e : score[e] >= score[gold]}
//     filtered rank = raw rank - #{e in known : score[e] >= score[gold]} + 1
// where `known` are the entities that complete a triple seen in train / valid / test for the same
// (entity, relation) pair (the gold entity among them).  The reference encodes the full graph again for
// every chunk of 1000 triples and ranks in numpy; here the codes of the last rgcn_forward (test mode on the
// full graph) are reused, the [queries, V] energies come from one NT GEMM per chunk, and one workgroup per
// query counts both ranks.
//
// Ties: the comparison is made on fp32 sigmoid values, as in the reference, so that energies that
// saturate to the same float tie (and count against the gold entity).  The sigmoid is evaluated in double
// and rounded once to float — reproducible on the host (oracle.distmult_ranks does the same).
// Round 4: that sigmoid is monotone in the energy, so  score[e] >= score[gold]  <=>  energy[e] >= t  with t the
// SMALLEST float whose score reaches the gold score; t is found once per query by bisection over the ordered float
// bit patterns (32 sigmoids per query) and the [queries, V] pass compares energies -- 64 thousand double-precision
// exponentials per 2,000 queries instead of 58 million, the same counts bit for bit.
//
// Ensemble ranks (rgcn_rank_mixed_device; the reference's code/tools/ensemble.py, WeightEnsemble.combine_prediction): the
// rank is taken on  m = w sigmoid(own energy) + (1 - w) sigmoid(partner energy),  the partner's [queries, V] energies being
// another model's RGCN_BUF_RANK_ENERGIES (or any device buffer of that shape).  The threshold bisection above does NOT carry
// over: m is monotone in each energy but is a function of two, so no single threshold on either energy separates the
// entities that reach the gold's mixed score from those that do not.  k_rank_rows_mixed therefore evaluates both sigmoids
// for every entity -- two double-precision exponentials where k_rank_rows evaluates none -- on rows read once, coalesced.
//
// Top-k prediction (rgcn_topk_device) selects from the same energies: same query kernel, same GEMM, same buffers; one
// workgroup per query picks and orders the k best entities that its exclusion list leaves (k_topk_rows below).
//
// Ensemble top-k (rgcn_topk_mixed_device) is the two together: k_mix_rows writes m for every entity of every query into a
// scratch of its own, through the mixed_score k_rank_rows_mixed compares with, and k_topk_rows selects from that scratch
// exactly as it selects from energies (it orders any floats).  rgcn_score_queries_device is how the partner produces its
// energies for queries that have no gold entity: the shared scoring and nothing after it.
//
// One scoring path: all calls are run_queries (bottom of the file) -- clear the verdict and launch k_rank_check,
// then per chunk score_chunk (k_rank_query + the NT GEMM into ranking.q / ranking.s) and the call's own tail, then read
// the verdict back -- and differ in the tail they hand it.  The two rank kernels are wrappers round one row template
// (rank_row) and differ in the comparison they hand it.
//
// Relation queries (rgcn_rank_relation_device, rgcn_topk_relation_device, rgcn_score_relation_queries_device): which
// relation holds between s and o.  The same path with another candidate table: side SIDE_RELATION makes k_rank_check read
// (s, o) as the given ids and r as the gold one, score_chunk form P = codes[s] * codes[o] (k_rank_pair) and multiply it
// with W_relation instead of the codes -- the same NT GEMM, N = R -- into ranking.rel, a [reserved queries, R] buffer of
// its own (ranking.s is never touched), and the tails run k_rank_threshold / k_rank_rows / k_topk_rows as they stand,
// with R where the entity side passes V: candidate count, row stride, range of the list entries, bits of the mask.
#include "pair_query.h"
#include "rgcn_internal.h"

namespace rgcn {

namespace {

// What a query asks for: the values of the entity sides are the entries' predict_object.  The candidates fill one column
// of the (s, r, o) rows -- the gold id of a rank query sits there, the top-k forms never read it -- and the two others
// are given.
enum : int { SIDE_SUBJECT = 0, SIDE_OBJECT = 1, SIDE_RELATION = 2 };
__host__ __device__ inline int gold_column(int side) { return side == SIDE_OBJECT ? 2 : side == SIDE_RELATION ? 1 : 0; }

__device__ __forceinline__ float sigmoid_f32(float x) {
  return (float)(1.0 / (1.0 + exp(-(double)x)));
}

// Q[n,:] = codes[s_n] * W_rel[r_n]  (object side)   or   W_rel[r_n + shift] * codes[o_n]  (subject side)
// shift: R on the subject side under reciprocal relations (rgcn_set_reciprocal_relations), else 0: the relation id is held
// to [0, R) as it always was, then moved to the inverse relation's row
__global__ void k_rank_query(const float* __restrict__ codes, const float* __restrict__ wrel,
                             const int32_t* __restrict__ X, int n, int d, int predict_object,
                             float* __restrict__ Q, int V, int R, int shift) {
  const int row = blockIdx.x;
  if (row >= n) return;
  // (an id out of range makes the whole call fail -- k_rank_check, read back at the end; until then nothing may fault;
  // pair_query.h holds the arithmetic, shared with the entity-softmax term)
  int rel = X[3 * row + 1];
  if ((unsigned)rel >= (unsigned)R) rel = 0;
  entity_query_row(codes, wrel, X[3 * row + (predict_object ? 0 : 2)], rel + shift, row, d, Q, V, R + shift);
}

// P[n,:] = codes[s_n] * codes[o_n]: the relation side's query row, one rounding per element
__global__ void k_rank_pair(const float* __restrict__ codes, const int32_t* __restrict__ X, int n, int d,
                            float* __restrict__ P, int V) {
  const int row = blockIdx.x;
  if (row >= n) return;
  // (as in k_rank_query: a bad id fails the call at the end and must not fault before; pair_query.h holds the arithmetic,
  // shared with the relation-softmax term)
  pair_query_row(codes, X, row, d, P, V);
}

// floats in their numeric order as unsigned integers (and back)
__device__ __forceinline__ uint32_t float_key(float x) {
  const uint32_t b = __float_as_uint(x);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key_float(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// thr[row] = the smallest float energy whose fp32 sigmoid is >= the gold candidate's: one thread per query.  V: the
// candidates of a row (and its stride); gold_col: the column of X that holds the gold id (gold_column)
__global__ void k_rank_threshold(const float* __restrict__ S, int V, const int32_t* __restrict__ X, int n,
                                 int gold_col, float* __restrict__ thr) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n) return;
  int gold = X[3 * row + gold_col];
  if ((unsigned)gold >= (unsigned)V) gold = 0;
  const float xg = S[(size_t)row * V + gold];
  const float g = sigmoid_f32(xg);
  uint32_t lo = float_key(-INFINITY), hi = float_key(xg);      // sigmoid(hi) >= g always; sigmoid(-inf) = 0
  if (sigmoid_f32(-INFINITY) >= g) {
    thr[row] = -INFINITY;                                        // the gold score is 0: everything ties with it
    return;
  }
  while (hi - lo > 1u) {                                         // invariant: score(lo) < g <= score(hi)
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (sigmoid_f32(key_float(mid)) >= g) hi = mid; else lo = mid;
  }
  thr[row] = key_float(hi);
}

// Both ranks of ONE query row, by one workgroup of four wave64s: reaches(e) says whether entity e scores at least what the
// gold entity does.  The row is walked once (lane-consecutive entities), the filter list 256 entries at a time, and the two
// integer counts are summed by shuffles inside each wave and through eight LDS words across the four.
template <class Reaches>
__device__ __forceinline__ void rank_row(int row, int V, Reaches reaches, const int64_t* __restrict__ filt_ptr,
                                         const int32_t* __restrict__ filt_idx, const int64_t* __restrict__ filt_end,
                                         int32_t* __restrict__ raw_rank, int32_t* __restrict__ filt_rank,
                                         int32_t* __restrict__ bad) {
  __shared__ int red[2][4];
  int cnt = 0, fcnt = 0;
  for (int e = threadIdx.x; e < V; e += 256) cnt += reaches(e) ? 1 : 0;
  int64_t fb = filt_ptr[row], fe = filt_ptr[row + 1];
  // a negative, decreasing or overlong range (k_rank_check has flagged it: the call fails) is not walked at all --
  // nothing may fault before the verdict is read back
  if (fb < 0 || fe < fb || fe > *filt_end) fb = fe = 0;
  bool oob = false;          // a filter entry out of range fails the call and is never dereferenced
  for (int64_t j = fb + threadIdx.x; j < fe; j += 256) {
    const int fi = filt_idx[j];
    const bool in = (unsigned)fi < (unsigned)V;
    oob = oob || !in;
    if (in) fcnt += reaches(fi) ? 1 : 0;
  }
  if (oob) atomicAdd(bad, 1);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    cnt += __shfl_down(cnt, off);
    fcnt += __shfl_down(fcnt, off);
  }
  if ((threadIdx.x & 63u) == 0) {
    red[0][threadIdx.x >> 6] = cnt;
    red[1][threadIdx.x >> 6] = fcnt;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int raw = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    raw_rank[row] = raw;
    filt_rank[row] = raw - (red[1][0] + red[1][1] + red[1][2] + red[1][3]) + 1;
  }
}

// (the wrappers' lambdas capture their scalars by value)
__global__ void __launch_bounds__(256)
k_rank_rows(const float* __restrict__ S, int V, int n, const int64_t* __restrict__ filt_ptr,
            const int32_t* __restrict__ filt_idx, const float* __restrict__ thr, int32_t* __restrict__ raw_rank,
            int32_t* __restrict__ filt_rank, int32_t* __restrict__ bad, const int64_t* __restrict__ filt_end) {
  const int row = blockIdx.x;
  if (row >= n) return;
  const float* s = S + (size_t)row * V;
  const float t = thr[row];
  rank_row(row, V, [=](int e) { return s[e] >= t; }, filt_ptr, filt_idx, filt_end, raw_rank, filt_rank, bad);
}

// The type-constrained twin (rgcn_rank_typed_device): the candidates of a row are the members of list side R + r and the
// gold entity.  The same lambda serves the filter loop, so a filter entry outside the candidates is not subtracted.  The 32
// lanes that walk consecutive entities read one mask word (one address per half wave, from L1 / L2: 1/32 of the row's bytes).
__global__ void __launch_bounds__(256)
k_rank_rows_typed(const float* __restrict__ S, int V, int n, const int32_t* __restrict__ X, int side, int R,
                  const uint32_t* __restrict__ type_mask, int words, const int64_t* __restrict__ filt_ptr,
                  const int32_t* __restrict__ filt_idx, const float* __restrict__ thr, int32_t* __restrict__ raw_rank,
                  int32_t* __restrict__ filt_rank, int32_t* __restrict__ bad, const int64_t* __restrict__ filt_end) {
  const int row = blockIdx.x;
  if (row >= n) return;
  const float* s = S + (size_t)row * V;
  const float t = thr[row];
  int rel = X[3 * row + 1], gold = X[3 * row + gold_column(side)];
  if ((unsigned)rel >= (unsigned)R) rel = 0;        // (k_rank_check has flagged it: the call fails, nothing may fault)
  if ((unsigned)gold >= (unsigned)V) gold = 0;
  const uint32_t* m = type_mask + ((size_t)side * R + rel) * words;
  rank_row(row, V, [=](int e) { return (((m[e >> 5] >> (e & 31)) & 1u) || e == gold) && s[e] >= t; }, filt_ptr, filt_idx,
           filt_end, raw_rank, filt_rank, bad);
}

// m = (float)(w s_a + (1 - w) s_b), both products and the sum in double, rounded once: numpy's float64 expression gives the
// same bits (no fused multiply-add: a contraction would round the first product differently from the host)
__device__ __forceinline__ float mixed_score(double w, float ea, float eb) {
#pragma clang fp contract(off)
  const double a = w * (double)sigmoid_f32(ea);
  const double b = (1.0 - w) * (double)sigmoid_f32(eb);
  return (float)(a + b);
}

// Sb = the partner's rows, same queries in the same order, row stride V
__global__ void __launch_bounds__(256)
k_rank_rows_mixed(const float* __restrict__ Sa, const float* __restrict__ Sb, int V, const int32_t* __restrict__ X, int n,
                  int predict_object, double w, const int64_t* __restrict__ filt_ptr, const int32_t* __restrict__ filt_idx,
                  int32_t* __restrict__ raw_rank, int32_t* __restrict__ filt_rank, int32_t* __restrict__ bad,
                  const int64_t* __restrict__ filt_end) {
  const int row = blockIdx.x;
  if (row >= n) return;
  const float* a = Sa + (size_t)row * V;
  const float* b = Sb + (size_t)row * V;
  int gold = X[3 * row + (predict_object ? 2 : 0)];
  if ((unsigned)gold >= (unsigned)V) gold = 0;      // (k_rank_check has flagged it: the call fails, nothing may fault)
  const float mg = mixed_score(w, a[gold], b[gold]);
  rank_row(row, V, [=](int e) { return mixed_score(w, a[e], b[e]) >= mg; }, filt_ptr, filt_idx, filt_end, raw_rank,
           filt_rank, bad);
}

// M[row, e] = mixed_score(w, Sa[row, e], Sb[row, e]): the mixed scores rgcn_topk_mixed_device selects from, the very
// floats k_rank_rows_mixed compares.  Its shape -- one workgroup of four wave64s per query, both energy rows read once with
// lane-consecutive entities -- and its cost, two double-precision exponentials per entity; the one write is the addition.
__global__ void __launch_bounds__(256)
k_mix_rows(const float* __restrict__ Sa, const float* __restrict__ Sb, int V, int n, double w, float* __restrict__ M) {
  const int row = blockIdx.x;
  if (row >= n) return;
  const float* a = Sa + (size_t)row * V;
  const float* b = Sb + (size_t)row * V;
  float* m = M + (size_t)row * V;
  for (int e = threadIdx.x; e < V; e += 256) m[e] = mixed_score(w, a[e], b[e]);
}

// The ids of a query that its call reads -- the given entity and the relation, and the gold entity where there is one
// (with_gold: the rank forms; the top-k forms never look at the predicted column) -- and the ranges of its filter or
// exclusion list, which may be absent (the last entry of list_ptr is the list's declared length: no range may end
// beyond it).  The list's entries are range-checked where they are read, 256 lanes wide, in the row kernels: one thread
// walking a list of 1,700 entries here was most of a call's time on the subject side of FB15k-237.
// The relation form (side SIDE_RELATION): both entities are given, the gold id is the relation.
__global__ void k_rank_check(const int32_t* __restrict__ X, int n, int V, int R, int side, int with_gold,
                             const int64_t* __restrict__ list_ptr, int32_t* __restrict__ bad) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n) return;
  bool ok;
  if (side == SIDE_RELATION) {
    const int s = X[3 * row], o = X[3 * row + 2];
    ok = s >= 0 && s < V && o >= 0 && o < V;
    if (with_gold) {
      const int gold = X[3 * row + 1];
      ok = ok && gold >= 0 && gold < R;
    }
  } else {
    const int ent = X[3 * row + (side == SIDE_OBJECT ? 0 : 2)], rel = X[3 * row + 1];
    ok = ent >= 0 && ent < V && rel >= 0 && rel < R;
    if (with_gold) {
      const int gold = X[3 * row + (side == SIDE_OBJECT ? 2 : 0)];
      ok = ok && gold >= 0 && gold < V;
    }
  }
  if (list_ptr)
    ok = ok && list_ptr[row] >= 0 && list_ptr[row] <= list_ptr[row + 1] && list_ptr[row + 1] <= list_ptr[n];
  if (!ok) atomicAdd(bad, 1);
}

// ---------------------------------------------------------------- top-k selection (rgcn_topk_device)
// One workgroup of four wave64s per query row.  The row's answer is a function of its energies alone:
//   1. the exclusion list becomes a bit mask of V bits in LDS (the energies are never touched);
//   2. a radix select over float_key -- four 8-bit passes, most significant first, each a 256-bin LDS histogram of
//      the non-excluded entries that match the digits found so far -- yields the key T of the kk-th best entry, how
//      many entries lie above it and how many equal it;
//   3. everything above T is gathered in any order (the sort below fixes the order); the entries EQUAL to T are all
//      taken when they all fit, else the lowest ids among them: a scan in id order, 256 ids per step, whose slot
//      is the entry's rank among the equals -- no counter is raced for, so the choice does not depend on timing;
//   4. the <= 1024 gathered (key, ~id) pairs are sorted in LDS (bitonic, descending: key descending, id ascending).
// The row is read five times (six where a tie straddles position k), after the first time from L2.
constexpr int TOPK_THREADS = 256;
constexpr int TOPK_WAVES = TOPK_THREADS / 64;
constexpr int TOPK_UNROLL = 4;
static_assert(RGCN_MAX_TOPK == 1024, "the sort buffer of k_topk_rows holds 1024 pairs");

__device__ __forceinline__ int lane_id() { return (int)(threadIdx.x & 63u); }
__device__ __forceinline__ uint64_t lanes_below() { return (1ull << lane_id()) - 1ull; }

// hist[digit] += 1 for every active lane, one LDS atomic per distinct digit of the wave: the lanes that hold the same
// digit find each other with eight ballots and the lowest of them adds their number.  (Energies of one row share their
// exponent: left to themselves, 64 lanes would queue on one or two bins.)  Every lane of the wave must call this.
__device__ __forceinline__ void hist_add(uint32_t* hist, uint32_t digit, bool active) {
  uint64_t peers = __ballot(active);
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    const uint64_t set = __ballot((digit >> b) & 1u);
    peers &= ((digit >> b) & 1u) ? set : ~set;
  }
  if (active && (peers & lanes_below()) == 0) atomicAdd(&hist[digit], (uint32_t)__popcll(peers));
}

// TYPED (rgcn_topk_typed_device): the mask of step 1 starts from the complement of the row of `type_mask` that belongs to
// list side R + r of the query (X) instead of from zero, so only members of the list are selected; the pad bits of the
// last word stay clear and `gone` counts entities only.  Everything after step 1 is the same text.
template <bool TYPED>
__global__ void __launch_bounds__(TOPK_THREADS)
k_topk_rows(const float* __restrict__ S, int V, int n, int k, const int64_t* __restrict__ excl_ptr,
            const int32_t* __restrict__ excl_idx, const int64_t* __restrict__ excl_end, int32_t* __restrict__ out_idx,
            float* __restrict__ out_energy, int32_t* __restrict__ bad, const int32_t* __restrict__ X, int side, int R,
            const uint32_t* __restrict__ type_mask) {
  extern __shared__ uint32_t excl_mask[];               // V bits, rounded up to whole words
  __shared__ uint32_t hist[256];
  __shared__ unsigned long long pairs[RGCN_MAX_TOPK];   // key << 32 | ~id
  __shared__ uint32_t wave_cnt[2][TOPK_WAVES];
  __shared__ uint32_t sh_bucket, sh_rank, sh_eq, sh_fill;
  __shared__ int red[TOPK_THREADS];
  const int row = blockIdx.x;
  if (row >= n) return;
  const int tid = (int)threadIdx.x, wave = tid >> 6;
  const float* s = S + (size_t)row * V;
  int32_t* oi = out_idx + (size_t)row * k;
  float* oe = out_energy + (size_t)row * k;
  const int words = (V + 31) >> 5;

  // 1. exclusion mask
  if (TYPED) {
    int rel = X[3 * row + 1];
    if ((unsigned)rel >= (unsigned)R) rel = 0;      // (k_rank_check has flagged it: the call fails, nothing may fault)
    const uint32_t* m = type_mask + ((size_t)side * R + rel) * words;
    const uint32_t last = (V & 31) ? (1u << (V & 31)) - 1u : 0xffffffffu;
    for (int w = tid; w < words; w += TOPK_THREADS) excl_mask[w] = ~m[w] & (w + 1 == words ? last : 0xffffffffu);
  } else {
    for (int w = tid; w < words; w += TOPK_THREADS) excl_mask[w] = 0u;
  }
  __syncthreads();
  if (excl_ptr) {
    int64_t fb = excl_ptr[row], fe = excl_ptr[row + 1];
    // (a negative, decreasing or overlong range has been flagged by k_rank_check: it is not walked at all)
    if (fb < 0 || fe < fb || fe > *excl_end) fb = fe = 0;
    bool oob = false;
    for (int64_t j = fb + tid; j < fe; j += TOPK_THREADS) {
      const int e = excl_idx[j];
      if ((unsigned)e < (unsigned)V) atomicOr(&excl_mask[e >> 5], 1u << (e & 31));
      else oob = true;
    }
    if (oob) atomicAdd(bad, 1);
  }
  __syncthreads();
  int gone = 0;
  for (int w = tid; w < words; w += TOPK_THREADS) gone += __popc(excl_mask[w]);
  red[tid] = gone;
  __syncthreads();
  for (int w = TOPK_THREADS / 2; w > 0; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  const int kk = min(k, V - red[0]);                    // answers this row has
  for (int j = kk + tid; j < k; j += TOPK_THREADS) {
    oi[j] = -1;
    oe[j] = -INFINITY;
  }
  if (kk <= 0) return;

  // 2. radix select: after pass p the top 8 (p + 1) bits of T are known; `rank` counts from the best of the entries
  // that share them
  uint32_t prefix = 0u, rank = (uint32_t)kk, n_eq = 0u;
  const int span = TOPK_THREADS * TOPK_UNROLL;
  for (int shift = 24; shift >= 0; shift -= 8) {
    const uint32_t known = shift == 24 ? 0u : 0xffffffffu << (shift + 8);
    hist[tid] = 0u;
    __syncthreads();
    for (int base = 0; base < V; base += span) {
      uint32_t key[TOPK_UNROLL];
#pragma unroll
      for (int u = 0; u < TOPK_UNROLL; ++u) {
        const int e = base + u * TOPK_THREADS + tid;
        key[u] = e < V ? float_key(s[e]) : 0u;
      }
#pragma unroll
      for (int u = 0; u < TOPK_UNROLL; ++u) {
        const int e = base + u * TOPK_THREADS + tid;
        const bool in = e < V && !((excl_mask[e >> 5] >> (e & 31)) & 1u) && (key[u] & known) == prefix;
        hist_add(hist, (key[u] >> shift) & 255u, in);
      }
    }
    __syncthreads();
    if (wave == 0) {
      // lane l owns bins 255 - 4 l ... 252 - 4 l; `above` = entries in better bins than its own
      uint32_t h[4], mine = 0u;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        h[j] = hist[255 - 4 * tid - j];
        mine += h[j];
      }
      uint32_t incl = mine;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const uint32_t up = __shfl_up(incl, off);
        if (tid >= off) incl += up;
      }
      uint32_t above = incl - mine;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (above < rank && rank <= above + h[j]) {      // true for exactly one bin: rank <= the pass's total
          sh_bucket = (uint32_t)(255 - 4 * tid - j);
          sh_rank = rank - above;
          sh_eq = h[j];
        }
        above += h[j];
      }
    }
    __syncthreads();
    prefix |= sh_bucket << shift;
    rank = sh_rank;
    n_eq = sh_eq;
    __syncthreads();                                     // (hist and the three words are rewritten by the next pass)
  }
  const uint32_t T = prefix;                             // the kk-th best key
  const uint32_t need = rank;                            // entries equal to T that belong to the answer (>= 1)
  const uint32_t n_gt = (uint32_t)kk - need;             // entries above T: all of them belong to it
  const bool all_eq = need == n_eq;

  // 3. gather
  int n2 = 1;
  while (n2 < kk) n2 <<= 1;
  for (int j = kk + tid; j < n2; j += TOPK_THREADS) pairs[j] = 0ull;     // below every real pair (~id has bit 31 set)
  if (tid == 0) sh_fill = 0u;
  __syncthreads();
  for (int base = 0; base < V; base += span) {
    uint32_t key[TOPK_UNROLL];
#pragma unroll
    for (int u = 0; u < TOPK_UNROLL; ++u) {
      const int e = base + u * TOPK_THREADS + tid;
      key[u] = e < V ? float_key(s[e]) : 0u;
    }
#pragma unroll
    for (int u = 0; u < TOPK_UNROLL; ++u) {
      const int e = base + u * TOPK_THREADS + tid;
      const bool in = e < V && !((excl_mask[e >> 5] >> (e & 31)) & 1u);
      const bool take = in && (key[u] > T || (all_eq && key[u] == T));
      const uint64_t takers = __ballot(take);
      if (takers) {
        uint32_t slot = 0u;
        if (lane_id() == __ffsll((unsigned long long)takers) - 1) slot = atomicAdd(&sh_fill, (uint32_t)__popcll(takers));
        slot = __shfl(slot, __ffsll((unsigned long long)takers) - 1) + (uint32_t)__popcll(takers & lanes_below());
        // (the select counted exactly kk takers, so slot < kk; the test only guards the buffer should the energies be
        // rewritten by someone else between the select passes and this one)
        if (take && slot < (uint32_t)kk) pairs[slot] = ((unsigned long long)key[u] << 32) | (uint32_t)~e;
      }
    }
  }
  if (!all_eq) {
    // the `need` lowest ids among the entries equal to T, in id order: slot n_gt + (rank among the equals)
    uint32_t before = 0u;                                // equals in the ids already passed (the same in every thread)
    int flip = 0;
    for (int base = 0; base < V && before < need; base += TOPK_THREADS, flip ^= 1) {
      const int e = base + tid;
      const bool eq = e < V && !((excl_mask[e >> 5] >> (e & 31)) & 1u) && float_key(s[e]) == T;
      const uint64_t eqs = __ballot(eq);
      if (lane_id() == 0) wave_cnt[flip][wave] = (uint32_t)__popcll(eqs);
      __syncthreads();
      uint32_t r = before + (uint32_t)__popcll(eqs & lanes_below()), total = 0u;
#pragma unroll
      for (int w = 0; w < TOPK_WAVES; ++w) {
        const uint32_t cw = wave_cnt[flip][w];
        if (w < wave) r += cw;
        total += cw;
      }
      if (eq && r < need) pairs[n_gt + r] = ((unsigned long long)T << 32) | (uint32_t)~e;
      before += total;
    }
  }
  __syncthreads();

  // 4. bitonic sort of n2 pairs, descending
  for (int size = 2; size <= n2; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = tid; t < (n2 >> 1); t += TOPK_THREADS) {
        const int lo = ((t & ~(stride - 1)) << 1) | (t & (stride - 1)), hi = lo + stride;
        const unsigned long long a = pairs[lo], b = pairs[hi];
        const bool descending = (lo & size) == 0;
        if ((a < b) == descending) {
          pairs[lo] = b;
          pairs[hi] = a;
        }
      }
      __syncthreads();
    }
  }
  for (int j = tid; j < kk; j += TOPK_THREADS) {
    const unsigned long long p = pairs[j];
    oi[j] = (int32_t)~(uint32_t)p;
    oe[j] = key_float((uint32_t)(p >> 32));
  }
}

}  // namespace

void rank_free(rgcn_ctx* c) {
  c->ranking.pool.release();
  c->ranking = RankBufs();
}

rgcn_status rank_reserve(rgcn_ctx* c, int64_t max_queries) {
  RankBufs& q = c->ranking;
  if (max_queries <= q.max) return RGCN_OK;
  rank_free(c);
  RGCN_TRY(dmalloc(c, q.pool, &q.q, (size_t)max_queries * c->dc, false));
  RGCN_TRY(dmalloc(c, q.pool, &q.s, (size_t)max_queries * c->V, false));
  RGCN_TRY(dmalloc(c, q.pool, &q.bad, 1, false));
  RGCN_TRY(dmalloc(c, q.pool, &q.thr, (size_t)max_queries, false));
  q.max = max_queries;
  return RGCN_OK;
}

// ---------------------------------------------------------------- the scoring path of all calls
// Ids are validated on the device (out-of-range ids are rejected, never clamped) and the verdict is read back at the END of
// the call, with no host wait in the middle: until then the kernels substitute id 0 for a bad id and skip a bad range so
// that nothing faults, and the (meaningless) answers of a rejected call are not to be used.
static rgcn_status verdict_begin(rgcn_ctx* c, const int32_t* X_dev, int64_t N, int side, bool with_gold,
                                 const int64_t* list_ptr) {
  RGCN_HIP(c, hipMemsetAsync(c->ranking.bad, 0, sizeof(int32_t), c->stream));
  hipLaunchKernelGGL(k_rank_check, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, c->stream, X_dev, (int)N, c->V, c->R,
                     side, with_gold ? 1 : 0, list_ptr, c->ranking.bad);
  RGCN_HIP(c, hipGetLastError());
  return RGCN_OK;
}

static rgcn_status verdict_end(rgcn_ctx* c, const char* refusal) {
  int32_t bad = 0;
  RGCN_HIP(c, hipMemcpyAsync(&bad, c->ranking.bad, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  RGCN_HIP(c, hipStreamSynchronize(c->stream));
  if (bad) RGCN_FAIL(c, RGCN_ERR_INVALID, refusal);
  return RGCN_OK;
}

// What a side's tails are launched with: how many candidates a row has (its stride, the range of its list's entries, the
// bits of its mask) and where score_chunk leaves their energies
static int candidates(const rgcn_ctx* c, int side) { return side == SIDE_RELATION ? c->R : c->V; }
static const float* energies(const rgcn_ctx* c, int side) { return side == SIDE_RELATION ? c->ranking.rel : c->ranking.s; }

// The relation side's [reserved queries, R] energies, allocated on the first relation call after a (growing) rank_reserve
// as ranking.mixed is: a context that is never asked about relations never holds them.
static rgcn_status relation_energies_reserve(rgcn_ctx* c) {
  RankBufs& q = c->ranking;
  if (!q.rel) RGCN_TRY(dmalloc(c, q.pool, &q.rel, (size_t)q.max * c->R, false));
  return RGCN_OK;
}

// the query rows of X[0, n) into ranking.q, their energies against every candidate into the side's buffer: every entity
// into ranking.s, or (SIDE_RELATION) every relation into ranking.rel
static rgcn_status score_chunk(rgcn_ctx* c, const int32_t* X, int n, int side) {
  const float* codes = c->codes;
  const int dc = c->dc;      // the code width: the query rows, W_relation and the codes
  if (side == SIDE_RELATION) {
    {
      ProfScope ps(c, "rank_query_relation", 4.0 * 3 * n * dc, 0);
      hipLaunchKernelGGL(k_rank_pair, dim3((unsigned)n), dim3(128), 0, c->stream, codes, X, n, dc, c->ranking.q, c->V);
      RGCN_HIP(c, hipGetLastError());
    }
    return gemm_f32(c, "rank_scores_relation", true, true, n, c->R, dc, c->ranking.q, dc, c->w_rel, dc, c->ranking.rel,
                    c->R, 1);
  }
  {
    ProfScope ps(c, "rank_query", 4.0 * 3 * n * dc, 0);
    hipLaunchKernelGGL(k_rank_query, dim3((unsigned)n), dim3(128), 0, c->stream, codes, c->w_rel, X, n, dc,
                       side, c->ranking.q, c->V, c->R, c->reciprocal && side == SIDE_SUBJECT ? c->R : 0);
    RGCN_HIP(c, hipGetLastError());
  }
  return gemm_f32(c, "rank_scores", true, true, n, c->V, dc, c->ranking.q, dc, codes, dc, c->ranking.s, c->V, 1);
}

// One call: the check, then chunk by chunk of the reserve the scoring and tail(b, n, X) -- what the call does with the
// energies of its queries [b, b + n), whose rows start at X -- then the verdict.  A call whose entry admits one chunk only
// (the mixed forms, score queries) runs the loop once, with b = 0.
template <class Tail>
static rgcn_status run_queries(rgcn_ctx* c, const int32_t* X_dev, int64_t N, int side, bool with_gold,
                               const int64_t* list_ptr, const char* refusal, Tail tail) {
  if (side == SIDE_RELATION) RGCN_TRY(relation_energies_reserve(c));
  RGCN_TRY(verdict_begin(c, X_dev, N, side, with_gold, list_ptr));
  for (int64_t b = 0; b < N; b += c->ranking.max) {
    const int n = (int)std::min<int64_t>(c->ranking.max, N - b);
    RGCN_TRY(score_chunk(c, X_dev + 3 * b, n, side));
    RGCN_TRY(tail(b, n, X_dev + 3 * b));
  }
  return verdict_end(c, refusal);
}

// k_rank_threshold + k_rank_rows on the side's energies
static rgcn_status rank_side(rgcn_ctx* c, const int32_t* X_dev, int64_t N, int side, const char* scope, const char* refusal,
                             const int64_t* filt_ptr, const int32_t* filt_idx, int32_t* raw_out, int32_t* filt_out,
                             bool typed = false) {
  const int cands = candidates(c, side);
  return run_queries(c, X_dev, N, side, true, filt_ptr, refusal, [=](int64_t b, int n, const int32_t* X) -> rgcn_status {
    const float* S = energies(c, side);
    ProfScope ps(c, scope, 4.0 * n * cands, 0);
    hipLaunchKernelGGL(k_rank_threshold, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, c->stream, S, cands, X, n,
                       gold_column(side), c->ranking.thr);
    if (typed)
      hipLaunchKernelGGL(k_rank_rows_typed, dim3((unsigned)n), dim3(256), 0, c->stream, S, cands, n, X, side, c->R,
                         c->types.mask, (int)c->types.words, filt_ptr + b, filt_idx, c->ranking.thr, raw_out + b,
                         filt_out + b, c->ranking.bad, filt_ptr + N);
    else
      hipLaunchKernelGGL(k_rank_rows, dim3((unsigned)n), dim3(256), 0, c->stream, S, cands, n, filt_ptr + b, filt_idx,
                         c->ranking.thr, raw_out + b, filt_out + b, c->ranking.bad, filt_ptr + N);
    RGCN_HIP(c, hipGetLastError());
    return RGCN_OK;
  });
}

rgcn_status rank_compute(rgcn_ctx* c, const int32_t* X_dev, int64_t N, int predict_object, const int64_t* filt_ptr,
                         const int32_t* filt_idx, int32_t* raw_out, int32_t* filt_out) {
  return rank_side(c, X_dev, N, predict_object, "rank_rows", "rank: entity / relation / filter index out of range", filt_ptr,
                   filt_idx, raw_out, filt_out);
}

rgcn_status rank_typed_compute(rgcn_ctx* c, const int32_t* X_dev, int64_t N, int predict_object, const int64_t* filt_ptr,
                               const int32_t* filt_idx, int32_t* raw_out, int32_t* filt_out) {
  return rank_side(c, X_dev, N, predict_object, "rank_rows_typed", "rank (typed): entity / relation / filter index out of range",
                   filt_ptr, filt_idx, raw_out, filt_out, true);
}

rgcn_status rank_relation_compute(rgcn_ctx* c, const int32_t* X_dev, int64_t N, const int64_t* filt_ptr,
                                  const int32_t* filt_idx, int32_t* raw_out, int32_t* filt_out) {
  return rank_side(c, X_dev, N, SIDE_RELATION, "rank_rows_relation",
                   "rank (relation): entity / relation / filter index out of range", filt_ptr, filt_idx, raw_out, filt_out);
}

// The counts on the mixed score.  c->ranking.s holds the context's own energies afterwards, unmodified; the partner's rows
// are only read.
rgcn_status rank_mixed_compute(rgcn_ctx* c, const int32_t* X_dev, int64_t N, int predict_object, const float* partner,
                               float weight, const int64_t* filt_ptr, const int32_t* filt_idx, int32_t* raw_out,
                               int32_t* filt_out) {
  return run_queries(c, X_dev, N, predict_object, true, filt_ptr,
                     "rank (mixed): entity / relation / filter index out of range",
                     [=](int64_t, int n, const int32_t* X) -> rgcn_status {
    ProfScope ps(c, "rank_rows_mixed", 8.0 * n * c->V, 0);
    hipLaunchKernelGGL(k_rank_rows_mixed, dim3((unsigned)n), dim3(256), 0, c->stream, c->ranking.s, partner, c->V, X, n,
                       predict_object, (double)weight, filt_ptr, filt_idx, raw_out, filt_out, c->ranking.bad, filt_ptr + N);
    RGCN_HIP(c, hipGetLastError());
    return RGCN_OK;
  });
}

// k_topk_rows' exclusion mask is dynamic LDS, above the default limit for large V: raise the kernel's limit on the context's
// device (every API entry selects it) the first time it launches there.  One bit per device id, per process and unguarded
// like the GEMM launchers' (a context is single-threaded); past 64 devices the attribute is set on every call.
static rgcn_status topk_rows_configure(rgcn_ctx* c) {
  static uint64_t lds_configured = 0;
  const uint64_t device_bit = c->cfg.device < 64 ? 1ull << c->cfg.device : 0;
  if (!(lds_configured & device_bit)) {
    RGCN_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void*>(k_topk_rows<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)((size_t)((RGCN_MAX_TOPK_ENTITIES + 31) / 32) * sizeof(uint32_t))));
    RGCN_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void*>(k_topk_rows<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)((size_t)((RGCN_MAX_TOPK_ENTITIES + 31) / 32) * sizeof(uint32_t))));
    lds_configured |= device_bit;
  }
  return RGCN_OK;
}

// k_topk_rows on the rows of `scores` (energies or mixed scores: it orders any floats), `cands` candidates each, for the
// queries [b, b + n) of a call of N, under the ProfScope `scope`.  Design bytes: four select passes and the gather read the
// row (from L2 after the first).
static rgcn_status topk_rows_launch(rgcn_ctx* c, const char* scope, const float* scores, int cands, int64_t b, int n,
                                    int64_t N, int k, const int64_t* excl_ptr, const int32_t* excl_idx, int32_t* idx_out,
                                    float* val_out, const int32_t* typed_X = nullptr, int side = 0) {
  const size_t mask_bytes = (size_t)((cands + 31) / 32) * sizeof(uint32_t);
  ProfScope ps(c, scope, 5.0 * 4.0 * n * cands + 8.0 * n * k, 0, 4.0 * n * cands + 8.0 * n * k);
  // typed_X: the rows of the chunk's queries, whose relation picks the list (the type-constrained form)
  if (typed_X)
    hipLaunchKernelGGL(k_topk_rows<true>, dim3((unsigned)n), dim3(TOPK_THREADS), mask_bytes, c->stream, scores, cands, n, k,
                       excl_ptr ? excl_ptr + b : nullptr, excl_idx, excl_ptr ? excl_ptr + N : nullptr,
                       idx_out + (size_t)b * k, val_out + (size_t)b * k, c->ranking.bad, typed_X, side, c->R,
                       c->types.mask);
  else
    hipLaunchKernelGGL(k_topk_rows<false>, dim3((unsigned)n), dim3(TOPK_THREADS), mask_bytes, c->stream, scores, cands, n, k,
                       excl_ptr ? excl_ptr + b : nullptr, excl_idx, excl_ptr ? excl_ptr + N : nullptr,
                       idx_out + (size_t)b * k, val_out + (size_t)b * k, c->ranking.bad, (const int32_t*)nullptr, 0, 0,
                       (const uint32_t*)nullptr);
  RGCN_HIP(c, hipGetLastError());
  return RGCN_OK;
}

// k_topk_rows on the side's energies
static rgcn_status topk_side(rgcn_ctx* c, const int32_t* X_dev, int64_t N, int side, const char* scope, const char* refusal,
                             int k, const int64_t* excl_ptr, const int32_t* excl_idx, int32_t* idx_out, float* energy_out) {
  RGCN_TRY(topk_rows_configure(c));
  return run_queries(c, X_dev, N, side, false, excl_ptr, refusal, [=](int64_t b, int n, const int32_t*) {
    return topk_rows_launch(c, scope, energies(c, side), candidates(c, side), b, n, N, k, excl_ptr, excl_idx, idx_out,
                            energy_out);
  });
}

rgcn_status topk_compute(rgcn_ctx* c, const int32_t* X_dev, int64_t N, int predict_object, int k,
                         const int64_t* excl_ptr, const int32_t* excl_idx, int32_t* idx_out, float* energy_out) {
  return topk_side(c, X_dev, N, predict_object, "topk_rows", "topk: entity / relation / exclusion index out of range", k,
                   excl_ptr, excl_idx, idx_out, energy_out);
}

rgcn_status topk_typed_compute(rgcn_ctx* c, const int32_t* X_dev, int64_t N, int predict_object, int k,
                               const int64_t* excl_ptr, const int32_t* excl_idx, int32_t* idx_out, float* energy_out) {
  RGCN_TRY(topk_rows_configure(c));
  return run_queries(c, X_dev, N, predict_object, false, excl_ptr,
                     "topk (typed): entity / relation / exclusion index out of range",
                     [=](int64_t b, int n, const int32_t* X) {
    return topk_rows_launch(c, "topk_rows_typed", c->ranking.s, c->V, b, n, N, k, excl_ptr, excl_idx, idx_out, energy_out,
                            X, predict_object);
  });
}

rgcn_status topk_relation_compute(rgcn_ctx* c, const int32_t* X_dev, int64_t N, int k, const int64_t* excl_ptr,
                                  const int32_t* excl_idx, int32_t* idx_out, float* energy_out) {
  return topk_side(c, X_dev, N, SIDE_RELATION, "topk_rows_relation", "topk (relation): entity / exclusion index out of range",
                   k, excl_ptr, excl_idx, idx_out, energy_out);
}

// The scoring and nothing after it: c->ranking.s holds the energies of queries that have no gold entity -- what the partner
// model of an ensemble top-k hands over
rgcn_status score_queries_compute(rgcn_ctx* c, const int32_t* X_dev, int64_t N, int predict_object) {
  return run_queries(c, X_dev, N, predict_object, false, nullptr, "score queries: entity / relation index out of range",
                     [](int64_t, int, const int32_t*) { return RGCN_OK; });
}

// The same for pairs: c->ranking.rel holds the energies of every relation between s and o
rgcn_status score_relation_queries_compute(rgcn_ctx* c, const int32_t* X_dev, int64_t N) {
  return run_queries(c, X_dev, N, SIDE_RELATION, false, nullptr, "score relation queries: entity index out of range",
                     [](int64_t, int, const int32_t*) { return RGCN_OK; });
}

// The mixed scores of every entity into c->ranking.mixed (k_mix_rows), then k_topk_rows, as it stands, on those instead of
// on the energies.  c->ranking.s holds the context's own energies afterwards, unmodified; the partner's rows are only read.
// The [reserved queries, V] scratch is allocated here, on the first call after a (growing) rank_reserve: a context that
// never asks the ensemble never holds it.
rgcn_status topk_mixed_compute(rgcn_ctx* c, const int32_t* X_dev, int64_t N, int predict_object, int k, const float* partner,
                               float weight, const int64_t* excl_ptr, const int32_t* excl_idx, int32_t* idx_out,
                               float* score_out) {
  RGCN_TRY(topk_rows_configure(c));
  RankBufs& q = c->ranking;
  if (!q.mixed) RGCN_TRY(dmalloc(c, q.pool, &q.mixed, (size_t)q.max * c->V, false));
  return run_queries(c, X_dev, N, predict_object, false, excl_ptr,
                     "topk (mixed): entity / relation / exclusion index out of range",
                     [=](int64_t b, int n, const int32_t*) -> rgcn_status {
    {
      // two rows read, one written, each byte once
      ProfScope ps(c, "topk_mix_rows", 12.0 * n * c->V, 0);
      hipLaunchKernelGGL(k_mix_rows, dim3((unsigned)n), dim3(256), 0, c->stream, c->ranking.s, partner, c->V, n,
                         (double)weight, c->ranking.mixed);
      RGCN_HIP(c, hipGetLastError());
    }
    return topk_rows_launch(c, "topk_rows_mixed", c->ranking.mixed, c->V, b, n, N, k, excl_ptr, excl_idx, idx_out, score_out);
  });
}

}  // namespace rgcn
