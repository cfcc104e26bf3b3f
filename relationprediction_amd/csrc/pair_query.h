// The relation side's query row, P[row,:] = codes[s] * codes[o], one rounding per element: ONE text for k_rank_pair
// (ranking.hip: which relation holds between s and o) and k_relsm_pair (relation_softmax.hip: the loss term that trains
// that answer), so that the term's energies are the query's energies bit for bit.  An id out of range is replaced by 0:
// the caller's check kernel fails the call, and nothing may fault before its verdict is read.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace rgcn {

#if defined(__HIPCC__)
__device__ __forceinline__ void pair_query_row(const float* __restrict__ codes, const int32_t* __restrict__ X, int row,
                                               int d, float* __restrict__ P, int V) {
  int s = X[3 * row], o = X[3 * row + 2];
  if ((unsigned)s >= (unsigned)V) s = 0;
  if ((unsigned)o >= (unsigned)V) o = 0;
  const float* a = codes + (size_t)s * d;
  const float* b = codes + (size_t)o * d;
  for (int k = threadIdx.x; k < d; k += blockDim.x) P[(size_t)row * d + k] = a[k] * b[k];
}

// The entity sides' query row, Q[row,:] = codes[ent] * W_relation[rel], one rounding per element: ONE text for
// k_rank_query (ranking.hip: which entity completes (s, r, ?) or (?, r, o)) and k_entsm_rows (entity_softmax.hip: the
// loss term that trains that answer).  ent is the given entity of the query, whichever side it stands on.  An id out of
// range is replaced by 0, as above.
__device__ __forceinline__ void entity_query_row(const float* __restrict__ codes, const float* __restrict__ wrel, int ent,
                                                 int rel, int row, int d, float* __restrict__ Q, int V, int R) {
  if ((unsigned)ent >= (unsigned)V) ent = 0;
  if ((unsigned)rel >= (unsigned)R) rel = 0;
  const float* e = codes + (size_t)ent * d;
  const float* r = wrel + (size_t)rel * d;
  for (int k = threadIdx.x; k < d; k += blockDim.x) Q[(size_t)row * d + k] = e[k] * r[k];
}
#endif

}  // namespace rgcn
