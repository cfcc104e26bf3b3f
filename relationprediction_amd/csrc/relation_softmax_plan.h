// How the relation-softmax term (relation_softmax.hip) cuts its work: the chunk of positives its [chunk, padded R]
// energy buffer holds, the padded relation count, and the split over K of the relation gradient's TN product.  Pure host
// arithmetic: nothing from HIP, no context, no environment (tests/sanitize/relation_softmax_plan_driver.cpp runs it under
// AddressSanitizer and UndefinedBehaviorSanitizer; tests/test_relation_softmax_host.py pins its table).
#ifndef RGCN_RELATION_SOFTMAX_PLAN_H_
#define RGCN_RELATION_SOFTMAX_PLAN_H_

#include <cstddef>
#include <cstdint>

namespace rgcn {

constexpr int kRelsmLongRow = 64;               // entity rows with more incidences of a chunk's positives are cut into pieces
constexpr int kRelsmPiece = 64;                 // incidences per piece: one wavefront sums it
constexpr int64_t kRelsmMaxChunk = 65536;       // positives per chunk at most
constexpr int64_t kRelsmEnergyFloats = (int64_t)1 << 24;   // floats of the energy buffer at most (64 MB)
constexpr int kRelsmSplitRows = 256;            // a slice of the TN product is at least this deep
constexpr int kRelsmMaxSplit = 64;
constexpr int kRelsmTargetTiles = 256;          // workgroups the TN product should reach: one per compute unit
constexpr size_t kRelsmSlabFloats = (size_t)1 << 23;   // split-K slabs the term allows itself at most (32 MB)

struct RelsmPlan {
  int64_t chunk = 0;      // positives per chunk: rows of Q, dQ and E / G
  int32_t padded_r = 0;   // leading dimension of E / G, rows of the padded relation table and of the TN product: R up to 4
  int32_t split_k = 1;    // GemmCall::split_k of dW = G^T Q at a full chunk
};

inline int32_t relsm_padded_r(int32_t R) { return R <= 0 ? 0 : (int32_t)(((int64_t)R + 3) / 4 * 4); }

// split over K = n positives of the [padded R, dc] product: enough 128 x 128 tiles x slices to occupy the chip, slices
// of kRelsmSplitRows rows or more, and no more slabs than slab_floats floats of split-K scratch hold
inline int32_t relsm_split(int64_t n, int32_t padded_r, int32_t dc, size_t slab_floats) {
  if (n <= 0 || padded_r <= 0 || dc <= 0) return 1;
  const int64_t tiles = (((int64_t)padded_r + 127) / 128) * (((int64_t)dc + 127) / 128);
  int64_t want = kRelsmTargetTiles / tiles;
  if (want > kRelsmMaxSplit) want = kRelsmMaxSplit;
  const int64_t deep = n / kRelsmSplitRows;
  if (want > deep) want = deep;
  const int64_t fit = (int64_t)(slab_floats / ((size_t)padded_r * (size_t)dc));
  if (want > fit) want = fit;
  return want < 2 ? 1 : (int32_t)want;
}

inline RelsmPlan relsm_plan(int64_t max_positives, int32_t R, int32_t dc, size_t slab_floats) {
  RelsmPlan p;
  if (max_positives <= 0 || R <= 0 || dc <= 0) return p;
  p.padded_r = relsm_padded_r(R);
  int64_t rows = kRelsmEnergyFloats / p.padded_r / 128 * 128;      // whole 128-row GEMM tiles
  if (rows < 128) rows = 128;
  if (rows > kRelsmMaxChunk) rows = kRelsmMaxChunk;
  p.chunk = max_positives < rows ? max_positives : rows;
  p.split_k = relsm_split(p.chunk, p.padded_r, dc, slab_floats);
  return p;
}

}  // namespace rgcn
#endif  // RGCN_RELATION_SOFTMAX_PLAN_H_
