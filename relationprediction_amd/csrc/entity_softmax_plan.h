// How the entity-softmax term (entity_softmax.hip) cuts its work: the chunk of ROWS (two per positive: the object row and
// the subject row) its [chunk, padded V] energy buffer holds, the padded entity count, the split over the rows of the
// candidate gradient's TN product, and the form of the NN product.  Pure host arithmetic: nothing from HIP, no context,
// no environment (tests/sanitize/entity_softmax_driver.cpp runs it under AddressSanitizer and UndefinedBehaviorSanitizer;
// tests/test_entity_softmax_host.py pins its table).
#ifndef RGCN_ENTITY_SOFTMAX_PLAN_H_
#define RGCN_ENTITY_SOFTMAX_PLAN_H_

#include <cstddef>
#include <cstdint>

namespace rgcn {

constexpr int kEntsmLongRow = 64;               // segments (query entities, relations) with more rows of a chunk are cut into pieces
constexpr int kEntsmPiece = 64;                 // rows per piece: one wavefront sums it
constexpr int64_t kEntsmMaxChunk = 65536;       // rows per chunk at most
// floats of the energy buffer at most: 256 MB.  The gradients overwrite the energies in place, so this is the term's one
// [rows, V] buffer; at FB15k-237 (V = 14,541, padded 14,544) it holds 4,608 rows, which leaves the TN product a few
// thousand rows to contract over.
constexpr int64_t kEntsmEnergyFloats = (int64_t)1 << 26;
constexpr int kEntsmSplitRows = 128;            // a slice of the TN product is at least this deep
constexpr int kEntsmMaxSplit = 64;
constexpr int kEntsmTargetTiles = 256;          // workgroups the TN product should reach: one per compute unit
constexpr size_t kEntsmSlabFloats = (size_t)1 << 24;   // split-K slabs the term allows itself at most (64 MB)

struct EntsmPlan {
  int64_t chunk = 0;      // rows per chunk: rows of Q, dQ and E (which becomes G)
  int32_t padded_v = 0;   // leading dimension of E / G, rows of the TN product and of its slabs: V up to 4
  int32_t split_k = 1;    // GemmCall::split_k of dC = G^T Q at a full chunk
  // The NN product dQ = G c contracts over the candidates.  V % 4 == 0: over K = V against the codes themselves.
  // Otherwise (FB15k-237) nn_padded = 1: over K = padded V against a copy of the codes with zero pad rows, so that the
  // product keeps its 16-byte loads of G -- the scalar form over K = V would quarter the width of every load of the
  // operand that is a whole chunk of rows wide, for the price of one [V, dc] copy per call.  Neither form is measured.
  int32_t nn_padded = 0;
};

inline int32_t entsm_padded_v(int32_t V) { return V <= 0 ? 0 : (int32_t)(((int64_t)V + 3) / 4 * 4); }

// split over K = n rows of the [padded V, dc] product: enough 128 x 128 tiles x slices to occupy the chip, slices of
// kEntsmSplitRows rows or more, and no more slabs than slab_floats floats hold.  Non-decreasing in n: a partial chunk
// never asks for more slabs than the full one reserved.
inline int32_t entsm_split(int64_t n, int32_t padded_v, int32_t dc, size_t slab_floats) {
  if (n <= 0 || padded_v <= 0 || dc <= 0) return 1;
  const int64_t tiles = (((int64_t)padded_v + 127) / 128) * (((int64_t)dc + 127) / 128);
  int64_t want = kEntsmTargetTiles / tiles;
  if (want > kEntsmMaxSplit) want = kEntsmMaxSplit;
  const int64_t deep = n / kEntsmSplitRows;
  if (want > deep) want = deep;
  const int64_t fit = (int64_t)(slab_floats / ((size_t)padded_v * (size_t)dc));
  if (want > fit) want = fit;
  return want < 2 ? 1 : (int32_t)want;
}

inline EntsmPlan entsm_plan(int64_t max_positives, int32_t V, int32_t dc, size_t slab_floats) {
  EntsmPlan p;
  if (max_positives <= 0 || V <= 0 || dc <= 0) return p;
  p.padded_v = entsm_padded_v(V);
  p.nn_padded = V % 4 != 0 ? 1 : 0;
  int64_t rows = kEntsmEnergyFloats / p.padded_v / 128 * 128;      // whole 128-row GEMM tiles
  if (rows < 128) rows = 128;
  if (rows > kEntsmMaxChunk) rows = kEntsmMaxChunk;
  const int64_t want = max_positives > kEntsmMaxChunk ? kEntsmMaxChunk : 2 * max_positives;      // (no overflow)
  p.chunk = want < rows ? want : rows;
  p.split_k = entsm_split(p.chunk, p.padded_v, dc, slab_floats);
  return p;
}

}  // namespace rgcn
#endif  // RGCN_ENTITY_SOFTMAX_PLAN_H_
