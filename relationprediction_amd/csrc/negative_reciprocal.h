// The per-row decision of reciprocal relations ([Decoder] ReciprocalRelations): what the pass behind the samplers does to
// row i of a decoder batch.  ONE text for k_reciprocal_rows (decoder.hip) and for the host: it depends on <cstdint>,
// counter_rng.h and include/rgcn.h only and compiles with a plain C++ compiler (tests/sanitize/negative_reciprocal_driver.cpp).
//
// The model keeps two vectors per relation: W_relation[r] answers (s, r, ?), W_relation[R + r] answers (?, r, o).  A batch
// of n positives, entity rate K and relation rate m has N = n (K + 2 + m) rows under the mode:
//   [0, n)                     the positives, as they are                                          RECIPROCAL_KEEP
//   [n, n (K + 1))             the entity corruptions.  Row i is negative row j = i - n; its coin is the samplers' own,
//                              drop_bits(seed, 0x6e65, 2 j) & 1 (negative_exclusive.h), drawn once and never redrawn: 1
//                              replaced the object (the row asks (s, r, ?): KEEP), 0 replaced the subject (the row asks
//                              (?, r, o): its relation becomes r + R)                              RECIPROCAL_SHIFT
//   [n (K + 1), n (K + 1 + m)) the relation rows: forward relations, as they are                   RECIPROCAL_KEEP
//   [n (K + 1 + m), N)         new: the inverse positive (s, r + R, o) of batch row i - n (K + 1 + m), label 1
//                                                                                                  RECIPROCAL_TAIL
// The samplers decide everything on the original r (known-triple lookup, type list, redraws); the rewrite comes behind
// them.  A relation outside [0, R) is left as it is (reciprocal_relation): the decoder's own check names such a row.
#pragma once

#include <cstdint>

#include "../../include/rgcn.h"
#include "counter_rng.h"

namespace rgcn {

enum : int32_t { RECIPROCAL_KEEP = 0, RECIPROCAL_SHIFT = 1, RECIPROCAL_TAIL = 2 };

struct ReciprocalChoice {
  int32_t action;   // RECIPROCAL_*
  int64_t source;   // RECIPROCAL_TAIL: the batch row the inverse positive copies; otherwise -1
};

// rows of the batch under the mode
RGCN_HD inline int64_t reciprocal_rows_total(int64_t n, int32_t K, int32_t m) { return n * ((int64_t)K + 2 + m); }

// the inverse relation's row of W_relation; an id out of range stays what it is
RGCN_HD inline int32_t reciprocal_relation(int32_t r, int32_t R) {
  return (uint32_t)r < (uint32_t)R ? r + R : r;
}

// row i of the batch, 0 <= i < reciprocal_rows_total(n, K, m); a row outside that range is kept
RGCN_HD inline ReciprocalChoice reciprocal_choice(int64_t i, int64_t n, int32_t K, int32_t m, int32_t R, uint64_t seed) {
  (void)R;
  ReciprocalChoice out;
  out.action = RECIPROCAL_KEEP;
  out.source = -1;
  const int64_t entity_end = n * ((int64_t)K + 1), tail = n * ((int64_t)K + 1 + m);
  if (i < n || i >= tail + n) return out;
  if (i < entity_end) {
    const uint64_t j = (uint64_t)(i - n);
    if ((drop_bits(seed, 0x6e65u, 2 * j) & 1u) == 0u) out.action = RECIPROCAL_SHIFT;
    return out;
  }
  if (i < tail) return out;
  out.action = RECIPROCAL_TAIL;
  out.source = i - tail;
  return out;
}

}  // namespace rgcn
