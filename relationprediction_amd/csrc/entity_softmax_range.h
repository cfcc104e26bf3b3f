// Which known entities leave the candidate set of one row of the entity-softmax term (entity_softmax.hip): the range of
// a sorted key array that holds every key in [base, base + V).  An object row (s, r, ?) asks the index sorted by
// (r V + s) V + o with base = (r V + s) V; a subject row (?, r, o) asks the one sorted by (r V + o) V + s
// (known_index_build_by_object) with base = (r V + o) V.  Either way key - base is the masked entity, and the range is
// found by two lower-bound searches, whatever V is.  ONE text for the row kernel and the host: plain C++, depends on
// <cstdint> and counter_rng.h's RGCN_HD only (tests/sanitize/entity_softmax_driver.cpp runs it under AddressSanitizer and
// UndefinedBehaviorSanitizer).
#pragma once

#include <cstdint>

#include "counter_rng.h"

namespace rgcn {

struct EntsmRange {
  int64_t lo, hi;      // keys[lo, hi) lie in [base, base + width); lo == hi: nothing is known for the pair
};

// first index whose key is not below x; every load is inside [keys, keys + count)
RGCN_HD inline int64_t entsm_lower_bound(const uint64_t* keys, int64_t count, uint64_t x) {
  int64_t lo = 0, hi = count > 0 ? count : 0;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// (base + width does not wrap: R V V < 2^63, known_index_limits)
RGCN_HD inline EntsmRange entsm_range(const uint64_t* keys, int64_t count, uint64_t base, uint64_t width) {
  EntsmRange r;
  r.lo = entsm_lower_bound(keys, count, base);
  r.hi = r.lo;
  // (an empty range costs one search: the key at lo already lies beyond it)
  if (r.lo < count && keys[r.lo] < base + width) r.hi = entsm_lower_bound(keys, count, base + width);
  return r;
}

// the base key of a row: query entity a, relation r (object row: a = s in the by-subject index; subject row: a = o in the
// by-object index)
RGCN_HD inline uint64_t entsm_base(int32_t a, int32_t r, int32_t V) {
  return ((uint64_t)r * (uint64_t)V + (uint64_t)a) * (uint64_t)V;
}

}  // namespace rgcn
