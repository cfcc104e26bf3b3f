// The index of known positives behind rgcn_known_positives_reserve: validation, limits and the build, on the host.
// Host-only; depends on include/rgcn.h and the standard library (tests/sanitize/negative_exclusive_driver.cpp runs it
// under AddressSanitizer and UndefinedBehaviorSanitizer).  Deterministic: the sorted unique packed keys of the triples.
#pragma once

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/rgcn.h"

namespace rgcn {

// What the packed 64-bit keys and the 32-bit key count can hold: arithmetic only, nothing is allocated.
// num_triples bounds the key count from above and is what is checked, before any deduplication.
inline rgcn_status known_index_limits(int64_t V, int64_t R, int64_t num_triples, std::string* err) {
  if (V <= 0 || R <= 0 || num_triples < 0) {
    if (err) *err = "known positives: EntityCount and RelationCount must be positive, num_triples not negative";
    return RGCN_ERR_INVALID;
  }
  // R V V >= 2^63  <=>  V V > floor((2^63 - 1) / R), with V V itself checked first
  if (V > INT64_MAX / V || V * V > INT64_MAX / R) {
    if (err) *err = "known positives: RelationCount x EntityCount^2 must be below 2^63 (packed 64-bit keys)";
    return RGCN_ERR_UNSUPPORTED;
  }
  if (num_triples >= ((int64_t)1 << 31)) {
    if (err) *err = "known positives: 2^31 or more keys";
    return RGCN_ERR_UNSUPPORTED;
  }
  return RGCN_OK;
}

// keys <- the sorted unique packed keys (r V + s) V + o of the [num_triples,3] rows (s, r, o).  An id out of range:
// RGCN_ERR_INVALID naming the row, *keys untouched.
inline rgcn_status known_index_build(const int32_t* triples, int64_t num_triples, int32_t V, int32_t R,
                                     std::vector<uint64_t>* keys, std::string* err) {
  const rgcn_status lim = known_index_limits(V, R, num_triples, err);
  if (lim != RGCN_OK) return lim;
  if (num_triples > 0 && !triples) {
    if (err) *err = "known positives: NULL triples";
    return RGCN_ERR_INVALID;
  }
  for (int64_t e = 0; e < num_triples; ++e) {
    const int32_t s = triples[3 * e], r = triples[3 * e + 1], o = triples[3 * e + 2];
    if (s < 0 || s >= V || o < 0 || o >= V || r < 0 || r >= R) {
      if (err) *err = "known positive " + std::to_string(e) + " has an id out of range";
      return RGCN_ERR_INVALID;
    }
  }
  std::vector<uint64_t> k((size_t)num_triples);
  for (int64_t e = 0; e < num_triples; ++e)
    k[(size_t)e] = ((uint64_t)triples[3 * e + 1] * (uint64_t)V + (uint64_t)triples[3 * e]) * (uint64_t)V +
                   (uint64_t)triples[3 * e + 2];
  std::sort(k.begin(), k.end());
  k.erase(std::unique(k.begin(), k.end()), k.end());
  keys->swap(k);
  return RGCN_OK;
}

// The same set in the other order: keys <- the sorted unique packed keys (r V + o) V + s, so that the known SUBJECTS of
// a pair (r, o) are one contiguous range (entity_softmax_range.h), as the known objects of (s, r) are one range of
// known_index_build's keys.  Same checks, same size; *keys untouched on an error.
inline rgcn_status known_index_build_by_object(const int32_t* triples, int64_t num_triples, int32_t V, int32_t R,
                                               std::vector<uint64_t>* keys, std::string* err) {
  const rgcn_status lim = known_index_limits(V, R, num_triples, err);
  if (lim != RGCN_OK) return lim;
  if (num_triples > 0 && !triples) {
    if (err) *err = "known positives: NULL triples";
    return RGCN_ERR_INVALID;
  }
  for (int64_t e = 0; e < num_triples; ++e) {
    const int32_t s = triples[3 * e], r = triples[3 * e + 1], o = triples[3 * e + 2];
    if (s < 0 || s >= V || o < 0 || o >= V || r < 0 || r >= R) {
      if (err) *err = "known positive " + std::to_string(e) + " has an id out of range";
      return RGCN_ERR_INVALID;
    }
  }
  std::vector<uint64_t> k((size_t)num_triples);
  for (int64_t e = 0; e < num_triples; ++e)
    k[(size_t)e] = ((uint64_t)triples[3 * e + 1] * (uint64_t)V + (uint64_t)triples[3 * e + 2]) * (uint64_t)V +
                   (uint64_t)triples[3 * e];
  std::sort(k.begin(), k.end());
  k.erase(std::unique(k.begin(), k.end()), k.end());
  keys->swap(k);
  return RGCN_OK;
}

}  // namespace rgcn
