// The per-relation entity sets behind rgcn_type_sets_reserve: validation, limits and the build, on the host.
// Host-only; depends on include/rgcn.h and the standard library (tests/sanitize/negative_typed_driver.cpp runs it under
// AddressSanitizer and UndefinedBehaviorSanitizer).  Deterministic: sorted unique members, list by list.
//
// For the triples T: domain(r) = the sorted unique subjects of r, range(r) = the sorted unique objects of r (the local
// closed-world assumption of Krompass et al., 2015).  List l = side R + r, side 0 = subjects, side 1 = objects -- the
// sampler's coin and the queries' predict_object.  A list with fewer than RGCN_TYPED_MIN_CANDIDATES members is OPEN: it
// stands for all V entities (its mask row has all V bits set; ptr / idx keep the members it has).
#pragma once

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/rgcn.h"

namespace rgcn {

struct TypeSetsHost {
  std::vector<int64_t> ptr;     // [2 R + 1]
  std::vector<int32_t> idx;     // [ptr[2 R]] members, ascending inside a list
  std::vector<uint32_t> mask;   // [2 R][words]: bit e of row l set iff e is in list l (all V bits for an open list);
                                // the pad bits of a row's last word are clear
  int64_t words = 0;            // ceil(V / 32)
};

// What the 32-bit word index of the mask and the 32-bit member count can hold: arithmetic only, nothing is allocated.
inline rgcn_status type_sets_limits(int64_t V, int64_t R, int64_t num_triples, std::string* err) {
  if (V <= 0 || R <= 0 || num_triples < 0) {
    if (err) *err = "type sets: EntityCount and RelationCount must be positive, num_triples not negative";
    return RGCN_ERR_INVALID;
  }
  const int64_t words = (V + 31) / 32, limit = (int64_t)1 << 31;
  // 2 R words >= 2^31  <=>  words > floor((2^31 - 1) / (2 R)), with 2 R itself checked first
  if (R >= limit / 2 || words > (limit - 1) / (2 * R)) {
    if (err) *err = "type sets: 2 x RelationCount x ceil(EntityCount / 32) must be below 2^31 (mask words)";
    return RGCN_ERR_UNSUPPORTED;
  }
  if (num_triples >= limit) {
    if (err) *err = "type sets: 2^31 or more triples";
    return RGCN_ERR_UNSUPPORTED;
  }
  return RGCN_OK;
}

// out <- the sets of the [num_triples,3] rows (s, r, o).  An id out of range: RGCN_ERR_INVALID naming the row, *out
// untouched.
inline rgcn_status type_sets_build(const int32_t* triples, int64_t num_triples, int32_t V, int32_t R, TypeSetsHost* out,
                                   std::string* err) {
  const rgcn_status lim = type_sets_limits(V, R, num_triples, err);
  if (lim != RGCN_OK) return lim;
  if (num_triples > 0 && !triples) {
    if (err) *err = "type sets: NULL triples";
    return RGCN_ERR_INVALID;
  }
  for (int64_t e = 0; e < num_triples; ++e) {
    const int32_t s = triples[3 * e], r = triples[3 * e + 1], o = triples[3 * e + 2];
    if (s < 0 || s >= V || o < 0 || o >= V || r < 0 || r >= R) {
      if (err) *err = "type sets: triple " + std::to_string(e) + " has an id out of range";
      return RGCN_ERR_INVALID;
    }
  }
  // (list, member) packed as l V + e: sorted and unique, the lists fall out in order (2 R V < 2^63: R, V < 2^31)
  std::vector<uint64_t> k((size_t)num_triples * 2);
  for (int64_t e = 0; e < num_triples; ++e) {
    const uint64_t s = (uint64_t)triples[3 * e], r = (uint64_t)triples[3 * e + 1], o = (uint64_t)triples[3 * e + 2];
    k[(size_t)(2 * e)] = r * (uint64_t)V + s;
    k[(size_t)(2 * e + 1)] = ((uint64_t)R + r) * (uint64_t)V + o;
  }
  std::sort(k.begin(), k.end());
  k.erase(std::unique(k.begin(), k.end()), k.end());
  TypeSetsHost t;
  const int64_t lists = 2 * (int64_t)R;
  t.words = ((int64_t)V + 31) / 32;
  t.ptr.assign((size_t)lists + 1, 0);
  t.idx.resize(k.size());
  for (size_t i = 0; i < k.size(); ++i) {
    ++t.ptr[(size_t)(k[i] / (uint64_t)V) + 1];
    t.idx[i] = (int32_t)(k[i] % (uint64_t)V);
  }
  for (int64_t l = 0; l < lists; ++l) t.ptr[(size_t)l + 1] += t.ptr[(size_t)l];
  t.mask.assign((size_t)(lists * t.words), 0u);
  const uint32_t last = (V & 31) ? (1u << (V & 31)) - 1u : 0xffffffffu;      // the valid bits of a row's last word
  for (int64_t l = 0; l < lists; ++l) {
    uint32_t* row = t.mask.data() + (size_t)(l * t.words);
    const int64_t b = t.ptr[(size_t)l], m = t.ptr[(size_t)l + 1] - b;
    if (m < RGCN_TYPED_MIN_CANDIDATES) {
      for (int64_t w = 0; w < t.words; ++w) row[w] = w + 1 == t.words ? last : 0xffffffffu;
    } else {
      for (int64_t i = 0; i < m; ++i) {
        const int32_t e = t.idx[(size_t)(b + i)];
        row[e >> 5] |= 1u << (e & 31);
      }
    }
  }
  *out = std::move(t);
  return RGCN_OK;
}

}  // namespace rgcn
