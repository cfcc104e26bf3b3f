// The per-row decision of the exclusive negative sampler (NegativeSampler.transform_exclusive,
// code/common/auxilliaries.py:35-73): which entity replaces the object or the subject of negative row j, given the set K
// of known positives.  ONE text for k_negative_sample_exclusive (decoder.hip) and for the host: it depends on <cstdint>,
// counter_rng.h and include/rgcn.h only and compiles with a plain C++ compiler (tests/sanitize/negative_exclusive_driver.cpp).
//
// K is a sorted array of unique packed keys (r V + s) V + o (known_positives_index.h builds it; R V V < 2^63).
//
// Streams of negative row j (j = row - n, T = RGCN_NEG_MAX_DRAWS), all drop_bits(seed, tag, index):
//   coin          tag 0x6e65, index 2 j: bit 0 set = the object is replaced.  Drawn once, never redrawn.
//   attempt 0     tags 0x6e66 / 0x6e67, indices 2 j / 2 j + 1: the plain sampler's draw, bit for bit.
//   attempt t     tags 0x6e68 / 0x6e69, indices 2 (j T + t) / 2 (j T + t) + 1, t = 1 .. T - 1
//                 (j < 2^29 = RGCN_MAX_DECODER_TRIPLES, so the index stays below 2^35 < 2^44).
// Each attempt is 48 bits u = a << 24 | c and the candidate (u V) >> 48.
#pragma once

#include <cstdint>

#include "../../include/rgcn.h"
#include "counter_rng.h"

namespace rgcn {

struct KnownIndex {
  const uint64_t* keys;   // sorted, unique; may be null when count == 0
  int64_t count;
  int32_t V, R;
};

RGCN_HD inline uint64_t known_key(int32_t s, int32_t r, int32_t o, int32_t V) {
  return ((uint64_t)r * (uint64_t)V + (uint64_t)s) * (uint64_t)V + (uint64_t)o;
}

// branch-free binary search: ceil(log2 count) dependent loads, every one of them inside [keys, keys + count)
RGCN_HD inline bool known_has(const KnownIndex& k, uint64_t key) {
  if (k.count <= 0) return false;
  const uint64_t* base = k.keys;
  int64_t n = k.count;
  while (n > 1) {
    const int64_t half = n >> 1;
    base = base[half] <= key ? base + half : base;
    n -= half;
  }
  return *base == key;
}

RGCN_HD inline int32_t negative_candidate(uint64_t seed, uint32_t tag_hi, uint32_t tag_lo, uint64_t idx, int32_t V) {
  const uint32_t a = drop_bits(seed, tag_hi, idx), c = drop_bits(seed, tag_lo, idx + 1);
  const uint64_t u = ((uint64_t)a << 24) | c;                        // 48 random bits
  return (int32_t)((u * (uint64_t)(uint32_t)V) >> 48);               // uniform in [0, V)
}

struct NegativeChoice {
  int32_t entity;       // what replaces the object (object_side) or the subject
  int32_t object_side;  // the coin
  int32_t lookups;      // searches of K this row made (0: an id of the row is out of range; 1: attempt 0 was free)
  int32_t unresolved;   // 1: every entity is known for this row; entity is attempt 0's candidate
};

// negative row j of a batch whose row is (s, r, o)
RGCN_HD inline NegativeChoice negative_exclusive_choice(const KnownIndex& k, uint64_t seed, uint64_t j, int32_t s,
                                                        int32_t r, int32_t o) {
  const int32_t V = k.V;
  NegativeChoice out;
  out.object_side = (int32_t)(drop_bits(seed, 0x6e65u, 2 * j) & 1u);
  const int32_t first = negative_candidate(seed, 0x6e66u, 0x6e67u, 2 * j, V);
  out.entity = first;
  out.lookups = 0;
  out.unresolved = 0;
  // a row the decoder will reject is corrupted as the plain sampler corrupts it: its key would not be one
  if ((uint32_t)s >= (uint32_t)V || (uint32_t)o >= (uint32_t)V || (uint32_t)r >= (uint32_t)k.R) return out;
  // the key of candidate e is base + e * stride
  const uint64_t base = out.object_side ? known_key(s, r, 0, V) : known_key(0, r, o, V);
  const uint64_t stride = out.object_side ? 1ull : (uint64_t)V;
  int32_t e = first;
  ++out.lookups;
  if (!known_has(k, base + (uint64_t)e * stride)) return out;
  for (uint64_t t = 1; t < (uint64_t)RGCN_NEG_MAX_DRAWS; ++t) {
    e = negative_candidate(seed, 0x6e68u, 0x6e69u, 2 * (j * (uint64_t)RGCN_NEG_MAX_DRAWS + t), V);
    ++out.lookups;
    if (!known_has(k, base + (uint64_t)e * stride)) {
      out.entity = e;
      return out;
    }
  }
  // all T candidates are known: the first free entity upward (cyclically) from the last one
  for (int32_t step = 1; step < V; ++step) {
    e = e + 1 == V ? 0 : e + 1;
    ++out.lookups;
    if (!known_has(k, base + (uint64_t)e * stride)) {
      out.entity = e;
      return out;
    }
  }
  out.unresolved = 1;      // (entity is still attempt 0's)
  return out;
}

}  // namespace rgcn
