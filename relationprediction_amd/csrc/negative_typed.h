// The per-row decision of the type-constrained negative sampler ([General] TypeConstrainedNegatives): which entity
// replaces the object or the subject of negative row j, drawn from the entities the training set has seen in that slot of
// the row's relation (type_sets.h builds the lists).  ONE text for k_negative_sample_typed (decoder.hip) and for the host:
// it depends on <cstdint>, counter_rng.h, negative_exclusive.h and include/rgcn.h only and compiles with a plain C++
// compiler (tests/sanitize/negative_typed_driver.cpp).
//
// Negative row j of a batch row (s, r, o): the coin is the plain sampler's, bits(0x6e65, 2 j) & 1 (1: the object is
// replaced), never redrawn.  L = list coin R + r, m its length, own = the entity the coin replaces, p = the position of
// own in L (-1: absent).
//   TYPED row  iff the ids are in range, m >= RGCN_TYPED_MIN_CANDIDATES and n = m - (p >= 0) >= 1:
//     attempt 0     tags 0x6e66 / 0x6e67, indices 2 j / 2 j + 1 (the plain sampler's 48 bits u): c = (u n) >> 48,
//                   c += (p >= 0 && c >= p), candidate L[c] -- uniform over the OTHER members of L, never own
//                   (negative_relation.h draws r' != r by the same skip)
//     exclusive     a candidate is known as in negative_exclusive.h; attempt t = 1 .. T - 1 redraws from tags
//                   0x6e68 / 0x6e69 at indices 2 (j T + t) / + 1 with the same skip; after T known candidates the first
//                   member that is not known, scanning positions upward cyclically from the last candidate and passing
//                   over p; if every other member is known the row goes open
//   OPEN row   otherwise: the plain sampler's draw, or with exclusive != 0 negative_exclusive_choice's, bit for bit.
#pragma once

#include <cstdint>

#include "../../include/rgcn.h"
#include "counter_rng.h"
#include "negative_exclusive.h"

namespace rgcn {

struct TypeSets {
  const int64_t* ptr;     // [2 R + 1]
  const int32_t* idx;     // [ptr[2 R]], ascending inside a list
  int32_t V, R;
};

// position of e in the ascending L[0, m), m >= 1, or -1: a branch-free binary search, ceil(log2 m) dependent loads,
// every one of them inside [L, L + m)
RGCN_HD inline int32_t typed_position(const int32_t* L, int32_t m, int32_t e) {
  const int32_t* base = L;
  int32_t n = m;
  while (n > 1) {
    const int32_t half = n >> 1;
    base = base[half] <= e ? base + half : base;
    n -= half;
  }
  return *base == e ? (int32_t)(base - L) : -1;
}

// draw `idx` / `idx + 1` of the two tags as 48 bits; position in [0, m) among the n = m - (p >= 0) members other than p
RGCN_HD inline int32_t typed_candidate(uint64_t seed, uint32_t tag_hi, uint32_t tag_lo, uint64_t idx, int32_t n,
                                       int32_t p) {
  const uint32_t a = drop_bits(seed, tag_hi, idx), b = drop_bits(seed, tag_lo, idx + 1);
  const uint64_t u = ((uint64_t)a << 24) | b;                        // 48 random bits
  int32_t c = (int32_t)((u * (uint64_t)(uint32_t)n) >> 48);          // uniform in [0, n)
  c += (p >= 0 && c >= p) ? 1 : 0;
  return c;
}

struct TypedChoice {
  int32_t entity;       // what replaces the object (object_side) or the subject
  int32_t object_side;  // the coin
  int32_t open;         // 1: the row was drawn over all V entities (RGCN_BUF_NEGATIVE_TYPED_OPEN counts it)
  int32_t lookups;      // searches of K this row made
  int32_t unresolved;   // the open exclusive decision's: every entity is known for this row
};

// the open decision: the plain sampler's, or negative_exclusive_choice's
RGCN_HD inline TypedChoice typed_open_choice(const KnownIndex& k, int32_t exclusive, uint64_t seed, uint64_t j, int32_t s,
                                             int32_t r, int32_t o, int32_t V, int32_t lookups) {
  TypedChoice out;
  out.open = 1;
  if (exclusive) {
    const NegativeChoice ch = negative_exclusive_choice(k, seed, j, s, r, o);
    out.entity = ch.entity;
    out.object_side = ch.object_side;
    out.lookups = lookups + ch.lookups;
    out.unresolved = ch.unresolved;
    return out;
  }
  out.object_side = (int32_t)(drop_bits(seed, 0x6e65u, 2 * j) & 1u);
  out.entity = negative_candidate(seed, 0x6e66u, 0x6e67u, 2 * j, V);
  out.lookups = lookups;
  out.unresolved = 0;
  return out;
}

// negative row j of a batch whose row is (s, r, o); k is read only with exclusive != 0 (k.V == t.V, k.R == t.R)
RGCN_HD inline TypedChoice negative_typed_choice(const TypeSets& t, const KnownIndex& k, int32_t exclusive, uint64_t seed,
                                                 uint64_t j, int32_t s, int32_t r, int32_t o) {
  const int32_t V = t.V;
  // a row the decoder will reject is open and makes no lookup of either structure
  if ((uint32_t)s >= (uint32_t)V || (uint32_t)o >= (uint32_t)V || (uint32_t)r >= (uint32_t)t.R)
    return typed_open_choice(k, exclusive, seed, j, s, r, o, V, 0);
  const int32_t coin = (int32_t)(drop_bits(seed, 0x6e65u, 2 * j) & 1u);
  const int64_t l = (int64_t)coin * t.R + r;
  const int64_t begin = t.ptr[l];
  const int32_t m = (int32_t)(t.ptr[l + 1] - begin);
  if (m < RGCN_TYPED_MIN_CANDIDATES) return typed_open_choice(k, exclusive, seed, j, s, r, o, V, 0);
  const int32_t* L = t.idx + begin;
  const int32_t own = coin ? o : s;
  const int32_t p = typed_position(L, m, own);
  const int32_t n = m - (p >= 0 ? 1 : 0);
  if (n < 1) return typed_open_choice(k, exclusive, seed, j, s, r, o, V, 0);
  TypedChoice out;
  out.object_side = coin;
  out.open = 0;
  out.lookups = 0;
  out.unresolved = 0;
  int32_t c = typed_candidate(seed, 0x6e66u, 0x6e67u, 2 * j, n, p);
  out.entity = L[c];
  if (!exclusive) return out;
  // the key of candidate e is base + e * stride (negative_exclusive.h)
  const uint64_t base = coin ? known_key(s, r, 0, V) : known_key(0, r, o, V);
  const uint64_t stride = coin ? 1ull : (uint64_t)V;
  ++out.lookups;
  if (!known_has(k, base + (uint64_t)L[c] * stride)) return out;
  for (uint64_t a = 1; a < (uint64_t)RGCN_NEG_MAX_DRAWS; ++a) {
    c = typed_candidate(seed, 0x6e68u, 0x6e69u, 2 * (j * (uint64_t)RGCN_NEG_MAX_DRAWS + a), n, p);
    ++out.lookups;
    if (!known_has(k, base + (uint64_t)L[c] * stride)) {
      out.entity = L[c];
      return out;
    }
  }
  // all T candidates are known: the first other member that is not, upward (cyclically) from the last one
  for (int32_t step = 1; step < m; ++step) {
    c = c + 1 == m ? 0 : c + 1;
    if (c == p) continue;
    ++out.lookups;
    if (!known_has(k, base + (uint64_t)L[c] * stride)) {
      out.entity = L[c];
      return out;
    }
  }
  // every other member of L is known: no typed row is left as a known positive, the row goes open
  return typed_open_choice(k, exclusive, seed, j, s, r, o, V, out.lookups);
}

}  // namespace rgcn
