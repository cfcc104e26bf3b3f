// The per-row decision of the relation corruptions ([General] RelationNegativeSampleRate): which relation r' replaces r
// in the negative row (s, r', o), in the plain form and against the set K of known positives.  ONE text for
// k_negative_sample_relation (decoder.hip) and for the host: it depends on <cstdint>, counter_rng.h, negative_exclusive.h
// and include/rgcn.h only and compiles with a plain C++ compiler (tests/sanitize/negative_relation_driver.cpp).
//
// A decoder batch with relation_rate = m > 0 has N = n (1 + rate + m) rows.  Rows [0, n (rate + 1)) are the entity
// samplers' (k_negative_sample / k_negative_sample_exclusive, untouched); row i >= n (rate + 1) is relation row
// j = i - n (rate + 1) of batch row j mod n = (s, r, o): label 0, s and o as they are, r replaced.
//
// Streams of relation row j (T = RGCN_NEG_MAX_DRAWS), all drop_bits(seed, tag, index); none is used by the entity samplers:
//   attempt 0     tags 0x6e6a / 0x6e6b, indices 2 j / 2 j + 1.
//   attempt t     tags 0x6e6c / 0x6e6d, indices 2 (j T + t) / 2 (j T + t) + 1, t = 1 .. T - 1
//                 (j < 2^29 = RGCN_MAX_DECODER_TRIPLES, so the index stays below 2^35 < 2^44).
// Each attempt is 48 bits u = a << 24 | c, the draw (u (R - 1)) >> 48 in [0, R - 1) and the candidate draw + (draw >= r):
// uniform over the R - 1 OTHER relations.  The row's own relation is never a candidate (a uniform draw over all R would
// label a positive as negative in 1 row of R).
#pragma once

#include <cstdint>

#include "../../include/rgcn.h"
#include "counter_rng.h"
#include "negative_exclusive.h"

namespace rgcn {

// draw in [0, R - 1); R >= 1 (R == 1 gives 0, and no caller lets such a context sample)
RGCN_HD inline int32_t relation_draw(uint64_t seed, uint32_t tag_hi, uint32_t tag_lo, uint64_t idx, int32_t R) {
  const uint32_t a = drop_bits(seed, tag_hi, idx), c = drop_bits(seed, tag_lo, idx + 1);
  const uint64_t u = ((uint64_t)a << 24) | c;                        // 48 random bits
  return (int32_t)((u * (uint64_t)(uint32_t)(R - 1)) >> 48);
}

struct RelationChoice {
  int32_t relation;    // what replaces r
  int32_t lookups;     // searches of K this row made (0: plain form, or an id of the row is out of range)
  int32_t unresolved;  // 1: every other relation is known for (s, ., o); relation is attempt 0's candidate
};

// relation row j of a batch whose row is (s, r, o).  exclusive == 0: attempt 0 alone, k.keys is not read (k carries V, R).
RGCN_HD inline RelationChoice negative_relation_choice(const KnownIndex& k, int32_t exclusive, uint64_t seed, uint64_t j,
                                                       int32_t s, int32_t r, int32_t o) {
  const int32_t V = k.V, R = k.R;
  RelationChoice out;
  const int32_t draw = relation_draw(seed, 0x6e6au, 0x6e6bu, 2 * j, R);
  out.relation = draw;
  out.lookups = 0;
  out.unresolved = 0;
  // a row the decoder will reject takes the draw itself (in range, no skip): its key would not be one
  if ((uint32_t)s >= (uint32_t)V || (uint32_t)o >= (uint32_t)V || (uint32_t)r >= (uint32_t)R) return out;
  const int32_t first = draw + (draw >= r ? 1 : 0);
  out.relation = first;
  if (!exclusive) return out;
  // the key of candidate e is base + e * stride
  const uint64_t base = known_key(s, 0, o, V);
  const uint64_t stride = (uint64_t)V * (uint64_t)V;
  int32_t e = first;
  ++out.lookups;
  if (!known_has(k, base + (uint64_t)e * stride)) return out;
  for (uint64_t t = 1; t < (uint64_t)RGCN_NEG_MAX_DRAWS; ++t) {
    const int32_t d = relation_draw(seed, 0x6e6cu, 0x6e6du, 2 * (j * (uint64_t)RGCN_NEG_MAX_DRAWS + t), R);
    e = d + (d >= r ? 1 : 0);
    ++out.lookups;
    if (!known_has(k, base + (uint64_t)e * stride)) {
      out.relation = e;
      return out;
    }
  }
  // all T candidates are known: the first free relation upward (cyclically) from the last one, r itself passed over
  for (int32_t step = 1; step < R; ++step) {
    e = e + 1 == R ? 0 : e + 1;
    if (e == r) continue;
    ++out.lookups;
    if (!known_has(k, base + (uint64_t)e * stride)) {
      out.relation = e;
      return out;
    }
  }
  out.unresolved = 1;      // (relation is still attempt 0's)
  return out;
}

}  // namespace rgcn
