// Stand-alone driver of the entity-softmax term's host-side code: csrc/entity_softmax_plan.h (the plan of every named
// case, one per line, for tests/test_entity_softmax_host.py to pin, then a sweep of the plan's invariants),
// csrc/entity_softmax_range.h (the range lookup's edge cases, then every pair of a small random index against a linear
// scan) and known_index_build_by_object of csrc/known_positives_index.h.  Built with g++ under AddressSanitizer and
// UndefinedBehaviorSanitizer and run as a program.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../relationprediction_amd/csrc/entity_softmax_plan.h"
#include "../../relationprediction_amd/csrc/entity_softmax_range.h"
#include "../../relationprediction_amd/csrc/known_positives_index.h"

using namespace rgcn;

static int failures = 0;

static void check(bool ok, const char* what, long long a, long long b, long long c, long long d) {
  if (ok) return;
  std::printf("FAILED %s at %lld %lld %lld %lld\n", what, a, b, c, d);
  ++failures;
}

static void show(const char* name, long long max_positives, int V, int dc, size_t slab) {
  const EntsmPlan p = entsm_plan(max_positives, V, dc, slab);
  std::printf("%s: chunk=%lld padded_v=%d split=%d nn_padded=%d\n", name, (long long)p.chunk, p.padded_v, p.split_k, p.nn_padded);
}

// the range of (a, r) in an index built from `triples`, printed and returned; by_object: the second index
static EntsmRange show_range(const char* name, const std::vector<int32_t>& triples, int V, int R, int a, int r, bool by_object) {
  std::vector<uint64_t> keys;
  std::string err;
  const int64_t n = (int64_t)triples.size() / 3;
  const rgcn_status st = by_object ? known_index_build_by_object(triples.data(), n, V, R, &keys, &err)
                                   : known_index_build(triples.data(), n, V, R, &keys, &err);
  check(st == RGCN_OK, "index build", a, r, V, R);
  // (an empty index is passed as a null pointer, as a context without keys would)
  const EntsmRange g = entsm_range(keys.empty() ? nullptr : keys.data(), (int64_t)keys.size(), entsm_base(a, r, V), (uint64_t)V);
  std::printf("%s: lo=%lld hi=%lld of %lld\n", name, (long long)g.lo, (long long)g.hi, (long long)keys.size());
  for (int64_t i = g.lo; i < g.hi; ++i) std::printf("%s[%lld]: %lld\n", name, (long long)(i - g.lo), (long long)(keys[(size_t)i] - entsm_base(a, r, V)));
  return g;
}

int main() {
  // ---- the plan.  What the library runs: the term's own slabs, kEntsmSlabFloats.  FB15k-237 (V = 14,541, d = 500): the
  // minibatch (30,000 positives) and the Name=embedding iteration (272,115)
  show("fb237_minibatch", 30000, 14541, 500, kEntsmSlabFloats);
  show("fb237_embedding", 272115, 14541, 500, kEntsmSlabFloats);
  // the 256 MB boundary at V = 14,541: 4,608 rows x 14,544 floats fit (268,075,008 bytes), a 37th tile of rows does not
  show("boundary_below", 2303, 14541, 500, kEntsmSlabFloats);
  show("boundary_at", 2304, 14541, 500, kEntsmSlabFloats);
  show("boundary_above", 2305, 14541, 500, kEntsmSlabFloats);
  show("reserve_64", 64, 90, 8, kEntsmSlabFloats);
  show("two_slices", 150, 300, 8, kEntsmSlabFloats);
  show("one_positive", 1, 2, 6, kEntsmSlabFloats);
  show("v_multiple_of_4", 4096, 256, 128, kEntsmSlabFloats);
  show("huge_v", 1000, 2000000, 8, kEntsmSlabFloats);
  show("bad_arguments", 0, 18, 8, kEntsmSlabFloats);
  show("bad_entities", 10, 0, 8, kEntsmSlabFloats);
  show("slab_limit_5", 3000, 300, 8, (size_t)5 * 300 * 8 + 7);
  show("slab_limit_0", 3000, 300, 8, 0);
  std::printf("own_slab_floats: %lld\n", (long long)kEntsmSlabFloats);
  std::printf("energy_floats: %lld\n", (long long)kEntsmEnergyFloats);
  std::printf("cuts: long_row=%d piece=%d\n", kEntsmLongRow, kEntsmPiece);

  const long long positives[] = {1, 2, 63, 64, 65, 127, 128, 129, 2303, 2304, 2305, 32767, 32768, 32769, 65536, 272115, 1ll << 29};
  const int entities[] = {1, 2, 3, 4, 5, 63, 64, 65, 257, 300, 14541, 40943, 1 << 24};
  const int dims[] = {1, 6, 8, 132, 500, 1024};
  const size_t slabs[] = {0, 1, 1024, (size_t)128 * 128, (size_t)16 * 500 * 500, (size_t)1 << 30};
  for (long long P : positives)
    for (int V : entities)
      for (int dc : dims)
        for (size_t slab : slabs) {
          const EntsmPlan p = entsm_plan(P, V, dc, slab);
          const long long rows = 2 * P;
          check(p.padded_v >= V && p.padded_v < V + 4 && p.padded_v % 4 == 0, "padded_v", P, V, dc, (long long)slab);
          check(p.nn_padded == (V % 4 != 0), "nn form", P, V, dc, (long long)slab);
          check(p.chunk >= 1 && p.chunk <= rows && p.chunk <= kEntsmMaxChunk, "chunk range", P, V, dc, (long long)slab);
          check(p.chunk == rows || p.chunk % 128 == 0, "chunk of whole tiles", P, V, dc, (long long)slab);
          check(p.chunk == rows || p.chunk == 128 || p.chunk * (long long)p.padded_v <= kEntsmEnergyFloats, "energy buffer",
                P, V, dc, (long long)slab);
          check(p.split_k >= 1 && p.split_k <= kEntsmMaxSplit, "split range", P, V, dc, (long long)slab);
          check(p.split_k == 1 || (size_t)p.split_k * (size_t)p.padded_v * (size_t)dc <= slab, "split fits the slab", P, V,
                dc, (long long)slab);
          check(p.split_k == 1 || p.chunk / p.split_k >= kEntsmSplitRows, "slice depth", P, V, dc, (long long)slab);
          int last = 1;
          for (long long n : {1ll, (long long)p.chunk / 2 + 1, (long long)p.chunk}) {
            const int s = entsm_split(n, p.padded_v, dc, slab);
            check(s >= last && s <= p.split_k, "a shorter chunk never splits further", P, V, dc, (long long)slab);
            check(s == 1 || n / s >= kEntsmSplitRows, "slice depth of a short chunk", P, V, dc, (long long)slab);
            last = s;
          }
        }

  // ---- the range lookup's edge cases (V = 5, R = 3)
  const int V = 5, R = 3;
  {
    const EntsmRange g = show_range("empty_index", {}, V, R, 2, 1, false);
    check(g.lo == 0 && g.hi == 0, "empty index", 0, 0, 0, 0);
  }
  {
    // key 0 is (s, r, o) = (0, 0, 0); the pair (0, 0) also knows object 3
    const EntsmRange g = show_range("range_at_key_0", {0, 0, 0, 0, 0, 3, 1, 0, 0}, V, R, 0, 0, false);
    check(g.lo == 0 && g.hi == 2, "range at key 0", g.lo, g.hi, 0, 0);
  }
  {
    // the last key there is: (V - 1, R - 1, V - 1)
    const EntsmRange g = show_range("range_at_last_key", {0, 0, 0, 4, 2, 4, 4, 2, 1}, V, R, 4, 2, false);
    check(g.lo == 1 && g.hi == 3, "range at the last key", g.lo, g.hi, 0, 0);
  }
  {
    const EntsmRange g = show_range("whole_index", {2, 1, 0, 2, 1, 4, 2, 1, 2, 2, 1, 4}, V, R, 2, 1, false);
    check(g.lo == 0 && g.hi == 3, "the whole index (a duplicate removed)", g.lo, g.hi, 0, 0);
  }
  {
    // (2, 1) between (1, 1, 4), the last key of the pair before it, and (3, 1, 0), the first key of the pair after it
    const std::vector<int32_t> t = {1, 1, 4, 2, 1, 0, 2, 1, 4, 3, 1, 0, 2, 0, 2, 2, 2, 2};
    const EntsmRange g = show_range("between_neighbours", t, V, R, 2, 1, false);
    check(g.hi - g.lo == 2, "between neighbours", g.lo, g.hi, 0, 0);
    const EntsmRange none = show_range("absent_between_neighbours", {1, 1, 4, 3, 1, 0}, V, R, 2, 1, false);
    check(none.lo == none.hi && none.lo == 1, "an absent pair between neighbours", none.lo, none.hi, 0, 0);
    // the same triples by object: the known subjects of (r, o) = (1, 0) are 2 and 3
    const EntsmRange sub = show_range("subjects_of_a_pair", t, V, R, 0, 1, true);
    check(sub.hi - sub.lo == 2, "subjects of a pair", sub.lo, sub.hi, 0, 0);
  }

  // ---- the second index: errors leave *keys alone; every pair of a random index against a linear scan, both orders
  {
    std::vector<uint64_t> keys = {42};
    std::string err;
    const int32_t bad[] = {0, 0, 0, 1, 0, 5};
    check(known_index_build_by_object(bad, 2, V, R, &keys, &err) == RGCN_ERR_INVALID && keys.size() == 1 && keys[0] == 42 &&
              err.find("known positive 1") != std::string::npos, "an id out of range", 0, 0, 0, 0);
    check(known_index_build_by_object(nullptr, 2, V, R, &keys, &err) == RGCN_ERR_INVALID && keys.size() == 1, "NULL triples", 0, 0, 0, 0);
    check(known_index_build_by_object(nullptr, 0, V, R, &keys, &err) == RGCN_OK && keys.empty(), "no triples", 0, 0, 0, 0);
  }
  unsigned state = 12345u;
  auto next = [&state](int mod) { state = state * 1664525u + 1013904223u; return (int)((state >> 8) % (unsigned)mod); };
  for (int round = 0; round < 20; ++round) {
    const int v = 2 + next(9), r = 1 + next(4), n = next(60);
    std::vector<int32_t> t;
    for (int i = 0; i < n; ++i) { t.push_back(next(v)); t.push_back(next(r)); t.push_back(next(v)); }
    std::vector<uint64_t> by_s, by_o;
    std::string err;
    check(known_index_build(t.data(), n, v, r, &by_s, &err) == RGCN_OK, "build", round, 0, 0, 0);
    check(known_index_build_by_object(t.data(), n, v, r, &by_o, &err) == RGCN_OK, "build by object", round, 0, 0, 0);
    check(by_s.size() == by_o.size(), "the two indexes hold the same set", round, (long long)by_s.size(), (long long)by_o.size(), 0);
    for (size_t i = 1; i < by_o.size(); ++i) check(by_o[i - 1] < by_o[i], "sorted and unique", round, (long long)i, 0, 0);
    for (int a = 0; a < v; ++a)
      for (int rel = 0; rel < r; ++rel)
        for (int order = 0; order < 2; ++order) {
          const std::vector<uint64_t>& keys = order ? by_o : by_s;
          const EntsmRange g = entsm_range(keys.empty() ? nullptr : keys.data(), (int64_t)keys.size(), entsm_base(a, rel, v), (uint64_t)v);
          std::vector<int> want(v, 0), got(v, 0);
          for (int i = 0; i < n; ++i)
            if (t[3 * i + 1] == rel && t[3 * i + (order ? 2 : 0)] == a) want[t[3 * i + (order ? 0 : 2)]] = 1;
          check(g.lo >= 0 && g.lo <= g.hi && g.hi <= (int64_t)keys.size(), "range inside the index", round, a, rel, order);
          for (int64_t i = g.lo; i < g.hi; ++i) {
            const uint64_t e = keys[(size_t)i] - entsm_base(a, rel, v);
            check(e < (uint64_t)v, "a key of the range names an entity", round, a, rel, order);
            if (e < (uint64_t)v) got[(size_t)e] = 1;
          }
          check(want == got, "range against a linear scan", round, a, rel, order);
        }
  }
  if (failures) return 1;
  std::printf("entity_softmax_driver: ok\n");
  return 0;
}
