// Stand-alone driver of csrc/relation_softmax_plan.h (host only): prints the plan of every named case, one per line, for
// tests/test_relation_softmax_host.py to pin, then sweeps the arguments and checks the plan's invariants.  Built with g++
// under AddressSanitizer and UndefinedBehaviorSanitizer and run as a program.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "../../relationprediction_amd/csrc/relation_softmax_plan.h"

using namespace rgcn;

static int failures = 0;

static void check(bool ok, const char* what, long long a, long long b, long long c, long long d) {
  if (ok) return;
  std::printf("FAILED %s at max_positives=%lld R=%lld dc=%lld slab=%lld\n", what, a, b, c, d);
  ++failures;
}

static void show(const char* name, long long max_positives, int R, int dc, size_t slab) {
  const RelsmPlan p = relsm_plan(max_positives, R, dc, slab);
  std::printf("%s: chunk=%lld padded_r=%d split=%d\n", name, (long long)p.chunk, p.padded_r, p.split_k);
}

int main() {
  // what the library runs: every context plans with the term's own slabs, kRelsmSlabFloats.  The FB15k-237 minibatch
  // (30,000 positives) and the Name=embedding iteration (272,115) at d = 500, FB15k's at d = 200
  show("fb237_minibatch", 30000, 237, 500, kRelsmSlabFloats);
  show("fb237_embedding", 272115, 237, 500, kRelsmSlabFloats);
  show("fb15k_embedding", 483142, 1345, 200, kRelsmSlabFloats);
  show("reserve_64", 64, 18, 8, kRelsmSlabFloats);
  show("one_positive", 1, 2, 6, kRelsmSlabFloats);
  show("r_multiple_of_4", 4096, 256, 128, kRelsmSlabFloats);
  show("huge_r", 1000, 200000, 8, kRelsmSlabFloats);
  show("bad_arguments", 0, 18, 8, kRelsmSlabFloats);
  show("bad_relations", 10, 0, 8, kRelsmSlabFloats);
  // the function's slab limit, which no context reaches with its own slabs: five slabs of [240, 500], and none
  show("slab_limit_5", 30000, 237, 500, (size_t)5 * 240 * 500 + 7);
  show("slab_limit_0", 30000, 237, 500, 0);
  std::printf("own_slab_floats: %lld\n", (long long)kRelsmSlabFloats);
  std::printf("cuts: long_row=%d piece=%d\n", kRelsmLongRow, kRelsmPiece);

  const long long positives[] = {1, 2, 63, 64, 127, 128, 129, 255, 256, 257, 4095, 65535, 65536, 65537, 272115, 1ll << 29};
  const int relations[] = {1, 2, 3, 4, 5, 18, 67, 237, 256, 257, 1345, 65536, 1 << 24};
  const int dims[] = {1, 6, 8, 132, 500, 1024};
  const size_t slabs[] = {0, 1, 1024, (size_t)128 * 128, (size_t)16 * 500 * 500, (size_t)1 << 30};
  for (long long P : positives)
    for (int R : relations)
      for (int dc : dims)
        for (size_t slab : slabs) {
          const RelsmPlan p = relsm_plan(P, R, dc, slab);
          check(p.padded_r >= R && p.padded_r < R + 4 && p.padded_r % 4 == 0, "padded_r", P, R, dc, (long long)slab);
          check(p.chunk >= 1 && p.chunk <= P && p.chunk <= kRelsmMaxChunk, "chunk range", P, R, dc, (long long)slab);
          check(p.chunk == P || p.chunk % 128 == 0, "chunk of whole tiles", P, R, dc, (long long)slab);
          check(p.chunk == P || p.chunk == 128 || p.chunk * (long long)p.padded_r <= kRelsmEnergyFloats, "energy buffer",
                P, R, dc, (long long)slab);
          check(p.split_k >= 1 && p.split_k <= kRelsmMaxSplit, "split range", P, R, dc, (long long)slab);
          check(p.split_k == 1 || (size_t)p.split_k * (size_t)p.padded_r * (size_t)dc <= slab, "split fits the slab", P, R,
                dc, (long long)slab);
          check(p.split_k == 1 || p.chunk / p.split_k >= kRelsmSplitRows, "slice depth", P, R, dc, (long long)slab);
          for (long long n : {1ll, (long long)p.chunk / 2 + 1, (long long)p.chunk}) {
            const int s = relsm_split(n, p.padded_r, dc, slab);
            check(s >= 1 && s <= kRelsmMaxSplit && (s == 1 || n / s >= kRelsmSplitRows), "split of a short chunk", P, R, dc,
                  (long long)slab);
            check(s == 1 || (size_t)s * (size_t)p.padded_r * (size_t)dc <= slab, "short split fits", P, R, dc, (long long)slab);
          }
        }
  if (failures) return 1;
  std::printf("relation_softmax_plan_driver: ok\n");
  return 0;
}
