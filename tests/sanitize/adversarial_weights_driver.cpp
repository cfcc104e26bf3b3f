// Stand-alone driver of the self-adversarial weights' host-and-device text, for a plain g++ build under AddressSanitizer
// and UndefinedBehaviorSanitizer (tests/test_adversarial_host.py):
//   csrc/adversarial_weights.h     the softmax of one group, which k_adv_weights evaluates element by element
//
//   adversarial_weights_driver CASES.txt
//
// CASES.txt holds
//   case NAME K ALPHA, then K energies -> "case NAME K", K lines "w VALUE" (%.9g: a float32 round trip), "end NAME".
// Every group is computed twice: into a separate array of exactly K floats, and in place over a copy of the energies
// (the header allows both); the two must agree bit for bit.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../relationprediction_amd/csrc/adversarial_weights.h"

using namespace rgcn;

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: adversarial_weights_driver CASES.txt\n");
    return 2;
  }
  FILE* f = fopen(argv[1], "r");
  if (!f) {
    fprintf(stderr, "cannot open %s\n", argv[1]);
    return 2;
  }
  char word[64], name[64];
  while (fscanf(f, "%63s", word) == 1) {
    if (strcmp(word, "case")) return 3;
    long long K;
    float alpha;
    if (fscanf(f, "%63s %lld %f", name, &K, &alpha) != 3 || K < 1) return 3;
    std::vector<float> x((size_t)K), w((size_t)K);
    for (long long i = 0; i < K; ++i)
      if (fscanf(f, "%f", &x[(size_t)i]) != 1) return 3;
    adversarial_group_weights(x.data(), (int32_t)K, alpha, w.data());
    std::vector<float> inplace(x);
    adversarial_group_weights(inplace.data(), (int32_t)K, alpha, inplace.data());
    if (memcmp(inplace.data(), w.data(), sizeof(float) * (size_t)K) != 0) return 4;
    printf("case %s %lld\n", name, K);
    for (long long i = 0; i < K; ++i) printf("w %.9g\n", (double)w[(size_t)i]);
    printf("end %s\n", name);
  }
  fclose(f);
  printf("adversarial_weights_driver: ok\n");
  return 0;
}
