// The counter-based generator of the negative samplers: one splitmix64 finaliser per draw, 24 bits out.  Nothing but
// <cstdint>: the device kernels, the host code of librgcn.so and a plain g++ build (tests/sanitize/) read the same text.
#pragma once

#include <cstdint>

// host-and-device qualifiers where the compiler knows them, nothing under a plain C++ compiler
#if defined(__HIPCC__) || defined(__CUDACC__)
#define RGCN_HD __host__ __device__
#else
#define RGCN_HD
#endif

namespace rgcn {

RGCN_HD inline uint64_t splitmix64_mix(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// draw `idx` (< 2^44) of stream `layer` under `seed`: uniform in [0, 2^24)
RGCN_HD inline uint32_t drop_bits(uint64_t seed, uint32_t layer, uint64_t idx) {
  return (uint32_t)(splitmix64_mix(seed + 0x9E3779B97F4A7C15ull * (idx + ((uint64_t)layer << 44) + 1ull)) >> 40);
}

}  // namespace rgcn
