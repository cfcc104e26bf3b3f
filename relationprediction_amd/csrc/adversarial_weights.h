// Self-adversarial weights of one positive's negatives ([General] AdversarialTemperature; Sun et al., RotatE, 2019): the
// softmax of the group's own energies at temperature alpha, scaled so that a group of K negatives sums to K.  ONE text for
// k_adv_weights (adversarial.hip) and for the host: it depends on <cmath>, <cstdint> and counter_rng.h's qualifiers only
// and compiles with a plain C++ compiler (tests/sanitize/adversarial_weights_driver.cpp).
//
//   p_i = exp(alpha x_i - M) / sum_j exp(alpha x_j - M),   M = max_j alpha x_j,   w_i = K p_i
//
// Everything is evaluated in double from the float energies and rounded once, at the end.  The largest term is
// exp(0) = 1, so the sum lies in [1, K] whatever the energies are: a dominating energy gets weight K (to rounding), the
// others underflow to 0, and nothing divides by zero.  An energy of -infinity marks a row that takes no part (an id out of
// range): its term and its weight are 0; a group of such rows alone gets weights 0.
//
// The kernel evaluates adv_scaled / adv_term / adv_weight per element and forms the maximum and the sum with wave
// reductions; adversarial_group_weights below is the same arithmetic with both taken in index order.
#pragma once

#include <cmath>
#include <cstdint>

#include "counter_rng.h"

namespace rgcn {

RGCN_HD inline double adv_scaled(float x, float alpha) { return (double)alpha * (double)x; }

// the term of one energy under the group's maximum M; M == -infinity (no row takes part): 0
RGCN_HD inline double adv_term(double scaled, double M) { return scaled > -INFINITY ? exp(scaled - M) : 0.0; }

// sum >= 1 whenever a row takes part; sum == 0: none does
RGCN_HD inline float adv_weight(double term, double sum, int32_t K) {
  return sum > 0.0 ? (float)((double)K * term / sum) : 0.0f;
}

// w[0..K) from x[0..K); K >= 1, alpha >= 0 finite.  x and w may be the same array.
RGCN_HD inline void adversarial_group_weights(const float* x, int32_t K, float alpha, float* w) {
  double M = -INFINITY;
  for (int32_t i = 0; i < K; ++i) {
    const double a = adv_scaled(x[i], alpha);
    M = a > M ? a : M;
  }
  double sum = 0.0;
  for (int32_t i = 0; i < K; ++i) sum += adv_term(adv_scaled(x[i], alpha), M);
  for (int32_t i = 0; i < K; ++i) w[i] = adv_weight(adv_term(adv_scaled(x[i], alpha), M), sum, K);
}

}  // namespace rgcn
