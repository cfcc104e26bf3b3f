// Driver of the optimizer's hyper-parameter rules (csrc/optimizer_check.h check_optimizer_params: pure host C++, nothing from
// HIP) for tests/test_optimizers_host.py, built with AddressSanitizer / UndefinedBehaviorSanitizer like
// config_check_driver.cpp.  One line per named parameter set: `name: status|message` as rgcn_optimizer_config_ex answers;
// the test holds the expected lines as literals.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../relationprediction_amd/csrc/optimizer_check.h"

using namespace rgcn;

// the settings files' values: Adam 0.01 with TensorFlow's defaults, clip at 1
static rgcn_optimizer_params base(int32_t algorithm) {
  rgcn_optimizer_params p{};
  p.struct_size = (int32_t)sizeof(rgcn_optimizer_params);
  p.algorithm = algorithm;
  p.learning_rate = 0.01f;
  p.beta1 = 0.9f;
  p.beta2 = 0.999f;
  p.epsilon = 1e-8f;
  p.max_grad_norm = 1.0f;
  p.initial_accumulator = 0.1f;
  return p;
}
static rgcn_optimizer_params with(rgcn_optimizer_params p, float rgcn_optimizer_params::*field, float value) {
  p.*field = value;
  return p;
}

static void show(const char* name, const rgcn_optimizer_params* p) {
  const OptimizerVerdict v = check_optimizer_params(p);
  std::printf("%s: %d|%s\n", name, (int)v.status, v.message.c_str());
}
static void show(const char* name, const rgcn_optimizer_params& p) { show(name, &p); }

int main() {
  const rgcn_optimizer_params adam = base(RGCN_OPT_ADAM), sgd = base(RGCN_OPT_GRADIENT_DESCENT),
                              adagrad = base(RGCN_OPT_ADAGRAD);
  using P = rgcn_optimizer_params;
  show("ok_adam", adam);
  show("ok_gradient_descent", sgd);
  show("ok_adagrad", adagrad);
  show("ok_no_clip", with(adagrad, &P::max_grad_norm, 0.f));
  show("ok_beta1_0", with(adam, &P::beta1, 0.f));
  show("null", (const rgcn_optimizer_params*)nullptr);
  // the struct: only struct_size is read of one that announces another size (the rest of this one is a byte pattern)
  {
    unsigned char raw[sizeof(P)];
    std::memset(raw, 0xA5, sizeof raw);
    P junk;
    std::memcpy(&junk, raw, sizeof junk);
    junk.struct_size = (int32_t)sizeof(P) - 4;
    show("struct_size_short", junk);
    junk.struct_size = (int32_t)sizeof(P) + 4;
    show("struct_size_long", junk);
    junk.struct_size = 0;
    show("struct_size_0", junk);
  }
  show("algorithm_3", base(3));
  show("algorithm_negative", base(-1));
  for (const P& p : {adam, sgd, adagrad}) {
    const char* tag = p.algorithm == RGCN_OPT_ADAM ? "adam" : p.algorithm == RGCN_OPT_ADAGRAD ? "adagrad" : "gradient_descent";
    char name[64];
    std::snprintf(name, sizeof name, "%s_rate_0", tag);
    show(name, with(p, &P::learning_rate, 0.f));
    std::snprintf(name, sizeof name, "%s_rate_negative", tag);
    show(name, with(p, &P::learning_rate, -0.01f));
    std::snprintf(name, sizeof name, "%s_rate_nan", tag);
    show(name, with(p, &P::learning_rate, std::nanf("")));
    std::snprintf(name, sizeof name, "%s_clip_negative", tag);
    show(name, with(p, &P::max_grad_norm, -1.f));
  }
  // Adam's ranges
  show("adam_beta1_1", with(adam, &P::beta1, 1.f));
  show("adam_beta1_negative", with(adam, &P::beta1, -0.1f));
  show("adam_beta2_1", with(adam, &P::beta2, 1.f));
  show("adam_epsilon_0", with(adam, &P::epsilon, 0.f));
  // ... are Adam's: the other two do not read them
  show("gradient_descent_ignores_beta1", with(sgd, &P::beta1, 7.f));
  show("adagrad_ignores_epsilon", with(adagrad, &P::epsilon, 0.f));
  // AdaGrad's accumulator
  show("adagrad_accumulator_0", with(adagrad, &P::initial_accumulator, 0.f));
  show("adagrad_accumulator_negative", with(adagrad, &P::initial_accumulator, -0.1f));
  show("adagrad_accumulator_nan", with(adagrad, &P::initial_accumulator, std::nanf("")));
  show("adam_ignores_accumulator", with(adam, &P::initial_accumulator, 0.f));
  show("gradient_descent_ignores_accumulator", with(sgd, &P::initial_accumulator, -1.f));
  // two rules at once: the struct, then the algorithm, then the rate, then the algorithm's own
  show("both_algorithm_and_rate", with(base(9), &P::learning_rate, 0.f));
  show("both_rate_and_accumulator", with(with(adagrad, &P::learning_rate, 0.f), &P::initial_accumulator, 0.f));
  std::printf("optimizer_check_driver: ok\n");
  return 0;
}
