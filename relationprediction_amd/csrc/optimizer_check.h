// check_optimizer_params: every set of hyper-parameters rgcn_optimizer_config / rgcn_optimizer_config_ex refuse before they
// touch the context, in the order below -- where a set breaks several rules, the first one decides the message.
// Pure host arithmetic on rgcn_optimizer_params: depends on include/rgcn.h and the standard library only, no HIP and no
// rgcn_ctx (tests/sanitize/optimizer_check_driver.cpp prints its answers, tests/test_optimizers_host.py holds them as literals).
#pragma once

#include <cstdint>
#include <string>

#include "../../include/rgcn.h"

namespace rgcn {

struct OptimizerVerdict {
  rgcn_status status;
  std::string message;      // empty when status is RGCN_OK
};

// Reads struct_size first and nothing else of a struct that announces another size.  beta1, beta2 and epsilon are Adam's
// and initial_accumulator is AdaGrad's: an algorithm does not look at the fields of another.
inline OptimizerVerdict check_optimizer_params(const rgcn_optimizer_params* p) {
  if (!p) return OptimizerVerdict{RGCN_ERR_INVALID, "rgcn_optimizer_config_ex: NULL parameters"};
  if (p->struct_size != (int32_t)sizeof(rgcn_optimizer_params))
    return OptimizerVerdict{RGCN_ERR_INVALID, "rgcn_optimizer_params::struct_size is not sizeof(rgcn_optimizer_params)"};
  if (p->algorithm != RGCN_OPT_ADAM && p->algorithm != RGCN_OPT_GRADIENT_DESCENT && p->algorithm != RGCN_OPT_ADAGRAD)
    return OptimizerVerdict{RGCN_ERR_INVALID, "unknown optimizer algorithm (0: Adam, 1: GradientDescent, 2: AdaGrad)"};
  // (the ranges rgcn_optimizer_config has always held Adam to; a NaN rate fails its test)
  if (!(p->learning_rate > 0.f) || p->max_grad_norm < 0.f)
    return OptimizerVerdict{RGCN_ERR_INVALID, "bad optimizer hyper-parameters"};
  if (p->algorithm == RGCN_OPT_ADAM &&
      (!(p->beta1 >= 0.f && p->beta1 < 1.f) || !(p->beta2 >= 0.f && p->beta2 < 1.f) || !(p->epsilon > 0.f)))
    return OptimizerVerdict{RGCN_ERR_INVALID, "bad optimizer hyper-parameters"};
  if (p->algorithm == RGCN_OPT_ADAGRAD && !(p->initial_accumulator > 0.f))
    return OptimizerVerdict{RGCN_ERR_INVALID, "AdaGrad's initial_accumulator must be positive (a zero accumulator under a "
                                              "zero gradient is 0 / 0)"};
  return OptimizerVerdict{RGCN_OK, ""};
}

}  // namespace rgcn
