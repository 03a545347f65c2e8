// oc_policy_rtrain.hip -- the recurrent learner's step of the train sequence (include/oc_policy.h, last section:
// oc_policy_recurrent_train_step).  A translation unit and code object of its own, between the recurrent update's
// and the train sequence's: it holds exactly the ten TRAIN = true instantiations of oc_policy_rppo_device.h's
// kernels (statistics, three row types of the forward, the backward, three row types of the weight gradients,
// the reduction, the finish with Adam), launched by the host half it shares with oc_policy_rppo.hip
// (oc_policy_rppo_host.h).  The sequence's other two calls, oc_policy_ppo_train_begin / _epoch_begin, are
// oc_policy_train.hip's as they are.  gfx950 only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/oc_policy.h"
#include "oc_policy_fail.h"
#include "oc_policy_ppo_device.h"
#include "oc_policy_rppo_host.h"

using namespace ocpol;

extern "C" {

int oc_policy_recurrent_train_step(const oc_rppo_cfg *cfg, const oc_ppo_train *train, const int32_t *envs, int32_t E,
                                   void *stream) {
  const char *who = "oc_policy_recurrent_train_step";
  if (rppo_check(who, cfg, envs, E, true) != 0 || train_check(who, train) != 0) return -1;
  return rppo_launch<true>(who, cfg, train, envs, E, stream, true);
}

}  // extern "C"
