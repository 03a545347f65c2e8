// oc_policy_ppo.hip -- the PPO update's entry points of liboc_policy.so (include/oc_policy.h:
// oc_policy_ppo_plan / _update / _grad); the kernels are in oc_policy_ppo_device.h.  A translation
// unit of its own: oc_policy.hip and its code object stay as they were.  gfx950 only.
// (The train sequence's entry points and its variants of these kernels: oc_policy_train.hip.)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/oc_policy.h"
#include "oc_policy_fail.h"
#include "oc_policy_ppo_device.h"

using namespace ocpol;

extern "C" {

int oc_policy_ppo_plan(int32_t F, int32_t C, int32_t B, int32_t max_groups, int32_t *plan) {
  if (!plan || F < 1 || F + 2 > 16 * ocpol::MAX_KSTEPS || C < 1 || C > OC_POLICY_MAX_COMM || B < 2 || max_groups < 0)
    return fail("oc_policy_ppo_plan: bad argument (1 <= F, F + 2 <= 48, 1 <= C <= 16, B >= 2, max_groups >= 0)");
  const int64_t tiles = ((int64_t)B + 31) / 32;
  int64_t G = (tiles + ocpol::PPO_WAVES - 1) / ocpol::PPO_WAVES;   // at most one tile per wave ...
  const int64_t cap = max_groups > 0 ? max_groups : 64;            // ... up to a cap: the finish sums G partials
  if (G > cap) G = cap;
  const int64_t waves = G * ocpol::PPO_WAVES, P = ocpol::PpoLayout(F, C).P;
  plan[0] = (int32_t)G, plan[1] = (int32_t)((tiles + waves - 1) / waves), plan[2] = (int32_t)P;
  plan[3] = (int32_t)(G * (P + ocpol::PPO_SUMS));
  return 0;
}

}  // extern "C"

// the checks of one minibatch, for both translation units (declared in oc_policy_ppo_device.h)
int ocpol::ppo_check(const char *who, const oc_ppo_cfg *c, const int32_t *idx, int32_t B, bool apply, int32_t *plan) {
  if (!c || !idx) return fail("%s: bad argument (cfg, idx)", who);
  if (oc_policy_ppo_plan(c->F, c->C, B, c->max_groups, plan) != 0)
    return fail("%s: bad argument (1 <= F, F + 2 <= 48, 1 <= C <= 16, B >= 2, max_groups >= 0)", who);
  if (c->obs_type < 0 || c->obs_type > 2 || c->T < 1 || c->n < 1 || (int64_t)c->T * c->n >= ((int64_t)1 << 31))
    return fail("%s: bad argument (obs_type 0..2, T >= 1, n >= 1, T * n must stay below 2^31)", who);
  if (!c->obs || !c->timestep || !c->actions || !c->log_probs || !c->advantages || !c->returns || !c->w1 || !c->w2 ||
      !c->b2 || !c->w2t || !c->grad || !c->scratch || !c->stats || !c->hyper)
    return fail("%s: a NULL pointer among the rollout tensors, packed weights, grad, scratch, stats, hyper", who);
  if (apply && (!c->p_w1 || !c->p_wt || !c->p_b1 || !c->p_w2 || !c->p_b2 || !c->p_wv || !c->p_bv || !c->m || !c->v || !c->step))
    return fail("%s: a NULL pointer among the master weights, m, v, step", who);
  return 0;
}

namespace {
int ppo_launch(const char *who, const oc_ppo_cfg *c, const int32_t *idx, int32_t B, void *stream, bool apply) {
  int32_t plan[4];
  if (ppo_check(who, c, idx, B, apply, plan) != 0) return -1;
  const PpoArgs<false> a{*c};
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_ppo_adv<false>, dim3(1), dim3(PPO_FINISH_THREADS), 0, st, c->advantages, idx, (int)B, AdvOut<false>{c->stats});
  const dim3 g((unsigned)plan[0]), b(64 * PPO_WAVES);
  if (c->obs_type == 1) hipLaunchKernelGGL((k_ppo_grad<1>), g, b, 0, st, a, idx, (int)B, (int)plan[1], c->scratch);
  else if (c->obs_type == 2) hipLaunchKernelGGL((k_ppo_grad<2>), g, b, 0, st, a, idx, (int)B, (int)plan[1], c->scratch);
  else hipLaunchKernelGGL((k_ppo_grad<0>), g, b, 0, st, a, idx, (int)B, (int)plan[1], c->scratch);
  if (apply) hipLaunchKernelGGL((k_ppo_finish<true>), dim3(1), dim3(PPO_FINISH_THREADS), 0, st, a, (int)B, (int)plan[0], (const float *)c->scratch);
  else hipLaunchKernelGGL((k_ppo_finish<false>), dim3(1), dim3(PPO_FINISH_THREADS), 0, st, a, (int)B, (int)plan[0], (const float *)c->scratch);
  return ppo_launched(who);
}

}  // namespace

extern "C" {
int oc_policy_ppo_update(const oc_ppo_cfg *cfg, const int32_t *idx, int32_t B, void *stream) {
  return ppo_launch("oc_policy_ppo_update", cfg, idx, B, stream, true);
}
int oc_policy_ppo_grad(const oc_ppo_cfg *cfg, const int32_t *idx, int32_t B, void *stream) {
  return ppo_launch("oc_policy_ppo_grad", cfg, idx, B, stream, false);
}

}  // extern "C"
