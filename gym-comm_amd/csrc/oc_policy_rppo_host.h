// oc_policy_rppo_host.h -- the host half the recurrent update's two units share: the argument checks, the plan, the
// carve of `scratch` and the six launches of one minibatch (include/oc_policy.h: oc_policy_rppo_update / _grad,
// oc_policy_recurrent_train_step).  Included by oc_policy_rppo.hip (TRAIN = false) and oc_policy_rtrain.hip
// (TRAIN = true): rppo_launch<TRAIN> instantiates that unit's kernels only.  gfx950 only.
#ifndef OC_POLICY_RPPO_HOST_H
#define OC_POLICY_RPPO_HOST_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/oc_policy.h"
#include "oc_policy_fail.h"
#include "oc_policy_layout.h"
#include "oc_policy_rppo_device.h"

namespace ocpol {

constexpr const char *RPPO_SHAPE_RULE =
    "1 <= F, F + 2 <= 64, 1 <= C <= 16, T >= 1, E >= 1, 2 <= E T < 2^31, max_groups >= 0";

inline bool rppo_bad_shape(int32_t F, int32_t C, int32_t T, int32_t E, int32_t max_groups) {
  return F < 1 || F + 2 > 64 || C < 1 || C > OC_POLICY_MAX_COMM || T < 1 || E < 1 || (int64_t)E * T < 2 ||
         (int64_t)E * T >= ((int64_t)1 << 31) || max_groups < 0;
}

// plan (include/oc_policy.h): Gf, Gw, tiles per weight-gradient workgroup, P, scratch floats, Gr, launches,
// scratch floats per sample
inline void rppo_make_plan(int32_t F, int32_t C, int32_t T, int32_t E, int32_t max_groups, int64_t *plan) {
  const int64_t tiles = ((int64_t)E + 31) / 32, total = tiles * T, P = RppoLayout(F, C).P;
  const int64_t cap = max_groups > 0 ? max_groups : RPPO_DEFAULT_GROUPS;
  const int64_t Gw = total < cap ? total : cap, Gr = (P + RPPO_REDUCE_THREADS - 1) / RPPO_REDUCE_THREADS;
  plan[0] = tiles, plan[1] = Gw, plan[2] = (total + Gw - 1) / Gw, plan[3] = P;
  plan[4] = 2 * Gr + (int64_t)RPPO_SAMPLE_FLOATS * T * E + Gw * P + tiles * RPPO_SUMS;
  plan[5] = Gr, plan[6] = 6, plan[7] = RPPO_SAMPLE_FLOATS;
}

inline RppoScratch rppo_carve(float *scratch, const int64_t *plan, int64_t T, int64_t E) {
  RppoScratch s;
  s.sq = (double *)scratch;                       // first: the doubles stay 8-byte aligned
  s.z = scratch + 2 * plan[5];
  s.hs = s.z + 256 * T * E;
  s.cs = s.hs + 64 * T * E;
  s.ds = s.cs + 64 * T * E;
  s.wpart = s.ds + 32 * T * E;
  s.fpart = s.wpart + plan[1] * plan[3];
  return s;
}

// the checks of one minibatch, made before any device work
inline int rppo_check(const char *who, const oc_rppo_cfg *c, const int32_t *envs, int32_t E, bool apply) {
  if (!c || !envs) return fail("%s: bad argument (cfg, envs)", who);
  if (rppo_bad_shape(c->F, c->C, c->T, E, c->max_groups)) return fail("%s: bad argument (%s)", who, RPPO_SHAPE_RULE);
  if (c->obs_type < 0 || c->obs_type > 2 || c->n < 1 || (int64_t)c->T * c->n >= ((int64_t)1 << 31) ||
      (int64_t)HIDDEN * c->n >= ((int64_t)1 << 31))
    return fail("%s: bad argument (obs_type 0..2, n >= 1, T * n and 64 * n must stay below 2^31)", who);
  if (!c->obs || !c->timestep || !c->actions || !c->log_probs || !c->advantages || !c->returns || !c->episode_starts ||
      !c->h0 || !c->c0 || !c->gates || !c->head || !c->head_bias || !c->bwd || !c->grad || !c->scratch || !c->stats ||
      !c->hyper)
    return fail("%s: a NULL pointer among the rollout tensors, h0 / c0, images, grad, scratch, stats, hyper", who);
  if (((uintptr_t)c->scratch & 7) != 0) return fail("%s: scratch must be 8-byte aligned", who);
  if (apply && (!c->p_wx || !c->p_wt || !c->p_b || !c->p_wh || !c->p_w2 || !c->p_b2 || !c->p_wv || !c->p_bv || !c->m ||
                !c->v || !c->step))
    return fail("%s: a NULL pointer among the master weights, m, v, step", who);
  return 0;
}

// the six launches of a checked minibatch.  TRAIN: `train` rides behind the cfg and the update is always applied
// (the unit holds k_rppo_finish<true, true> only); otherwise `train` is not looked at
template <bool TRAIN>
int rppo_launch(const char *who, const oc_rppo_cfg *c, const oc_ppo_train *train, const int32_t *envs, int32_t E,
                void *stream, bool apply) {
  int64_t plan[8];
  rppo_make_plan(c->F, c->C, c->T, E, c->max_groups, plan);
  const RppoScratch sc = rppo_carve(c->scratch, plan, c->T, E);
  const int B = (int)((int64_t)E * c->T), Gf = (int)plan[0], Gw = (int)plan[1], per = (int)plan[2], P = (int)plan[3];
  const int Gr = (int)plan[5];
  RppoArgs<TRAIN> a;
  static_cast<oc_rppo_cfg &>(a) = *c;
  RppoOut<TRAIN> stats, grad;
  stats.to = c->stats, grad.to = c->grad;
  if constexpr (TRAIN) a.tr = *train, stats.ctl = train->ctl, grad.ctl = train->ctl;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_rppo_adv<TRAIN>, dim3(1), dim3(PPO_FINISH_THREADS), 0, st, c->advantages, envs, (int)E, B,
                     (uint32_t)c->n, stats);
  const dim3 gf((unsigned)Gf), gw((unsigned)Gw);
  if (c->obs_type == 1) hipLaunchKernelGGL((k_rppo_forward<1, TRAIN>), gf, dim3(64), 0, st, a, envs, (int)E, sc);
  else if (c->obs_type == 2) hipLaunchKernelGGL((k_rppo_forward<2, TRAIN>), gf, dim3(64), 0, st, a, envs, (int)E, sc);
  else hipLaunchKernelGGL((k_rppo_forward<0, TRAIN>), gf, dim3(64), 0, st, a, envs, (int)E, sc);
  hipLaunchKernelGGL(k_rppo_backward<TRAIN>, gf, dim3(64), 0, st, a, envs, (int)E, sc);
  if (c->obs_type == 1) hipLaunchKernelGGL((k_rppo_wgrad<1, TRAIN>), gw, dim3(256), 0, st, a, envs, (int)E, Gf, per, sc);
  else if (c->obs_type == 2) hipLaunchKernelGGL((k_rppo_wgrad<2, TRAIN>), gw, dim3(256), 0, st, a, envs, (int)E, Gf, per, sc);
  else hipLaunchKernelGGL((k_rppo_wgrad<0, TRAIN>), gw, dim3(256), 0, st, a, envs, (int)E, Gf, per, sc);
  hipLaunchKernelGGL(k_rppo_reduce<TRAIN>, dim3((unsigned)Gr), dim3(RPPO_REDUCE_THREADS), 0, st, sc, Gw, P, (float)B, grad);
  if constexpr (TRAIN) {
    hipLaunchKernelGGL((k_rppo_finish<true, true>), dim3(1), dim3(PPO_FINISH_THREADS), 0, st, a, B, Gf, Gr, sc);
  } else {
    if (apply) hipLaunchKernelGGL((k_rppo_finish<true>), dim3(1), dim3(PPO_FINISH_THREADS), 0, st, a, B, Gf, Gr, sc);
    else hipLaunchKernelGGL((k_rppo_finish<false>), dim3(1), dim3(PPO_FINISH_THREADS), 0, st, a, B, Gf, Gr, sc);
  }
  return ppo_launched(who);
}

}  // namespace ocpol
#endif
