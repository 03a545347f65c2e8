// oc_policy_train.hip -- the train sequence's entry points of liboc_policy.so (include/oc_policy.h, the
// last section: oc_policy_ppo_train_begin / _epoch_begin / _train_step / _perm_host).  The third
// translation unit and code object of the library: the two before it stay as they were.  Its kernels
// are the TRAIN = true variants of oc_policy_ppo_device.h's and the three small ones below.  gfx950 only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/oc_policy.h"
#include "oc_policy_fail.h"
#include "oc_policy_ppo_device.h"
#include "oc_policy_shuffle.h"

using namespace ocpol;

namespace {

constexpr int PERM_THREADS = 256;

// one thread: a new train() -- everything but the epoch counter and the error word
__global__ void __launch_bounds__(64) k_ppo_train_begin(const oc_ppo_train t) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  t.ctl[OC_PPO_CTL_STOP] = 0, t.ctl[OC_PPO_CTL_UPDATES] = 0, t.ctl[OC_PPO_CTL_EPOCHS] = 0;
  for (int k = 0; k < OC_PPO_ACC_WORDS; k++) t.acc[k] = 0.0;
}

// one thread: the epoch before is closed (the KL rule, in double), a new one opened
__global__ void __launch_bounds__(64) k_ppo_epoch_close(const oc_ppo_train t) {
  if (blockIdx.x != 0 || threadIdx.x != 0 || ppo_halted(t.ctl)) return;
  const double count = t.acc[OC_PPO_ACC_EPOCH_COUNT];
  if (count > 0.0) {
    const float target = t.hyper_ext[1];
    t.ctl[OC_PPO_CTL_EPOCHS] += 1;
    const double mean = t.acc[OC_PPO_ACC_EPOCH_KL] / count;
    if (target > 0.0f && mean > 1.5 * (double)target) t.ctl[OC_PPO_CTL_STOP] = 1;
  }
  t.acc[OC_PPO_ACC_EPOCH_KL] = 0.0, t.acc[OC_PPO_ACC_EPOCH_COUNT] = 0.0;
  if (t.ctl[OC_PPO_CTL_STOP] == 0) t.ctl[OC_PPO_CTL_EPOCH] += 1;
}

// one thread per element of idx: element e = i * granule + j takes perm[i] * granule + j.  The
// epoch number was fixed by the launch before; no thread of this launch writes a word another reads.
__global__ void __launch_bounds__(PERM_THREADS) k_ppo_perm(const oc_ppo_train t, int32_t *idx, const int32_t count,
                                                           const int32_t granule, const uint32_t seed) {
  if (ppo_halted(t.ctl)) return;   // (no barrier below: a thread that sees the error word of this launch just stops)
  const int64_t e = (int64_t)blockIdx.x * PERM_THREADS + threadIdx.x;
  if (e >= (int64_t)count) return;
  const int32_t i = (int32_t)(e / granule), j = (int32_t)(e % granule);
  const Shuffle sh(seed, (uint32_t)(t.ctl[OC_PPO_CTL_EPOCH] - 1), count / granule);
  const int32_t p = sh.at(i);
  if (p < 0) {
    idx[e] = -1;
    t.ctl[OC_PPO_CTL_ERROR] = 1;   // read by LATER launches only: they halt
  } else {
    idx[e] = p * granule + j;
  }
}

}  // namespace

extern "C" {

int oc_policy_ppo_perm_host(uint32_t seed, int32_t epoch, int32_t N, int32_t *out) {
  if (!out || N < 1 || N > SHUFFLE_MAX_N || epoch < 0)
    return fail("oc_policy_ppo_perm_host: bad argument (out, 1 <= N <= 2^30, epoch >= 0)");
  const Shuffle sh(seed, (uint32_t)epoch, N);
  bool cut = false;
  for (int32_t i = 0; i < N; i++) cut |= (out[i] = sh.at(i)) < 0;
  return cut ? fail("oc_policy_ppo_perm_host: a walk reached its cap of %d passes", SHUFFLE_WALK_CAP) : 0;
}

int oc_policy_ppo_train_begin(const oc_ppo_train *train, void *stream) {
  if (train_check("oc_policy_ppo_train_begin", train) != 0) return -1;
  hipLaunchKernelGGL(k_ppo_train_begin, dim3(1), dim3(64), 0, (hipStream_t)stream, *train);
  return ppo_launched("oc_policy_ppo_train_begin");
}

int oc_policy_ppo_epoch_begin(const oc_ppo_train *train, int32_t *idx, int32_t count, int32_t granule, uint32_t seed,
                              void *stream) {
  const char *who = "oc_policy_ppo_epoch_begin";
  if (train_check(who, train) != 0) return -1;
  if (!idx) return fail("%s: bad argument (idx)", who);
  if (count < 1 || granule < 1 || count % granule != 0 || count / granule > SHUFFLE_MAX_N)
    return fail("%s: bad argument (count >= 1, granule >= 1 and dividing count, count / granule <= 2^30)", who);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_ppo_epoch_close, dim3(1), dim3(64), 0, st, *train);
  const unsigned groups = (unsigned)(((int64_t)count + PERM_THREADS - 1) / PERM_THREADS);
  hipLaunchKernelGGL(k_ppo_perm, dim3(groups), dim3(PERM_THREADS), 0, st, *train, idx, count, granule, seed);
  return ppo_launched(who);
}

int oc_policy_ppo_train_step(const oc_ppo_cfg *cfg, const oc_ppo_train *train, const int32_t *idx, int32_t B,
                             void *stream) {
  const char *who = "oc_policy_ppo_train_step";
  int32_t plan[4];
  if (ppo_check(who, cfg, idx, B, true, plan) != 0 || train_check(who, train) != 0) return -1;
  PpoArgs<true> a;
  static_cast<oc_ppo_cfg &>(a) = *cfg;
  a.tr = *train;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_ppo_adv<true>, dim3(1), dim3(PPO_FINISH_THREADS), 0, st, cfg->advantages, idx, (int)B,
                     AdvOut<true>{cfg->stats, train->ctl});
  const dim3 g((unsigned)plan[0]), b(64 * PPO_WAVES);
  if (cfg->obs_type == 1) hipLaunchKernelGGL((k_ppo_grad<1, true>), g, b, 0, st, a, idx, (int)B, (int)plan[1], cfg->scratch);
  else if (cfg->obs_type == 2) hipLaunchKernelGGL((k_ppo_grad<2, true>), g, b, 0, st, a, idx, (int)B, (int)plan[1], cfg->scratch);
  else hipLaunchKernelGGL((k_ppo_grad<0, true>), g, b, 0, st, a, idx, (int)B, (int)plan[1], cfg->scratch);
  hipLaunchKernelGGL((k_ppo_finish<true, true>), dim3(1), dim3(PPO_FINISH_THREADS), 0, st, a, (int)B, (int)plan[0],
                     (const float *)cfg->scratch);
  return ppo_launched(who);
}

}  // extern "C"
