/* oc_rollout.h -- C ABI of liboc_rollout.so: the rollout buffer of a learner seated beside the env.
 *
 * What it stands in for: the buffer calls pantheonrl's OnPolicyAgent makes around every env step
 * (pantheonrl/common/agents.py:112-214) -- `buf.add(obs, action, [0], episode_start, value,
 * log_prob)` in get_action, `buf.rewards[pos - 1] += reward` in update, and, when the buffer is
 * full, `buf.compute_returns_and_advantage(last_values, dones)` (stable-baselines3's
 * RolloutBuffer: generalised advantage estimation, newest step to oldest) -- for a whole batch of
 * envs, as ONE launch each.  The buffer is `vec_env.RolloutSink`'s: preallocated [T][...][n]
 * device tensors whose write position is itself a device word, so a call neither synchronises nor
 * depends on anything the host knows: it can sit inside a captured graph.
 *
 * The counters.  `pos` is the next slot, `last` the slot of the most recent add, `count` the adds
 * since the last reset; past T the position wraps (a ring).  oc_rollout_add reads `*pos` in every
 * workgroup before that workgroup's first store; after its last store a workgroup takes a ticket
 * (one returning atomic add on `ticket`, release/acquire at agent scope), and the workgroup that
 * draws the last ticket -- every other one has read `*pos` and finished by then -- alone advances
 * pos / last / count and puts `ticket` back to 0.  `ticket` must be 0 before the first call.  Calls
 * on ONE buffer are ordered by one stream.  A position outside 0..T-1 (only a caller's own write
 * can produce one) is taken modulo T.
 *
 * Chronology.  With L = min(*count, T), step k (0 = oldest .. L-1 = newest) lives in slot
 * (*pos - L + k) mod T: an exactly filled buffer, a wrapped ring and a partly filled one are all
 * described by the two words.
 *
 * oc_rollout_gae, per env, in float32, in exactly this order, never contracted (the library is
 * built with -ffp-contract=off -fno-fast-math):
 *     g = (float)gamma;  gl = (float)(gamma * gae_lambda)      [the product in double]
 *     last = 0
 *     for k = L-1 .. 0:
 *         nnt   = 1 - (k == L-1 ? last_dones : episode_starts[k+1])
 *         nv    =      k == L-1 ? last_values : values[k+1]
 *         delta = ((float)rewards[k] + (g * nv) * nnt) - values[k]
 *         last  = delta + ((gl * nnt) * last)
 *         advantages[k] = last
 *         returns[k]    = last + values[k]
 * Slots that hold no step are not written.
 *
 * Every pointer is a DEVICE pointer of a caller-owned tensor; nothing is allocated, freed or
 * synchronised; arguments are checked before any device work. */
#ifndef OC_ROLLOUT_H
#define OC_ROLLOUT_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#ifndef OC_API
#define OC_API __attribute__((visibility("default")))
#endif

#define OC_ROLLOUT_ABI_VERSION 1

typedef struct {
  void *obs;              /* [T][F][n], element type `obs_type` */
  double *timestep;       /* [T][n] */
  int32_t *actions;       /* [T][2][n] (move, comm) */
  float *log_probs;       /* [T][n] */
  float *values;          /* [T][n] */
  float *episode_starts;  /* [T][n] */
  double *rewards;        /* [T][n] */
  int32_t *dones;         /* [T][n] */
  int64_t *pos;           /* [1] next slot */
  int64_t *last;          /* [1] slot of the most recent add */
  int64_t *count;         /* [1] adds since the last reset */
  int32_t *ticket;        /* one word, 0 between calls */
  float *advantages;      /* [T][n]; may be NULL for add / add_reward */
  float *returns;         /* [T][n]; may be NULL for add / add_reward */
  int64_t n;              /* envs */
  int32_t T;              /* slots */
  int32_t F;              /* observation rows per slot */
  int32_t obs_type;       /* 0 int32, 1 int8, 2 float32 (as include/oc_hostio.h) */
} oc_rollout_buf;

OC_API int oc_rollout_abi_version(void);
OC_API const char *oc_rollout_last_error(void);

/* ONE launch: slot *pos takes the F observation rows ([F][n], as they lie), timestep [n], the two
 * action rows, log_prob, episode_start and (unless NULL) value; its reward row is zeroed; then
 * *last = *pos, *pos = (*pos + 1) % T, *count += 1.  A slot (F * n elements) of 2 GiB or more is
 * refused. */
OC_API int oc_rollout_add(const oc_rollout_buf *buf, const void *rows, const double *timestep,
                          const int32_t *move, const int32_t *comm, const float *log_prob,
                          const float *value /* may be NULL */, const float *episode_start, void *stream);

/* No device work: the launch oc_rollout_add would make on `buf`, plan = {gridDim.x, groups, per_group}. */
OC_API int oc_rollout_add_plan(const oc_rollout_buf *buf, int32_t plan[3]);

/* ONE launch: rewards[*last] += rewards, dones[*last] = dones. */
OC_API int oc_rollout_add_reward(const oc_rollout_buf *buf, const double *rewards, const int32_t *dones,
                                 void *stream);

/* ONE launch: advantages and returns of the L recorded steps (above); last_values, last_dones
 * float [n]. */
OC_API int oc_rollout_gae(const oc_rollout_buf *buf, const float *last_values, const float *last_dones,
                          double gamma, double gae_lambda, void *stream);

#ifdef __cplusplus
}
#endif
#endif
