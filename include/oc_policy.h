/* oc_policy.h -- C ABI of liboc_policy.so: a small MLP policy evaluated on the observation
 * rows oc_multi_step / oc_obs leave in HBM, its action sampled and written as the [n][2]
 * (move, comm) pairs oc_step_opts.ego_pairs / alt_pairs consume (include/oc_hip.h).
 *
 * What it stands in for: the per-step partner / ego forward of the reference's training loop --
 * pantheonrl's OnPolicyAgent.get_action (pantheonrl/common/agents.py:112-194: one
 * policy.forward on ONE observation per env step) behind MultiAgentEnv.step
 * (pantheonrl/common/multiagentenv.py:149-215) -- for the stable-baselines3 default MlpPolicy
 * shape: one hidden layer of 64 tanh units per head group.  SURVEY section 8 (f) 2: "the partner
 * policy batched".  It is NOT part of the environment's semantics: no oracle, a PyTorch fp32
 * reference of the same network in the tests (fp16 operands, fp32 accumulation: logits within
 * 2e-2 of it).  Everything else (any torch module) runs through vec_env.TorchPolicyPartner.
 *
 * The network (gym-comm_amd/vec_env.py: MLPPolicy), per env, F = oc_obs_rows() features x:
 *     h      = tanh(W1 x + wt * timestep + b1)              64 hidden units
 *     logits = W2 h + b2                                    4 move logits, C <= 16 comm logits
 *     move ~ softmax(logits[0:4]),  comm ~ softmax(logits[4:4+C])   (from the env's two PCG32
 *     streams), or the argmax of each (rng == NULL).
 *
 * Both GEMMs run on the matrix cores (v_mfma_f32_32x32x16_f16): one wave = 32 envs; the hidden
 * layer comes out with the env on the lane and the hidden units in the accumulator registers,
 * which IS the B-operand layout of the second product -- no LDS, no lane movement.  Weights are
 * passed pre-arranged in MFMA fragment order with the activation's constants folded in
 * (`oc_policy_pack_*` below do it; host only).  With a = 2 log2(e) h, tanh(h) = 1 - 2 r where
 * r = 1 / (2^a + 1), so the kernel evaluates r (exp2, add, rcp) and the second product yields the
 * logits in base 2, which is what the sampler's 2^x wants:
 *   w1   fp16 [2][ksteps][64 lanes][8]  A fragments of 2 log2(e) [W1 | wt | b1 | 0...]
 *        (64 x 16*ksteps), ksteps = ceil((F + 2) / 16): element j of lane l, M-tile m, k-step s =
 *        2 log2(e) W1aug[32 m + (l & 31)][16 s + 8 (l >> 5) + j]
 *   w2   fp16 [4][64 lanes][8]           A fragments of -2 log2(e) W2 padded to 32 rows, k permuted
 *        to the accumulator order: element j of lane l, k-step s = -2 log2(e) W2row[l & 31][16 s +
 *        8 (j >> 2) + 4 (l >> 5) + (j & 3)], where row o holds move logit o (o < 4) and comm
 *        logit c sits in row 4 + (c & 3) + 8 (c >> 2)
 *   b2   fp32 [64 lanes][16]             the second product's initial accumulator: log2(e) (b2 +
 *        sum_j W2[.][j]) of row (r & 3) + 8 (r >> 2) + 4 (l >> 5) in register r of lane l (the sum
 *        over the ROUNDED fp16 weights, so that the fold is exact)
 * Sampling: inverse CDF of the softmax, one uniform draw per head and step from the env's stream.
 * Every pointer but the pack functions' is a DEVICE pointer of a caller-owned tensor; nothing is
 * allocated, freed or synchronised; calls are ordered by `stream`. */
#ifndef OC_POLICY_H
#define OC_POLICY_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#ifndef OC_API
#define OC_API __attribute__((visibility("default")))
#endif

#define OC_POLICY_ABI_VERSION 1
#define OC_POLICY_HIDDEN 64
#define OC_POLICY_MAX_COMM 16

typedef struct {
  const void *obs;      /* this player's observation rows: [F][n], element type `obs_type` */
  const uint16_t *w1;   /* fp16 bits, fragment order (above) */
  const uint16_t *w2;
  const float *b2;
  uint32_t *rng;        /* uint32 [2][n] PCG32 states (move stream, comm stream), advanced in
                           place; NULL = greedy (argmax) */
  int32_t *pairs;       /* out: int32 [n][2] = (move 0..3, comm 0..C-1) */
  float *logits;        /* optional out (tests): float [4 + C][n]; NULL = not written */
} oc_policy_player;

OC_API int oc_policy_abi_version(void);
OC_API const char *oc_policy_last_error(void);

/* number of 16-feature k-steps of the first product for F observation rows (+ timestep + bias) */
OC_API int32_t oc_policy_ksteps(int32_t F);

/* Host-side packing (plain row-major fp32 in, fragment order out).
 *   w1 [64][F], wt [64], b1 [64]  ->  out fp16 [2][ksteps][64][8]
 *   w2 [4 + C][64]                ->  out fp16 [4][64][8]
 *   b2 [4 + C], w2 [4 + C][64]    ->  out fp32 [64][16] */
OC_API int oc_policy_pack_w1(const float *w1, const float *wt, const float *b1, int32_t F, uint16_t *out);
OC_API int oc_policy_pack_w2(const float *w2, int32_t C, uint16_t *out);
OC_API int oc_policy_pack_b2(const float *b2, const float *w2, int32_t C, float *out);

/* One launch: `num_players` (1 or 2) policies, each on its own observation rows, for n envs.
 *   timestep  double [n] (oc_multi_step's / oc_obs's timestep tensor)
 *   F         observation rows per viewer (oc_obs_rows());  C  comm channels (1..16)
 *   obs_type  element type of the rows: 0 int32, 1 int8, 2 float32 (oc_obs_cfg.obs_int8) */
OC_API int oc_policy_mlp(const oc_policy_player *players, int32_t num_players, const double *timestep,
                         int32_t F, int32_t C, int32_t obs_type, int64_t n, void *stream);

/* ---- the actor-critic form: the same network with a value head, for a player that learns ----
 *
 * What OnPolicyAgent.get_action needs of its one forward per step (pantheonrl/common/agents.py:
 * 112-194): the action, its log-probability under the policy and the state's value.
 *     value    = wv . tanh(W1 x + wt * timestep + b1) + bv       on the same 64 hidden units
 *     log_prob = ln softmax(logits[0:4])[move] + ln softmax(logits[4:4+C])[comm]
 * for the (move, comm) that is written -- sampled, greedy, or GIVEN (`given`: score these actions
 * instead of choosing, what a learner's update evaluates).
 *
 * The value head is row 8 of the second product, a row no logit uses: register 4 of the lower
 * half-wave's lanes.  It is folded exactly as a logit row is -- -2 log2(e) wv in fp16 at element j
 * of lanes 8 and 40 (h = l >> 5) of k-step s = hidden unit 16 s + 8 (j >> 2) + 4 h + (j & 3), and
 * the start value log2(e) bv - 1/2 sum_j (rounded weights) in register 4 of lanes 0..31 -- and the
 * kernel reads it back as out[4] * ln 2.  oc_policy_pack_w2v / _b2v produce oc_policy_pack_w2's /
 * _b2's output with that row filled in: every other element is the same.
 *
 * The log-probability, per head, in float32 and in this order, with the head's base-2 logits L_c
 * (c = 0 .. count-1 in candidate order), a the action:
 *     m = max_c L_c;   e_c = 2^(L_c - m);   S = sum_c e_c   (from 0, c ascending: the sampler's own total)
 *     lp = ((L_a - m) - log2 S) * ln 2          (v_exp_f32, v_log_f32; ln 2 the float 0.6931471805599453f)
 *     log_prob = lp_move + lp_comm
 * A `given` index outside its head's range makes log_prob -inf for that env and touches nothing
 * else (it is echoed into pairs / move_row / comm_row where those are asked for).
 * For the same packed logit rows, observations and stream states, pairs, logits and the advanced
 * streams are bit for bit oc_policy_mlp's. */
typedef struct {
  oc_policy_player p;     /* obs, w1, w2, b2, rng, pairs, logits as above; pairs may be NULL here;
                             w2 / b2 packed WITH the value row (oc_policy_pack_w2v / _b2v) */
  const int32_t *given;   /* optional int32 [n][2]: score THESE (move, comm) instead of choosing;
                             p.rng is then neither read nor advanced */
  int32_t *move_row;      /* optional out, int32 [n] */
  int32_t *comm_row;      /* optional out, int32 [n]; given together with move_row */
  float *log_prob;        /* optional out, float [n] */
  float *value;           /* optional out, float [n] */
} oc_policy_ac_player;

/* Host-side packing with the value row.  w2, b2 as for oc_policy_pack_w2 / _b2; wv [64], bv [1]. */
OC_API int oc_policy_pack_w2v(const float *w2, const float *wv, int32_t C, uint16_t *out);
OC_API int oc_policy_pack_b2v(const float *b2, const float *w2, const float *bv, const float *wv,
                              int32_t C, float *out);

/* One launch, as oc_policy_mlp (same arguments, grid and checks): lane l < 32 of a wave stores
 * log_prob, value and move_row of its env, lane l + 32 comm_row. */
OC_API int oc_policy_mlp_ac(const oc_policy_ac_player *players, int32_t num_players, const double *timestep,
                            int32_t F, int32_t C, int32_t obs_type, int64_t n, void *stream);

/* ---- the PPO update of the actor-critic form: loss, backward, clip, Adam, repack -------------
 *
 * What it restates: train() of the reference's PPO (pantheonrl/algos/modular/learn.py:222-334, which
 * is stable-baselines3's), with clip_range_vf = None and use_sde = False as its trainer configures
 * it.  OUT OF SCOPE: the marginal-regularisation term (learn.py:299-318, several partners' logits
 * composed), hidden sizes other than 64.  (clip_range_vf and target_kl early stopping: the train
 * sequence, the last section of this header.)
 *
 * A minibatch is idx, int32 [B], B >= 2: sample i is slot idx[i] / n, env idx[i] % n of tensors
 * shaped as an oc_rollout_buf's (include/oc_rollout.h): obs [T][F][n], timestep double [T][n],
 * actions int32 [T][2][n], log_probs / advantages / returns float [T][n] (the recorded values are
 * not read: there is no value clipping).  Any order, repeats allowed; an index outside 0 .. T n - 1
 * is a caller error and is NOT checked on the device.
 *
 * With lp_i, v_i and the heads' probabilities p from the same forward as oc_policy_mlp_ac in `given`
 * mode (the same operations in the same order: lp_out / v_out are its bits):
 *     A^_i = (A_i - mean(A)) / (std(A) + 1e-8)        mean and UNBIASED std over the B samples
 *     rho_i = exp(lp_i - old_lp_i)
 *     policy_loss  = -mean(min(A^ rho, A^ clamp(rho, 1 - c, 1 + c)))
 *     value_loss   =  mean((ret_i - v_i)^2)
 *     entropy_loss = -mean(H_move,i + H_comm,i)        H = -sum_c p_c ln p_c
 *     loss = policy_loss + ent_coef entropy_loss + vf_coef value_loss
 * The gradient is taken with respect to the fp32 master weights, flat [P] in this order:
 * w1 [64][F], wt [64], b1 [64], w2 [4 + C][64], b2 [4 + C], wv [64], bv [1].  It is evaluated at the
 * network the packed fragments represent -- features, 2 log2(e) W1aug and -2 log2(e) W2 in fp16, r
 * rounded to fp16 on its way into the second product -- and those roundings are not differentiated
 * (ordinary mixed precision).  Behind the forward everything is float32 (fp32-operand matrix
 * products), with h = 1 - 2 r and tanh' = 4 r (1 - r) from the UNROUNDED float32 r:
 *     d loss / d lp   = -A^ rho / B  where the unclipped term is the minimum or rho lies inside
 *                       [1 - c, 1 + c], 0 otherwise
 *     per head:  d lp / d logit_c = 1[c = a] - p_c,   d H / d logit_c = -p_c (ln p_c + H)
 *     d loss / d v    = 2 vf_coef (v - ret) / B
 *     columns F and F + 1 of the first layer's augmented gradient are wt and b1.
 * The 1 / B is applied to the summed gradient, in float32, not to the operands.
 * A recorded action outside its head's range makes lp = -inf: that sample contributes nothing to any
 * loss term or gradient and is counted in `bad`; B stays the divisor, and the advantage statistics
 * (which do not look at actions) still include it.
 * Clip (clip_grad_norm_): norm = sqrt(sum g^2) over all P, in double; g *= min(1, max_grad_norm /
 * (norm + 1e-6)).  Adam: torch's, amsgrad = False, no weight decay, in float32; m, v [P] and the int32
 * step counter live on the device, the bias corrections come from that counter.  Afterwards the
 * packed w1 / w2 / b2 are rewritten IN PLACE (captured graphs keep the addresses), bit for bit what
 * oc_policy_pack_w1 / _w2v / _b2v produce on the host from the same fp32 weights, and so is `w2t`,
 * the learner's own image: float [2][16][64], element (m, t, l) = the fp16 value of -2 log2(e) W2row
 * [(t & 3) + 8 (t >> 2) + 4 (l >> 5)][32 m + (l & 31)] (the value head is row 8) -- W2 transposed and
 * k-permuted to the order in which d logits sit in the accumulators.  oc_policy_pack_w2t (below)
 * produces it on the host, for a learner's first image.
 *
 * stats, float [10], written on the device and never read by the library except [6], [7] within
 * one call: policy_loss, value_loss, entropy_loss, approx_kl = mean(old_lp - lp), clip_fraction
 * (|rho - 1| > c), grad_norm (before clipping), adv_mean, adv_std, bad, loss.
 *
 * Three launches per minibatch, none allocates or synchronises, all capturable: the advantage
 * statistics (double, an order fixed by B alone); the loss-and-gradient kernel, whose workgroups
 * write partials [G][P + 8] to `scratch` (no floating-point atomics: the same call gives the same
 * bits); one workgroup that sums the partials over g ascending, clips, and (oc_policy_ppo_update) applies
 * Adam and repacks.  hyper = (lr, clip_range) is read on the device: a schedule needs no new capture. */
typedef struct {
  const void *obs;            /* the rollout tensors (above) */
  const double *timestep;
  const int32_t *actions;
  const float *log_probs, *advantages, *returns;
  int64_t n;
  int32_t T, F, C, obs_type;  /* obs_type: 0 int32, 1 int8, 2 float32 */
  uint16_t *w1, *w2;          /* the seat's packed weights (with the value row): read by the forward, */
  float *b2;                  /*   rewritten by oc_policy_ppo_update */
  float *w2t;                 /* float [2][16][64], the learner's (above) */
  float *p_w1, *p_wt, *p_b1, *p_w2, *p_b2, *p_wv, *p_bv;   /* fp32 master weights (oc_policy_ppo_update only) */
  float *m, *v;               /* Adam state, float [P] each (oc_policy_ppo_update only) */
  int32_t *step;              /* int32 [1], Adam's step counter (oc_policy_ppo_update only) */
  float *grad;                /* out: the clipped gradient, float [P] */
  float *scratch;             /* float [plan[3]] */
  float *stats;               /* float [10] */
  const float *hyper;         /* float [2] on the device: lr, clip_range */
  float ent_coef, vf_coef, max_grad_norm, beta1, beta2, eps;
  int32_t max_groups;         /* 0 = the library's choice; otherwise a cap on the workgroups */
  float *lp_out, *v_out;      /* optional out, float [B]: the forward's log_prob and value */
} oc_ppo_cfg;

/* Host-side packing of `w2t` (above): w2 [4 + C][64], wv [64]  ->  out fp32 [2][16][64]. */
OC_API int oc_policy_pack_w2t(const float *w2, const float *wv, int32_t C, float *out);

/* No device work: plan =(workgroups G of the gradient kernel, tiles of 32 samples per wave, P,
 * floats of scratch).  Wave w of the 4 G takes tiles w, w + 4 G, ...: no workgroup is empty. */
OC_API int oc_policy_ppo_plan(int32_t F, int32_t C, int32_t B, int32_t max_groups, int32_t *plan);

/* One minibatch update (3 launches), or the first of it (oc_policy_ppo_grad: the same launches without Adam
 * and the repack; leaves the clipped gradient and the statistics).  Checked before any device work:
 * F >= 1, F + 2 <= 48, 1 <= C <= 16, B >= 2, obs_type, T n < 2^31, non-NULL pointers. */
OC_API int oc_policy_ppo_update(const oc_ppo_cfg *cfg, const int32_t *idx, int32_t B, void *stream);
OC_API int oc_policy_ppo_grad(const oc_ppo_cfg *cfg, const int32_t *idx, int32_t B, void *stream);

/* ---- a whole train() as a fixed sequence of launches on device-side state ----------------------
 *
 * What it restates: the loops of the reference's train() around the minibatch (learn.py:222-334) --
 * the epoch's shuffle, the statistics it logs (means over all minibatches of a train()), its
 * early stop -- and stable-baselines3's clip_range_vf.  Every decision is taken on the device, so the
 * sequence
 *     oc_policy_ppo_train_begin,
 *     n_epochs x (oc_policy_ppo_epoch_begin, then oc_policy_ppo_train_step per minibatch)
 * is the same serial list of launches whatever happens in it, never allocates or synchronises, and can
 * be captured into ONE graph.  A sequence is HALTED when ctl[OC_PPO_CTL_STOP] or
 * ctl[OC_PPO_CTL_ERROR] is non-zero: every later launch of it returns having written nothing.
 *
 * The state, all on the device, the caller's:
 *   values     float [T][n]  the recorded values (oc_rollout_buf.values), read by value clipping
 *   hyper_ext  float [2]     clip_range_vf, target_kl; a value <= 0 (or NaN) means off.  Read on the
 *                            device, like oc_ppo_cfg.hyper: a change needs no new capture
 *   ctl        int32 [OC_PPO_CTL_WORDS], zero at first:
 *                [OC_PPO_CTL_STOP]     1 once the KL rule has ended this train
 *                [OC_PPO_CTL_EPOCH]    permutations drawn since the state was zeroed.  NEVER reset by the
 *                                      library: each train() sees new permutations
 *                [OC_PPO_CTL_UPDATES]  minibatch updates applied in this train
 *                [OC_PPO_CTL_EPOCHS]   epochs of this train CLOSED by a later oc_policy_ppo_epoch_begin; the
 *                                      epoch still open is complete iff acc[OC_PPO_ACC_EPOCH_COUNT] > 0
 *                [OC_PPO_CTL_ERROR]    1 if a permutation walk hit its cap (below); sticky, never
 *                                      cleared by the library; the rest reserved
 *   acc        double [OC_PPO_ACC_WORDS]:
 *                [OC_PPO_ACC_EPOCH_KL], [OC_PPO_ACC_EPOCH_COUNT]   the open epoch's sum of the minibatches'
 *                                      approx_kl, and their number
 *                [OC_PPO_ACC_SUMS + k], k = 0 .. 5   this train's sums of policy_loss, value_loss,
 *                                      entropy_loss, approx_kl, clip_fraction, loss
 *              What is added is the FLOAT statistic oc_policy_ppo_train_step has just written to
 *              cfg.stats, converted to double, by one thread, in launch order: no atomics, and the same
 *              sequence gives the same bits.
 *
 * The KL rule is the reference's (learn.py:328-332), not stable-baselines3's break in mid-epoch: at
 * the END of an epoch, if target_kl > 0 and the mean over that epoch's minibatches of approx_kl =
 * mean(old_lp - lp) exceeds 1.5 target_kl, no further epoch runs.  The comparison is
 * acc[EPOCH_KL] / acc[EPOCH_COUNT] > 1.5 * (double)target_kl, in double.
 *
 * Value clipping, where c = clip_range_vf > 0 (otherwise every output of oc_policy_ppo_train_step is bit
 * for bit oc_policy_ppo_update's): with old_v the recorded value of the sample, in float32,
 *     v_pred = old_v + clamp(v - old_v, -c, c)
 *     value_loss = mean((ret - v_pred)^2)
 *     d loss / d v = 2 vf_coef (v_pred - ret) / B  where -c <= v - old_v <= c (the ends included, as
 *                    in torch's clamp backward), 0 elsewhere
 * and a bad-action sample is excluded as it is from every other term.
 *
 * The permutation (gym-comm_amd/csrc/oc_policy_shuffle.h), of 0 .. N - 1, 1 <= N <= 2^30, a function of
 * (seed, epoch, N) alone, every element on its own; all words uint32, arithmetic modulo 2^32:
 *     fmix32(h):  h ^= h >> 16;  h *= 0x85EBCA6B;  h ^= h >> 13;  h *= 0xC2B2AE35;  h ^= h >> 16
 *     bits  = the smallest even number >= 2 with 2^bits >= N;  half = bits / 2;  mask = 2^half - 1
 *     key_r = fmix32(seed ^ (0x9E3779B9 * (4 epoch + r + 1))),  r = 0 .. 3
 *     pass(x):  L = x >> half,  R = x & mask;  for r = 0 .. 3:  (L, R) = (R, L ^ (fmix32(R ^ key_r) & mask));
 *               the result is (L << half) | R           -- a balanced Feistel network: a bijection of 0 .. 2^bits - 1
 *     perm[i]:  x = pass(i);  while x >= N:  x = pass(x)        -- cycle walking: a bijection of 0 .. N - 1
 * The walk is cut after 4096 passes: the element is then -1 and the error word is set.  No bijection
 * can do that to a walk that starts below N before 2^bits - N + 1 < 3 N + 1 passes, and this one lands below N
 * with a chance above 1/4 per pass: the cap is there so that a bug cannot hang a GPU. */
#define OC_PPO_CTL_STOP 0
#define OC_PPO_CTL_EPOCH 1
#define OC_PPO_CTL_UPDATES 2
#define OC_PPO_CTL_EPOCHS 3
#define OC_PPO_CTL_ERROR 4
#define OC_PPO_CTL_WORDS 8
#define OC_PPO_ACC_EPOCH_KL 0
#define OC_PPO_ACC_EPOCH_COUNT 1
#define OC_PPO_ACC_SUMS 2
#define OC_PPO_ACC_WORDS 8

typedef struct {
  const float *values;      /* float [T][n] */
  const float *hyper_ext;   /* float [2]: clip_range_vf, target_kl */
  int32_t *ctl;             /* int32 [OC_PPO_CTL_WORDS] */
  double *acc;              /* double [OC_PPO_ACC_WORDS] */
} oc_ppo_train;

/* Host only: out int32 [N] = the permutation above.  Returns non-zero (and says why) for a bad
 * argument, or if an element came out -1. */
OC_API int oc_policy_ppo_perm_host(uint32_t seed, int32_t epoch, int32_t N, int32_t *out);

/* One launch of one thread: clears stop, updates, epochs and every sum of acc.  Touches neither the
 * epoch counter nor the error word. */
OC_API int oc_policy_ppo_train_begin(const oc_ppo_train *train, void *stream);

/* Two launches; nothing at all is written by either if the sequence is halted when it runs.
 *   1. one thread closes the epoch before: if this train has an open epoch with minibatches, the KL
 *      rule (above) is applied to it -- it may set stop, which ends this call's effect here -- and epochs
 *      is bumped; then the epoch sums are zeroed and the epoch counter is bumped.
 *   2. the permutation of epoch number (epoch counter - 1), N = count / granule, expanded by the
 *      granule into idx, int32 [count]:  idx[i * granule + j] = perm[i] * granule + j.
 * (Two launches: no workgroup reads an epoch number that another one of its launch changes.)
 * Checked before any device work: non-NULL pointers, granule >= 1 dividing count, count >= 1,
 * count / granule <= 2^30. */
OC_API int oc_policy_ppo_epoch_begin(const oc_ppo_train *train, int32_t *idx, int32_t count, int32_t granule,
                                     uint32_t seed, void *stream);

/* One minibatch of the sequence: oc_policy_ppo_update's three launches and checks (and the train state's
 * pointers), with value clipping, and with the minibatch's statistics added to the sums and updates
 * bumped after cfg.stats is written.  Halted: none of the three writes anything -- not the
 * parameters, m, v, step, the fragments, w2t, grad, scratch, stats (stats[6], [7] included), the sums
 * or lp_out / v_out. */
OC_API int oc_policy_ppo_train_step(const oc_ppo_cfg *cfg, const oc_ppo_train *train, const int32_t *idx, int32_t B,
                                    void *stream);

/* ---- the recurrent seat: an LSTM actor-critic step in one launch ---------------------------------
 *
 * What it stands in for: the forward of the RECURRENT learner the reference seats on both sides of the
 * env (trainer.py:92-112: RecurrentPPO('MultiInputPolicy', ...), for the partner inside OnPolicyAgent) --
 * one LSTM cell of 64 units shared by actor and critic, its state kept per env and put back to zero
 * where an episode starts.  OUT OF SCOPE: hidden sizes other than 64, a separate critic LSTM.  (The update,
 * backpropagation through time: the section after the next.)
 *
 * The network (gym-comm_amd/partners.py: LSTMActorCritic), per env, H = 64, F observation rows x, gates
 * in torch.nn.LSTMCell's order i, f, g, o:
 *     s      = episode_start > 0                                  (float [n]; NULL = no env starts)
 *     h_in   = s ? 0 : h_prev;   c_in = s ? 0 : c_prev            a SELECT, not a product: a NaN or an
 *                                                                 infinity in a starting env's old state
 *                                                                 does not survive
 *     z      = Wx x + wt * timestep + b + Wh h_in                 256 = 4 x 64 rows, row 64 gate + unit
 *     i, f, o = sigmoid(z_i), sigmoid(z_f), sigmoid(z_o);   g = tanh(z_g)
 *     c      = f * c_in + i * g;   h = o * tanh(c)
 *     logits = W2 h + b2   (4 move, C <= 16 comm);   value = wv . h + bv
 * and the action, its log-probability and the value leave through oc_policy_mlp_ac's tail as it is: the
 * same sampler, streams, `given` mode and -inf rule, the value in row 8 of the head product.
 *
 * Roundings (everything not named here is float32; r(a) = 1 / (2^a + 1) by v_exp_f32, an add, v_rcp_f32):
 *   - features, timestep and the constant 1 go to fp16 as in oc_policy_mlp; h_in is the stored float32
 *     value (after the select) rounded to fp16
 *   - the gate weights are folded and rounded to fp16: -log2(e) [Wx | wt | b | Wh] for i, f, o, so that
 *     sigmoid(z) = r(a) of the product a; 2 log2(e) [...] for g, so that tanh(z) = 1 - 2 r(a).  One product
 *     per row, accumulated in float32 from 0: the x k-steps first, then the four over h
 *   - c = (f * c_in) + (i * g): two products and their sum, each rounded (no contraction); it is stored
 *     unrounded.  tanh(c) = 1 - 2 r((2 log2(e)) * c), with the float 2 log2(e) = 2.885390043258667f
 *   - h = o * tanh(c) is stored as float32, unrounded; the head product takes fp16(h) against log2(e) [W2; wv]
 *     in fp16, starts from log2(e) [b2; bv] in float32 (the float32 product, no row-sum fold) and delivers
 *     the logits and the value in base 2, which the tail converts (out * ln 2)
 * Against the plain float32 module the logits stay within 1.5e-3 and the value within 1.4e-3: the largest
 * difference MEASURED over a 60-step trajectory of 64 envs with the weights at 4 x the init scale, each step
 * taken from the kernel's own previous state (tests/test_recurrent_seat_gpu.py; a figure, not a bound).
 *
 * One wave = 32 envs (v_mfma_f32_32x32x16_f16).  The 256 gate rows are 8 M-tiles; tile (gate, m) holds
 * units 32 m .. 32 m + 31, so the four gates of a unit arrive in the same lane and the same accumulator
 * register and the cell update is lane-local; h leaves the accumulators already in the B-operand order of
 * the head product and of the next step's recurrent product.
 *   gates      fp16 [4][2][ks][64 lanes][8], ks = oc_policy_lstm_ksteps(F) = oc_policy_ksteps(F) + 4:
 *              element j of lane l, tile (gate, m), k-step s.  For s < oc_policy_ksteps(F) the folded
 *              [Wx | wt | b | 0...][64 gate + 32 m + (l & 31)][16 s + 8 (l >> 5) + j]; for the four k-steps
 *              over h, s' = s - oc_policy_ksteps(F): the folded Wh[64 gate + 32 m + (l & 31)][16 s' +
 *              8 (j >> 2) + 4 (l >> 5) + (j & 3)] (k permuted to the accumulator order, as w2's)
 *   head       fp16 [4][64 lanes][8]: oc_policy_pack_w2v's layout (the value head in row 8) holding
 *              log2(e) [W2; wv]
 *   head_bias  fp32 [64 lanes][16]: oc_policy_pack_b2v's layout holding log2(e) [b2; bv]
 * State: h, c float [64][n], unit-major with the envs contiguous, like the observation rows.  Lane l of
 * a wave reads exactly the units it writes, of its own env -- those whose accumulator row has its
 * 4 (l >> 5) half: unit 32 m + (q & 3) + 8 (q >> 2) + 4 (l >> 5) for register q of tile m -- and reads all of
 * them before it writes any, so h_out / c_out MAY ALIAS h_in / c_in (a seat updates its state in place).
 * No other overlap between the tensors of a call is allowed. */
typedef struct {
  const void *obs;            /* the player's observation rows: [F][n], element type `obs_type` */
  const uint16_t *gates;      /* the three images (above) */
  const uint16_t *head;
  const float *head_bias;
  const float *h_in, *c_in;   /* float [64][n] */
  float *h_out, *c_out;       /* float [64][n]; NULL = not written; may alias h_in / c_in */
  const float *episode_start; /* optional float [n]: > 0 = this env starts from the zero state */
  uint32_t *rng;              /* the rest with oc_policy_ac_player's meanings: uint32 [2][n] or NULL (greedy) */
  const int32_t *given;       /* optional int32 [n][2]: score THESE actions; rng is then left alone */
  int32_t *pairs;             /* optional out, int32 [n][2] */
  int32_t *move_row;          /* optional out, int32 [n] */
  int32_t *comm_row;          /* optional out, int32 [n]; given together with move_row */
  float *log_prob;            /* optional out, float [n] */
  float *value;               /* optional out, float [n] */
  float *logits;              /* optional out (tests), float [4 + C][n], natural log */
} oc_policy_lstm_player;

/* k-steps of the gate product for F observation rows: oc_policy_ksteps(F) over x, then 4 over h */
OC_API int32_t oc_policy_lstm_ksteps(int32_t F);

/* Host-side packing (plain row-major fp32 in, fragment order out).
 *   wx [256][F], wt [256], b [256], wh [256][64]  ->  out fp16 [4][2][ks][64][8]
 *   w2 [4 + C][64], wv [64]                       ->  out fp16 [4][64][8]
 *   b2 [4 + C], bv [1]                            ->  out fp32 [64][16] */
OC_API int oc_policy_lstm_pack_gates(const float *wx, const float *wt, const float *b, const float *wh, int32_t F,
                                     uint16_t *out);
OC_API int oc_policy_lstm_pack_head(const float *w2, const float *wv, int32_t C, uint16_t *out);
OC_API int oc_policy_lstm_pack_head_bias(const float *b2, const float *bv, int32_t C, float *out);

/* One launch for n envs; timestep, F, C, obs_type as for oc_policy_mlp.  Checked before any device work:
 * F >= 1, F + 2 <= 64, 1 <= C <= 16, obs_type, n >= 0, 64 n < 2^31, non-NULL timestep, obs, images and
 * h_in / c_in, move_row and comm_row together.  Never allocates or synchronises; capturable. */
OC_API int oc_policy_lstm_ac(const oc_policy_lstm_player *pl, const double *timestep, int32_t F, int32_t C,
                             int32_t obs_type, int64_t n, void *stream);

/* ---- windows of a rollout: states recorded mid-rollout, and minibatches of windows -----------------------
 *
 * What it stands in for: the way the reference's RecurrentPPO (sb3_contrib, seated by trainer.py:92-112 with
 * n_steps = 5000 and batch_size = 1000) trains on stretches SHORTER than the rollout: its buffer keeps the LSTM
 * state along the rollout, and a minibatch is a set of short stretches of the envs' sequences, each unrolled from
 * the state recorded where it begins.  Here a rollout of T steps is cut into T / W windows of W steps, the seat's
 * state is recorded where each window begins (oc_policy_window_snapshot, one launch per step in front of the
 * cell's), and a minibatch of windows is PACKED into a "window batch" -- tensors laid out as a sink of W slots and
 * E envs with a start state of their own (oc_policy_window_gather, one launch) -- which the update of the
 * sections below unrolls exactly as it unrolls a whole sink.  Those sections' kernels are unchanged: to them a
 * window batch IS a full sink with T = W and n = E, and envs = 0 .. E - 1.
 *
 * What windows mean for the gradient: a window's start state (h0, c0 of the batch) is a CONSTANT, as the
 * rollout's start state is in the sections below; nothing flows across a window's first step, so a weight's
 * gradient sees at most W steps of history (truncated backpropagation through time), while the forward's values
 * are those of the whole sequence -- the recorded state is the one the rollout really had there.  An episode
 * start inside a window cuts state and gradient as it does anywhere.
 *
 * OUT OF SCOPE: windows that do not divide the rollout (T % W != 0 is refused, not padded: a shorter last window
 * would need per-sample masks, which the update does not have); a state recorded at every step; sb3_contrib's
 * exact minibatches (contiguous chunks of the env-major flattened buffer, padded to the longest stretch).
 *
 * Sequence ids.  With n envs and T / W windows, sequence s = k n + env, 0 <= s < n T / W, is window k (slots
 * k W .. k W + W - 1) of env `env`.  32 neighbouring envs of one window are 32 neighbouring ids: a shuffle in
 * granules that divide n keeps a wave's reads of a row contiguous.
 *
 *   states   float [T / W][2][64][n]: states[k][0] = h and states[k][1] = c BEFORE the step recorded in slot k W
 *            (so states[0] is the rollout's start state) */
typedef struct {
  const void *obs;            /* the sink's tensors (an oc_rollout_buf's): obs [T][F][n] of `obs_type` */
  const double *timestep;     /* double [T][n] */
  const int32_t *actions;     /* int32 [T][2][n] */
  const float *log_probs, *advantages, *returns, *episode_starts, *values;   /* float [T][n] each */
  const float *states;        /* float [T / W][2][64][n] (above) */
  int64_t n;
  int32_t T, W, F, obs_type;  /* obs_type: 0 int32, 1 int8, 2 float32 */
} oc_window_src;

typedef struct {              /* the same tensors laid out as a sink of W slots and E envs */
  void *obs;                  /* [W][F][E] of the source's element type */
  double *timestep;           /* double [W][E] */
  int32_t *actions;           /* int32 [W][2][E] */
  float *log_probs, *advantages, *returns, *episode_starts, *values;         /* float [W][E] each */
  float *h0, *c0;             /* float [64][E]: the start state of each sequence */
} oc_window_batch;

/* One launch, capturable, never allocates or synchronises.  Every workgroup reads the sink's position word
 * *pos (the slot the NEXT oc_rollout_add writes; a value outside 0 .. T - 1 is taken modulo T, as oc_rollout_add
 * takes it) and, if slot % W == 0, the launch copies h and c, float [64][n] each, into states[slot / W], bit for
 * bit; otherwise it writes nothing and costs an empty launch (a few workgroups per CU at most are started).  16-byte
 * accesses where h, c and states are 16-byte aligned, scalar ones otherwise.  Launched in front of the cell's launch
 * on the same stream it records the state before the step.  Checked before any device work: non-NULL pointers,
 * W >= 1, T % W == 0, n >= 1, 64 n < 2^31. */
OC_API int oc_policy_window_snapshot(const int64_t *pos, int32_t T, int32_t W, const float *h, const float *c,
                                     float *states, int64_t n, void *stream);

/* One launch, capturable, never allocates or synchronises.  seqs, int32 [E]: sequence ids (above), any order,
 * repeats allowed; an id outside 0 .. n T / W - 1 is a caller error and is NOT checked on the device.  For
 * sequence e = (k, env) of seqs and t = 0 .. W - 1, element (t, ., e) of every tensor of dst is element
 * (k W + t, ., env) of the same tensor of src, copied bit for bit; h0[u][e] = states[k][0][u][env] and c0[u][e] =
 * states[k][1][u][env].  e is the fastest-varying index on both sides.  No tensor of dst may overlap one of src.
 * Checked before any device work: non-NULL pointers (all of both structs), W >= 1, T % W == 0, E >= 1, n >= 1,
 * F >= 1, F + 2 <= 64, obs_type, T n < 2^31, 64 n < 2^31, W F E < 2^31.
 *
 * In a train sequence (the header's last section) the gather runs in front of every minibatch's step and is NOT
 * held back when the sequence is halted: it writes only the window batch, the learner's own staging, and
 * nothing the learner's state is made of -- no parameter, Adam word, image, statistic or sum. */
OC_API int oc_policy_window_gather(const oc_window_src *src, const oc_window_batch *dst, const int32_t *seqs,
                                   int32_t E, void *stream);

/* ---- the recurrent seat's PPO update: forward over whole sequences, BPTT, clip, Adam, repack ----------
 *
 * What it restates: one minibatch of train() of the reference's RecurrentPPO (trainer.py:92-112 seats it) for
 * the network of the section above: advantage normalisation, the forward over whole recorded sequences, the
 * clipped loss, the gradient through time, the norm clip, Adam, and the repack of the seat's three images in
 * place.  OUT OF SCOPE:
 *   - truncated windows inside the update: it unrolls the tensors it is given, whole (windows shorter than the
 *     rollout reach it packed as a sink of their own: the section above)
 *   - the marginal-regularisation term
 *   - hidden sizes other than 64
 *   - a separate critic LSTM
 *   - the cell inside the step kernel
 *
 * Sequences.  A sequence is one env over the whole sink: steps t = 0 .. T - 1 in slots 0 .. T - 1 of tensors
 * shaped as an oc_rollout_buf's (obs [T][F][n], timestep double [T][n], actions int32 [T][2][n], log_probs /
 * advantages / returns / episode_starts float [T][n]).  It is the CALLER's duty that the buffer is full with
 * count == T and pos == 0, so that slot order is chronological.  A minibatch is envs, int32 [E], E >= 1 and
 * E T >= 2; any order, repeats allowed; sample (t, e) is slot t of env envs[e].  An index outside 0 .. n - 1 is
 * a caller error and is NOT checked on the device.  B = E T is the divisor everywhere oc_policy_ppo_update uses B.
 *
 * Forward.  The start state is (h0, c0), float [64][n]: the seat's state before the first step of the rollout,
 * a constant in the gradient.  Step t applies exactly the network of the section above to the running state
 * with episode_starts[t] as its select -- oc_policy_lstm_ac's arithmetic in `given` mode, operation for
 * operation; the state is float32 and is fed back as fp16(h) -- so lp_out / v_out (optional, float [T][E]) are
 * bit for bit what T successive scoring launches return, each carrying the state the previous one produced.
 *
 * Loss.  oc_policy_ppo_update's over the B samples: A^ from the mean and the UNBIASED std of the B gathered
 * advantages (+ 1e-8), rho = exp(lp - old_lp), the clipped policy term, the value loss without value clipping,
 * the entropy term.  A recorded action outside its head's range makes lp = -inf: that sample contributes
 * nothing to any loss term and is counted in `bad`; B stays the divisor.  The same ten stats are written.
 *
 * Gradient.  With respect to the fp32 master weights, flat [P] in this order: wx [256][F], wt [256], b [256],
 * wh [256][64], w2 [4 + C][64], b2 [4 + C], wv [64], bv [1]; P = 256 (F + 2) + 16384 + 65 (4 + C) + 65.  It is
 * evaluated at the network the images represent, as oc_policy_ppo_update's is: the folded fp16 gate and head
 * weights divided back by their fold constants, fp16 features and fp16(h) in the products, the roundings not
 * differentiated.  Behind the forward everything is float32 with fp32-operand matrix products.  The
 * activations' derivatives come from the unrounded r values: i, f, o = r(a) gives sigma' = r (1 - r); g = 1 - 2 r
 * gives tanh' = 4 r (1 - r); tanh(c) uses its own r.  Per step, going backwards, with D_t = d (B loss) / d
 * [logits; value] as in the MLP section and dh_next, dc_next zero behind the last step:
 *     dh   = [W2; wv]^T D_t + dh_next
 *     do   = dh tanh(c_t)
 *     dc   = dc_next + dh o (1 - tanh^2(c_t))
 *     dz_i = dc g i (1 - i);  dz_f = dc c_in f (1 - f);  dz_g = dc i (1 - g^2);  dz_o = do o (1 - o)
 *     gWx += dz x^T;  gwt += dz ts;  gb += sum dz;  gWh += dz h_in^T;  gW2 += D h_t^T;  gb2, gwv, gbv likewise
 *     dh_next = s_t ? 0 : Wh^T dz;    dc_next = s_t ? 0 : dc f
 * c_in and h_in are the values after the select; s_t is a select by episode_starts[t] > 0: the start cuts the
 * gradient (and a NaN or an infinity in a starting env's h0 / c0 reaches nothing).  The 1 / B is applied to
 * the summed gradient in float32.
 *
 * Against the float64 restatement with the same roundings (tests/recurrent_ppo_ref.py) the clipped gradient
 * lies within TOL_G of each tensor's largest element and the statistics within TOL_S; both constants are 4 x
 * the largest difference seen on an MI355X over the test's three cases -- measured, not a bound; the figures
 * are in tests/recurrent_ppo_ref.py.
 *
 * Clip, Adam, repack.  clip_grad_norm_ with the norm in double, in a fixed order; Adam as in
 * oc_policy_ppo_update (m, v [P] and the int32 step on the device, hyper = (lr, clip_range) read on the device).
 * Afterwards gates, head and head_bias are rewritten IN PLACE, bit for bit what oc_policy_lstm_pack_gates /
 * _head / _head_bias produce from the same fp32 weights, and so is `bwd`, the learner's own image, float
 * [oc_policy_rppo_pack_bwd_elems()]: first Wh^T, float [2][8][16][64], element (m, u, q, l) = the fp16 value of
 * the folded Wh[64 (u >> 1) + 32 (u & 1) + (q & 3) + 8 (q >> 2) + 4 (l >> 5)][32 m + (l & 31)] times the inverse
 * of its fold (-ln 2; ln 2 / 2 for gate g), one float32 product -- Wh transposed and k-permuted to the order
 * in which d z sits in the gate product's accumulators; then [W2; wv]^T in w2t's layout (float [2][16][64],
 * oc_policy_ppo_update's section) holding the fp16 value of log2(e) W times ln 2.
 *
 * Determinism: no floating-point atomics; workgroups write partials and one kernel sums them in a fixed
 * order: the same call gives the same bits.  Six launches, whatever (T, E, F, C, max_groups) are; none
 * allocates or synchronises; all are capturable:
 *   1. the advantage statistics (double, an order fixed by B)
 *   2. the forward: one wave per 32 sequences, t ascending, the state in registers; leaves per sample the
 *      gates, h, c and D in `scratch` (416 floats per sample) and per workgroup the loss sums
 *   3. the backward: the same mapping, t descending; overwrites the gates with d z
 *   4. the weight gradients: products over samples, parallel over (t, tile of 32 sequences); partials [Gw][P]
 *   5. the partials summed over g ascending, times 1 / B; the squared norm's partial sums in double
 *   6. one workgroup: the norm, the clip, the statistics and (oc_policy_rppo_update) Adam and the repack */
typedef struct {
  const void *obs;            /* the rollout tensors (above) */
  const double *timestep;
  const int32_t *actions;
  const float *log_probs, *advantages, *returns, *episode_starts;
  const float *h0, *c0;       /* float [64][n]: the state before the rollout's first step */
  int64_t n;
  int32_t T, F, C, obs_type;  /* obs_type: 0 int32, 1 int8, 2 float32 */
  uint16_t *gates, *head;     /* the seat's three images: read by the forward, rewritten by oc_policy_rppo_update */
  float *head_bias;
  float *bwd;                 /* float [oc_policy_rppo_pack_bwd_elems()], the learner's (above) */
  float *p_wx, *p_wt, *p_b, *p_wh, *p_w2, *p_b2, *p_wv, *p_bv;   /* fp32 master weights (oc_policy_rppo_update only) */
  float *m, *v;               /* Adam state, float [P] each (oc_policy_rppo_update only) */
  int32_t *step;              /* int32 [1], Adam's step counter (oc_policy_rppo_update only) */
  float *grad;                /* out: the clipped gradient, float [P] */
  float *scratch;             /* float [plan[4]], 8-byte aligned */
  float *stats;               /* float [10] */
  const float *hyper;         /* float [2] on the device: lr, clip_range */
  float ent_coef, vf_coef, max_grad_norm, beta1, beta2, eps;
  int32_t max_groups;         /* 0 = the library's choice (256); otherwise a cap on the weight-gradient workgroups */
  float *lp_out, *v_out;      /* optional out, float [T][E]: the forward's log_prob and value */
} oc_rppo_cfg;

/* No device work: plan, int64 [8] (the scratch can pass 2^31 floats) = (workgroups of the forward and the
 * backward = ceil(E / 32); workgroups Gw of the weight-gradient kernel = min(T ceil(E / 32), cap); (t, tile)
 * pairs per such workgroup; P; floats of scratch; workgroups of the reduction; launches per call; floats of
 * scratch per sample). */
OC_API int oc_policy_rppo_plan(int32_t F, int32_t C, int32_t T, int32_t E, int32_t max_groups, int64_t *plan);

/* Host-side packing of `bwd` (above): wh [256][64], w2 [4 + C][64], wv [64]  ->  out fp32 [_elems()]. */
OC_API int32_t oc_policy_rppo_pack_bwd_elems(void);
OC_API int oc_policy_rppo_pack_bwd(const float *wh, const float *w2, const float *wv, int32_t C, float *out);

/* One minibatch update (6 launches), or the same launches without Adam and the repack (oc_policy_rppo_grad:
 * leaves the clipped gradient and the statistics).  Checked before any device work: F >= 1, F + 2 <= 64,
 * 1 <= C <= 16, T >= 1, E >= 1, 2 <= E T < 2^31, obs_type, T n < 2^31, 64 n < 2^31, non-NULL pointers. */
OC_API int oc_policy_rppo_update(const oc_rppo_cfg *cfg, const int32_t *envs, int32_t E, void *stream);
OC_API int oc_policy_rppo_grad(const oc_rppo_cfg *cfg, const int32_t *envs, int32_t E, void *stream);

/* ---- the recurrent learner's train(): the train sequence over whole sequences -------------------------
 *
 * What it restates: the loops of train() around the minibatch of the section above -- the epoch's shuffle of the
 * ENVS, the logged means, the early stop -- and clip_range_vf, exactly as the MLP seat's train sequence does
 * (the section "a whole train() as a fixed sequence of launches on device-side state": the same oc_ppo_train
 * state, the same halting rule, the same permutation).  The sequence is
 *     oc_policy_ppo_train_begin,
 *     n_epochs x ( oc_policy_ppo_epoch_begin(train, idx, count = n, granule, seed),
 *                  oc_policy_recurrent_train_step per cut of idx )
 * whose first two calls are unchanged: with count = n and a granule dividing n they write a permutation of the
 * sink's envs into idx, int32 [n], and a cut of E consecutive elements of idx (E >= 1, E T >= 2) is a minibatch
 * of E whole sequences.  The same serial list of launches whatever happens in it; it never allocates or
 * synchronises and can be captured into ONE graph.
 *
 * The KL rule is the sequence's own, the reference's modular learner (learn.py:328-332): at the END of an epoch,
 * applied by the next oc_policy_ppo_epoch_begin to the mean over that epoch's minibatches of approx_kl =
 * mean(old_lp - lp); where it exceeds 1.5 target_kl no further epoch runs.  It is NOT sb3_contrib RecurrentPPO's
 * rule, which breaks in mid-epoch, before the minibatch that crosses the line is applied, on the estimator
 * mean((rho - 1) - log rho) (ppo_recurrent.py:407-412).  OUT OF SCOPE: sb3_contrib's mid-epoch break and its
 * estimator; truncated windows inside the step (a minibatch of windows reaches it packed, by
 * oc_policy_window_gather in front of it); the marginal-regularisation term.
 *
 * Value clipping, where c = hyper_ext[0] = clip_range_vf > 0: with old_v = values[t * n + env] the recorded value
 * of sample (t, env), in float32,
 *     v_pred = old_v + clamp(v - old_v, -c, c)
 *     value_loss = mean((ret - v_pred)^2)
 *     the value head's row of D_t = 2 vf_coef (v_pred - ret)  where -c <= v - old_v <= c (the ends included),
 *                                   0 elsewhere
 * and everything behind D_t is the section above's: the gradient through time is linear in D.  A bad-action
 * sample stays excluded.  Where c <= 0 or c is NaN every output is bit for bit oc_policy_rppo_update's.
 *
 * oc_policy_recurrent_train_step: oc_policy_rppo_update's six launches (the TRAIN variants of its kernels, a
 * code object of their own) and all of its argument checks, and the train state's non-NULL pointers; everything
 * is checked before any device work.  After cfg.stats is written, the one thread that wrote it adds the six
 * float statistics, converted to double, to acc[OC_PPO_ACC_SUMS + k], adds approx_kl to acc[OC_PPO_ACC_EPOCH_KL]
 * and 1 to acc[OC_PPO_ACC_EPOCH_COUNT], and bumps ctl[OC_PPO_CTL_UPDATES]: no atomics, and the same sequence
 * gives the same bits.  HALTED (ctl[OC_PPO_CTL_STOP] or ctl[OC_PPO_CTL_ERROR] non-zero): each of the six
 * launches returns at once, having written nothing -- not the parameters, m, v, step, the three images, bwd,
 * grad, scratch, stats (stats[6], [7] included), the sums or lp_out / v_out.  Never allocates or synchronises;
 * capturable. */
OC_API int oc_policy_recurrent_train_step(const oc_rppo_cfg *cfg, const oc_ppo_train *train, const int32_t *envs,
                                          int32_t E, void *stream);

#ifdef __cplusplus
}
#endif
#endif
