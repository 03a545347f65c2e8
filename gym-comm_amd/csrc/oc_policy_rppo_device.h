// oc_policy_rppo_device.h -- the kernels of the recurrent PPO update (include/oc_policy.h, the recurrent update's section:
// oc_policy_rppo_update, oc_policy_rppo_grad) for the fused recurrent seat, and -- the same templates with
// TRAIN = true -- of a step of the recurrent learner's train sequence (oc_policy_recurrent_train_step).  Included
// through oc_policy_rppo_host.h by oc_policy_rppo.hip, which instantiates the TRAIN = false kernels only, and by
// oc_policy_rtrain.hip, which instantiates the TRAIN = true ones only.  gfx950 only.
//
// Six launches per minibatch of E sequences of T steps (B = E T samples), all sized at launch:
//
//   k_rppo_adv       one workgroup: mean and unbiased std of the B gathered advantages, in double
//                    (k_ppo_adv's sums over the samples (t, envs[e])).
//   k_rppo_forward   one wave = 32 sequences, one wave per workgroup; t ascending with the state in
//                    registers.  The body is k_policy_lstm's (oc_policy_lstm.hip) and k_ppo_grad's loss, operation
//                    for operation: lp and v are score()'s bits.  Per step it leaves in scratch the four gates'
//                    r values (where the backward will put d z), h_t, c_t and D_t = d (B loss) / d [logits; value];
//                    at the end the workgroup's loss sums.
//   k_rppo_backward  the same mapping, t descending, d h and d c carried in registers.  d h = [W2; wv]^T D_t
//                    and d h_next = Wh^T d z are fp32 products whose B operand is the accumulator layout the
//                    forward left D and the gates in (v_mfma_f32_32x32x2_f32: register q of half-wave h is
//                    k-step q's row): the learner keeps transposed, k-permuted fp32 images of both matrices and
//                    no lane moves.  The cell's backward is lane-local (the four gates of a unit share a lane
//                    and a register).  d z overwrites the gates' r values in place: a lane reads exactly the
//                    elements it writes.
//   k_rppo_wgrad     the products whose K runs over samples: gW = sum d z [x; ts; 1; h_in]^T and the head's
//                    D h_t^T, parallel over (t, tile of 32 sequences).  Four waves per workgroup, wave w owns
//                    gate w's 64 rows (2 x 4 accumulator tiles; waves 0 and 1 one tile of the head's each), so
//                    no wave adds to another's; operands pass through LDS ([row][sample], stride 33).
//                    The workgroup writes ITS partial gradient: no atomics.
//   k_rppo_reduce    partials summed over g ascending, one thread per parameter, times 1 / B; the squared
//                    norm's per-workgroup sums in double.
//   k_rppo_finish    one workgroup: the norm (double, fixed order), the clip, the statistics, and (APPLY) Adam
//                    on the fp32 master weights and the repack of the three seat images and the backward
//                    image through the host packers' own maps (oc_policy_layout.h).  A thread owns the
//                    parameters tid, tid + 1024, ...
//
// No loop's trip count depends on data; no workgroup waits on another.
//
// TRAIN = true: every kernel returns at once, having written nothing, when the train sequence is halted
// (ppo_halted: ctl.stop or ctl.error) -- a wave-uniform test at the very top, before any LDS use or barrier;
// k_rppo_forward clips the value prediction around the recorded value where hyper_ext[0] > 0; k_rppo_finish adds
// the minibatch's statistics to the epoch's and the train's sums.  TRAIN = false takes the arguments, and compiles
// to the code, it had before the variants existed: RppoArgs<false> and RppoOut<false> add no member.
#ifndef OC_POLICY_RPPO_DEVICE_H
#define OC_POLICY_RPPO_DEVICE_H
#include "../../include/oc_policy.h"
#include "oc_policy_ac_device.h"
#include "oc_policy_fail.h"
#include "oc_policy_layout.h"
#include "oc_policy_ppo_device.h"

namespace ocpol {

constexpr int RPPO_STRIDE = 33;                       // floats between two rows of the LDS tile
constexpr int RPPO_ROW_X = 256, RPPO_ROW_HIN = 320, RPPO_ROW_D = 384, RPPO_ROW_H = 416, RPPO_ROWS = 480;
constexpr int RPPO_SUMS = 8;                          // loss sums a forward workgroup writes
constexpr int RPPO_REDUCE_THREADS = 256;
constexpr int RPPO_SAMPLE_FLOATS = 256 + 64 + 64 + 32;   // scratch per sample: gates / d z, h, c, D
constexpr int RPPO_DEFAULT_GROUPS = 256;              // the weight-gradient kernel's cap where max_groups == 0
constexpr float RPPO_K_TANH = 2.0f * K_LOG2E;         // k_policy_lstm's K_TANH

// the kernels' arguments: the update's alone, or with the train sequence's device state behind them
template <bool TRAIN>
struct RppoArgs : oc_rppo_cfg {};
template <>
struct RppoArgs<true> : oc_rppo_cfg {
  oc_ppo_train tr;
};
// the output of a kernel that takes no cfg (k_rppo_adv: stats; k_rppo_reduce: grad), with the control words behind it
template <bool TRAIN>
struct RppoOut {
  float *to;
};
template <>
struct RppoOut<true> {
  float *to;
  const int32_t *ctl;
};

// where the regions of `scratch` begin (the plan's arithmetic, made once on the host)
struct RppoScratch {
  double *sq;      // [Gr]
  float *z;        // [T][256][E]
  float *hs, *cs;  // [T][64][E]
  float *ds;       // [T][32][E]
  float *wpart;    // [Gw][P]
  float *fpart;    // [Gf][RPPO_SUMS]
};

__device__ __forceinline__ float *rppo_param(const oc_rppo_cfg &p, const RppoLayout &lay, int pi) {
  if (pi < lay.wt) return p.p_wx + pi;
  if (pi < lay.b) return p.p_wt + (pi - lay.wt);
  if (pi < lay.wh) return p.p_b + (pi - lay.b);
  if (pi < lay.w2) return p.p_wh + (pi - lay.wh);
  if (pi < lay.b2) return p.p_w2 + (pi - lay.w2);
  if (pi < lay.wv) return p.p_b2 + (pi - lay.b2);
  if (pi < lay.bv) return p.p_wv + (pi - lay.wv);
  return p.p_bv;
}

__device__ __forceinline__ float rppo_f16(float v) { return (float)(_Float16)v; }

// fold() (oc_policy_layout.h) as the HOST packers' code evaluates it: the product rounded to float32, then to
// fp16.  Left to itself the device compiler fuses product and conversion (v_fma_mixlo_f16: one rounding), and
// one element in about 2^13 comes out one fp16 ulp from the host's; the empty asm keeps the product a float.
__device__ __forceinline__ _Float16 rppo_fold(float w, float scale) {
  float prod = scale * w;
  asm volatile("" : "+v"(prod));
  return (_Float16)prod;
}

// ---- a. advantage statistics: sample i is step i / E of env envs[i % E] --------------------------------
template <bool TRAIN = false>
__global__ void __launch_bounds__(PPO_FINISH_THREADS) k_rppo_adv(const float *adv, const int32_t *envs, const int E,
                                                                const int B, const uint32_t n32,
                                                                const RppoOut<TRAIN> out) {
  if constexpr (TRAIN) {
    if (ppo_halted(out.ctl)) return;   // uniform
  }
  float *stats = out.to;
  __shared__ double red[PPO_FINISH_THREADS];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int i = tid; i < B; i += PPO_FINISH_THREADS) s += (double)adv[(uint32_t)(i / E) * n32 + (uint32_t)envs[i % E]];
  const double mean = ppo_block_sum(red, s) / (double)B;
  double q = 0.0;
  for (int i = tid; i < B; i += PPO_FINISH_THREADS) {
    const double d = (double)adv[(uint32_t)(i / E) * n32 + (uint32_t)envs[i % E]] - mean;
    q += d * d;
  }
  const double var = ppo_block_sum(red, q) / (double)(B - 1);
  if (tid == 0) stats[6] = (float)mean, stats[7] = (float)sqrt(var);
}

// ---- b. the forward over whole sequences, the loss and D ------------------------------------------------
template <int OT, bool TRAIN = false>
__global__ void __launch_bounds__(64) k_rppo_forward(const RppoArgs<TRAIN> p, const int32_t *envs, const int E,
                                                     const RppoScratch sc) {
  if constexpr (TRAIN) {
    if (ppo_halted(p.tr.ctl)) return;   // uniform
  }
  __shared__ float sums[64 * RPPO_SUMS];
  const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
  const int e0 = (int)blockIdx.x * 32 + r;
  const bool valid = e0 < E;
  // lanes past the minibatch compute on its last sequence and store nothing
  const uint32_t env = (uint32_t)envs[valid ? e0 : E - 1], n32 = (uint32_t)p.n;
  const size_t n = (size_t)p.n, Es = (size_t)E, at0 = (size_t)e0;
  const int F = p.F, C = p.C, T = p.T, kx = ksteps(F), ks = kx + LSTM_HSTEPS;
  const half8 *wg = (const half8 *)p.gates + lane;
  const float mean = p.stats[6], denom = p.stats[7] + 1e-8f, clip = p.hyper[1];
  const float lo = 1.0f - clip, hi = 1.0f + clip;
  float cvf = 0.0f;                      // clip_range_vf; <= 0 (or NaN): no value clipping
  if constexpr (TRAIN) cvf = p.tr.hyper_ext[0];
  const bool vclip = cvf > 0.0f;         // uniform

  float hst[2][16], cst[2][16];   // the running state: unit 32 m + acc_row(q, h) in [m][q]
#pragma unroll
  for (int m = 0; m < 2; m++)
#pragma unroll
    for (int q = 0; q < 16; q++) {
      const uint32_t at = (uint32_t)(32 * m + acc_row(q, h)) * n32 + env;
      hst[m][q] = p.h0[at], cst[m][q] = p.c0[at];
    }
  float s_pol = 0.0f, s_val = 0.0f, s_ent = 0.0f, s_kl = 0.0f, s_clip = 0.0f, s_bad = 0.0f;

  for (int t = 0; t < T; t++) {
    const uint32_t smp = (uint32_t)t * n32 + env;
    const size_t base = (size_t)t * (size_t)F * n + env;
    const float ts = (float)p.timestep[smp];
    const bool start = p.episode_starts[smp] > 0.0f;
    // value clipping (TRAIN): the recorded value is asked for here, ahead of the products, and only where it is
    // used -- at the point of use its latency would stand exposed in every one of the T steps
    float oldv = 0.0f;
    if constexpr (TRAIN) {
      if (vclip) oldv = p.tr.values[smp];   // uniform
    }
    float cin[2][16];
#pragma unroll
    for (int m = 0; m < 2; m++)
#pragma unroll
      for (int q = 0; q < 16; q++) {
        hst[m][q] = start ? 0.0f : hst[m][q];   // a select: whatever the old state held is gone
        cin[m][q] = start ? 0.0f : cst[m][q];
      }

    // ---- k_policy_lstm's gate product: the x k-steps, then the four over h ----
    f32x16 acc[8];   // tile 2 gate + m
#pragma unroll
    for (int u = 0; u < 8; u++)
#pragma unroll
      for (int q = 0; q < 16; q++) acc[u][q] = 0.0f;
    for (int s = 0; s < kx; s++) {
      half8 b;
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const int k = 16 * s + 8 * h + j;
        const float xv = ppo_obs_at<OT>(p.obs, base + (size_t)(k < F ? k : 0) * n);   // (always a readable element)
        b[j] = (_Float16)(k < F ? xv : k == F ? ts : k == F + 1 ? 1.0f : 0.0f);
      }
#pragma unroll
      for (int u = 0; u < 8; u++)
        acc[u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wg[(size_t)(u * ks + s) * 64], b, acc[u], 0, 0, 0);
    }
#pragma unroll
    for (int s = 0; s < LSTM_HSTEPS; s++) {
      half8 b;
#pragma unroll
      for (int j = 0; j < 8; j++) b[j] = (_Float16)hst[s >> 1][8 * (s & 1) + j];
#pragma unroll
      for (int u = 0; u < 8; u++)
        acc[u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wg[(size_t)(u * ks + kx + s) * 64], b, acc[u], 0, 0, 0);
    }

    // ---- the cell, lane-local; h straight into the head product's B operand ----
    f32x16 out;
    {
      const float4 *hb = (const float4 *)p.head_bias + lane * 4;
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const float4 v = hb[q];
        out[4 * q + 0] = v.x, out[4 * q + 1] = v.y, out[4 * q + 2] = v.z, out[4 * q + 3] = v.w;
      }
    }
    half8 wh[4];
#pragma unroll
    for (int s = 0; s < 4; s++) wh[s] = ((const half8 *)p.head)[s * 64 + lane];
#pragma unroll
    for (int s = 0; s < 4; s++) {
      const int m = s >> 1;
      half8 b;
#pragma unroll
      for (int j = 0; j < 8; j++) {
#pragma clang fp contract(off)
        const int q = 8 * (s & 1) + j;
        const float gi = sigmoid_complement(acc[2 * LSTM_I + m][q]);
        const float gf = sigmoid_complement(acc[2 * LSTM_F + m][q]);
        const float rg = sigmoid_complement(acc[2 * LSTM_G + m][q]);
        const float gg = 1.0f - 2.0f * rg;
        const float go = sigmoid_complement(acc[2 * LSTM_O + m][q]);
        const float keep = gf * cin[m][q], add = gi * gg;
        const float c = keep + add;
        const float hv = go * (1.0f - 2.0f * sigmoid_complement(RPPO_K_TANH * c));
        if (valid) {
          const size_t unit = (size_t)(32 * m + acc_row(q, h));
          float *z = sc.z + ((size_t)t * 256 + unit) * Es + at0;
          z[(size_t)(64 * LSTM_I) * Es] = gi, z[(size_t)(64 * LSTM_F) * Es] = gf;
          z[(size_t)(64 * LSTM_G) * Es] = rg, z[(size_t)(64 * LSTM_O) * Es] = go;
          sc.cs[((size_t)t * 64 + unit) * Es + at0] = c;
          sc.hs[((size_t)t * 64 + unit) * Es + at0] = hv;
        }
        cst[m][q] = c, hst[m][q] = hv;
        b[j] = (_Float16)hv;
      }
      out = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[s], b, out, 0, 0, 0);
    }

    // ---- AcTail's `given` arithmetic (pick_lp), as k_ppo_grad restates it ----
    const int count = h ? C : 4;
    const int a = p.actions[((size_t)t * 2 + h) * n + env];
    float x[16], e[16], mx = -3.0e38f;
#pragma unroll
    for (int c = 0; c < 16; c++) {
      x[c] = c < count ? out[c] : -3.0e38f;
      mx = fmaxf(mx, x[c]);
    }
    float total = 0.0f;
#pragma unroll
    for (int c = 0; c < 16; c++) {
      e[c] = __builtin_amdgcn_exp2f(x[c] - mx);
      total += e[c];
    }
    float la = x[0];
#pragma unroll
    for (int c = 1; c < 16; c++) la = (c == a) ? x[c] : la;
    const float lg = __builtin_amdgcn_logf(total);
    float lp;
    {
#pragma clang fp contract(off)
      lp = ((la - mx) - lg) * K_LN2;
    }
    if (a < 0 || a >= count) lp = -__builtin_inff();
    const uint32_t bits = __float_as_uint(lp);
    const auto sw = __builtin_amdgcn_permlane32_swap(bits, bits, false, false);
    float lp_sum;
    {
#pragma clang fp contract(off)
      lp_sum = lp + __uint_as_float(h ? sw[0] : sw[1]);   // the other head's term of the same sample
    }
    const float val = out[4] * K_LN2;                     // lower half-wave: row 8 of the product
    if (valid && h == 0) {
      if (p.lp_out != nullptr) p.lp_out[(size_t)t * Es + at0] = lp_sum;
      if (p.v_out != nullptr) p.v_out[(size_t)t * Es + at0] = val;
    }

    // ---- the loss and D_t = d (B loss) / d [logits; value], in the accumulator layout ----
    const bool good = lp_sum > -__builtin_inff();         // false for -inf (a bad action) and for NaN
    const bool ok = valid && good;
    const float old = p.log_probs[smp], ret = p.returns[smp];
    const float ahat = (p.advantages[smp] - mean) / denom;
    const float ratio = expf(lp_sum - old);
    const float t1 = ahat * ratio, t2 = ahat * fminf(fmaxf(ratio, lo), hi);
    const bool through = t1 <= t2 || (ratio >= lo && ratio <= hi);
    const float glp = through ? -t1 : 0.0f;
    float H = 0.0f, lnp[16], pr[16];
    const float inv_total = 1.0f / total;
#pragma unroll
    for (int c = 0; c < 16; c++) {
      pr[c] = e[c] * inv_total;
      lnp[c] = ((x[c] - mx) - lg) * K_LN2;
      H -= c < count ? pr[c] * lnp[c] : 0.0f;
    }
    float d[16];
#pragma unroll
    for (int c = 0; c < 16; c++) {
      const float v = glp * ((c == a ? 1.0f : 0.0f) - pr[c]) + p.ent_coef * (pr[c] * (lnp[c] + H));
      d[c] = (ok && c < count) ? v : 0.0f;
    }
    // value clipping (TRAIN), as k_ppo_grad's: the prediction moves at most cvf from the recorded value, and the
    // gradient passes where it has not been cut (the ends included, as torch's clamp backward does)
    // (selects on the value loaded at the top of the step: no branch, and no load, in the step's tail)
    float vp = val;
    bool vopen = true;
    if constexpr (TRAIN) {
      const float dv = val - oldv;
      vp = vclip ? oldv + fminf(fmaxf(dv, -cvf), cvf) : val;
      vopen = !vclip || (dv >= -cvf && dv <= cvf);
    }
    if (h == 0 && ok) d[4] = vopen ? 2.0f * p.vf_coef * (vp - ret) : 0.0f;
    if (ok) {
      s_ent -= H;
      if (h == 0) {
        s_pol -= fminf(t1, t2);
        s_val += (ret - vp) * (ret - vp);
        s_kl += old - lp_sum;
        s_clip += fabsf(ratio - 1.0f) > clip ? 1.0f : 0.0f;
      }
    }
    if (valid && !good && h == 0) s_bad += 1.0f;
    if (valid) {
#pragma unroll
      for (int q = 0; q < 16; q++) sc.ds[((size_t)t * 32 + (size_t)acc_row(q, h)) * Es + at0] = d[q];
    }
  }

  // ---- the workgroup's loss sums: the 64 lanes in lane order, in double ----
  {
    float *S = sums + lane * RPPO_SUMS;
    S[0] = s_pol, S[1] = s_val, S[2] = s_ent, S[3] = s_kl, S[4] = s_clip, S[5] = s_bad, S[6] = 0.0f, S[7] = 0.0f;
  }
  __syncthreads();
  if (lane < RPPO_SUMS) {
    double s = 0.0;
    for (int l = 0; l < 64; l++) s += (double)sums[l * RPPO_SUMS + lane];
    sc.fpart[(size_t)blockIdx.x * RPPO_SUMS + lane] = (float)s;
  }
}

// ---- c. backpropagation through time ----------------------------------------------------------------------
template <bool TRAIN = false>
__global__ void __launch_bounds__(64) k_rppo_backward(const RppoArgs<TRAIN> p, const int32_t *envs, const int E,
                                                      const RppoScratch sc) {
  if constexpr (TRAIN) {
    if (ppo_halted(p.tr.ctl)) return;   // uniform
  }
  const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
  const int e0 = (int)blockIdx.x * 32 + r;
  const bool valid = e0 < E;
  const int ec = valid ? e0 : E - 1;                     // a lane past the minibatch reads its last sequence
  const uint32_t env = (uint32_t)envs[ec], n32 = (uint32_t)p.n;
  const size_t Es = (size_t)E, at = (size_t)ec;
  const int T = p.T;
  const float *w2t_ = p.bwd + LSTM_WHT_ELEMS + lane;
  // Wh^T's image stays in LDS for the whole sequence: 64 KiB, read one k-step (64 consecutive floats) at a time
  __shared__ float wht_lds[LSTM_WHT_ELEMS];
  for (int i = lane; i < LSTM_WHT_ELEMS; i += 64) wht_lds[i] = p.bwd[i];
  __syncthreads();
  const float *wht = wht_lds + lane;

  float w2t[2][16];
#pragma unroll
  for (int m = 0; m < 2; m++)
#pragma unroll
    for (int q = 0; q < 16; q++) w2t[m][q] = w2t_[(m * 16 + q) * 64];

  f32x16 dhn[2];
  float dcn[2][16];
#pragma unroll
  for (int m = 0; m < 2; m++)
#pragma unroll
    for (int q = 0; q < 16; q++) dhn[m][q] = 0.0f, dcn[m][q] = 0.0f;

  for (int t = T - 1; t >= 0; t--) {
    const bool start = p.episode_starts[(uint32_t)t * n32 + env] > 0.0f;
    // d h = [W2; wv]^T D_t + d h_next
    f32x16 dh[2] = {dhn[0], dhn[1]};
#pragma unroll
    for (int q = 0; q < 16; q++) {
      const float dq = sc.ds[((size_t)t * 32 + (size_t)acc_row(q, h)) * Es + at];
      dh[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(w2t[0][q], dq, dh[0], 0, 0, 0);
      dh[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(w2t[1][q], dq, dh[1], 0, 0, 0);
    }
    // the cell, lane-local: d z in the gate product's accumulator layout, where it is at once the B operand of
    // d h_next = Wh^T d z (k-step (tile, q)); an episode start cuts both carries
    f32x16 nx[2];
#pragma unroll
    for (int q = 0; q < 16; q++) nx[0][q] = 0.0f, nx[1][q] = 0.0f;
#pragma unroll
    for (int m = 0; m < 2; m++)
#pragma unroll
      for (int q = 0; q < 16; q++) {
        const size_t unit = (size_t)(32 * m + acc_row(q, h));
        float *z = sc.z + ((size_t)t * 256 + unit) * Es + at;
        const float gi = z[(size_t)(64 * LSTM_I) * Es], gf = z[(size_t)(64 * LSTM_F) * Es];
        const float rg = z[(size_t)(64 * LSTM_G) * Es], go = z[(size_t)(64 * LSTM_O) * Es];
        const float c = sc.cs[((size_t)t * 64 + unit) * Es + at];
        const float cprev = t > 0 ? sc.cs[((size_t)(t - 1) * 64 + unit) * Es + at] : p.c0[(uint32_t)unit * n32 + env];
        const float cin = start ? 0.0f : cprev;
        const float rc = sigmoid_complement(RPPO_K_TANH * c);
        const float th = 1.0f - 2.0f * rc, gg = 1.0f - 2.0f * rg;
        const float dhv = dh[m][q];
        const float dov = dhv * th;
        const float dc = dcn[m][q] + dhv * go * (4.0f * (rc * (1.0f - rc)));
        float dz[LSTM_GATES];
        dz[LSTM_I] = dc * gg * (gi * (1.0f - gi));
        dz[LSTM_F] = dc * cin * (gf * (1.0f - gf));
        dz[LSTM_G] = dc * gi * (4.0f * (rg * (1.0f - rg)));
        dz[LSTM_O] = dov * (go * (1.0f - go));
        dcn[m][q] = start ? 0.0f : dc * gf;
#pragma unroll
        for (int g = 0; g < LSTM_GATES; g++) {
          if (valid) z[(size_t)(64 * g) * Es] = dz[g];
          const int u = 2 * g + m;
          nx[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(wht[((0 * 8 + u) * 16 + q) * 64], dz[g], nx[0], 0, 0, 0);
          nx[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(wht[((1 * 8 + u) * 16 + q) * 64], dz[g], nx[1], 0, 0, 0);
        }
      }
#pragma unroll
    for (int q = 0; q < 16; q++) {
      dhn[0][q] = start ? 0.0f : nx[0][q];
      dhn[1][q] = start ? 0.0f : nx[1][q];
    }
  }
}

// ---- d. the weight gradients: products over samples ------------------------------------------------------------
template <int OT, bool TRAIN = false>
__global__ void __launch_bounds__(256) k_rppo_wgrad(const RppoArgs<TRAIN> p, const int32_t *envs, const int E,
                                                    const int tiles, const int per, const RppoScratch sc) {
  if constexpr (TRAIN) {
    if (ppo_halted(p.tr.ctl)) return;   // uniform over the four waves: none reaches a barrier
  }
  __shared__ float L[RPPO_ROWS * RPPO_STRIDE];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 31, h = lane >> 5;
  const int col_ = tid & 31, grp = tid >> 5;             // staging: a thread fills column col_ of rows grp, grp + 8, ...
  const int F = p.F, C = p.C, T = p.T;
  const size_t n = (size_t)p.n, Es = (size_t)E;
  const uint32_t n32 = (uint32_t)p.n;
  const int total = T * tiles;
  const bool wide = F + 2 > 32;                          // uniform: a second tile of x columns
  const RppoLayout lay(F, C);

  f32x16 gG[2][4], gH;   // gate w's rows 32 m .. x columns 32 c ..: c < 2 over x, c >= 2 over h_in
#pragma unroll
  for (int q = 0; q < 16; q++) {
    gH[q] = 0.0f;
#pragma unroll
    for (int c = 0; c < 4; c++) gG[0][c][q] = 0.0f, gG[1][c][q] = 0.0f;
  }
  float gb2 = 0.0f;

  for (int k = 0; k < per; k++) {
    const int it = (int)blockIdx.x + (int)gridDim.x * k;
    if (it < total) {   // uniform
      const int t = it / tiles, e0 = (it % tiles) * 32 + col_;
      const bool v = e0 < E;                              // a column past the minibatch holds zeros
      const uint32_t env = (uint32_t)envs[v ? e0 : E - 1];
      const size_t at = (size_t)(v ? e0 : E - 1);
      const uint32_t smp = (uint32_t)t * n32 + env;
      const bool start = p.episode_starts[smp] > 0.0f;
      const float ts = (float)p.timestep[smp];
      const size_t base = (size_t)t * (size_t)F * n + env;
      for (int row = grp; row < 256; row += 8) {
        const float zv = sc.z[((size_t)t * 256 + row) * Es + at];
        L[row * RPPO_STRIDE + col_] = v ? zv : 0.0f;
      }
      for (int kk = grp; kk < 64; kk += 8) {
        const float xv = ppo_obs_at<OT>(p.obs, base + (size_t)(kk < F ? kk : 0) * n);
        const float xf = rppo_f16(kk < F ? xv : kk == F ? ts : kk == F + 1 ? 1.0f : 0.0f);
        L[(RPPO_ROW_X + kk) * RPPO_STRIDE + col_] = v ? xf : 0.0f;
        const float hp = t > 0 ? sc.hs[((size_t)(t - 1) * 64 + kk) * Es + at] : p.h0[(uint32_t)kk * n32 + env];
        L[(RPPO_ROW_HIN + kk) * RPPO_STRIDE + col_] = (v && !start) ? rppo_f16(hp) : 0.0f;
        const float ht = sc.hs[((size_t)t * 64 + kk) * Es + at];
        L[(RPPO_ROW_H + kk) * RPPO_STRIDE + col_] = v ? rppo_f16(ht) : 0.0f;
      }
      for (int row = grp; row < 32; row += 8) {
        const float dv = sc.ds[((size_t)t * 32 + row) * Es + at];
        L[(RPPO_ROW_D + row) * RPPO_STRIDE + col_] = v ? dv : 0.0f;
      }
      __syncthreads();
#pragma unroll
      for (int s = 0; s < 16; s++) {
        const int col = 2 * s + h;
        const float a0 = L[(64 * wv + r) * RPPO_STRIDE + col], a1 = L[(64 * wv + 32 + r) * RPPO_STRIDE + col];
#pragma unroll
        for (int c = 0; c < 4; c++)
          if (c != 1 || wide) {
            const float b = L[(RPPO_ROW_X + 32 * c + r) * RPPO_STRIDE + col];
            gG[0][c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b, gG[0][c], 0, 0, 0);
            gG[1][c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b, gG[1][c], 0, 0, 0);
          }
        if (wv < 2) {   // uniform per wave
          const float ad = L[(RPPO_ROW_D + r) * RPPO_STRIDE + col];
          gb2 += ad;
          gH = __builtin_amdgcn_mfma_f32_32x32x2f32(ad, L[(RPPO_ROW_H + 32 * wv + r) * RPPO_STRIDE + col], gH, 0, 0, 0);
        }
      }
      __syncthreads();
    }
  }

  // ---- the workgroup's partial: every parameter has exactly one owner ----
  float *mine = sc.wpart + (size_t)blockIdx.x * (size_t)lay.P;
#pragma unroll
  for (int m = 0; m < 2; m++)
#pragma unroll
    for (int c = 0; c < 4; c++)
#pragma unroll
      for (int q = 0; q < 16; q++) {
        const int row = 64 * wv + 32 * m + acc_row(q, h), kk = 32 * c + r;
        const int pi = c < 2 ? lay.gate(row, kk) : lay.rec(row, kk - 64);
        if (pi >= 0) mine[pi] = gG[m][c][q];
      }
  if (wv < 2) {
#pragma unroll
    for (int q = 0; q < 16; q++) {
      const int pi = lay.second(acc_row(q, h), 32 * wv + r);
      if (pi >= 0) mine[pi] = gH[q];
    }
  }
  __syncthreads();
  if (wv == 0) L[lane] = gb2;
  __syncthreads();
  if (tid < 32) {          // row tid of the head product: lanes tid and tid + 32 of wave 0
    const int pi = lay.bias(tid);
    if (pi >= 0) mine[pi] = L[tid] + L[tid + 32];
  }
}

// ---- e. reduce, clip, statistics; Adam and the repack ----------------------------------------------------------
template <bool TRAIN = false>
__global__ void __launch_bounds__(RPPO_REDUCE_THREADS) k_rppo_reduce(const RppoScratch sc, const int G, const int P,
                                                                    const float fB, const RppoOut<TRAIN> out) {
  if constexpr (TRAIN) {
    if (ppo_halted(out.ctl)) return;   // uniform
  }
  float *grad = out.to;
  __shared__ double red[RPPO_REDUCE_THREADS];
  const int tid = threadIdx.x, pi = (int)blockIdx.x * RPPO_REDUCE_THREADS + tid;
  float s = 0.0f;
  if (pi < P) {
    for (int g = 0; g < G; g++) s += sc.wpart[(size_t)g * (size_t)P + pi];
    s /= fB;
    grad[pi] = s;
  }
  red[tid] = (double)s * (double)s;
  __syncthreads();
  for (int off = RPPO_REDUCE_THREADS / 2; off > 0; off >>= 1) {
    if (tid < off) red[tid] += red[tid + off];
    __syncthreads();
  }
  if (tid == 0) sc.sq[blockIdx.x] = red[0];
}

template <bool APPLY, bool TRAIN = false>
__global__ void __launch_bounds__(PPO_FINISH_THREADS) k_rppo_finish(const RppoArgs<TRAIN> p, const int B, const int Gf,
                                                                   const int Gr, const RppoScratch sc) {
  if constexpr (TRAIN) {
    if (ppo_halted(p.tr.ctl)) return;   // uniform
  }
  __shared__ double red[PPO_FINISH_THREADS];
  const int tid = threadIdx.x, F = p.F, C = p.C;
  const RppoLayout lay(F, C);
  double sq = 0.0;
  for (int i = tid; i < Gr; i += PPO_FINISH_THREADS) sq += sc.sq[i];
  const float norm = (float)sqrt(ppo_block_sum(red, sq));
  const float coef = fminf(1.0f, p.max_grad_norm / (norm + 1e-6f));
  if (tid == 0) {
    double s[6];
    for (int w = 0; w < 6; w++) {
      s[w] = 0.0;
      for (int k = 0; k < Gf; k++) s[w] += (double)sc.fpart[(size_t)k * RPPO_SUMS + w];
    }
    const double pol = s[0] / B, val = s[1] / B, ent = s[2] / B;   // s[2] = -sum H
    p.stats[0] = (float)pol, p.stats[1] = (float)val, p.stats[2] = (float)ent;
    p.stats[3] = (float)(s[3] / B), p.stats[4] = (float)(s[4] / B), p.stats[5] = norm;
    p.stats[8] = (float)s[5];
    p.stats[9] = (float)(pol + (double)p.ent_coef * ent + (double)p.vf_coef * val);
    if constexpr (TRAIN) {
      // the float values just written, added in double by this one thread (k_ppo_finish's accounting): the
      // same sequence of minibatches gives the same sums, bit for bit
      double *acc = p.tr.acc;
      acc[OC_PPO_ACC_EPOCH_KL] += (double)p.stats[3];
      acc[OC_PPO_ACC_EPOCH_COUNT] += 1.0;
      acc[OC_PPO_ACC_SUMS + 0] += (double)p.stats[0], acc[OC_PPO_ACC_SUMS + 1] += (double)p.stats[1];
      acc[OC_PPO_ACC_SUMS + 2] += (double)p.stats[2], acc[OC_PPO_ACC_SUMS + 3] += (double)p.stats[3];
      acc[OC_PPO_ACC_SUMS + 4] += (double)p.stats[4], acc[OC_PPO_ACC_SUMS + 5] += (double)p.stats[9];
      p.tr.ctl[OC_PPO_CTL_UPDATES] += 1;
    }
  }
  int step = 0;
  float step_size = 0.0f, bc2s = 1.0f;
  if constexpr (APPLY) {
    step = p.step[0] + 1;
    const float lr = p.hyper[0];
    const float bc1 = (float)(1.0 - pow((double)p.beta1, (double)step));
    bc2s = (float)sqrt(1.0 - pow((double)p.beta2, (double)step));
    step_size = lr / bc1;
  }
  for (int pi = tid; pi < lay.P; pi += PPO_FINISH_THREADS) {
    const float g = p.grad[pi] * coef;
    p.grad[pi] = g;
    if constexpr (APPLY) {
      float *w = rppo_param(p, lay, pi);
      const float m = p.beta1 * p.m[pi] + (1.0f - p.beta1) * g;
      const float v = p.beta2 * p.v[pi] + (1.0f - p.beta2) * (g * g);
      p.m[pi] = m, p.v[pi] = v;
      *w = *w - step_size * (m / (sqrtf(v) / bc2s + p.eps));
    }
  }
  if constexpr (APPLY) {
    __threadfence_block();
    __syncthreads();     // every new weight is written: the repack reads them back
    if (tid == 0) p.step[0] = step;
    // the repack: the host packers' values through the same maps and the same fold (oc_policy_layout.h)
    _Float16 *og = (_Float16 *)p.gates, *oh = (_Float16 *)p.head;
    for (int el = tid; el < lstm_gate_elems(F); el += PPO_FINISH_THREADS) {
      const GateSrc s = lstm_gate_source(el, F);
      const int row = HIDDEN * s.gate + s.unit;
      const int pi = s.k < 0 ? lay.rec(row, s.hid) : lay.gate(row, s.k);
      og[el] = rppo_fold(pi >= 0 ? *rppo_param(p, lay, pi) : 0.0f, lstm_gate_fold(s.gate));
    }
    for (int el = tid; el < W2_ELEMS; el += PPO_FINISH_THREADS) {
      const RowHid s = w2_source(el);
      const int pi = lay.second(s.row, s.hid);
      oh[el] = pi >= 0 ? rppo_fold(*rppo_param(p, lay, pi), FOLD_LOG2E) : (_Float16)0.0f;
    }
    for (int el = tid; el < B2_ELEMS; el += PPO_FINISH_THREADS) {
      const int pi = lay.bias(b2_row(el));
      p.head_bias[el] = pi >= 0 ? FOLD_LOG2E * *rppo_param(p, lay, pi) : 0.0f;
    }
    for (int el = tid; el < LSTM_WHT_ELEMS; el += PPO_FINISH_THREADS) {
      const GateHid s = lstm_wht_source(el);
      const float w = *rppo_param(p, lay, lay.rec(HIDDEN * s.gate + s.unit, s.hid));
      p.bwd[el] = (float)rppo_fold(w, lstm_gate_fold(s.gate)) * lstm_gate_unfold(s.gate);
    }
    for (int el = tid; el < W2T_ELEMS; el += PPO_FINISH_THREADS) {
      const RowHid s = w2t_source(el);
      const int pi = lay.second(s.row, s.hid);
      p.bwd[LSTM_WHT_ELEMS + el] = pi >= 0 ? (float)rppo_fold(*rppo_param(p, lay, pi), FOLD_LOG2E) * FOLD_LN2 : 0.0f;
    }
  }
}

}  // namespace ocpol
#endif
