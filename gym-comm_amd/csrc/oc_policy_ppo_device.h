// oc_policy_ppo_device.h -- the kernels of the PPO update (include/oc_policy.h: oc_policy_ppo_update,
// oc_policy_ppo_grad) for the fused actor-critic seat, and -- the same templates with TRAIN = true -- of
// a step of the train sequence (oc_policy_ppo_train_step).  Included by oc_policy_ppo.hip, which
// instantiates the TRAIN = false kernels only, and by oc_policy_train.hip, which instantiates the
// TRAIN = true ones only.  gfx950 only.
//
// Three launches per minibatch, all sized by B alone:
//
//   k_ppo_adv      one workgroup: mean and unbiased std of the gathered advantages, in double.
//   k_ppo_grad     the hot kernel.  One wave = one TILE of 32 samples at a time, the sample on the
//                  lane, exactly as the forward lays the envs out (oc_policy_device.h); four waves
//                  per workgroup, one per SIMD (512 registers per lane, no scratch).
//                    forward    policy_pass's two fp16 products and AcTail's `given` arithmetic,
//                               operation for operation: lp and v are score()'s bits
//                    dlogits    formed in place, in the second product's accumulator layout
//                               (lower half-wave: 4 move rows and the value row, upper: C comm rows)
//                    dh         = W2^T . dlogits -- that accumulator layout IS the B-operand layout
//                               of a product over rows (v_mfma_f32_32x32x2_f32: register t of the
//                               half-wave h is row (t & 3) + 8 (t >> 2) + 4 h = k-step t), so no lane
//                               moves: the learner keeps a transposed, k-permuted fp32 image of W2
//                               (`w2t`).  dh comes out in the first product's accumulator layout,
//                               next to r: dpre = dh * 4 r (1 - r) elementwise.
//                    the three products that sum over SAMPLES (dW2 = dlogits . h^T, dW1aug = dpre .
//                    x^T, db2 = row sums of dlogits) need the sample along K: dlogits, h, dpre and
//                    the input tile make one round trip through LDS ([row][sample], stride 33
//                    floats: a wave's 32 rows of one sample column fall into 32 banks) and come back
//                    as fp32 MFMA operands.  The gradient lives in 6 x 16 accumulator registers
//                    across the wave's tiles; the 1/B factor is applied afterwards, in fp32.
//                  At the end the four waves' accumulators are summed through LDS in wave order
//                  and the workgroup writes ITS partial gradient and loss sums: no atomics.
//   k_ppo_finish   one workgroup: partials summed over g ascending, one thread per parameter; the
//                  squared norm in double, in a fixed order; clip; statistics; and (APPLY) Adam on
//                  the fp32 master weights and the repack of every fragment image on the device,
//                  through the host packers' own maps (oc_policy_layout.h).
//
// TRAIN = true (oc_policy_ppo_train_step): every kernel returns at once, having written nothing, when
// the train sequence is halted (ctl.stop or ctl.error); k_ppo_grad clips the value prediction around
// the recorded value where hyper_ext[0] > 0; k_ppo_finish adds the minibatch's statistics to the
// epoch's and the train's sums.  TRAIN = false takes the arguments, and compiles to the code, it had
// before the variants existed: PpoArgs<false> and AdvOut<false> add no member.
#ifndef OC_POLICY_PPO_DEVICE_H
#define OC_POLICY_PPO_DEVICE_H
#include "../../include/oc_policy.h"
#include "oc_policy_ac_device.h"
#include "oc_policy_fail.h"
#include "oc_policy_layout.h"

namespace ocpol {

constexpr int PPO_WAVES = 4;          // waves per workgroup of k_ppo_grad
constexpr int PPO_STRIDE = 33;        // floats between two rows of a wave's LDS tile
constexpr int PPO_ROWS = 112;         // phase A: dlogits 32 + h 64; phase B: dpre 64 + x 48
constexpr int PPO_SUMS = 8;           // loss sums a workgroup appends to its partial gradient
constexpr int PPO_FINISH_THREADS = 1024;
constexpr int PPO_MAX_P = 5 * PPO_FINISH_THREADS;   // >= 64 * 46 + 128 + 20 * 64 + 20 + 65 = 4437

// the kernels' arguments: the update's alone, or with the train sequence's device state behind them
template <bool TRAIN>
struct PpoArgs : oc_ppo_cfg {};
template <>
struct PpoArgs<true> : oc_ppo_cfg {
  oc_ppo_train tr;
};
template <bool TRAIN>
struct AdvOut {
  float *stats;
};
template <>
struct AdvOut<true> {
  float *stats;
  const int32_t *ctl;
};

// a halted train sequence: stopped by the KL rule, or an error word set (oc_policy.h)
__device__ __forceinline__ bool ppo_halted(const int32_t *ctl) {
  return (ctl[OC_PPO_CTL_STOP] | ctl[OC_PPO_CTL_ERROR]) != 0;
}

__device__ __forceinline__ float *ppo_param(const oc_ppo_cfg &p, const PpoLayout &lay, int pi) {
  if (pi < lay.wt) return p.p_w1 + pi;
  if (pi < lay.b1) return p.p_wt + (pi - lay.wt);
  if (pi < lay.w2) return p.p_b1 + (pi - lay.b1);
  if (pi < lay.b2) return p.p_w2 + (pi - lay.w2);
  if (pi < lay.wv) return p.p_b2 + (pi - lay.b2);
  if (pi < lay.bv) return p.p_wv + (pi - lay.wv);
  return p.p_bv;
}

// obs_at with a 64-bit index: T * F * n exceeds 32 bits, and obs_at is 32-bit on purpose (oc_policy_device.h)
template <int OT>
__device__ __forceinline__ float ppo_obs_at(const void *obs, size_t idx) {
  if (OT == 1) return (float)((const int8_t *)obs)[idx];
  if (OT == 2) return ((const float *)obs)[idx];
  return (float)((const int32_t *)obs)[idx];
}

// sum of red[0 .. PPO_FINISH_THREADS) in a fixed tree order; every thread gets the result
__device__ __forceinline__ double ppo_block_sum(double *red, double mine) {
  const int tid = threadIdx.x;
  __syncthreads();
  red[tid] = mine;
  __syncthreads();
  for (int off = PPO_FINISH_THREADS / 2; off > 0; off >>= 1) {
    if (tid < off) red[tid] += red[tid + off];
    __syncthreads();
  }
  return red[0];
}

// ---- a. advantage statistics ----------------------------------------------------------------
template <bool TRAIN = false>
__global__ void __launch_bounds__(PPO_FINISH_THREADS) k_ppo_adv(const float *adv, const int32_t *idx, const int B,
                                                               const AdvOut<TRAIN> out) {
  if constexpr (TRAIN) {
    if (ppo_halted(out.ctl)) return;   // uniform
  }
  float *stats = out.stats;
  __shared__ double red[PPO_FINISH_THREADS];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int i = tid; i < B; i += PPO_FINISH_THREADS) s += (double)adv[idx[i]];
  const double mean = ppo_block_sum(red, s) / (double)B;
  double q = 0.0;
  for (int i = tid; i < B; i += PPO_FINISH_THREADS) {
    const double d = (double)adv[idx[i]] - mean;
    q += d * d;
  }
  const double var = ppo_block_sum(red, q) / (double)(B - 1);
  if (tid == 0) stats[6] = (float)mean, stats[7] = (float)sqrt(var);
}

// ---- b. loss and gradient -------------------------------------------------------------------
template <int OT, bool TRAIN = false>
__global__ void __launch_bounds__(64 * PPO_WAVES) k_ppo_grad(const PpoArgs<TRAIN> p, const int32_t *idx, const int B,
                                                             const int tpw, float *part) {
  if constexpr (TRAIN) {
    if (ppo_halted(p.tr.ctl)) return;   // uniform
  }
  __shared__ float lds[PPO_WAVES * PPO_ROWS * PPO_STRIDE];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 31, h = lane >> 5;
  float *L = lds + wv * (PPO_ROWS * PPO_STRIDE);
  const int F = p.F, C = p.C, ks = ksteps(F);
  const size_t n = (size_t)p.n;
  const uint32_t n32 = (uint32_t)p.n;
  const int W = (int)gridDim.x * PPO_WAVES, gw = (int)blockIdx.x * PPO_WAVES + wv;
  const PpoLayout lay(F, C);
  const float mean = p.stats[6], denom = p.stats[7] + 1e-8f, clip = p.hyper[1];
  const float lo = 1.0f - clip, hi = 1.0f + clip;
  float cvf = 0.0f;                      // clip_range_vf; <= 0 (or NaN): no value clipping
  if constexpr (TRAIN) cvf = p.tr.hyper_ext[0];
  const bool vclip = cvf > 0.0f;         // uniform

  Weights wt;
  load_weights(wt, p.w1, p.w2, p.b2, lane, ks);
  float w2t[2][16];
#pragma unroll
  for (int m = 0; m < 2; m++)
#pragma unroll
    for (int t = 0; t < 16; t++) w2t[m][t] = p.w2t[(m * 16 + t) * 64 + lane];

  f32x16 gW1[2][2], gW2[2];
#pragma unroll
  for (int q = 0; q < 16; q++)
    gW1[0][0][q] = gW1[0][1][q] = gW1[1][0][q] = gW1[1][1][q] = gW2[0][q] = gW2[1][q] = 0.0f;
  float gb2 = 0.0f, s_pol = 0.0f, s_val = 0.0f, s_ent = 0.0f, s_kl = 0.0f, s_clip = 0.0f, s_bad = 0.0f;

  for (int k = 0; k < tpw; k++) {
    const int i0 = (gw + W * k) * 32 + r;
    const bool valid = i0 < B;             // a tile past the batch: every lane computes on the last sample, adds zeros
    const uint32_t smp = (uint32_t)idx[valid ? i0 : B - 1];
    const uint32_t slot = smp / n32, env = smp % n32;
    const size_t base = (size_t)slot * (size_t)F * n + env;
    const float ts = (float)p.timestep[smp];

    // ---- the forward: policy_pass's products, AcTail's `given` arithmetic ----
    f32x16 acc0, acc1;
#pragma unroll
    for (int q = 0; q < 16; q++) acc0[q] = 0.0f, acc1[q] = 0.0f;
    half8 xb[MAX_KSTEPS];
#pragma unroll
    for (int s = 0; s < MAX_KSTEPS; s++)
      if (s < ks) {   // uniform
        half8 b;
#pragma unroll
        for (int j = 0; j < 8; j++) {
          const int kk = 16 * s + 8 * h + j;
          const float xv = ppo_obs_at<OT>(p.obs, base + (size_t)(kk < F ? kk : 0) * n);
          b[j] = (_Float16)(kk < F ? xv : kk == F ? ts : kk == F + 1 ? 1.0f : 0.0f);
        }
        xb[s] = b;
        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(wt.w1[0][s], b, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(wt.w1[1][s], b, acc1, 0, 0, 0);
      }
    f32x16 out;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const float4 v = wt.b2[q];
      out[4 * q + 0] = v.x, out[4 * q + 1] = v.y, out[4 * q + 2] = v.z, out[4 * q + 3] = v.w;
    }
    float rv[2][16];
#pragma unroll
    for (int s = 0; s < 4; s++) {
      half8 b;
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const float av = (s >> 1) ? acc1[8 * (s & 1) + j] : acc0[8 * (s & 1) + j];
        const float rr = sigmoid_complement(av);
        rv[s >> 1][8 * (s & 1) + j] = rr;
        b[j] = (_Float16)rr;
      }
      out = __builtin_amdgcn_mfma_f32_32x32x16_f16(wt.w2[s], b, out, 0, 0, 0);
    }
    const int count = h ? C : 4;
    const int a = p.actions[((size_t)slot * 2 + h) * n + env];
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
      if (p.lp_out != nullptr) p.lp_out[i0] = lp_sum;
      if (p.v_out != nullptr) p.v_out[i0] = val;
    }

    // ---- the loss and d loss / d logits (times B), in the accumulator layout ----
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
    f32x16 d;
#pragma unroll
    for (int c = 0; c < 16; c++) {
      const float v = glp * ((c == a ? 1.0f : 0.0f) - pr[c]) + p.ent_coef * (pr[c] * (lnp[c] + H));
      d[c] = (ok && c < count) ? v : 0.0f;
    }
    // value clipping (TRAIN): the prediction moves at most cvf from the recorded value, and the
    // gradient passes where it has not been cut (the ends included, as torch's clamp backward does)
    float vp = val;
    bool vopen = true;
    if constexpr (TRAIN) {
      if (vclip) {
        const float oldv = p.tr.values[smp], dv = val - oldv;
        vp = oldv + fminf(fmaxf(dv, -cvf), cvf);
        vopen = dv >= -cvf && dv <= cvf;
      }
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

    // ---- dh = W2^T . dlogits, dpre = dh tanh' ----
    f32x16 dh0, dh1;
#pragma unroll
    for (int q = 0; q < 16; q++) dh0[q] = 0.0f, dh1[q] = 0.0f;
#pragma unroll
    for (int t = 0; t < 16; t++) {
      dh0 = __builtin_amdgcn_mfma_f32_32x32x2f32(w2t[0][t], d[t], dh0, 0, 0, 0);
      dh1 = __builtin_amdgcn_mfma_f32_32x32x2f32(w2t[1][t], d[t], dh1, 0, 0, 0);
    }

    // ---- phase A: dlogits and h through LDS; dW2 and db2 ----
#pragma unroll
    for (int q = 0; q < 16; q++) {
      const int row = acc_row(q, h);
      L[row * PPO_STRIDE + r] = d[q];
      L[(32 + row) * PPO_STRIDE + r] = 1.0f - 2.0f * rv[0][q];
      L[(64 + row) * PPO_STRIDE + r] = 1.0f - 2.0f * rv[1][q];
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 16; t++) {
      const int col = 2 * t + h;
      const float av = L[r * PPO_STRIDE + col];
      gb2 += av;
      gW2[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, L[(32 + r) * PPO_STRIDE + col], gW2[0], 0, 0, 0);
      gW2[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, L[(64 + r) * PPO_STRIDE + col], gW2[1], 0, 0, 0);
    }
    __syncthreads();

    // ---- phase B: dpre and the input tile through LDS; dW1aug ----
    // dh is in units of the folded weights: W2 = W2' / (-2 log2 e), so dpre = (-ln 2 / 2) dh 4 r (1 - r)
#pragma unroll
    for (int q = 0; q < 16; q++) {
      const int row = acc_row(q, h);
      L[row * PPO_STRIDE + r] = (-2.0f * K_LN2 * dh0[q]) * (rv[0][q] * (1.0f - rv[0][q]));
      L[(32 + row) * PPO_STRIDE + r] = (-2.0f * K_LN2 * dh1[q]) * (rv[1][q] * (1.0f - rv[1][q]));
    }
#pragma unroll
    for (int s = 0; s < MAX_KSTEPS; s++)
      if (s < ks) {
#pragma unroll
        for (int j = 0; j < 8; j++) L[(64 + 16 * s + 8 * h + j) * PPO_STRIDE + r] = (float)xb[s][j];
      }
    __syncthreads();
    const int xr1 = 32 + (r & 15);     // second feature tile: 16 rows; its upper columns are never stored
#pragma unroll
    for (int t = 0; t < 16; t++) {
      const int col = 2 * t + h;
      const float a0 = L[r * PPO_STRIDE + col], a1 = L[(32 + r) * PPO_STRIDE + col];
      const float b0 = L[(64 + r) * PPO_STRIDE + col];
      gW1[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, gW1[0][0], 0, 0, 0);
      gW1[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, gW1[1][0], 0, 0, 0);
      if (ks > 2) {   // uniform
        const float b1 = L[(64 + xr1) * PPO_STRIDE + col];
        gW1[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, gW1[0][1], 0, 0, 0);
        gW1[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, gW1[1][1], 0, 0, 0);
      }
    }
    __syncthreads();
  }

  // ---- the four waves' shares, summed in wave order; the workgroup's partial ----
  float *mine = part + (size_t)blockIdx.x * (size_t)(lay.P + PPO_SUMS);
  auto flush = [&](const f32x16 &acc, auto index_of) {
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 16; q++) lds[wv * 1024 + q * 64 + lane] = acc[q];
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int el = tid + 256 * u, q = el >> 6, ln = el & 63;
      const float s = ((lds[el] + lds[1024 + el]) + lds[2048 + el]) + lds[3072 + el];
      const int pi = index_of(acc_row(q, ln >> 5), ln & 31);
      if (pi >= 0) mine[pi] = s;
    }
  };
  flush(gW1[0][0], [&](int i, int j) { return lay.first(i, j); });
  flush(gW1[1][0], [&](int i, int j) { return lay.first(32 + i, j); });
  if (ks > 2) {
    flush(gW1[0][1], [&](int i, int j) { return j < 16 ? lay.first(i, 32 + j) : -1; });
    flush(gW1[1][1], [&](int i, int j) { return j < 16 ? lay.first(32 + i, 32 + j) : -1; });
  }
  flush(gW2[0], [&](int i, int j) { return lay.second(i, j); });
  flush(gW2[1], [&](int i, int j) { return lay.second(i, 32 + j); });
  __syncthreads();
  {
    float *S = lds + wv * 64 * 8 + lane * 8;
    S[0] = gb2, S[1] = s_pol, S[2] = s_val, S[3] = s_ent, S[4] = s_kl, S[5] = s_clip, S[6] = s_bad, S[7] = 0.0f;
  }
  __syncthreads();
  if (tid < 32) {          // row tid of the second product: lanes tid and tid + 32 of the four waves
    float s = 0.0f;
    for (int w = 0; w < PPO_WAVES; w++) s += lds[(w * 64 + tid) * 8] + lds[(w * 64 + tid + 32) * 8];
    const int pi = lay.bias(tid);
    if (pi >= 0) mine[pi] = s;
  } else if (tid >= 64 && tid < 64 + 6) {
    const int which = tid - 64 + 1;
    double s = 0.0;
    for (int t = 0; t < 64 * PPO_WAVES; t++) s += (double)lds[t * 8 + which];
    mine[lay.P + which - 1] = (float)s;
  }
}

// ---- c, d. reduce, clip, statistics; Adam and the repack ---------------------------------------
template <bool APPLY, bool TRAIN = false>
__global__ void __launch_bounds__(PPO_FINISH_THREADS) k_ppo_finish(const PpoArgs<TRAIN> p, const int B, const int G,
                                                                  const float *part) {
  if constexpr (TRAIN) {
    if (ppo_halted(p.tr.ctl)) return;   // uniform
  }
  __shared__ double red[PPO_FINISH_THREADS];
  __shared__ float neww[APPLY ? PPO_MAX_P : 1];
  __shared__ float start[OC_POLICY_MAX_COMM + 5];   // b2's value per logit row, then the value head's
  const int tid = threadIdx.x, F = p.F, C = p.C;
  const PpoLayout lay(F, C);
  const size_t stride = (size_t)(lay.P + PPO_SUMS);
  const float fB = (float)B;

  float g[5];
  double sq = 0.0;
#pragma unroll
  for (int u = 0; u < 5; u++) {
    const int pi = tid + PPO_FINISH_THREADS * u;
    float s = 0.0f;
    if (pi < lay.P) {
      for (int k = 0; k < G; k++) s += part[k * stride + pi];
      s /= fB;
    }
    g[u] = s;
    sq += (double)s * (double)s;
  }
  const float norm = (float)sqrt(ppo_block_sum(red, sq));
  const float coef = fminf(1.0f, p.max_grad_norm / (norm + 1e-6f));
#pragma unroll
  for (int u = 0; u < 5; u++) {
    const int pi = tid + PPO_FINISH_THREADS * u;
    g[u] *= coef;
    if (pi < lay.P) p.grad[pi] = g[u];
  }
  if (tid == 0) {
    double s[6];
    for (int w = 0; w < 6; w++) {
      s[w] = 0.0;
      for (int k = 0; k < G; k++) s[w] += (double)part[k * stride + lay.P + w];
    }
    const double pol = s[0] / B, val = s[1] / B, ent = s[2] / B;   // s[2] = -sum H
    p.stats[0] = (float)pol, p.stats[1] = (float)val, p.stats[2] = (float)ent;
    p.stats[3] = (float)(s[3] / B), p.stats[4] = (float)(s[4] / B), p.stats[5] = norm;
    p.stats[8] = (float)s[5];
    p.stats[9] = (float)(pol + (double)p.ent_coef * ent + (double)p.vf_coef * val);
    if constexpr (TRAIN) {
      // the float values just written, added in double by this one thread: the same sequence of
      // minibatches gives the same sums, bit for bit
      double *acc = p.tr.acc;
      acc[OC_PPO_ACC_EPOCH_KL] += (double)p.stats[3];
      acc[OC_PPO_ACC_EPOCH_COUNT] += 1.0;
      acc[OC_PPO_ACC_SUMS + 0] += (double)p.stats[0], acc[OC_PPO_ACC_SUMS + 1] += (double)p.stats[1];
      acc[OC_PPO_ACC_SUMS + 2] += (double)p.stats[2], acc[OC_PPO_ACC_SUMS + 3] += (double)p.stats[3];
      acc[OC_PPO_ACC_SUMS + 4] += (double)p.stats[4], acc[OC_PPO_ACC_SUMS + 5] += (double)p.stats[9];
      p.tr.ctl[OC_PPO_CTL_UPDATES] += 1;
    }
  }
  if constexpr (APPLY) {
    const int step = p.step[0] + 1;
    const float lr = p.hyper[0];
    const float bc1 = (float)(1.0 - pow((double)p.beta1, (double)step));
    const float bc2s = (float)sqrt(1.0 - pow((double)p.beta2, (double)step));
    const float step_size = lr / bc1;
#pragma unroll
    for (int u = 0; u < 5; u++) {
      const int pi = tid + PPO_FINISH_THREADS * u;
      if (pi < lay.P) {
        float *w = ppo_param(p, lay, pi);
        const float m = p.beta1 * p.m[pi] + (1.0f - p.beta1) * g[u];
        const float v = p.beta2 * p.v[pi] + (1.0f - p.beta2) * (g[u] * g[u]);
        const float nw = *w - step_size * (m / (sqrtf(v) / bc2s + p.eps));
        p.m[pi] = m, p.v[pi] = v, *w = nw, neww[pi] = nw;
      }
    }
    __syncthreads();
    if (tid == 0) p.step[0] = step;
    // the repack, from the new weights in LDS: the host packers' values through the same maps and the
    // same fold (oc_policy_layout.h), looked up in the flat parameter vector
    const int rows2 = 4 + C;                     // logit rows; row `rows2` stands for the value head
    if (tid <= rows2)
      start[tid] = b2_start(neww[tid < rows2 ? lay.b2 + tid : lay.bv], neww + (tid < rows2 ? lay.w2 + tid * HIDDEN : lay.wv));
    __syncthreads();
    const int ks = ksteps(F);
    _Float16 *o1 = (_Float16 *)p.w1, *o2 = (_Float16 *)p.w2;
    for (int el = tid; el < w1_elems(ks); el += PPO_FINISH_THREADS) {
      const HidK s = w1_source(el, ks);
      const int pi = lay.first(s.hid, s.k);
      o1[el] = fold(pi >= 0 ? neww[pi] : 0.0f, FOLD_W1);
    }
    for (int el = tid; el < W2_ELEMS; el += PPO_FINISH_THREADS) {
      const RowHid s = w2_source(el);
      const int pi = lay.second(s.row, s.hid);
      o2[el] = pi >= 0 ? fold(neww[pi], FOLD_W2) : (_Float16)0.0f;
    }
    for (int el = tid; el < B2_ELEMS; el += PPO_FINISH_THREADS) {
      const int pi = lay.bias(b2_row(el));
      p.b2[el] = pi >= 0 ? start[pi < lay.wv ? pi - lay.b2 : rows2] : 0.0f;
    }
    for (int el = tid; el < W2T_ELEMS; el += PPO_FINISH_THREADS) {
      const RowHid s = w2t_source(el);
      const int pi = lay.second(s.row, s.hid);
      p.w2t[el] = pi >= 0 ? (float)fold(neww[pi], FOLD_W2) : 0.0f;
    }
  }
}

// ---- host side, shared by the two units --------------------------------------------------------
// the checks of one minibatch, made before any device work (oc_policy_ppo.hip); plan as oc_policy_ppo_plan's
int ppo_check(const char *who, const oc_ppo_cfg *c, const int32_t *idx, int32_t B, bool apply, int32_t *plan);

// the train state's pointers (oc_policy_train.hip, oc_policy_rtrain.hip)
inline int train_check(const char *who, const oc_ppo_train *t) {
  if (!t) return fail("%s: bad argument (train)", who);
  if (!t->values || !t->hyper_ext || !t->ctl || !t->acc)
    return fail("%s: a NULL pointer among the train state's values, hyper_ext, ctl, acc", who);
  return 0;
}

// after a unit's launches: 0, or the launch error, recorded under the entry point's name
inline int ppo_launched(const char *who) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    fail("%s: kernel launch: %s", who, hipGetErrorString(e));
    return (int)e;
  }
  return 0;
}

}  // namespace ocpol
#endif
