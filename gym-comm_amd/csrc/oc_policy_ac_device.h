// oc_policy_ac_device.h -- the actor-critic tail of the MLP policy (include/oc_policy.h:
// oc_policy_mlp_ac): behind the two products of policy_pass (oc_policy_device.h: its `Tail`) it
// chooses -- or is given -- the action, and reports its log-probability and the value head.
// Included by oc_policy.hip only: the stepper's libraries gain no code.  gfx950 only.
//
// After the second product the LOWER half-wave's lane r holds env r's four move logits (registers
// 0..3) and its value (register 4 = row 8, which no logit uses), the UPPER half's lane r + 32 the
// env's comm logits (registers 0..C-1).  Each lane forms the log-probability of its own head's
// action from the softmax normaliser the sampler computes anyway; ONE half-wave exchange
// (v_permlane32_swap) brings the comm head's term down to the lane that holds the move head's,
// which adds them and stores log_prob, value and move_row; lane r + 32 stores comm_row.
#ifndef OC_POLICY_AC_DEVICE_H
#define OC_POLICY_AC_DEVICE_H
#include "oc_policy_device.h"

namespace ocpol {

enum { AC_GREEDY = 0, AC_SAMPLE = 1, AC_GIVEN = 2 };

// pick<CMAX> (oc_policy_device.h) with the log-probability of the action it returns.  The
// sampler's arithmetic is pick's, operation for operation -- same maximum, same 2^(x - m) terms,
// same total in candidate order, same draw, same cumulative sums -- so from equal stream states
// both choose the same action; here the terms and the total are formed in every mode:
//     lp = ((L_a - m) - log2 S) ln 2                           (v_log_f32 is the base-2 logarithm)
// AC_GIVEN: the action is `given`; outside 0..count-1 its log-probability is -inf and nothing is
// indexed with it (the logit is taken by a chain of selects, as everywhere in this file: no
// private memory).
template <int CMAX>
__device__ __forceinline__ int pick_lp(const f32x16 &v, int count, int mode, int given, uint32_t &state, float &lp) {
  float x[CMAX], e[CMAX], m = -3.0e38f;
#pragma unroll
  for (int c = 0; c < CMAX; c++) {
    x[c] = c < count ? v[c] : -3.0e38f;
    m = fmaxf(m, x[c]);
  }
  float total = 0.0f;
#pragma unroll
  for (int c = 0; c < CMAX; c++) {
    e[c] = __builtin_amdgcn_exp2f(x[c] - m);   // 2^-huge = 0 for the padding candidates
    total += e[c];
  }
  int arg = 0;
  if (mode == AC_SAMPLE) {   // uniform
    const float u = ((float)(pcg32(state) >> 8) + 0.5f) * (1.0f / 16777216.0f);   // (0, 1)
    const float t = u * total;
    float cum = 0.0f;
#pragma unroll
    for (int c = 0; c < CMAX - 1; c++) {
      cum += e[c];
      arg += (cum <= t && c < count - 1) ? 1 : 0;
    }
  } else if (mode == AC_GREEDY) {
#pragma unroll
    for (int c = CMAX - 1; c >= 0; c--) arg = (x[c] == m) ? c : arg;   // the first maximum wins
  } else {
    arg = given;
  }
  float la = x[0];
#pragma unroll
  for (int c = 1; c < CMAX; c++) la = (c == arg) ? x[c] : la;
  {
#pragma clang fp contract(off)
    lp = ((la - m) - __builtin_amdgcn_logf(total)) * K_LN2;
  }
  if (arg < 0 || arg >= count) lp = -__builtin_inff();   // a given index out of range
  return arg;
}

// Choose and store, as policy_pass's tail: `out` holds the second product (packed WITH the value
// row, oc_policy_pack_w2v / _b2v).  pairs, logits, rng as policy_pass stores them (pairs may be NULL
// here); given int32 [n][2] or NULL; move_row / comm_row int32 [n], log_prob / value float [n], each
// NULL = not written.  Lanes past the batch (`valid` false) store nothing.
struct AcTail {
  const int32_t *given;
  int32_t *move_row, *comm_row;
  float *log_prob, *value;

  template <int CMAX>
  __device__ __forceinline__ void run(const f32x16 &out, uint32_t n32, uint32_t env, bool valid, int lane,
                                      uint32_t *rng, int32_t *pairs, float *logits, int C) const {
    const int h = lane >> 5;
    const int count = h ? C : 4;
    const int mode = given != nullptr ? AC_GIVEN : rng != nullptr ? AC_SAMPLE : AC_GREEDY;   // uniform
    uint32_t state = 0;
    int g = 0;
    if (mode == AC_SAMPLE) state = rng[(size_t)h * n32 + env];
    if (mode == AC_GIVEN) g = given[(size_t)env * 2 + h];
    float lp;
    const int choice = pick_lp<CMAX>(out, count, mode, g, state, lp);
    // the half-wave exchange: afterwards the second result holds, in lanes 0..31, what lanes 32..63
    // held -- the comm head's term of the same env (every lane takes part: outside `valid`)
    const uint32_t bits = __float_as_uint(lp);
    const auto sw = __builtin_amdgcn_permlane32_swap(bits, bits, false, false);
    float lp_sum;
    {
#pragma clang fp contract(off)
      lp_sum = lp + __uint_as_float(sw[1]);   // lower half: lp_move + lp_comm, in this order
    }
    if (valid) {
      if (pairs != nullptr) pairs[(size_t)env * 2 + h] = choice;
      if (mode == AC_SAMPLE) rng[(size_t)h * n32 + env] = state;
      if (logits != nullptr) {
#pragma unroll
        for (int c = 0; c < CMAX; c++)
          if (c < count) logits[(size_t)((h ? 4 : 0) + c) * n32 + env] = out[c] * K_LN2;   // natural-log logits
      }
      if (h == 0) {
        if (log_prob != nullptr) log_prob[env] = lp_sum;
        if (value != nullptr) value[env] = out[4] * K_LN2;   // row 8 of the product
        if (move_row != nullptr) move_row[env] = choice;
      } else {
        if (comm_row != nullptr) comm_row[env] = choice;
      }
    }
  }
};

}  // namespace ocpol
#endif
